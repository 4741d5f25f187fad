"""The explicit step with F-bar on lattice-cell patches (nlps_gpu_set_explicit_fbar) against the composition of
the oracle's stage calls with the insertion include/nlps_gpu.h defines (explicit_fbar_ref.py, held to orc.ExplicitStepper and
to that definition on the CPU by test_explicit_fbar_ref.py): Neo-Hookean clouds at nu = 0.49 with patches of one cell and
of 3 cells a side across the tile seam at node 16, the fluid, mixed clouds, re-sorts, contour loads with the step record and
snapshots, a restart, the switch and its refusals.

Bounds (the project's): 1e-10 after one step against the composition, 1e-9 after several, 1e-12 between equivalent runs."""
import numpy as np
import pytest

import explicit_fbar_ref as xb
import explicit_fluid_ref as xf
from test_gpu_snapshot import assert_same as assert_same_bits
from test_gpu_step_record import ALL, check_last_row, probe_ids
from util import assert_close, gpu_setup, nlps, relerr

pytestmark = pytest.mark.gpu

PARTICLE = (("x_GC", "x"), ("dis", "dis"), ("vel", "vel"), ("acc", "acc"), ("F_n", "F_n"), ("J_n", "J_n"), ("rho", "rho"),
            ("Stress", "stress"), ("W", "W"))
NODAL = ("mass", "dU", "force", "accel", "reaction")
FLUID_TYPE = xb.FLUID["type"]


def has_fluid(case):
    return any(m["type"] == FLUID_TYPE for m in case["materials"])


def w_tol(tol, materials, W_ref):
    """The bound W is held to: the project's bound `tol` relative to max |W|, like every field, but never below what one
    EVALUATION of W in binary64 can repeat.  Neo-Hookean-Wriggers' W = mu / 2 (I1 - 3) - mu ln J + lambda / 4 (J^2 - 1) -
    lambda / 2 ln J forms I1 = F : F, a sum of d^2 products of size 3 in all, and takes 3 from it: terms of size T = 1.5 mu
    that cancel down to a W of mu x strain.  Eight roundings of half a unit in the last place on terms of that size are
    4 eps T -- measured: two runs whose F_n agree to ONE unit in the last place (2.2e-16) differ in W by 1.3e-12 of max |W|
    at nu = 0.49 after one step, where 4 eps T / max |W| is 4.2e-12.  So the bound is max(tol, 4 eps T / max |W|), with T
    from the stiffest hyperelastic material of the cloud: a floor of a few 1e-12 that only the 1e-12 comparisons between
    equivalent runs ever reach; against the checker W is held to the project's 1e-10 / 1e-9 as it stands."""
    mu = max([m["E"] / (2.0 * (1.0 + m["nu"])) for m in materials if m["type"] in (0, 1)] + [0.0])
    floor = 4.0 * np.finfo(np.float64).eps * 1.5 * mu / max(float(np.abs(W_ref).max()), 1e-300)
    return max(tol, floor), floor


def setup(case, **kw):
    S = gpu_setup(case, **kw)
    S.materials = case["materials"]
    return S


def solver(case, alpha, block=1, prepare=None, **kw):
    """alpha None: the handle without F-bar"""
    n = nlps()
    S = setup(case, nsteps=xb.NSTEPS, **kw)
    if has_fluid(case):
        S.set_explicit_fluid(True)
    if prepare:
        prepare(S)
    if alpha is not None:
        S.set_explicit_fbar(alpha, block)
    return S, n.BccSet(xb.dirichlet(case))


def step(S, bset, t):
    S.explicit_step(bset, t, xb.DT, xb.GAMMA, gravity=xb.gravity(S.ndim))


def results(S, fbar=True):
    return S.explicit_nodal(), S.download_state(), (S.download_fbar() if fbar else None)


def compare(S, snap, what, tol, fbar=True):
    nod, st, bar = results(S, fbar)
    assert S.status_flags() == 0, what
    assert S.nactive == snap["na"], what
    worst = 0.0
    for k in NODAL:
        worst = max(worst, relerr(nod[k], snap["nodal"][k]))
        assert_close(nod[k], snap["nodal"][k], tol, f"{what} nodal {k}")
    fl = snap["fluid"]
    for k, ok in PARTICLE:
        # (the fluid law writes no W; the checker's rows hold the W of the Neo-Hookean stand-in of fluid_ref.OracleFluid)
        rows = ~fl if k == "W" else np.ones_like(fl)
        if rows.any():
            bound = tol
            if k == "W":
                bound, floor = w_tol(tol, S.materials, snap[ok][rows])
                print(f"{what} W: {relerr(st[k][rows], snap[ok][rows]):.2e} of max |W| (bound {bound:.1e}: project {tol:.0e}, "
                      f"evaluation floor {floor:.1e})")
            else:
                worst = max(worst, relerr(st[k][rows], snap[ok][rows]))
            assert_close(st[k][rows], snap[ok][rows], bound, f"{what} {k}")
    assert not st["W"][fl].any(), f"{what}: the fluid law writes no W"
    if fl.any():  # the unbarred rate of the step, in both slots
        for k in ("dt_F_n", "dt_F_n1"):
            worst = max(worst, relerr(st[k][fl], snap[k][fl]))
            assert_close(st[k][fl], snap[k][fl], tol, f"{what} {k} of the fluid particles")
    if fbar:
        for got, k in zip(bar, ("Fbar_n", "Jbar_n")):
            worst = max(worst, relerr(got, snap[k]))
            assert_close(got, snap[k], tol, f"{what} {k}")
    print(f"{what}: largest relative difference against the composition {worst:.2e} (bound {tol:.0e})")
    return nod, st, bar


def equal_to(a, b, tol, what, materials=(xb.NH49,)):
    for k in NODAL:
        assert_close(a[0][k], b[0][k], tol, f"{what}: nodal {k}")
    for k, _ in PARTICLE:
        bound = tol
        if k == "W":
            bound, floor = w_tol(tol, materials, b[1][k])
            print(f"{what}: W {relerr(a[1][k], b[1][k]):.2e} of max |W| (bound {bound:.1e}: project {tol:.0e}, evaluation floor "
                  f"{floor:.1e})")
        assert_close(a[1][k], b[1][k], bound, f"{what}: {k}")
    if a[2] is not None and b[2] is not None:
        for x, y, k in zip(a[2], b[2], ("Fbar_n", "Jbar_n")):
            assert_close(x, y, tol, f"{what}: {k}")


def tol_at(t):
    return 1e-10 if t == 0 else 1e-9


@pytest.mark.parametrize("block", [1, 3])
@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("ndim", [2, 3])
def test_neo_hookean_cloud(ndim, alpha, block):
    """nu = 0.49 under gravity on a Dirichlet plane, four steps: every particle field, the barred state and the nodal arrays
    after every step.  Block 3: cells 15 - 17 are one patch across the seam between the tiles at node 16."""
    ref = xb.reference(ndim, (0,), (alpha,), block)
    case = xb.fbar_case(ndim)
    S, bset = solver(case, [alpha], block)
    I0 = S.download_state()["I0"]
    g = case["grid_n"]
    ijk = np.stack([(I0 // int(np.prod(g[:k]))) % g[k] for k in range(ndim)], axis=1)
    assert (ijk.min(axis=0) < 16).all() and (ijk.max(axis=0) >= 16).all(), "closest nodes on both sides of node 16, every axis"
    if block == 3:
        cells = ref[0]["last"]["cells"]
        assert ((cells >= 15) & (cells <= 17)).all(axis=1).any() and (cells < 15).any()
    for t in range(xb.NSTEPS):
        step(S, bset, t)
        nod, st, bar = compare(S, ref[t], f"Neo-Hookean {ndim}-D alpha {alpha} block {block} step {t}", tol_at(t))
        assert np.abs(nod["reaction"]).max() > 0.0
    assert relerr(bar[0], st["F_n"]) > 1e-6 or alpha == 1.0, "the barred gradient is not the plain one"
    assert relerr(bar[1], st["J_n"]) > 1e-6
    S.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_fluid_cloud(ndim):
    """the fluid with alpha = 0: the pressure from Jbar, the viscous part from the unbarred rate of nlps_gpu_set_explicit_fluid"""
    ref = xb.reference(ndim, (1,), (0.0,), 1)
    case = xb.fbar_case(ndim, (1,))
    S, bset = solver(case, [0.0])
    for t in range(xb.NSTEPS):
        step(S, bset, t)
        _, st, _ = compare(S, ref[t], f"fluid {ndim}-D step {t}", tol_at(t))
        assert np.abs(st["dt_F_n"]).max() > 1.0 and not st["W"].any()
    S.close()


@pytest.mark.parametrize("layout", ["interleaved", "tiles"])
def test_mixed_cloud_of_fluid_and_plain_neo_hookean(layout):
    """fluid with alpha = 0 beside Neo-Hookean with alpha < 0, in turn and one law per tile: one launch per law present (the
    only launch mode there is for a cloud with the fluid); the solid's stress is the law's at the unbarred state, and its
    volume is in the patch sums"""
    mats, alpha = (1, 2), (0.0, -1.0)
    ref = xb.reference(3, mats, alpha, 1, layout)
    case = xb.fbar_case(3, mats, layout)
    fl = ref[0]["fluid"]
    assert 0 < np.count_nonzero(fl) < fl.size
    S, bset = solver(case, list(alpha))
    with pytest.raises(nlps().NlpsError, match="dispatch kernel does not hold Newtonian-Fluid-Compressible"):
        S.set_law_launch_mode(2)
    for t in range(3):
        step(S, bset, t)
        _, st, _ = compare(S, ref[t], f"mixed {layout} step {t}", tol_at(t))
        assert np.abs(st["Stress"][~fl]).max() > 0.0 and np.abs(st["Stress"][fl]).max() > 0.0
    S.close()


@pytest.mark.parametrize("name,partner", [("Hencky", 3), ("Drucker-Prager", 4)])
def test_mixed_cloud_of_two_solids_in_both_launch_modes(name, partner):
    """Neo-Hookean (nu = 0.49) with alpha = 0.5 beside a solid with alpha < 0, dealt in turn: one launch per law present
    (mode 1) and the kernel that dispatches on the law (mode 2).  With Drucker-Prager the stress kernel writes the internal
    variables of a plastic law back (b_e, kappa, eps to their n slots, as the state half of the damage step does)."""
    mats, alpha = (0, partner), (0.5, -1.0)
    ref = xb.reference(3, mats, alpha, 3, "interleaved")
    case = xb.fbar_case(3, mats, "interleaved")
    runs = []
    for mode in (1, 2):
        S, bset = solver(case, list(alpha), 3, prepare=lambda S, m=mode: S.set_law_launch_mode(m))
        for t in range(2):
            step(S, bset, t)
            r = compare(S, ref[t], f"{name}, launch mode {mode}, step {t}", tol_at(t))
            for k, ok in (("b_e_n", "b_e_n"), ("Kappa_n", "kappa_n"), ("EPS_n", "eps_n")):
                assert_close(r[1][k], ref[t][ok], tol_at(t), f"{name}, launch mode {mode}, step {t}: {k}")
        if partner == 4:
            assert relerr(r[1]["b_e_n"], case["cloud"]["b_e_n"]) > 1e-6, "the elastic left Cauchy-Green tensor has moved"
        runs.append(r)
        S.close()
    equal_to(runs[0], runs[1], 1e-12, f"{name}: one launch per law against the dispatch kernel", case["materials"])
    for k in ("b_e_n", "Kappa_n", "EPS_n"):
        assert_close(runs[0][1][k], runs[1][1][k], 1e-12, f"{name}: one launch per law against the dispatch kernel: {k}")


@pytest.mark.parametrize("ndim", [2, 3])
def test_resorts(ndim):
    """nlps_gpu_resort between the steps, and a re-sort interval of 1, against no re-sort: Fbar_n / Jbar_n travel with the
    particles and come back in the caller's order"""
    ref = xb.reference(ndim, (0,), (0.5,), 3)
    case = xb.fbar_case(ndim)
    (A, ba), (B, bb), (X, bx) = (solver(case, [0.5], 3), solver(case, [0.5], 3, prepare=lambda S: S.set_resort_interval(1)),
                                 solver(case, [0.5], 3, prepare=lambda S: S.set_resort_interval(0)))
    for t in range(xb.NSTEPS):
        if t > 0:
            A.resort()
        for S, b in ((A, ba), (B, bb), (X, bx)):
            step(S, b, t)
        ra = compare(A, ref[t], f"nlps_gpu_resort {ndim}-D step {t}", 1e-9)
        rb = compare(B, ref[t], f"re-sort interval 1 {ndim}-D step {t}", 1e-9)
        rx = results(X)
        equal_to(ra, rx, 1e-12, f"nlps_gpu_resort against no re-sort, step {t}")
        equal_to(rb, rx, 1e-12, f"re-sort interval 1 against no re-sort, step {t}")
    for S in (A, B, X):
        S.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_contour_loads_step_record_and_snapshots_on_the_same_handle(ndim):
    n = nlps()
    ref, plain = xb.reference(ndim, (0,), (0.5,), 3, loaded=True), xb.reference(ndim, (0,), (0.5,), 3)
    case = xb.fbar_case(ndim)
    bcs = xb.dirichlet(case)

    def prepare(S):
        S.set_explicit_loads(n.BccSet(xf.face_contour(case)), 1.0, xf.area0(case))
    S, bset = solver(case, [0.5], 3, prepare=prepare)
    probes = probe_ids(S.np)
    S.set_step_record(every=1, capacity=2, nsets=1, probes=probes, probe_fields=ALL)
    S.set_snapshots(n.SNAP_ALL, 1)
    time = 0.0
    for t in range(2):
        step(S, bset, t)
        time += xb.DT
        slot = S.snapshot_begin(t)
        rec, st = check_last_row(S, bcs, t, n.REC_KIND_EXPLICIT, xb.DT, time, probes, ALL, f"F-bar {ndim}-D step {t}")
        snap = S.snapshot_wait(slot)
        assert_same_bits(snap, st, f"snapshot behind F-bar step {t}")
        S.snapshot_release(slot)
        assert rec["total"] == t + 1, "a record row behind every step"
        assert rec["status"][-1] == 0.0 and rec["strain"][-1] > 0.0
        nod, _, _ = compare(S, ref[t], f"loaded, recorded {ndim}-D step {t}", tol_at(t))
    assert relerr(nod["force"], plain[1]["nodal"]["force"]) > 1e-3, "the tractions are in it"
    S.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_a_restart_from_the_downloads_continues_the_run(ndim):
    """four steps straight against two steps, a new handle made from download_state and download_fbar, two more: 1e-12"""
    ref = xb.reference(ndim, (0,), (0.5,), 3)
    case = xb.fbar_case(ndim)
    A, ba = solver(case, [0.5], 3)
    for t in range(2):
        step(A, ba, t)
    st, (Fb, Jb) = A.download_state(), A.download_fbar()
    cloud = dict(case["cloud"])
    for ck, k in (("x_GC", "x"), ("dis", "dis"), ("vel", "vel"), ("acc", "acc"), ("F_n", "F_n"), ("J_n", "J_n"), ("rho", "rho"),
                  ("lambda_", "lambda"), ("Beta", "beta"), ("I0", "I0")):
        cloud[k] = st[ck].copy()
    B = setup(dict(case, cloud=cloud), init=False, nsteps=xb.NSTEPS)
    B.set_explicit_fbar([0.5], 3, Fbar_n=Fb, Jbar_n=Jb)
    bb = nlps().BccSet(xb.dirichlet(case))
    for t in (2, 3):
        step(A, ba, t)
        step(B, bb, t)
        rb = compare(B, ref[t], f"restarted {ndim}-D step {t}", 1e-9)
        equal_to(rb, results(A), 1e-12, f"restarted against straight, step {t}")
    A.close()
    B.close()


def test_switch():
    """off by default: the step of the same cloud is today's; NULL drops, and the next step is plain again"""
    case = xb.fbar_case(3)
    plain = xb.reference(3, (0,), None)
    ref = xb.reference(3, (0,), (0.0,), 1)
    n = nlps()
    S, bset = solver(case, None)
    with pytest.raises(n.NlpsError, match="F-bar is not set"):
        S.download_fbar()
    step(S, bset, 0)
    compare(S, plain[0], "off by default", 1e-10, fbar=False)
    S.close()
    S, bset = solver(case, [0.0])
    step(S, bset, 0)
    compare(S, ref[0], "set", 1e-10)
    assert relerr(S.download_state()["Stress"], plain[0]["stress"]) > 1e-3
    S.close()
    # dropped behind two F-bar steps: the next steps are plain steps from the state those left (tau and W stored, J in its n
    # slot, the twins freed), which is the plain checker started from the F-bar checker's state after step 1
    S, bset = solver(case, [0.0])
    for t in range(2):
        step(S, bset, t)
    S.set_explicit_fbar(None)
    with pytest.raises(n.NlpsError, match="F-bar is not set"):
        S.download_fbar()
    cont = dict(case, cloud=dict(case["cloud"]))
    for ck, k in (("x", "x"), ("dis", "dis"), ("vel", "vel"), ("acc", "acc"), ("F_n", "F_n"), ("J_n", "J_n"), ("rho", "rho")):
        cont["cloud"][ck] = ref[1][k].copy()
    R = xf.FluidStepRef(cont, xb.dirichlet(case), (), xb.NSTEPS, xb.gravity(3))
    for k in ("lambda", "beta", "I0"):
        R.P[k][...] = ref[1][k]
    for t in (2, 3):
        step(S, bset, t)
        R.step(t, xb.DT)
        compare(S, R.snapshot(), f"dropped behind two F-bar steps, step {t}", 1e-9, fbar=False)
    S.close()
    # set and dropped in front of the first step: plain from the start
    S, bset = solver(case, [0.0])
    S.set_explicit_fbar(None)
    for t in range(2):
        step(S, bset, t)
        compare(S, plain[t], f"dropped, step {t}", tol_at(t), fbar=False)
    S.close()


def test_refusals_of_the_setter_and_of_the_step():
    """every refusal is followed by a good step that still matches the checker: nothing of the refused call is left"""
    n = nlps()
    case = xb.fbar_case(3, (0, 3), "interleaved")
    alpha = [0.5, -1.0]
    ref = xb.reference(3, (0, 3), (0.5, -1.0), 3, "interleaved")
    S, bset = solver(case, alpha, 3)
    t = 0
    for bad_alpha, bad_block, match in (
            (alpha, [1, 0, 1], "block entry is < 1"),
            ([1.5, -1.0], 3, "alpha is > 1"),
            ([0.5, 0.5], 3, "neither Neo-Hookean nor Newtonian-Fluid-Compressible"),
            ([-1.0, -1.0], 3, "every alpha is < 0")):
        with pytest.raises(n.NlpsError, match="nlps_gpu_set_explicit_fbar: .*" + match):
            S.set_explicit_fbar(bad_alpha, bad_block)
        step(S, bset, t)  # the configuration of before the refused call is still the handle's
        compare(S, ref[t], f"behind the refusal '{match}'", tol_at(t))
        t += 1
    S.close()
    # a handle with an exchange attached; F-bar set first and the exchange attached later: the step refuses
    S, bset = solver(case, None)
    S.set_halo_exchange(lambda dptr, nfield, elem, kind: 0)
    with pytest.raises(n.NlpsError, match="nlps_gpu_set_explicit_fbar: .*one rank"):
        S.set_explicit_fbar(alpha, 3)
    S.set_halo_exchange(None)
    S.set_explicit_fbar(alpha, 3)
    S.set_halo_exchange(lambda dptr, nfield, elem, kind: 0)
    with pytest.raises(n.NlpsError, match="nlps_gpu_explicit_step: F-bar is built for one rank"):
        step(S, bset, 0)
    S.set_halo_exchange(None)
    S.set_deterministic(True)
    with pytest.raises(n.NlpsError, match="nlps_gpu_explicit_step: F-bar is not built for the deterministic mode"):
        step(S, bset, 0)
    S.set_deterministic(False)
    step(S, bset, 0)
    compare(S, ref[0], "behind the refused steps", 1e-10)
    S.close()
    # a cloud with a damage driver
    prm = n.default_params()
    prm.driver_eigenerosion = 1
    D = setup(dict(xb.fbar_case(3), materials=[dict(xb.NH49, Ceps=1.5, Gf=1e300)]), nsteps=xb.NSTEPS, params=prm)
    with pytest.raises(n.NlpsError, match="nlps_gpu_set_explicit_fbar: .*driver_eigenerosion"):
        D.set_explicit_fbar([0.5], 1)
    # ... and the handle goes on as a damage cloud: with Gf = 1e300 nobody fails, so its step is the plain checker's
    D.set_explicit_damage(True)
    bd = n.BccSet(xb.dirichlet(xb.fbar_case(3)))
    plain = xb.reference(3, (0,), None)
    for t in range(2):
        step(D, bd, t)
        compare(D, plain[t], f"behind the refusal of a damage cloud, step {t}", tol_at(t), fbar=False)
    D.close()


def test_a_fluid_material_still_needs_the_fluid_switch():
    n = nlps()
    case = xb.fbar_case(3, (1,))
    ref = xb.reference(3, (1,), (0.0,), 1)
    S = setup(case, nsteps=xb.NSTEPS)
    S.set_explicit_fbar([0.0], 1)
    bset = n.BccSet(xb.dirichlet(case))
    with pytest.raises(n.NlpsError, match="nlps_gpu_explicit_step.*Newtonian-Fluid-Compressible.*implicit path only"):
        step(S, bset, 0)
    S.set_explicit_fluid(True)
    step(S, bset, 0)
    compare(S, ref[0], "behind the refusal", 1e-10)
    S.close()


def test_a_migrated_handle_is_refused():
    n = nlps()
    case = xb.fbar_case(3)
    S, bset = solver(case, None)
    step(S, bset, 0)
    n_down, n_up, _, _, dptr_up = S.migration_select(0, 15)  # the particles of the node layers above 15 leave ...
    assert n_down == 0 and 0 < n_up < S.np
    S.migration_commit(dptr_up, n_up, 0, 0)                 # ... and come straight back: the same cloud, rows by global id
    assert S.num_particles() == case["cloud"]["x"].shape[0]
    with pytest.raises(n.NlpsError, match="nlps_gpu_set_explicit_fbar: .*migration"):
        S.set_explicit_fbar([0.5], 1)
    plain = xb.reference(3, (0,), None)
    step(S, bset, 1)  # nothing of the refused call is left: the plain step goes on
    compare(S, plain[1], "behind the refusal of a migrated handle", 1e-9, fbar=False)
    S.close()


def test_the_level_b_and_implicit_calls_are_refused_while_fbar_is_set():
    n = nlps()
    case = xb.fbar_case(2)
    ref = xb.reference(2, (0,), (0.5,), 1)
    S, bset = solver(case, [0.5], 1)
    S.active_masks(bset, 0)
    z = np.zeros(S.nactive * 2)
    calls = {"nlps_gpu_compatibility": lambda: S.local_compatibility_conditions(z),
             "nlps_gpu_constitutive": lambda: S.constitutive_update(),
             "nlps_gpu_lagrangian_evaluation": lambda: S.lagrangian_evaluation(z, z, z, z + 1.0, (1.0, 1.0, 1.0, 1.0, 1.0, 1.0)),
             "nlps_gpu_tangent_assemble": lambda: S.jacobian_evaluation(),
             "nlps_gpu_tangent_operator": lambda: S.tangent_operator(),
             "nlps_gpu_tangent_csr_pattern": lambda: S.tangent_csr_pattern(),
             "nlps_gpu_tangent_bsr_pattern": lambda: S.tangent_bsr_pattern(),
             "nlps_gpu_tangent_lambda_max": lambda: S.tangent_lambda_max(z + 1.0),
             "nlps_gpu_newton_solve": lambda: S.newton_solve(z.copy(), z, z, z + 1.0, (1.0, 1.0, 1.0, 1.0, 1.0, 1.0)),
             "nlps_gpu_newmark_step": lambda: S.newmark_step(bset, 0, xb.DT, xb.gravity(2))}
    for name, call in calls.items():
        with pytest.raises(n.NlpsError, match=name + ": F-bar is set on this handle"):
            call()
    step(S, bset, 0)
    compare(S, ref[0], "behind the refused level-B calls", 1e-10)
    S.set_explicit_fbar(None)
    S.constitutive_update()  # dropped: the stages are back
    S.close()
