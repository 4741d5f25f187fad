"""The Neumann contours inside the explicit step (nlps_gpu_set_explicit_loads) against the composition of
the oracle's stage calls (explicit_loads_ref.py; the composition and the margins of its scenarios are checked on the CPU by
test_explicit_loads_ref.py): every one-rank launch form of the step, re-sorts, replacement and removal, the level-B
traction stage beside it, and the refusals."""
import numpy as np
import pytest

import explicit_damage_ref as xr
import explicit_loads_ref as lr
from test_gpu_parity import masks
from util import assert_close, gpu_setup, nlps, orc, relerr

pytestmark = pytest.mark.gpu

PARTICLE = (("x_GC", "x"), ("dis", "dis"), ("vel", "vel"), ("acc", "acc"), ("F_n", "F_n"), ("J_n", "J_n"), ("rho", "rho"),
            ("Stress", "stress"))
NODAL = ("mass", "dU", "force", "accel", "reaction")


def loaded_solver(case, loads="default", prepare=None, params=None, bcs=True):
    """-> (handle, its Dirichlet sets); `loads`: a list of contours, None for a handle that never hears of loads"""
    n = nlps()
    kw = {} if params is None else {"params": params}
    S = gpu_setup(case, nsteps=lr.NSTEPS, **kw)
    if prepare:
        prepare(S)
    if loads == "default":
        loads = lr.contours(case)
    if loads is not None:
        S.set_explicit_loads(n.BccSet(loads), lr.THICKNESS, lr.area0(case))
    return S, n.BccSet(lr.dirichlet(case) if bcs else [])


def step(S, bset, t):
    S.explicit_step(bset, t, lr.DT[t], lr.GAMMA, gravity=lr.gravity(S.ndim))


def results(S):
    nod = S.explicit_nodal()
    st = S.download_state()
    return nod, st


def compare(S, snap, what, case, loads, t, tol=1e-9):
    nod, st = results(S)
    assert S.nactive == snap["na"], what
    for k in NODAL:
        assert_close(nod[k], snap["nodal"][k], tol, f"{what} nodal {k}")
    for k, ok in PARTICLE:
        assert_close(st[k], snap[ok], tol, f"{what} {k}")
    # partition of unity: the nodal force sums to sum T A0 over the contour entries (the internal forces sum to zero)
    got = nod["force"].reshape(-1, S.ndim).sum(axis=0)
    want = lr.total_traction(case, loads, t, lr.THICKNESS, lr.area0(case))
    e = np.abs(got - want).max() / np.abs(want).max()
    print(f"{what}: sum of the nodal force against sum T A0: {e:.2e}")
    assert e <= 1e-10, f"{what}: sum of the nodal force {got}, sum T A0 {want}"
    return nod, st


def run_against_checker(ndim, laws=0, prepare=None, nsteps=lr.NSTEPS):
    ref = lr.reference(ndim, laws)
    case = lr.loaded_case(ndim, laws)
    S, bset = loaded_solver(case, prepare=prepare)
    for t in range(nsteps):
        step(S, bset, t)
        compare(S, ref[t], f"{ndim}-D step {t}", case, lr.contours(case), t)
    S.close()


def assert_same(a, b, what):
    for k in NODAL:
        assert np.array_equal(a[0][k], b[0][k]), f"{what}: nodal {k}"
    for k, _ in PARTICLE:
        assert np.array_equal(a[1][k], b[1][k]), f"{what}: {k}"


@pytest.mark.parametrize("ndim", [2, 3])
def test_loaded_steps_default_form(ndim):
    """the folded form with the lists of the next step on the side stream"""
    run_against_checker(ndim)


@pytest.mark.parametrize("ndim", [2, 3])
def test_loaded_steps_without_async_lists(ndim):
    run_against_checker(ndim, prepare=lambda S: S.debug_option("async_lists", 0))


@pytest.mark.parametrize("ndim", [2, 3])
def test_loaded_steps_non_folded_form(ndim):
    run_against_checker(ndim, prepare=lambda S: S.debug_option("lazy_nodal", 0))


@pytest.mark.parametrize("ndim", [2, 3])
def test_loaded_steps_lane_mapping(ndim):
    """the one-lane-per-particle mapping of the kernel, kept behind the developer switch to measure against"""
    run_against_checker(ndim, prepare=lambda S: S.debug_option("loads_lane_map", 1), nsteps=3)


@pytest.mark.parametrize("ndim", [2, 3])
def test_loaded_steps_with_resorts(ndim):
    """the caller's indices keep addressing the same particles under a permutation of the slots"""
    def prepare(S):
        S.resort()
        S.set_resort_interval(2)
    run_against_checker(ndim, prepare=prepare)


@pytest.mark.parametrize("mode", [1, 2])
def test_loaded_steps_interleaved_laws(mode):
    """Neo-Hookean and Hencky particles in turn: one K3 launch per law, or the kernel that dispatches on the law"""
    run_against_checker(3, (0, 1), prepare=lambda S: S.set_law_launch_mode(mode))


@pytest.mark.parametrize("ndim", [2, 3])
def test_deterministic_mode_repeats_bit_for_bit(ndim):
    ref = lr.reference(ndim)
    case = lr.loaded_case(ndim)

    def prepare(S):
        S.set_deterministic(True)
        S.set_resort_interval(2)
    (A, ba), (B, bb) = loaded_solver(case, prepare=prepare), loaded_solver(case, prepare=prepare)
    for t in range(lr.NSTEPS):
        step(A, ba, t)
        step(B, bb, t)
        ra = compare(A, ref[t], f"deterministic {ndim}-D step {t}", case, lr.contours(case), t)
        assert_same(ra, results(B), f"two runs, step {t}")
    A.close()
    B.close()


def test_damage_step_with_loads_is_the_plain_loaded_step():
    """set_explicit_damage with an unreachable Gf: the non-folded damage form against the plain step, both loaded, 1e-12
    (the project's bound for equivalent launch forms)"""
    n = nlps()
    case = xr.erosion_case(3, 0, Gf=1e300)
    prm = n.default_params()
    prm.driver_eigenerosion = 1
    A, ba = loaded_solver(case, prepare=lambda S: S.set_explicit_damage(True), params=prm)
    B, bb = loaded_solver(case)
    worst = 0.0
    for t in range(3):
        step(A, ba, t)
        step(B, bb, t)
        (na, a), (nb, b) = results(A), results(B)
        assert A.nactive == B.nactive
        assert not a["Damage_n1"].any()
        for k in NODAL:
            worst = max(worst, relerr(na[k], nb[k]))
            assert_close(na[k], nb[k], 1e-12, f"step {t} nodal {k}")
        for k in [k for k, _ in PARTICLE] + ["DF", "F_n1", "J_n1"]:
            worst = max(worst, relerr(a[k], b[k]))
            assert_close(a[k], b[k], 1e-12, f"step {t} {k}")
    print(f"loaded damage form with an unreachable Gf against the loaded plain step: worst relative difference {worst:.2e}")
    # and the loads are in it
    assert_close(nb["force"], lr.reference(3)[2]["nodal"]["force"], 1e-9, "loaded force")
    A.close()
    B.close()


def deterministic(S):
    S.set_deterministic(True)


@pytest.mark.parametrize("ndim", [2, 3])
def test_replacement_and_removal(ndim):
    """deterministic mode, where equal inputs give equal bits: whatever an earlier set of loads left behind would show"""
    n = nlps()
    case = lr.loaded_case(ndim)
    loads_b = lr.contours(case)
    loads_a = [dict(loads_b[1], value=-3.0 * loads_b[1]["value"]), dict(loads_b[0], nodes=loads_b[0]["nodes"][:7]),
               dict(loads_b[0], value=0.5 * loads_b[0]["value"])]
    # A then B against B only
    (AB, b1), (B, b2) = loaded_solver(case, loads_a, deterministic), loaded_solver(case, loads_b, deterministic)
    AB.set_explicit_loads(n.BccSet(loads_b), lr.THICKNESS, lr.area0(case))
    # removed against never set, and contours that switch nothing on against never set
    (gone, b3), (never, b4) = loaded_solver(case, loads_b, deterministic), loaded_solver(case, None, deterministic)
    gone.set_explicit_loads(None)
    off, b5 = loaded_solver(case, lr.contours(case, all_off=True), deterministic)
    plain = lr.reference(ndim, 0, False)
    for t in range(3):
        for S, b in ((AB, b1), (B, b2), (gone, b3), (never, b4), (off, b5)):
            step(S, b, t)
        rb, rn = results(B), results(never)
        assert_same(results(AB), rb, f"loads A then B against B only, step {t}")
        assert_same(results(gone), rn, f"loads removed against never set, step {t}")
        assert_same(results(off), rn, f"dir 0 everywhere against never set, step {t}")
        assert_close(rn[0]["force"], plain[t]["nodal"]["force"], 1e-9, f"unloaded force, step {t}")
        assert relerr(rb[0]["force"], rn[0]["force"]) > 1e-3
    # one step of A on the handle that had B: the replacement works in this direction too
    AB.set_explicit_loads(n.BccSet(loads_a), lr.THICKNESS, lr.area0(case))
    step(AB, b1, 3)
    got = results(AB)[0]["force"].reshape(-1, ndim).sum(axis=0)
    want = lr.total_traction(case, loads_a, 3, lr.THICKNESS, lr.area0(case))
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    for S in (AB, B, gone, never, off):
        S.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_level_b_traction_stage_beside_the_explicit_loads(ndim):
    """nlps_gpu_nodal_traction_forces on a handle with explicit loads set answers as before, in front of the steps and on
    top of them, and the steps between are the checker's"""
    o, n = orc(), nlps()
    case = lr.loaded_case(ndim)
    bcs, a0 = lr.dirichlet(case), lr.area0(case)
    rng = np.random.default_rng(4)
    pick = rng.choice(case["cloud"]["x"].shape[0], size=24, replace=False).astype(np.int32)
    d2 = np.ones((ndim, lr.NSTEPS), dtype=np.int32)
    d2[0, 1] = 0
    other = [{"nodes": pick[:14], "dim": ndim, "dir": np.ones((ndim, lr.NSTEPS), dtype=np.int32),
              "value": rng.normal(size=(ndim, lr.NSTEPS)) * 1e7},
             {"nodes": pick[14:], "dim": ndim, "dir": d2, "value": rng.normal(size=(ndim, lr.NSTEPS)) * 1e7}]
    R = lr.LoadsRef(case, bcs, lr.contours(case), lr.NSTEPS, lr.gravity(ndim), lr.THICKNESS, a0)
    S, bset = loaded_solver(case)

    def stage(what):
        n2m, d2m, na = masks(S, R.M, bcs, 1, lr.NSTEPS)
        want = np.zeros(na * ndim)
        assert o.nodal_traction_forces(want, R.P, R.M, n2m, d2m, other, 1, lr.NSTEPS, 0.7, a0) == 0
        got = S.nodal_traction_forces(np.zeros(na * ndim), n.BccSet(other), 1, 0.7, a0)
        assert np.abs(want).max() > 0.0
        assert_close(got, want, 1e-10, what)

    stage("level-B tractions in front of the steps")
    ref = lr.reference(ndim)
    for t in range(2):
        R.step(t, lr.DT[t])
        step(S, bset, t)
        compare(S, ref[t], f"{ndim}-D step {t}", case, lr.contours(case), t)
    assert o.local_search(R.P, R.M, R.prm) == 0
    S.local_search()
    stage("level-B tractions on top of two loaded steps")
    S.close()


def test_refusals_leave_the_handle_usable():
    n = nlps()
    case = lr.loaded_case(3)
    loads, a0 = lr.contours(case), lr.area0(case)
    npart = case["cloud"]["x"].shape[0]
    S, bset = loaded_solver(case, None)
    bad = [dict(loads[0]), dict(loads[1], nodes=np.append(loads[1]["nodes"][:-1], npart).astype(np.int32))]
    with pytest.raises(n.NlpsError, match="particle index outside the cloud"):
        S.set_explicit_loads(n.BccSet(bad), lr.THICKNESS, a0)
    with pytest.raises(n.NlpsError, match="area0"):
        S.set_explicit_loads(n.BccSet(loads), lr.THICKNESS, None)
    S.set_halo_exchange(lambda dptr, nfield, elem, kind: 0)
    with pytest.raises(n.NlpsError, match="built for one rank"):
        S.set_explicit_loads(n.BccSet(loads), lr.THICKNESS, a0)
    S.set_halo_exchange(None)
    S.set_explicit_loads(n.BccSet(loads), lr.THICKNESS, a0)
    S.set_halo_exchange(lambda dptr, nfield, elem, kind: 0)
    with pytest.raises(n.NlpsError, match="built for one rank"):
        step(S, bset, 0)
    S.set_halo_exchange(None)
    with pytest.raises(n.NlpsError, match="step outside"):
        S.explicit_step(n.BccSet([]), lr.NSTEPS, lr.DT[0], lr.GAMMA)
    with pytest.raises(n.NlpsError, match="step outside"):
        S.explicit_step(n.BccSet([]), -1, lr.DT[0], lr.GAMMA)
    # nothing of the refused calls is left: the steps are the checker's
    ref = lr.reference(3)
    for t in range(2):
        step(S, bset, t)
        compare(S, ref[t], f"step {t} behind the refusals", case, loads, t)
    S.close()
    # 2-D: the thickness divides
    case2 = lr.loaded_case(2)
    P, b2 = loaded_solver(case2, None)
    with pytest.raises(n.NlpsError, match="thickness"):
        P.set_explicit_loads(n.BccSet(lr.contours(case2)), 0.0)
    P.set_explicit_loads(n.BccSet(lr.contours(case2)), lr.THICKNESS)
    step(P, b2, 0)
    compare(P, lr.reference(2)[0], "2-D step 0 behind the refusal", case2, lr.contours(case2), 0)
    P.close()
