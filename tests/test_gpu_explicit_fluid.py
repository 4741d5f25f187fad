"""The explicit step of a cloud that holds the compressible Newtonian fluid (nlps_gpu_set_explicit_fluid)
against the composition of the oracle's stage calls with the rate the header defines (explicit_fluid_ref.py, held to
orc.ExplicitStepper and to that definition on the CPU by test_explicit_fluid_ref.py): plain and mixed clouds, re-sorts,
the deterministic mode, contour loads, the step record and the snapshot behind such a step, a Newmark step behind it, the
switch with its refusals, and the failure path.

Bounds (the project's): 1e-10 after one step against the composition, 1e-9 after several, 1e-12 between equivalent launch
forms, bit equality where the deterministic mode or the snapshot promises it."""
import numpy as np
import pytest

import explicit_fluid_ref as xf
from test_gpu_fluid import FLUID, SOFT_NH
from test_gpu_snapshot import assert_same as assert_same_bits
from test_gpu_step_record import ALL, check_last_row, probe_ids
from util import assert_close, gpu_setup, nlps, relerr

pytestmark = pytest.mark.gpu

PARTICLE = (("x_GC", "x"), ("dis", "dis"), ("vel", "vel"), ("acc", "acc"), ("F_n", "F_n"), ("J_n", "J_n"), ("rho", "rho"),
            ("Stress", "stress"))
RATES = ("dt_F_n", "dt_F_n1")
NODAL = ("mass", "dU", "force", "accel", "reaction")
MATS = (FLUID, SOFT_NH)
ST_JACOBIAN = 4


def test_the_materials_are_those_of_the_implicit_tests():
    assert xf.FLUID == FLUID and xf.SOFT_NH == SOFT_NH


def gpu_case(ndim, materials=(0,), layout=None):
    """the checker's case with a rate history on every particle: the step carries nothing over from it, and the solid
    particles keep theirs"""
    case = xf.fluid_case(ndim, [MATS[m] for m in materials], layout)
    cloud = case["cloud"]
    cloud["dt_F_n"] = 0.1 * np.random.default_rng(21).normal(size=cloud["F_n"].shape)
    if ndim == 2:
        cloud["dt_F_n"][:, 4] = 0.0
    return case


def solver(case, prepare=None, switch=True, **kw):
    n = nlps()
    S = gpu_setup(case, nsteps=xf.NSTEPS, **kw)
    if switch:
        S.set_explicit_fluid(True)
    if prepare:
        prepare(S)
    return S, n.BccSet(xf.dirichlet(case))


def step(S, bset, t):
    S.explicit_step(bset, t, xf.DT, xf.GAMMA, gravity=xf.gravity(S.ndim))


def results(S):
    return S.explicit_nodal(), S.download_state()


def compare(S, snap, what, tol, nodal=NODAL):
    nod, st = results(S)
    assert S.status_flags() == 0, what
    assert S.nactive == snap["na"], what
    worst = 0.0
    for k in nodal:
        worst = max(worst, relerr(nod[k], snap["nodal"][k]))
        assert_close(nod[k], snap["nodal"][k], tol, f"{what} nodal {k}")
    for k, ok in PARTICLE:
        worst = max(worst, relerr(st[k], snap[ok]))
        assert_close(st[k], snap[ok], tol, f"{what} {k}")
    fl = snap["fluid"]
    for k in RATES:  # the step's rate in both slots, for the fluid particles
        worst = max(worst, relerr(st[k][fl], snap[k][fl]))
        assert_close(st[k][fl], snap[k][fl], tol, f"{what} {k} of the fluid particles")
    assert np.array_equal(st["dt_F_n"][fl], st["dt_F_n1"][fl]), what
    assert not st["W"][fl].any(), f"{what}: the fluid law writes no W"
    print(f"{what}: largest relative difference against the composition {worst:.2e}")
    return nod, st


def equal_to(a, b, tol, what):
    for k in NODAL:
        assert_close(a[0][k], b[0][k], tol, f"{what}: nodal {k}")
    for k in [k for k, _ in PARTICLE] + list(RATES):
        assert_close(a[1][k], b[1][k], tol, f"{what}: {k}")


def same_bits(a, b, what):
    for k in NODAL:
        assert np.array_equal(a[0][k], b[0][k]), f"{what}: nodal {k}"
    for k in a[1]:
        assert np.array_equal(a[1][k], b[1][k]), f"{what}: {k}"


@pytest.mark.parametrize("ndim", [2, 3])
def test_fluid_cloud(ndim):
    """four steps, every particle field, both rate slots and the nodal arrays after every step"""
    ref = xf.reference(ndim)
    case = gpu_case(ndim)
    S, bset = solver(case)
    for t in range(xf.NSTEPS):
        step(S, bset, t)
        nod, st = compare(S, ref[t], f"fluid {ndim}-D step {t}", 1e-10 if t == 0 else 1e-9)
        assert np.abs(nod["reaction"]).max() > 0.0 and np.abs(st["dt_F_n"]).max() > 1.0
    # the viscous term is in it: about the size of p_ref
    fl = np.arange(S.np)
    vis = np.array([xf.fluid_ref.stress_terms(FLUID, st["F_n"][p], st["dt_F_n"][p], st["J_n"][p], ndim)[2] for p in fl])
    assert np.abs(vis).max() > 0.1 * FLUID["p_ref"]
    S.close()


@pytest.mark.parametrize("layout", ["interleaved", "layers"])
def test_mixed_cloud(layout):
    """fluid + Neo-Hookean in one 3-D cloud: one K3 launch per law present; the solid particles' dt_F_n is untouched"""
    ref = xf.reference(3, (0, 1), layout)
    case = gpu_case(3, (0, 1), layout)
    fl = ref[0]["fluid"]
    assert 0 < np.count_nonzero(fl) < fl.size
    S, bset = solver(case)
    with pytest.raises(nlps().NlpsError, match="dispatch kernel does not hold Newtonian-Fluid-Compressible"):
        S.set_law_launch_mode(2)
    for t in range(3):
        step(S, bset, t)
        _, st = compare(S, ref[t], f"mixed {layout} step {t}", 1e-10 if t == 0 else 1e-9)
        assert np.array_equal(st["dt_F_n"][~fl], case["cloud"]["dt_F_n"][~fl]), "the solids keep their dt_F_n"
        assert np.abs(st["Stress"][~fl]).max() > 0.0 and np.abs(st["Stress"][fl]).max() > 0.0
    S.close()


@pytest.mark.parametrize("ndim,materials", [(2, (0,)), (3, (0, 1))])
def test_resorts(ndim, materials):
    """a re-sort in front of every second step against none: the rate slot travels with the particle"""
    layout = "interleaved" if len(materials) > 1 else None
    ref = xf.reference(ndim, materials, layout)
    case = gpu_case(ndim, materials, layout)

    def resorted(S):
        S.resort()
        S.set_resort_interval(2)
    (A, ba), (B, bb) = solver(case, prepare=resorted), solver(case)
    for t in range(xf.NSTEPS):
        step(A, ba, t)
        step(B, bb, t)
        ra = compare(A, ref[t], f"re-sorted {ndim}-D step {t}", 1e-9)
        equal_to(ra, results(B), 1e-12, f"re-sorted against not, step {t}")
    A.close()
    B.close()


@pytest.mark.parametrize("ndim,materials", [(2, (0,)), (3, (0,)), (3, (0, 1))])
def test_deterministic_mode(ndim, materials):
    """two fresh handles repeat bit for bit (one wave per tile and law, slabs); against the atomic run 1e-12"""
    layout = "interleaved" if len(materials) > 1 else None
    ref = xf.reference(ndim, materials, layout)
    case = gpu_case(ndim, materials, layout)

    def det(S):
        S.set_deterministic(True)
    (A, ba), (B, bb), (X, bx) = solver(case, prepare=det), solver(case, prepare=det), solver(case)
    for t in range(xf.NSTEPS):
        for S, b in ((A, ba), (B, bb), (X, bx)):
            step(S, b, t)
        ra = compare(A, ref[t], f"deterministic {ndim}-D step {t}", 1e-9)
        same_bits(ra, results(B), f"two deterministic runs, step {t}")
        equal_to(ra, results(X), 1e-12, f"deterministic against atomic, step {t}")
    for S in (A, B, X):
        S.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_contour_loads(ndim):
    """the +x face as a Neumann contour: nodal force and acceleration after one step"""
    n = nlps()
    ref, plain = xf.reference(ndim, loaded=True), xf.reference(ndim)
    case = gpu_case(ndim)
    S, bset = solver(case, prepare=lambda S: S.set_explicit_loads(n.BccSet(xf.face_contour(case)), 1.0, xf.area0(case)))
    step(S, bset, 0)
    nod, _ = compare(S, ref[0], f"loaded {ndim}-D", 1e-10)
    assert relerr(nod["force"], plain[0]["nodal"]["force"]) > 1e-3, "the tractions are in it"
    S.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_step_record_and_snapshot_behind_a_fluid_step(ndim):
    n = nlps()
    case = gpu_case(ndim)
    bcs = xf.dirichlet(case)
    S, bset = solver(case)
    probes = probe_ids(S.np)
    S.set_step_record(every=1, capacity=2, nsets=1, probes=probes, probe_fields=ALL)
    S.set_snapshots(n.SNAP_ALL, 1)
    time = 0.0
    for t in range(2):
        step(S, bset, t)
        time += xf.DT
        slot = S.snapshot_begin(t)
        rec, st = check_last_row(S, bcs, t, n.REC_KIND_EXPLICIT, xf.DT, time, probes, ALL, f"fluid {ndim}-D step {t}")
        snap = S.snapshot_wait(slot)
        assert {"Stress", "F_n", "J_n", "rho"} <= set(snap)
        assert_same_bits(snap, st, f"snapshot behind fluid step {t}")
        S.snapshot_release(slot)
        assert rec["status"][-1] == 0.0 and np.abs(rec["reactions"][-1]).max() > 0.0
        assert np.abs(st["Stress"]).max() > 1.0 and rec["strain"][-1] == 0.0
    S.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_a_newmark_step_behind_an_explicit_step(ndim):
    """the rolled rate is what the implicit path reads: the same Newmark step on a handle re-created from a download
    taken behind the explicit step, dt_F_n included"""
    case = gpu_case(ndim)
    A, ba = solver(case)
    step(A, ba, 0)
    st = A.download_state()
    assert np.abs(st["dt_F_n"]).max() > 1.0
    cloud = dict(case["cloud"])
    for ck, k in (("x_GC", "x"), ("dis", "dis"), ("vel", "vel"), ("acc", "acc"), ("F_n", "F_n"), ("b_e_n", "b_e_n"),
                  ("J_n", "J_n"), ("rho", "rho"), ("dt_F_n", "dt_F_n"), ("lambda_", "lambda"), ("Beta", "beta"), ("I0", "I0")):
        cloud[k] = st[ck].copy()
    B, bb = solver(dict(case, cloud=cloud), init=False)
    kw = dict(max_it=50, atol=1e-8, rtol=1e-10, stol=1e-8, linesearch="bt",
              ksp=dict(pc="pbjacobi", restart=200, max_it=2000, rtol=1e-12))
    for S, b in ((A, ba), (B, bb)):
        info = S.newmark_step(b, 1, xf.DT, xf.gravity(ndim), **kw)
        assert info["reason"] > 0 and info["iterations"] >= 1, info
    a, b = A.download_state(), B.download_state()
    for k in ("x", "vel", "acc", "F_n", "Stress", "J_n", "dt_F_n"):
        assert_close(a[k], b[k], 1e-10, f"Newmark step behind the explicit step: {k}")
    assert relerr(a["dt_F_n"], st["dt_F_n"]) > 1e-6, "the Newmark step made a rate of its own from the rolled one"
    A.close()
    B.close()


def test_switch_and_refusals():
    n = nlps()
    case = gpu_case(3)
    ref = xf.reference(3)
    S, bset = solver(case, switch=False)
    with pytest.raises(n.NlpsError, match="nlps_gpu_explicit_step.*Newtonian-Fluid-Compressible.*implicit path only"):
        step(S, bset, 0)
    S.set_explicit_fluid(True)
    S.set_explicit_fluid(False)
    with pytest.raises(n.NlpsError, match="implicit path only"):
        step(S, bset, 0)
    S.set_explicit_fluid(True)
    S.set_halo_exchange(lambda dptr, nfield, elem, kind: 0)
    with pytest.raises(n.NlpsError, match="built for one rank"):
        step(S, bset, 0)
    S.set_halo_exchange(None)
    with pytest.raises(n.NlpsError, match="dt must be positive"):
        S.explicit_step(bset, 0, 0.0, xf.GAMMA, gravity=xf.gravity(3))
    step(S, bset, 0)  # nothing of the refused calls is left
    compare(S, ref[0], "behind the refusals", 1e-10)
    S.close()
    # a cloud without the law
    N, _ = solver(xf.fluid_case(3, [SOFT_NH]), switch=False)
    with pytest.raises(n.NlpsError, match="nlps_gpu_set_explicit_fluid: .*no Newtonian-Fluid-Compressible"):
        N.set_explicit_fluid(True)
    N.close()
    # the fluid in a cloud with the damage driver
    prm = n.default_params()
    prm.driver_eigenerosion = 1
    D, bd = solver(dict(case, materials=[dict(FLUID, Ceps=1.5, Gf=1e300)]), params=prm)
    with pytest.raises(n.NlpsError, match="driver_eigenerosion"):
        step(D, bd, 0)
    D.close()


def test_a_singular_F_raises_the_jacobian_flag_and_stays_alone():
    """One particle with a singular F_n (one zero row): F_n1 = DF F_n has a zero column, J_n1 = 0 exactly, so the step sets
    the Jacobian bit (4) as MODE 1 does for J <= 0; the law fails on it (bit 8) and the particle contributes neither
    stress nor force, so every other particle's fields stay finite."""
    case = gpu_case(3)
    cloud = case["cloud"]
    bad = cloud["x"].shape[0] // 2
    F = cloud["F_n"].copy()
    F[bad] = np.eye(3).ravel()
    F[bad, 3:6] = 0.0
    cloud["F_n"] = F
    S, bset = solver(case)
    step(S, bset, 0)
    flags = S.status_flags()
    assert flags & ST_JACOBIAN, flags
    st = S.download_state()
    others = np.arange(S.np) != bad
    for k, a in st.items():
        assert np.isfinite(a[others]).all(), k
    assert np.abs(st["Stress"][others]).max() > 1.0
    S.close()
