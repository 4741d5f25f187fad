"""nlps_gpu_set_deterministic on the implicit path: the fused residual, the separate stage calls, the lumped
mass and the nodal field, the matrix-free product and its diagonal blocks, the traction loads, the Newton solve and the
one-call Newmark step return the SAME BITS on two runs from the same inputs -- on one handle and across handles.  The
default path (f64 atomics in arrival order) agrees with them to the bounds below.

Clouds: those of tests/test_gpu_deterministic.py (three tiles per axis in 3-D, so interior nodes sit in up to eight
windows; tile counts that are no multiple of 64).  Dirichlet plane, gravity and Newmark parameters: those of
tests/test_gpu_newton_solve.py.

ATOMIC_BOUND, "agrees with the atomic path": the project's atomic-versus-deterministic bound, 1e-11 of the largest
magnitude of the compared array, unless ten times the spread between two ATOMIC evaluations of the same quantity on
these clouds (measured on the library before this mode existed) is larger; no bound comes from the
deterministic results."""
import functools

import numpy as np
import pytest

from test_gpu_deterministic import dense_case
from test_gpu_fluid import FLUID
from test_gpu_newton_solve import DRIVER, _alpha
from util import DP, NH, assert_close, dirichlet_plane, gpu_setup, make_case, nlps, oracle_setup, orc

pytestmark = pytest.mark.gpu

# Largest spread between two atomic evaluations of one quantity on these clouds, measured on the MI355X with the library
# as it was before this mode covered the implicit path, relative to the largest magnitude: lumped mass
# 1.5e-15, nodal velocity 2.1e-15, residual 1.1e-16 (fused and separate stages, every law), K x 1.6e-16, diagonal blocks
# 2.8e-16, residual with traction loads 0 (24 contour particles).  Ten times each stays below the project's 1e-11, which
# therefore is the bound for every quantity.
ATOMIC_BOUND = 1e-11
STATE = ("DF", "F_n1", "J_n1", "Stress", "b_e_n1")
NSTEPS = 3
DT = 1.0e-2


@functools.lru_cache(maxsize=None)
def cloud(ndim, law):
    """The clouds of tests/test_gpu_deterministic.py; law: "nh", "dp", "mixed" (three laws interleaved p % 3), "fluid"."""
    material = {"nh": NH, "dp": DP, "mixed": DP, "fluid": FLUID}[law]
    vel = [0.0] * (ndim - 1) + [-10.0 if law == "nh" else -0.2]
    if ndim == 3:
        case = make_case(3, [14, 13, 12], [3, 3, 2], [8, 7, 7], material=material, velocity=vel)
    else:
        case = make_case(2, [40, 30], [3, 3], [34, 22], material=material, velocity=vel)
    npart = case["cloud"]["x"].shape[0]
    if law == "mixed":
        case["materials"] = [{"type": 0, "E": 2.0e4, "nu": 0.3}, {"type": 1, "E": 1.0e4, "nu": 0.25}, DP]
        case["cloud"]["matidx"] = (np.arange(npart) % 3).astype(np.int32)
    if law == "fluid":  # a rate history: dt_F_n1 = dt_DF F_n + DF dt_F_n
        case["cloud"]["dt_F_n"] = 0.1 * np.random.default_rng(3).normal(size=case["cloud"]["F_n"].shape)
    return case


def problem(case):
    ndim = case["ndim"]
    bcs = nlps().BccSet([dirichlet_plane(case, ndim - 1, 3 if ndim == 2 else 2, NSTEPS)])
    return bcs, [0.0] * (ndim - 1) + [-9.81]


class Handle:
    """A handle at the start of a time step: searched and masked, with M, V, A -- all made in the mode given."""

    def __init__(self, case, deterministic, step=0, bcs=None, search_deterministic=None):
        self.S = S = gpu_setup(case, nsteps=NSTEPS)
        self.bcs, self.gravity = problem(case)
        if bcs is not None:
            self.bcs = bcs
        S.set_deterministic(deterministic if search_deterministic is None else search_deterministic)
        S.local_search()
        self.n2m, self.d2m = S.active_masks(self.bcs, step)
        S.set_deterministic(deterministic)
        self.M = S.compute_nodal_lumped_mass()
        self.V, self.A = S.get_nodal_field_n(self.M)
        self.n = S.nactive * S.ndim
        self.alpha = _alpha(DT)

    def residual(self, dU, other=None, **kw):
        """at dU with this handle's M, V, A (or another handle's: then only the residual's own sums differ)"""
        o = other or self
        return self.S.lagrangian_evaluation(np.ascontiguousarray(dU), o.V, o.A, o.M, self.alpha, self.gravity, **kw)

    def state(self):
        st = self.S.download_state()
        return {k: st[k] for k in STATE}

    def close(self):
        self.S.close()


def increment(n, seed=7, size=1.0e-3):
    return size * np.random.default_rng(seed).normal(size=n)


def same(a, b, what):
    assert np.array_equal(a, b), f"{what}: not bit-identical, largest difference {np.abs(np.asarray(a) - np.asarray(b)).max():.3e}"


@pytest.mark.parametrize("ndim,law", [(3, "nh"), (2, "nh"), (3, "dp"), (3, "mixed"), (3, "fluid")])
def test_residual_repeats_bit_for_bit(ndim, law):
    case = cloud(ndim, law)
    a, b = Handle(case, True), Handle(case, True)
    same(a.M, b.M, "M of two handles")
    dU = increment(a.n)
    for flags, what in ((0, "fused"), (a.S.LAGR_SEPARATE, "separate stages")):
        R = [a.residual(dU, flags=flags) for _ in range(20)] + [b.residual(dU, flags=flags)]
        assert np.abs(R[0]).max() > 0.0 and np.isfinite(R[0]).all()
        worst = max(np.abs(r - R[0]).max() for r in R[1:]) / np.abs(R[0]).max()
        print(f"{ndim}-D {law} {what}: largest relative difference over 21 residuals {worst:.3e}")
        for q, r in enumerate(R[1:]):
            same(r, R[0], f"{ndim}-D {law} {what}: residual {q + 1}" + (" (second handle)" if q == 19 else ""))
        sa, sb = a.state(), b.state()
        for k in STATE:
            same(sa[k], sb[k], f"{ndim}-D {law} {what}: state {k} of the two handles")
        if flags == 0:
            fused = R[0]
    c = Handle(case, False)
    Rc = c.residual(dU, other=a)
    assert_close(Rc, fused, ATOMIC_BOUND, f"{ndim}-D {law}: atomic vs deterministic residual")
    for h in (a, b, c):
        h.close()


@pytest.mark.parametrize("ndim", [3, 2])
def test_lumped_mass_and_nodal_field_repeat(ndim):
    case = cloud(ndim, "nh")
    a, b = Handle(case, True), Handle(case, True)
    for k in ("M", "V", "A"):
        same(getattr(a, k), getattr(b, k), f"{ndim}-D {k} of two handles")
    same(a.S.compute_nodal_lumped_mass(), a.M, f"{ndim}-D M again on one handle")
    assert np.abs(a.V).max() > 0.0
    # the oracle: one thread, particles in the caller's order
    o = orc()
    M, P, prm, mats = oracle_setup(case)
    assert o.local_search(P, M, prm) == 0
    n2m, na = o.active_nodes(M)
    assert np.array_equal(n2m, a.n2m)
    m_o = o.lumped_mass(P, M, n2m, na)
    ulp = np.abs(a.M - m_o) / np.maximum(np.spacing(np.abs(m_o)), 1e-300)
    print(f"{ndim}-D lumped mass: {ulp.max():.0f} ulp from the oracle's summation order")
    assert ulp.max() <= 64, f"lumped mass: {ulp.max():.0f} ulp from the oracle's summation order"
    a.close()
    b.close()


@pytest.mark.parametrize("ndim,law", [(3, "nh"), (2, "nh"), (3, "dp")])
def test_product_and_blocks_repeat(ndim, law):
    case = cloud(ndim, law)
    a, b, c = Handle(case, True), Handle(case, True), Handle(case, False)
    dU = increment(a.n)
    x = np.random.default_rng(11).normal(size=a.n)
    ys, bs = [], []
    for h in (a, b, c):
        h.residual(dU, other=a)
        h.S.tangent_operator(a.alpha[0], a.M, True)
        ys.append([h.S.tangent_apply(x) for _ in range(10 if h is a else 1)])
        bs.append([h.S.tangent_block_diagonal() for _ in range(3 if h is a else 1)])
    assert np.abs(ys[0][0]).max() > 0.0 and np.isfinite(ys[0][0]).all() and np.isfinite(bs[0][0]).all()
    for q, y in enumerate(ys[0][1:] + ys[1]):
        same(y, ys[0][0], f"{ndim}-D {law}: K x, repeat {q + 1}")
    for q, blk in enumerate(bs[0][1:] + bs[1]):
        same(blk, bs[0][0], f"{ndim}-D {law}: diagonal blocks, repeat {q + 1}")
    assert_close(ys[2][0], ys[0][0], ATOMIC_BOUND, f"{ndim}-D {law}: atomic vs deterministic K x")
    assert_close(bs[2][0], bs[0][0], ATOMIC_BOUND, f"{ndim}-D {law}: atomic vs deterministic diagonal blocks")
    for h in (a, b, c):
        h.close()


def test_traction_loads_repeat():
    """The 2-D contours of tests/test_gpu_parity.py::test_nodal_traction_forces inside the residual."""
    n = nlps()
    case = make_case(2, [12, 11], [3, 3], [5, 4], material=NH, velocity=[1.0, -2.0])
    step = 1
    bcs = n.BccSet([dirichlet_plane(case, 1, 3, NSTEPS)])
    rng = np.random.default_rng(4)
    npart = case["cloud"]["x"].shape[0]
    pick = rng.choice(npart, size=24, replace=False).astype(np.int32)
    d1, d2 = np.ones((2, NSTEPS), dtype=np.int32), np.ones((2, NSTEPS), dtype=np.int32)
    d2[0, step] = 0
    loads = n.BccSet([{"nodes": pick[:14], "dim": 2, "dir": d1, "value": rng.normal(size=(2, NSTEPS)) * 1e7},
                      {"nodes": pick[14:], "dim": 2, "dir": d2, "value": rng.normal(size=(2, NSTEPS)) * 1e7}])
    a, c = Handle(case, True, step=step, bcs=bcs), Handle(case, False, step=step, bcs=bcs)
    dU = increment(a.n)
    kw = dict(loads=loads, step=step, thickness=0.5)
    R = [a.residual(dU, **kw) for _ in range(10)]
    assert np.abs(R[0] - a.residual(dU)).max() > 0.1 * np.abs(R[0]).max(), "the tractions must matter"
    for q, r in enumerate(R[1:]):
        same(r, R[0], f"residual with traction loads, evaluation {q + 1}")
    assert_close(c.residual(dU, other=a, **kw), R[0], ATOMIC_BOUND, "atomic vs deterministic residual with traction loads")
    a.close()
    c.close()


@pytest.mark.parametrize("ndim,law", [(3, "nh"), (2, "nh"), (3, "dp")])
def test_newton_and_newmark_replay(ndim, law):
    case = cloud(ndim, law)
    bcs, gravity = problem(case)
    kw = dict(max_it=50, atol=1e-8, rtol=1e-10, stol=1e-8, linesearch="bt", ksp=DRIVER)
    runs = []
    for deterministic in (True, True, False):
        S = gpu_setup(case, nsteps=NSTEPS)
        S.set_deterministic(deterministic)
        steps = []
        for step in range(NSTEPS):
            dU_out = np.zeros(S.nnodes * ndim)
            info = S.newmark_step(bcs, step, DT, gravity, dU_out=dU_out, **kw)
            steps.append((dU_out, info))
        runs.append((steps, S.download_state()))
        S.close()
    (sa, sta), (sb, stb), (sc, _) = runs
    for step in range(NSTEPS):
        (da, ia), (db, ib), (dc, ic) = sa[step], sb[step], sc[step]
        what = f"{ndim}-D {law} step {step}"
        print(what, ia["reason_name"], ia["fnorm_history"], ia["lambda_history"], ia["ksp_iterations"])
        assert ia["reason"] > 0, f"{what}: the solve must converge for the particles to advance: {ia}"
        same(da, db, f"{what}: dU_out")
        for k in ("fnorm_history", "lambda_history", "ksp_iterations"):
            same(ia[k], ib[k], f"{what}: {k}")
        assert ia["reason"] == ib["reason"] and ia["iterations"] == ib["iterations"]
        assert ic["reason"] == ia["reason"], f"{what}: reason {ic['reason']} with atomics, {ia['reason']} deterministic"
        assert_close(dc, da, 1e-8, f"{what}: dU, atomic vs deterministic", scale=np.abs(da).max())
    for k, v in sta.items():
        if isinstance(v, np.ndarray):
            same(v, stb[k], f"{ndim}-D {law}: state {k} after {NSTEPS} steps")


def test_dense_cloud_beyond_the_layer_table():
    """40 particles per closest node: the layer table of the per-tile ordering overflows, the lists are by slot index."""
    case = dense_case(5)
    a, b = Handle(case, True), Handle(case, True)
    dU = increment(a.n)
    x = np.random.default_rng(11).normal(size=a.n)
    out = []
    for h in (a, a, b):
        R = h.residual(dU, other=a)
        h.S.tangent_operator(a.alpha[0], a.M, True)
        out.append((R, h.S.tangent_apply(x)))
    for q in (1, 2):
        same(out[q][0], out[0][0], f"dense cloud: residual, repeat {q}")
        same(out[q][1], out[0][1], f"dense cloud: K x, repeat {q}")
    a.close()
    b.close()


def test_mode_switched_after_the_search():
    """Lists built with the mode off are not exact: a deterministic call over them sorts them first, so the result is the
    one of a handle that searched with the mode on.  Switching back off works as before."""
    case = cloud(3, "nh")
    ref = Handle(case, True)
    late = Handle(case, True, search_deterministic=False)
    dU = increment(ref.n)
    for k in ("M", "V", "A"):
        same(getattr(late, k), getattr(ref, k), f"{k}: mode switched on after the search")
    R = ref.residual(dU)
    same(late.residual(dU), R, "residual: mode switched on after the search")
    late.S.set_deterministic(False)
    assert_close(late.residual(dU), R, ATOMIC_BOUND, "residual after switching the mode off again")
    ref.close()
    late.close()
