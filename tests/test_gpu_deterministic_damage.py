"""nlps_gpu_set_deterministic_damage: with nlps_gpu_set_deterministic on, a cloud created with
driver_eigenerosion or driver_eigensoftening returns the SAME BITS on two runs from the same inputs -- the explicit step
with the damage hooks, the level-B scatters, the residual in its three forms, the matrix-free product and its diagonal
blocks, the Newmark step --, stays on the oracle at the bounds the atomic path is held to, and agrees with the atomic path
to the bound below.  The node runs the hooks sum over are read back and checked to be ascending in the memory slot.

Scenarios: those of explicit_damage_ref.py and implicit_damage_ref.py (thresholds and margins checked on the CPU by
test_explicit_damage_ref.py and test_implicit_damage_ref.py) and the residual cases of test_gpu_implicit_damage.py.

ATOMIC_BOUND, "agrees with the atomic path": the project's atomic-versus-deterministic bound, 1e-11 of the largest
magnitude of the compared array, unless ten times the spread between two ATOMIC evaluations of the same quantity on
these clouds is larger.  That spread, measured on the MI355X with the library as it was before this switch existed, mode
off, two handles, 20 evaluations of each quantity, relative to the largest magnitude:
lumped mass 4.4e-16 (2-D erosion and softening clouds) and 5.7e-16 (3-D); residual 1.8e-20 / 4.5e-17 / 4.3e-20 in the fused
damage form, 1.0e-20 / 1.7e-19 / 4.0e-20 with NLPS_LAGR_SEPARATE, 1.9e-20 / 1.7e-19 / 3.1e-20 with the switch off (2-D erosion /
3-D erosion / 2-D softening; the largest entries are inertial terms of 1e5 to 1e6, the atomic sums sit in much smaller ones);
K x 0 / 2.9e-21 / 8.8e-19; diagonal blocks 7.6e-21 / 4.1e-21 / 8.7e-21; nodal field: the clouds of these cases are at rest,
V = A = 0 on every handle; on the moving erosion clouds of test_nodal_field_of_a_moving_damage_cloud (2-D / 3-D) lumped
mass 4.4e-16 / 4.6e-16, nodal velocity 3.6e-16 / 4.8e-16, nodal acceleration 2.3e-16 / 2.0e-16.  Ten times each stays below 1e-11, which therefore is the bound for every quantity; no bound comes from the deterministic
results.  Damage fields are compared with array_equal."""
import numpy as np
import pytest

import explicit_damage_ref as xr
import implicit_damage_ref as ir
from test_gpu_deterministic import dense_case
from test_gpu_eigenerosion import stretch_field
from test_gpu_explicit_damage import NODAL, compare, damage_solver
from test_gpu_implicit_damage import CASES, alpha_of, block, energy_release_rates, solver
from test_gpu_newton_solve import TIGHT
from test_gpu_parity import masks
from util import assert_close, gpu_setup, nlps, oracle_setup, orc, relerr

pytestmark = pytest.mark.gpu

ATOMIC_BOUND = 1e-11
N1_FIELDS = ("DF", "F_n1", "J_n1", "Stress", "Damage_n1", "Strain_f_n1")


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a, b), \
        f"{what}: not bit-identical, largest difference {np.abs(a.astype(np.float64) - b.astype(np.float64)).max():.3e}"


def same_state(A, B, what):
    sa, sb = A.download_state(), B.download_state()
    for k, v in sa.items():
        if isinstance(v, np.ndarray):
            same(v, sb[k], f"{what}: {k}")
    return sa


def deterministic(S):
    S.set_deterministic(True)
    S.set_deterministic_damage(True)
    return S


# ------------------------------------------------------------------------------------------------ the explicit step
def replay_erosion(ndim, laws, prepare=None):
    n = nlps()
    ref = xr.erosion_reference(ndim, laws)
    case = xr.erosion_case(ndim, laws, Gf=xr.erosion_Gf(ndim, laws))
    A, B = deterministic(damage_solver(case)), deterministic(damage_solver(case))
    none = n.BccSet([])
    for S in (A, B):
        if prepare:
            prepare(S)
    for t, snap in enumerate(ref):
        for S in (A, B):
            S.explicit_step(none, t, xr.DT[t], xr.GAMMA)
        na, nb = A.explicit_nodal(), B.explicit_nodal()
        for k in NODAL:
            same(na[k], nb[k], f"step {t}: nodal {k} of the two handles")
        st = same_state(A, B, f"step {t}: state of the two handles")
        failed = int(st["Damage_n1"].sum())
        print(f"{ndim}-D {laws} step {t}: {failed} of {A.np} failed, bit-identical on two handles")
        for S in (A, B):
            compare(S, snap, f"step {t}")  # damage exact, fields and nodal arrays 1e-9
    assert 0 < failed < A.np
    A.close()
    B.close()


@pytest.mark.parametrize("ndim,laws", [(2, 0), (3, 0), (3, (0, 1))])
def test_explicit_eigenerosion_replays(ndim, laws):
    replay_erosion(ndim, laws)


def test_explicit_eigenerosion_replays_with_resorts():
    """the snapshot tables under a permutation of the slots: they are rebuilt, and sorted again, after every re-sort"""
    def prepare(S):
        S.resort()
        S.set_resort_interval(2)
    replay_erosion(3, 0, prepare)


@pytest.mark.parametrize("ndim,law", [(2, 0), (3, 0)])
def test_explicit_eigensoftening_replays(ndim, law):
    n = nlps()
    ref = xr.softening_reference(ndim, law)
    case = xr.softening_case(ndim, law, ft=xr.softening_ft(ndim, law))
    A, B = (deterministic(damage_solver(case, "softening", nsteps=3)) for _ in range(2))
    none = n.BccSet([])
    for t, snap in enumerate(ref):
        for S in (A, B):
            S.explicit_step(none, t, xr.DT[t], xr.GAMMA)
        na, nb = A.explicit_nodal(), B.explicit_nodal()
        for k in NODAL:
            same(na[k], nb[k], f"step {t}: nodal {k} of the two handles")
        d = same_state(A, B, f"step {t}: state of the two handles")
        assert np.array_equal(d["Strain_f_n1"] > 0, snap["strain_f"] > 0), f"step {t}: which particles start to fracture"
        assert_close(d["Strain_f_n1"], snap["strain_f"], 1e-9, f"step {t}: fracture strain")
        assert_close(d["Strain_f_n"], snap["strain_f"], 1e-9, f"step {t}: rolled fracture strain")
        assert_close(d["Damage_n1"], snap["damage"], 1e-9, f"step {t}: damage")
        assert_close(d["Damage_n"], snap["damage"], 1e-9, f"step {t}: rolled damage")
        assert_close(d["Stress"], snap["stress"], 1e-9, f"step {t}: scaled Kirchhoff stress")
        for k, ok in (("x_GC", "x"), ("vel", "vel"), ("F_n", "F_n")):
            assert_close(d[k], snap[ok], 1e-9, f"step {t} {k}")
    A.close()
    B.close()


# ------------------------------------------------------------------------------------------------ the node runs
def check_runs(S, snapshot, what):
    key, first, last, srt = S.debug_damage_runs(snapshot)
    listed = key >= 0
    count = np.bincount(key[listed], minlength=first.size)
    assert np.array_equal(last - first, count), f"{what}: last - first is the count of the key"
    nodes = np.nonzero(count)[0]
    assert nodes.size > 0 and first.min() >= 0 and last.max() <= key.size
    by_start = nodes[np.argsort(first[nodes])]
    assert (last[by_start][:-1] <= first[by_start][1:]).all(), f"{what}: runs overlap"
    seen = np.zeros(key.size, dtype=np.int64)
    for A in nodes:
        run = srt[first[A]:last[A]]
        assert (np.diff(run) > 0).all(), f"{what}: the run of node {A} is not strictly ascending: {run}"
        assert run.min() >= 0 and run.max() < key.size and (key[run] == A).all(), f"{what}: the run of node {A} holds a foreign slot"
        seen[run] += 1
    assert np.array_equal(seen, listed.astype(np.int64)), f"{what}: every listed slot exactly once"
    print(f"{what}: {nodes.size} runs, longest {count.max()}, {int(listed.sum())} slots")
    return int(count.max())


def test_node_runs_are_exact():
    n = nlps()
    none = n.BccSet([])
    case = xr.erosion_case(3, 0, Gf=xr.erosion_Gf(3, 0))
    S = deterministic(damage_solver(case))
    with pytest.raises(n.NlpsError, match="no such run table"):
        S.debug_damage_runs(False)
    S.resort()  # (slots are no longer the caller's order)
    S.explicit_step(none, 0, xr.DT[0], xr.GAMMA)
    check_runs(S, False, "3-D erosion cloud, current closest nodes")
    check_runs(S, True, "3-D erosion cloud, snapshot")
    S.close()


def test_node_runs_of_the_dense_cloud():
    """40 particles per closest node, beyond the layer table of the per-tile ordering: long runs.  The threshold is the
    median energy release rate scale of a first step nobody fails in (Ceps h W), so that the decisions matter."""
    n = nlps()
    none = n.BccSet([])
    case = dense_case(5)
    case["cloud"]["vel"] = xr.velocity_field(case["cloud"]["x"])
    case["materials"] = [dict(case["materials"][0], Ceps=xr.CEPS, Gf=1e300)]
    probe = damage_solver(case)
    probe.explicit_step(none, 0, xr.DT[0], xr.GAMMA)
    W = probe.download_state()["W"]
    probe.close()
    assert (W > 0).all()
    case["materials"][0]["Gf"] = float(xr.CEPS * case["h"] * np.median(W))
    A, B = deterministic(damage_solver(case)), deterministic(damage_solver(case))
    for S in (A, B):
        S.explicit_step(none, 0, xr.DT[0], xr.GAMMA)
    assert check_runs(A, False, "dense cloud, current closest nodes") >= 40
    assert check_runs(A, True, "dense cloud, snapshot") >= 40
    na, nb = A.explicit_nodal(), B.explicit_nodal()
    for k in NODAL:
        same(na[k], nb[k], f"dense cloud: nodal {k} of the two handles")
    st = same_state(A, B, "dense cloud: state of the two handles")
    failed = int(st["Damage_n1"].sum())
    print(f"dense cloud: {failed} of {A.np} failed")
    assert 0 < failed < A.np
    A.close()
    B.close()


# ------------------------------------------------------------------------------------------------ the implicit path
class Handle:
    """A damage handle at the start of a step: searched and masked, with M, V, A -- all made in the mode given."""

    def __init__(self, case, driver, M_oracle, det, fused=True, det_at_search=None):
        self.S = S = solver(case, driver, fused, 2)
        early = det if det_at_search is None else det_at_search
        if early:
            deterministic(S)
        S.local_search()
        self.n2m, self.d2m, self.na = masks(S, M_oracle, [], 0, 2)
        if det:
            deterministic(S)
        self.det = det
        self.M = S.compute_nodal_lumped_mass()
        self.V, self.A = S.get_nodal_field_n(self.M)
        self.alpha = alpha_of(1.0e-3)[1]

    def switch_on(self):
        deterministic(self.S)

    def residual(self, dU, other=None, flags=0):
        o = other or self
        return self.S.lagrangian_evaluation(np.ascontiguousarray(dU), o.V, o.A, o.M, self.alpha, None, flags=flags)

    def state(self):
        st = self.S.download_state()
        return {k: st[k] for k in N1_FIELDS}

    def close(self):
        self.S.close()


def erosion_problem(name):
    """the case of test_gpu_implicit_damage.py::test_eigenerosion_residual: Gf between two candidates of the first evaluation"""
    o = orc()
    ndim, mats_in, stretch = CASES[name]
    case = block(ndim, [dict(m) for m in mats_in])
    M, P, prm, mats = oracle_setup(case)
    n2m, na = o.active_nodes(M)
    dU = stretch_field(M, n2m, na, ndim, stretch, np.random.default_rng(21))
    cand, G = energy_release_rates(o, P, M, mats, prm, n2m, dU, case["h"])
    gs = np.sort(G)
    Gf = float(0.5 * (gs[gs.size // 2 - 1] + gs[gs.size // 2]))
    assert np.count_nonzero(np.abs(G - Gf) < 1e-9 * Gf) == 0, "no particle may sit on the threshold"
    for m in case["materials"]:
        m["Gf"] = Gf
    return case, "erosion", dU


def softening_problem(ndim):
    """the case of test_gpu_implicit_damage.py::test_eigensoftening_residual"""
    o = orc()
    case = xr.softening_case(ndim, 0, ft=0.0)
    case["cloud"]["vel"] = np.zeros_like(case["cloud"]["x"])
    damage0 = case["cloud"]["damage_n"].copy()
    M, P, prm, mats = oracle_setup(case)
    n2m, na = o.active_nodes(M)
    dU = stretch_field(M, n2m, na, ndim, 0.02, np.random.default_rng(33))
    assert o.compatibility(dU, None, P, M, n2m) == 0 and o.constitutive_eroded(P, mats, prm, damage0) == 0
    T0 = xr.min_principal(P["stress"], ndim)
    cand = (damage0 == 0.0) & (T0 > 0.0)
    case["materials"][0]["ft"] = float(np.median(T0[cand]))
    return case, "softening", dU


PROBLEMS = {"2-D eigenerosion": lambda: erosion_problem("2-D Neo-Hookean"),
            "3-D eigenerosion": lambda: erosion_problem("3-D Neo-Hookean"),
            "2-D eigensoftening": lambda: softening_problem(2)}


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_implicit_residual_replays(name):
    case, driver, dU = PROBLEMS[name]()
    M_o = oracle_setup(case)[0]
    a, b, c = Handle(case, driver, M_o, True), Handle(case, driver, M_o, True), Handle(case, driver, M_o, False)
    for k in ("M", "V", "A"):
        same(getattr(a, k), getattr(b, k), f"{name}: {k} of two handles")
        assert_close(getattr(c, k), getattr(a, k), ATOMIC_BOUND, f"{name}: atomic vs deterministic {k}")
    SEP = a.S.LAGR_SEPARATE
    fused = None
    for what, on, flags in (("fused damage form", True, 0), ("NLPS_LAGR_SEPARATE", True, SEP), ("separate stages, switch off", False, 0)):
        for h in (a, b):
            h.S.set_implicit_damage(on)
        R = [a.residual(dU, flags=flags) for _ in range(20)] + [b.residual(dU, flags=flags)]
        assert np.abs(R[0]).max() > 0.0 and np.isfinite(R[0]).all()
        for q, r in enumerate(R[1:]):
            same(r, R[0], f"{name}, {what}: residual {q + 1}" + (" (second handle)" if q == 19 else ""))
        sa, sb = a.state(), b.state()
        for k in N1_FIELDS:
            same(sa[k], sb[k], f"{name}, {what}: state {k} of the two handles")
        if fused is None:
            fused, fused_state = R[0], sa
        else:
            same(sa["Damage_n1"], fused_state["Damage_n1"], f"{name}, {what}: damage field vs the fused form")
            assert_close(R[0], fused, 1e-10, f"{name}, {what}: residual vs the fused form")
    evals = a.S.debug_damage_counters()
    assert evals == (1, 20), f"{name}: one build of the node runs, 20 fused evaluations: {evals}"
    # the operator after a fused evaluation
    x = np.random.default_rng(11).normal(size=a.na * a.S.ndim)
    ys, blocks = [], []
    for h in (a, b, c):
        h.S.set_implicit_damage(True)
        Rh = h.residual(dU, other=a)
        h.S.tangent_operator(a.alpha[0], a.M, True)
        ys.append([h.S.tangent_apply(x) for _ in range(10 if h is a else 1)])
        blocks.append(h.S.tangent_block_diagonal())
    for q, y in enumerate(ys[0][1:] + ys[1]):
        same(y, ys[0][0], f"{name}: K x, repeat {q + 1}")
    same(blocks[1], blocks[0], f"{name}: diagonal blocks of the two handles")
    # the atomic handle
    sc = c.state()
    failed = int(sc["Damage_n1"].sum()) if driver == "erosion" else int((sc["Strain_f_n1"] > 0).sum())
    print(f"{name}: {failed} of {a.S.np} failed or fracturing; atomic vs deterministic: R {relerr(Rh, fused):.3e}, "
          f"K x {relerr(ys[2][0], ys[0][0]):.3e}, blocks {relerr(blocks[2], blocks[0]):.3e} (bound {ATOMIC_BOUND:.0e})")
    assert 0 < failed < a.S.np
    same(sc["Damage_n1"], fused_state["Damage_n1"], f"{name}: damage field, atomic vs deterministic")
    assert np.array_equal(sc["Strain_f_n1"] > 0, fused_state["Strain_f_n1"] > 0), f"{name}: which particles fracture, atomic vs deterministic"
    assert_close(Rh, fused, ATOMIC_BOUND, f"{name}: atomic vs deterministic residual")
    assert_close(ys[2][0], ys[0][0], ATOMIC_BOUND, f"{name}: atomic vs deterministic K x")
    assert_close(blocks[2], blocks[0], ATOMIC_BOUND, f"{name}: atomic vs deterministic diagonal blocks")
    for h in (a, b, c):
        h.close()


def moving_case(ndim):
    """the erosion cloud of explicit_damage_ref.py with its velocity field and an acceleration field on top"""
    case = xr.erosion_case(ndim, 0, Gf=xr.erosion_Gf(ndim, 0))
    case["cloud"]["acc"] = np.random.default_rng(5).normal(size=case["cloud"]["x"].shape)
    return case


@pytest.mark.parametrize("ndim", [2, 3])
def test_nodal_field_of_a_moving_damage_cloud(ndim):
    """The residual cases above are at rest (V = A = 0): the lumped mass and the nodal field of a damage cloud that moves."""
    case = moving_case(ndim)
    M_o = oracle_setup(case)[0]
    a, b, c = (Handle(case, "erosion", M_o, det) for det in (True, True, False))
    assert np.abs(a.V).max() > 0.0 and np.abs(a.A).max() > 0.0
    for k in ("M", "V", "A"):
        same(getattr(a, k), getattr(b, k), f"{ndim}-D moving cloud: {k} of two handles")
        print(f"{ndim}-D moving cloud: atomic vs deterministic {k} {relerr(getattr(c, k), getattr(a, k)):.3e} (bound {ATOMIC_BOUND:.0e})")
        assert_close(getattr(c, k), getattr(a, k), ATOMIC_BOUND, f"{ndim}-D moving cloud: atomic vs deterministic {k}")
    V2, A2 = a.S.get_nodal_field_n(a.M)
    same(V2, a.V, f"{ndim}-D moving cloud: V again on one handle")
    same(A2, a.A, f"{ndim}-D moving cloud: A again on one handle")
    for h in (a, b, c):
        h.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_newmark_replays(ndim):
    n = nlps()
    none = n.BccSet([])
    ref = ir.erosion_reference(ndim, 0)[:3]
    case = xr.erosion_case(ndim, 0, Gf=ir.erosion_Gf(ndim, 0))
    A, B = deterministic(solver(case, "erosion", True)), deterministic(solver(case, "erosion", True))
    for t, snap in enumerate(ref):
        ia, ib = (S.newmark_step(none, t, ir.DT[t], None, beta=ir.BETA, gamma=ir.GAMMA, ksp=TIGHT, **ir.SNES) for S in (A, B))
        what = f"{ndim}-D step {t}"
        print(what, ia["fnorm_history"], ia["lambda_history"], ia["ksp_iterations"])
        assert ia["reason"] > 0 and ia["nactive"] == snap["na"], ia
        for k in ("reason", "iterations", "linear_iterations"):
            assert ia[k] == ib[k], f"{what}: {k} {ia[k]} vs {ib[k]}"
        for k in ("fnorm_history", "lambda_history", "ksp_iterations"):
            same(ia[k], ib[k], f"{what}: {k}")
        st = same_state(A, B, f"{what}: state of the two handles")
        assert np.array_equal(st["Damage_n1"], snap["damage"]), f"{what}: Damage_n1"
        assert np.array_equal(st["Damage_n"], snap["damage"]), f"{what}: Damage_n after the roll"
        for k, ok in (("x_GC", "x"), ("vel", "vel"), ("acc", "acc"), ("F_n", "F_n"), ("J_n", "J_n"), ("Stress", "stress")):
            assert_close(st[k], snap[ok], 1e-8, f"{what}: {k}")
    assert 0 < st["Damage_n1"].sum() < A.np
    A.close()
    B.close()


def test_mode_switched_late():
    """Node runs built in arrival order (a fused damage residual with the switches off) are dropped when the switches go
    on: the next evaluation is the one of a handle that never saw the atomic path."""
    case, driver, dU = erosion_problem("3-D Neo-Hookean")
    M_o = oracle_setup(case)[0]
    ref = Handle(case, driver, M_o, True)
    late = Handle(case, driver, M_o, False)
    R_atomic = late.residual(dU, other=ref)
    assert late.S.debug_damage_counters() == (1, 1)
    late.switch_on()
    R = ref.residual(dU)
    same(late.residual(dU, other=ref), R, "residual: switches on after an atomic evaluation")
    assert late.S.debug_damage_counters() == (2, 2), "the cached runs have to be rebuilt"
    sa, sb = ref.state(), late.state()
    for k in N1_FIELDS:
        same(sb[k], sa[k], f"state {k}: switches on after an atomic evaluation")
    assert_close(R_atomic, R, ATOMIC_BOUND, "atomic vs deterministic residual")
    ref.close()
    late.close()


def test_contract():
    n = nlps()
    none = n.BccSet([])
    case = xr.erosion_case(3, 0, Gf=1e300)
    P = gpu_setup(case)
    with pytest.raises(n.NlpsError, match="without driver_eigenerosion"):
        P.set_deterministic_damage(True)
    P.close()
    S = damage_solver(case)
    S.set_deterministic(True)  # the switch off: the explicit step refuses with the message it always had
    with pytest.raises(n.NlpsError, match="not built for the deterministic mode .their node runs take ranks and run starts from atomics"):
        S.explicit_step(none, 0, 1e-4)
    S.local_search()
    S.set_deterministic_damage(True)
    S.set_deterministic_damage(False)
    with pytest.raises(n.NlpsError, match="not built for the deterministic mode"):
        S.explicit_step(none, 0, 1e-4)
    S.local_search()
    S.set_deterministic_damage(True)
    S.set_halo_exchange(lambda dptr, nfield, elem, kind: 0)  # the refusals of a multi-rank handle are unchanged
    with pytest.raises(n.NlpsError, match="ghost particles"):
        S.explicit_step(none, 0, 1e-4)
    with pytest.raises(n.NlpsError, match="ghost particles"):
        S.set_implicit_damage(True)
    S.set_halo_exchange(None)
    S.set_implicit_damage(True)
    S.local_search()
    S.active_masks(none, 0)
    M = S.compute_nodal_lumped_mass()
    V, A = S.get_nodal_field_n(M)
    S.set_halo_exchange(lambda dptr, nfield, elem, kind: 0)
    with pytest.raises(n.NlpsError, match="ghost particles"):
        S.lagrangian_evaluation(np.zeros_like(M), V, A, M, alpha_of(1e-3)[1])
    S.set_halo_exchange(None)
    S.explicit_step(none, 0, 1e-4)  # and with everything back in place it steps
    assert S.status_flags() == 0
    S.close()
