"""The eigenerosion and eigensoftening hooks inside the fused residual, the Newton solve and the one-call Newmark step
(nlps_gpu_set_implicit_damage): against the composition of the oracle's stage calls, against a twin handle
that runs the separate stages (the switch off), and against implicit_damage_ref.py, whose scenarios and margins
test_implicit_damage_ref.py checks on the CPU.  Every case switches the fused form on."""
import numpy as np
import pytest

import explicit_damage_ref as xr
import implicit_damage_ref as ir
import snes_ref
from newmark import newmark_parameters
from test_gpu_eigenerosion import stretch_field
from test_gpu_newton_solve import TIGHT, _same_counts, _Step
from test_gpu_parity import masks
from util import DP, gpu_setup, make_case, nlps, oracle_setup, orc, relerr

pytestmark = pytest.mark.gpu

N1_STATE = (("Stress", "stress"), ("W", "W"), ("DF", "DF"), ("F_n1", "F_n1"), ("J_n1", "J_n1"), ("b_e_n1", "b_e_n1"),
            ("Kappa_n1", "kappa_n1"), ("EPS_n1", "eps_n1"), ("C_ep", "C_ep"))
N_STATE = ("x_GC", "dis", "vel", "acc", "F_n", "J_n", "b_e_n", "Kappa_n", "EPS_n", "Damage_n", "Strain_f_n")
TOL = 1e-10  # the level-B tolerance of test_gpu_eigenerosion.py
WORST = {}


def close(a, b, tol, what, key, scale=None):
    """assert_close that prints every figure and keeps the largest per bound (the figures DESIGN.md 5i records)"""
    e = relerr(a, b, scale)
    WORST[key] = max(WORST.get(key, 0.0), e)
    print(f"{what}: {e:.3e} (bound {tol:.0e}; largest so far under '{key}' {WORST[key]:.3e})")
    assert e <= tol, f"{what}: relative error {e:.3e} > {tol:.1e}"


def solver(case, driver, on, nsteps=4):
    n = nlps()
    params = n.default_params()
    if driver == "erosion":
        params.driver_eigenerosion = 1
    elif driver == "softening":
        params.driver_eigensoftening = 1
    S = gpu_setup(case, nsteps=nsteps, params=params)
    if on:
        S.set_implicit_damage(True)
    return S


def block(ndim, mats):
    """the clouds of explicit_damage_ref.erosion_case for any list of materials (dealt to the particles in turn)"""
    if ndim == 3:
        case = make_case(3, [11, 10, 9], [3, 3, 2], [5, 4, 4], material=mats[0])  # 640 particles, 3 x 3 x 3 tiles
    else:
        case = make_case(2, [22, 12], [6, 3], [12, 6], material=mats[0])  # 288 particles across the tile boundary at node 16
    case["materials"] = mats
    if len(mats) > 1:
        case["cloud"]["matidx"] = (np.arange(case["cloud"]["x"].shape[0]) % len(mats)).astype(np.int32)
    return case


def alpha_of(dt):
    a = newmark_parameters(ir.BETA, ir.GAMMA, dt)
    return a, [a["a1"], a["a2"], a["a3"], a["a4"], a["a5"], a["a6"]]


def energy_release_rates(o, P, M, mats, prm, n2m, dU, h):
    """G of every candidate of a first evaluation at dU (a pass of the oracle nobody fails in)"""
    beps = o.compute_beps(P, M, mats, initialize=True)
    assert o.compatibility(dU, None, P, M, n2m) == 0 and o.constitutive_eroded(P, mats, prm, np.zeros(P.np)) == 0
    T0 = xr.min_principal(P["stress"], P.ndim)
    V, W = P["vol0"] * P["J_n1"], P["W"]
    cand = np.where(T0 > 0.0)[0]
    G = np.zeros(cand.size)
    for i, p in enumerate(cand):
        q = beps[1][p, : beps[0][p]]
        G[i] = mats[P["matidx"][p]].Ceps * h / (V[p] + V[q].sum()) * (V[p] * W[p] + (V[q] * W[q]).sum())
    return cand, G


ELASTIC = {"E": 1.0e6, "nu": 0.25, "Ceps": 1.5, "Gf": 0.0}
CASES = {"2-D Neo-Hookean": (2, [dict(ELASTIC, type=0)], 0.02),
         "3-D Neo-Hookean": (3, [dict(ELASTIC, type=0)], 0.02),
         "3-D Hencky": (3, [dict(ELASTIC, type=1)], 0.02),
         "3-D Drucker-Prager, one material (UMAT)": (3, [dict(DP, Ceps=1.5, Gf=0.0)], 0.004),
         "3-D Neo-Hookean / Hencky interleaved (FILT)": (3, [dict(ELASTIC, type=0), dict(ELASTIC, type=1, E=0.8e6)], 0.02)}


def compare_evaluation(what, S, T, R_on, R_off, P, R_o, plastic, E):
    """the switch-on handle S against the oracle (P, R_o) and against the twin T (switch off)"""
    a, b = S.download_state(), T.download_state()
    close(R_on, R_o, TOL, f"{what}: R vs the oracle", "residual 1e-10")
    close(R_on, R_off, TOL, f"{what}: R vs the twin", "residual 1e-10")
    for k, ok in N1_STATE:
        scale = E if k == "C_ep" else None
        if plastic or k not in ("b_e_n1", "Kappa_n1", "EPS_n1", "C_ep"):
            close(a[k], P[ok], TOL, f"{what}: {k} vs the oracle", "residual 1e-10", scale)
        close(a[k], b[k], TOL, f"{what}: {k} vs the twin", "residual 1e-10", scale)
    return a, b


@pytest.mark.parametrize("name", list(CASES))
def test_eigenerosion_residual(name):
    o = orc()
    ndim, mats_in, stretch = CASES[name]
    rng = np.random.default_rng(21)
    case = block(ndim, [dict(m) for m in mats_in])
    M, P, prm, mats = oracle_setup(case)
    n2m, na = o.active_nodes(M)
    dU = stretch_field(M, n2m, na, ndim, stretch, rng)
    cand, G = energy_release_rates(o, P, M, mats, prm, n2m, dU, case["h"])
    assert cand.size > P.np // 4, f"{name}: {cand.size} candidates of {P.np}"
    gs = np.sort(G)
    Gf = float(0.5 * (gs[gs.size // 2 - 1] + gs[gs.size // 2]))  # between two candidates, never on one
    assert np.count_nonzero(np.abs(G - Gf) < 1e-9 * Gf) == 0, "no particle may sit on the threshold"
    for m in case["materials"]:
        m["Gf"] = Gf
    # ---- the oracle, the switch-on handle and its twin from scratch with that Gf
    M, P, prm, mats = oracle_setup(case)
    S, T = solver(case, "erosion", True, 2), solver(case, "erosion", False, 2)
    n2m, d2m, na = masks(S, M, [], 0, 2)
    masks(T, M, [], 0, 2)
    beps = o.compute_beps(P, M, mats, initialize=True)
    Mv = o.lumped_mass(P, M, n2m, na)
    V, A = o.nodal_field_n(Mv, P, M, n2m, d2m, na)
    a, alpha = alpha_of(1.0e-3)
    damage_n, damage_n1 = np.zeros(P.np), np.zeros(P.np)
    plastic = mats_in[0]["type"] == 2
    for rnd in range(2):  # second round: the failed particles are skipped by the constitutive update
        before = S.download_state()
        assert o.compatibility(dU, None, P, M, n2m) == 0
        assert o.constitutive_eroded(P, mats, prm, damage_n) == 0
        assert o.eigenerosion_hook(damage_n1, damage_n, P, mats, beps, case["h"]) == 0
        R_o, st = o.internal_forces(P, M, n2m, d2m, na)
        assert st == 0
        R_o += Mv * (a["a1"] * dU - a["a2"] * V - a["a3"] * A)
        R_on = S.lagrangian_evaluation(dU, V, A, Mv, alpha)
        R_off = T.lagrangian_evaluation(dU, V, A, Mv, alpha)
        what = f"{name}, round {rnd}"
        sa, sb = compare_evaluation(what, S, T, R_on, R_off, P, R_o, plastic, mats_in[0]["E"])
        assert np.array_equal(sa["Damage_n1"], damage_n1), f"{what}: damage field vs the oracle"
        assert np.array_equal(sa["Damage_n1"], sb["Damage_n1"]), f"{what}: damage field vs the twin"
        for k in N_STATE:
            assert np.array_equal(sa[k], before[k]), f"{what}: the n state ({k}) is touched"
        failed = int(damage_n1.sum())
        print(f"{what}: {failed} of {P.np} failed")
        assert 0 < failed < P.np
        assert rnd == 0 or int(damage_n.sum()) > 0, "the second round skips failed particles"
        o.roll_state(P)
        damage_n[:] = damage_n1
        S.update_particles_internal_variables()
        T.update_particles_internal_variables()
        assert np.array_equal(S.download_state(["Damage_n"])["Damage_n"], damage_n)
        dU = 0.5 * dU
    S.close()
    T.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_eigensoftening_residual(ndim):
    """the pre-damaged, partly moved cloud of test_gpu_eigensoftening.py"""
    o = orc()
    rng = np.random.default_rng(33)
    case = xr.softening_case(ndim, 0, ft=0.0)
    case["cloud"]["vel"] = np.zeros_like(case["cloud"]["x"])
    damage0, strain_f0 = case["cloud"]["damage_n"].copy(), case["cloud"]["strain_f_n"].copy()
    M, P, prm, mats = oracle_setup(case)
    n2m, na = o.active_nodes(M)
    dU = stretch_field(M, n2m, na, ndim, 0.02, rng)
    assert o.compatibility(dU, None, P, M, n2m) == 0 and o.constitutive_eroded(P, mats, prm, damage0) == 0
    T0 = xr.min_principal(P["stress"], ndim)
    cand = (damage0 == 0.0) & (T0 > 0.0)
    assert cand.sum() > P.np // 4
    case["materials"][0]["ft"] = float(np.median(T0[cand]))
    # ---- from scratch with that ft
    M, P, prm, mats = oracle_setup(case)
    S, T = solver(case, "softening", True, 2), solver(case, "softening", False, 2)
    n2m, d2m, na = masks(S, M, [], 0, 2)
    masks(T, M, [], 0, 2)
    beps = (np.zeros(P.np, dtype=np.int32), np.full((P.np, o.BEPS_STRIDE), -1, dtype=np.int32))
    Mv = o.lumped_mass(P, M, n2m, na)
    V, A = o.nodal_field_n(Mv, P, M, n2m, d2m, na)
    a, alpha = alpha_of(1.0e-3)
    damage_n, damage_n1, strain_f = damage0.copy(), damage0.copy(), strain_f0.copy()
    threads = o.num_threads()
    o.set_num_threads(1)  # (the reference's sequential loop)
    try:
        for rnd in range(2):
            before = S.download_state()
            o.compute_beps(P, M, mats, beps=beps, initialize=False)  # U-Newmark-beta.c:213-215
            assert o.compatibility(dU, None, P, M, n2m) == 0
            assert o.constitutive_eroded(P, mats, prm, damage_n) == 0
            sf_before = strain_f.copy()
            assert o.eigensoftening_hook(damage_n1, damage_n, strain_f, P, mats, beps) == 0
            R_o, st = o.internal_forces(P, M, n2m, d2m, na)
            assert st == 0
            R_o += Mv * (a["a1"] * dU - a["a2"] * V - a["a3"] * A)
            R_on = S.lagrangian_evaluation(dU, V, A, Mv, alpha)
            R_off = T.lagrangian_evaluation(dU, V, A, Mv, alpha)
            what = f"eigensoftening {ndim}-D, round {rnd}"
            sa, sb = compare_evaluation(what, S, T, R_on, R_off, P, R_o, False, 1.0)
            assert np.array_equal(sa["Strain_f_n1"] > 0, strain_f > 0), f"{what}: which particles start to fracture"
            assert np.array_equal(sa["Strain_f_n1"] > 0, sb["Strain_f_n1"] > 0), f"{what}: which particles start, vs the twin"
            close(sa["Strain_f_n1"], strain_f, 1e-9, f"{what}: fracture strain vs the oracle", "softening 1e-9")
            close(sa["Damage_n1"], damage_n1, 1e-9, f"{what}: damage vs the oracle", "softening 1e-9")
            close(sa["Strain_f_n1"], sb["Strain_f_n1"], 1e-9, f"{what}: fracture strain vs the twin", "softening 1e-9")
            close(sa["Damage_n1"], sb["Damage_n1"], 1e-9, f"{what}: damage vs the twin", "softening 1e-9")
            for k in N_STATE:
                assert np.array_equal(sa[k], before[k]), f"{what}: the n state ({k}) is touched"
            started = np.count_nonzero((strain_f > 0) & (sf_before == 0))
            grew = np.count_nonzero(damage_n1 > damage_n)
            assert started > 0 and (rnd == 0 or grew > 0), (started, grew)
            o.roll_state(P)
            damage_n[:] = damage_n1
            S.update_particles_internal_variables()
            T.update_particles_internal_variables()
            dU = 1.5 * dU
    finally:
        o.set_num_threads(threads)
    S.close()
    T.close()


def _erosion_pair(ndim, dts, nsteps=4):
    case = xr.erosion_case(ndim, 0, Gf=ir.erosion_Gf(ndim, 0, tuple(dts)))
    return case, solver(case, "erosion", True, nsteps), solver(case, "erosion", False, nsteps)


def _operator_against_the_twin(S, T, alpha_1, Mv, rng, what):
    n = S.nactive * S.ndim
    S.tangent_operator(alpha_1, Mv, True)
    T.tangent_operator(alpha_1, Mv, True)
    x = rng.normal(size=n)
    close(S.tangent_apply(x), T.tangent_apply(x), 1e-9, f"{what}: K x", "operator 1e-9")
    close(S.tangent_block_diagonal(), T.tangent_block_diagonal(), 1e-9, f"{what}: block diagonal", "operator 1e-9")


class _Handle:
    """a handle at the start of a step: search, masks, M, Un_dt, Un_dt2 (no Dirichlet set, no gravity)"""

    def __init__(self, S, step, dt):
        self.S = S
        self.begin(step, dt)

    def begin(self, step, dt):
        S = self.S
        S.local_search()
        self.n2m, _ = S.active_masks(nlps().BccSet([]), step)
        self.M = S.compute_nodal_lumped_mass()
        self.V, self.A = S.get_nodal_field_n(self.M)
        self.alpha = alpha_of(dt)[1]

    def residual(self, x):
        return self.S.lagrangian_evaluation(np.ascontiguousarray(x), self.V, self.A, self.M, self.alpha)


def _node_field(case, n2m, na, f):
    """masked nodal vectors from a function of the node coordinates"""
    nn = case["grid_n"]
    idx = np.stack(np.meshgrid(*[np.arange(k) for k in nn], indexing="ij"), axis=-1)
    idx = idx.transpose(*reversed(range(len(nn))), len(nn)).reshape(-1, len(nn))  # node = i + nx (j + ny k)
    X = np.asarray(case["origin"]) + case["h"] * idx
    act = np.where(n2m >= 0)[0]
    out = np.zeros((na, len(nn)))
    out[n2m[act]] = f(X[act])
    return out.ravel()


@pytest.mark.parametrize("ndim", [2, 3])
def test_operator_and_node_runs(ndim):
    n = nlps()
    rng = np.random.default_rng(9)
    none = n.BccSet([])
    case, S, T = _erosion_pair(ndim, ir.DT)
    F = solver(case, "erosion", True)  # a handle whose runs are always freshly built
    hs = [_Handle(h, 0, ir.DT[0]) for h in (S, T, F)]
    dev = hs[0]
    dU = S.form_initial_guess(dev.V, dev.A, ir.DT[0], none, 0)

    def evaluate(x, what, rebuild):
        if rebuild:  # a search and the masks make the runs stale; nothing has moved, the numbering stays
            F.local_search()
            F.active_masks(none, 0)
        R = [h.residual(x) for h in hs]
        st = [h.S.download_state() for h in hs]
        for other, name in ((1, "the twin"), (2, "freshly built runs")):
            close(R[0], R[other], TOL, f"{what}: R vs {name}", "residual 1e-10")
            close(st[0]["Stress"], st[other]["Stress"], TOL, f"{what}: Stress vs {name}", "residual 1e-10")
            assert np.array_equal(st[0]["Damage_n1"], st[other]["Damage_n1"]), f"{what}: damage vs {name}"
        return int(st[0]["Damage_n1"].sum())

    f1 = evaluate(dU, f"{ndim}-D first evaluation", False)
    assert 0 < f1 < S.np
    assert S.debug_damage_counters() == (1, 1) and T.debug_damage_counters() == (0, 0)
    _operator_against_the_twin(S, T, dev.alpha[0], dev.M, rng, f"{ndim}-D after the fused damage residual")
    # (1.1 dU: 174 of 288 / 479 of 640 failed on the oracle, smallest G margin 1.5e-4 / 9.6e-5)
    f2 = evaluate(1.1 * dU, f"{ndim}-D second evaluation (runs reused)", True)
    assert f1 < f2 < S.np
    assert S.debug_damage_counters() == (1, 2), "the second evaluation reuses the node runs"
    assert F.debug_damage_counters() == (2, 2), "a search and the masks make the runs stale"
    _operator_against_the_twin(S, T, dev.alpha[0], dev.M, rng, f"{ndim}-D after the second evaluation")
    # move the upper-x half of the cloud by a third of a cell (the lower half keeps its frozen neighbourhoods), so that
    # closest nodes change: the runs are rebuilt after the next search and masks
    i0 = S.download_state()["I0"].copy()
    xmid = 0.5 * (case["cloud"]["x"][:, 0].min() + case["cloud"]["x"][:, 0].max())
    amp = 1.0 + 0.2 * rng.uniform()

    def shift(X):
        d = np.zeros_like(X)
        d[X[:, 0] > xmid, 0] = 0.34 * case["h"] * amp
        return d

    move = _node_field(case, dev.n2m, S.nactive, shift)
    zero = np.zeros_like(move)
    for h in hs:
        h.S.update_particles_internal_variables()
        h.S.update_particles_kinetics_FLIP_PIC(1.0, move, zero, zero, zero)
        h.begin(1, ir.DT[1])
    moved = np.count_nonzero(S.download_state()["I0"] != i0)
    print(f"{ndim}-D: {moved} of {S.np} particles changed their closest node")
    assert moved > 0
    centre = case["cloud"]["x"].mean(axis=0)
    dU2 = _node_field(case, dev.n2m, S.nactive, lambda X: 0.01 * (X - centre))
    f3 = evaluate(dU2, f"{ndim}-D after the move", False)
    assert f2 <= f3 <= S.np  # (Damage_n holds the f2 particles since the roll)
    assert S.debug_damage_counters() == (2, 3), "the runs are rebuilt once after the move"
    _operator_against_the_twin(S, T, dev.alpha[0], dev.M, rng, f"{ndim}-D after the move")
    for h in (S, T, F):
        h.close()


def test_newton_solve_two_iterates():
    """the 2-D step of dt = 5e-3 (two iterates, 76 of 288 fail): the device solve with the switch on against
    snes_ref.newton over the twin's switch-off residual and assembled tangent"""
    n = nlps()
    none = n.BccSet([])
    dt = ir.DT_TWO_ITERATES[0]
    case, S, T = _erosion_pair(2, ir.DT_TWO_ITERATES)
    a, alpha = alpha_of(dt)
    dev, ref = _Step(S, none, 0, alpha, None), _Step(T, none, 0, alpha, None)
    guess = S.form_initial_guess(dev.V, dev.A, dt, none, 0)
    dU, info = dev.solve(guess, ksp=TIGHT, **ir.SNES)
    xr_, ir_ = snes_ref.newton(ref.residual, ref.tangent, guess, linear="dense", **ir.SNES)
    print("device", info["fnorm_history"], info["lambda_history"], "reference", ir_["fnorm_history"], ir_["lambda_history"])
    assert info["reason"] == snes_ref.CONVERGED_FNORM_RELATIVE and info["iterations"] == 2, info
    _same_counts(info, ir_, "newton_solve on a damage cloud")
    assert S.debug_damage_counters() == (1, info["function_evaluations"]), "one build of the node runs per solve"
    close(dU, xr_, 1e-8, "newton_solve: dU", "newton dU 1e-8", scale=np.abs(xr_).max())
    ref.residual(dU)
    sa, sb = S.download_state(), T.download_state()
    assert np.array_equal(sa["Damage_n1"], sb["Damage_n1"]), "newton_solve: damage field"
    assert 0 < sa["Damage_n1"].sum() < S.np
    for k in ("DF", "F_n1", "J_n1", "Stress", "W"):
        close(sa[k], sb[k], TOL, f"newton_solve: state {k}", "newton state 1e-10")
    cpu = ir.erosion_reference(2, 0, tuple(ir.DT_TWO_ITERATES))[0]
    assert np.array_equal(sa["Damage_n1"], cpu["damage"]), "newton_solve: damage field vs the CPU reference"
    S.close()
    T.close()


@pytest.mark.parametrize("ndim,resort", [(2, False), (3, False), (3, True)])
def test_newmark_steps(ndim, resort):
    n = nlps()
    none = n.BccSet([])
    ref = ir.erosion_reference(ndim, 0)
    case = xr.erosion_case(ndim, 0, Gf=ir.erosion_Gf(ndim, 0))
    S = solver(case, "erosion", True)
    for t, snap in enumerate(ref):
        if resort and t > 0:
            S.resort()
        info = S.newmark_step(none, t, ir.DT[t], None, beta=ir.BETA, gamma=ir.GAMMA, ksp=TIGHT, **ir.SNES)
        what = f"{ndim}-D{' with re-sorts' if resort else ''}, step {t}"
        print(what, info["fnorm_history"], info["ksp_iterations"], "reference", snap["info"]["fnorm_history"])
        assert info["reason"] > 0 and info["nactive"] == snap["na"], info
        st = S.download_state()
        failed = int(st["Damage_n1"].sum())
        print(f"{what}: {failed} of {S.np} failed")
        assert failed == int(snap["damage"].sum()), f"{what}: failed count"
        assert np.array_equal(st["Damage_n1"], snap["damage"]), f"{what}: Damage_n1"
        assert np.array_equal(st["Damage_n"], snap["damage"]), f"{what}: Damage_n after the roll"
        for k, ok in (("x_GC", "x"), ("vel", "vel"), ("acc", "acc"), ("F_n", "F_n"), ("J_n", "J_n"), ("Stress", "stress")):
            close(st[k], snap[ok], 1e-8, f"{what}: {k}", "newmark 1e-8")
    S.close()


def test_contract():
    """Who the setter refuses, and that the switch changes nothing outside the fused damage form: with the switch off the
    default call against NLPS_LAGR_SEPARATE, and the switch on with NLPS_LAGR_SEPARATE against the switch-off default, all
    on ONE handle from the same vectors.  The particle state -- every particle's arithmetic is its own -- is compared with
    array_equal.  The residual is a sum of floating-point atomics in arrival order, which two runs of the same kernels do
    not repeat bit for bit on either commit: array_equal does not hold for it (measured on the MI355X, one handle, of the
    largest entry: 2.4e-16, 2.7e-16 and 3.3e-16 in three runs), so it is bound at ten times the largest measured value,
    3.3e-15.  Which path ran is read from
    the library's counter of fused damage evaluations: a NLPS_LAGR_SEPARATE call must not move it."""
    n = nlps()
    none = n.BccSet([])
    case = xr.erosion_case(2, 0, Gf=ir.erosion_Gf(2, 0))
    P = gpu_setup(case)
    with pytest.raises(n.NlpsError, match="without driver_eigenerosion"):
        P.set_implicit_damage(True)
    P.close()
    fluid = {"type": 6, "E": 0.0, "nu": 0.0, "p_ref": 1.0e3, "viscosity": 40.0, "compressibility": 2.0e5, "n_macdonald": 7.0,
             "Ceps": 1.5, "Gf": 1.0}
    W = solver(block(2, [dict(ELASTIC, type=0), fluid]), "erosion", False)
    with pytest.raises(n.NlpsError, match="Newtonian-Fluid-Compressible"):
        W.set_implicit_damage(True)
    W.close()
    S = solver(case, "erosion", False)
    S.set_halo_exchange(lambda dptr, nfield, elem, kind: 0)
    with pytest.raises(n.NlpsError, match="ghost particles"):
        S.set_implicit_damage(True)
    S.set_halo_exchange(None)
    S.set_implicit_damage(True)
    a, alpha = alpha_of(ir.DT[0])
    dev = _Step(S, none, 0, alpha, None)
    dU = S.form_initial_guess(dev.V, dev.A, ir.DT[0], none, 0)
    S.set_halo_exchange(lambda dptr, nfield, elem, kind: 0)  # attached after the setter: the evaluation refuses
    with pytest.raises(n.NlpsError, match="ghost particles"):
        dev.residual(dU)
    S.set_halo_exchange(None)
    fields = [k for k, _ in N1_STATE] + ["Damage_n1"]
    R_BOUND = 3.3e-15

    def same(what, Ra, sa, Rb, sb):
        for k in fields:
            assert np.array_equal(sa[k], sb[k]), f"{what}: {k}"
        print(f"{what}: R bit-equal {np.array_equal(Ra, Rb)}, relative difference {relerr(Ra, Rb):.3e} (bound {R_BOUND:.1e})")
        assert relerr(Ra, Rb) <= R_BOUND, f"{what}: R"

    def evaluate(H, flags):
        return H.lagrangian_evaluation(dU, dev.V, dev.A, dev.M, alpha, None, flags=flags), H.download_state()

    # the switch off: the default call is the separate stages
    S.set_implicit_damage(False)
    assert S.debug_damage_counters()[1] == 0
    R_def, s_def = evaluate(S, 0)
    R_sep, s_sep = evaluate(S, S.LAGR_SEPARATE)
    assert S.debug_damage_counters()[1] == 0, "switch off: no evaluation takes the fused damage form"
    same("switch off: default vs NLPS_LAGR_SEPARATE", R_def, s_def, R_sep, s_sep)
    # the switch on: NLPS_LAGR_SEPARATE still runs the separate stages, the default call the fused form
    S.set_implicit_damage(True)
    R_on_sep, s_on_sep = evaluate(S, S.LAGR_SEPARATE)
    assert S.debug_damage_counters()[1] == 0, "the switch leaks into the NLPS_LAGR_SEPARATE path"
    same("switch on with NLPS_LAGR_SEPARATE vs the switch-off default", R_on_sep, s_on_sep, R_def, s_def)
    R_on, s_on = evaluate(S, 0)
    assert S.debug_damage_counters() == (1, 1), "switch on: the default call takes the fused damage form"
    close(R_on, R_def, TOL, "contract: fused form vs the separate stages, R", "residual 1e-10")
    assert np.array_equal(s_on["Damage_n1"], s_def["Damage_n1"])
    assert 0 < s_def["Damage_n1"].sum() < S.np
    S.close()
