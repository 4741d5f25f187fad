"""Constructions that drive the device GMRES, Lanczos and Newton solves down their rare exits (tests only), shared by
tests/test_gpu_solver_exits.py (the device beside the references on the device-assembled COO) and
tests/test_solver_exits_ref.py (the references alone on the oracle's matrices of the same states).

Every construction exists twice, *_oracle (no GPU: the CPU oracle's stages and its dense tangent) and *_device (a handle at
the same state), built from one description so that the two files cannot drift apart:
  1. one particle: test_gpu_tangent_csr.py::test_single_particle's cloud, fewer dofs than any restart;
  2. the fully eroded cloud: test_gpu_tangent_operator.py::test_eigenerosion_damage_scaling with Gf below every
     particle's energy release rate, tangent_vol = V0 (1 - 1) = 0 exactly;
  3. the partly eroded cloud: Gf at a low quantile of G, so that some active nodes lose every particle of theirs;
  4. right-hand sides that live on the fixed dofs of _linearised's states, where K b = b exactly.
No function here calls a solver under test."""
import numpy as np

import krylov_ref
from test_gpu_tangent_operator import LAWS, _case
from util import NH, dirichlet_plane, gpu_setup, make_case, nlps, oracle_setup, orc

ALPHA_1 = 4.0e4
AMP = {"neo-hookean": 2e-2, "hencky": 2e-2, "drucker-prager": 8e-3}  # test_gpu_tangent_operator._linearised's
PART_QUANTILE = 0.12  # Gf of construction 3: 88 % of the particles fail, whole corners of the block with them
# the seeds of the right-hand sides, one per case: tests/test_solver_exits_ref.py holds each to its conditions
SEED_FIXED, SEED_DIAGONAL, SEED_ONE_PARTICLE, SEED_SINGULAR, SEED_REFUSAL, SEED_ATOL, SEED_NAN, SEED_WIDE = 7, 8, 41, 9, 10, 102, 11, 31
SEED_LANCZOS = 4
SNES_STOL = 0.1
ERODED = [(2, 0), (3, 0)]  # (ndim, law) of the eroded clouds
REFUSAL_KSP = dict(restart=40, max_it=40, rtol=1e-5)  # the solve without preconditioner after a refused one
# restart 256 over full cycles: alpha_1 = 1e3 and no Dirichlet rows.  With (ALPHA_1, Mv, True) the identity rows beside
# the stiffness (cond 2e7) bring the estimate to its rounding floor, 1e-10 ||b||, by step 230: the entries around step 256
# then differ by a fifth between two orders of summation.  Here (cond 7e4) the estimate is 3e-3 ||b|| at step 256.
WIDE_256_OPERATOR = (1.0e3, False)
_cache = {}


# ------------------------------------------------------------------------------------------------ the oracle side
def _oracle_matrix(st, alpha_1, mass, dirichlet):
    o = orc()
    o.set_tangent_damage(st.get("damage"))
    try:
        K, _, status = o.tangent_matrix(st["P"], st["M"], st["mats"], st["n2m"], st["d2m"] if dirichlet else None, st["na"],
                                        alpha_1, mass, with_pattern=False)
    finally:
        o.set_tangent_damage(None)
    assert status == 0
    return K


def oracle_matrix(st, alpha_1=0.0, mass=None, dirichlet=False):
    """The oracle's dense tangent of a *_oracle state; with st["damage"] scaled by 1 - Damage_n1 (orc.set_tangent_damage)."""
    return _oracle_matrix(st, alpha_1, mass, dirichlet)


def linearised_oracle(ndim, law, seed=13):
    """test_gpu_tangent_operator._linearised without a handle: the same cloud, masks (step 1, the floor fixed) and dU."""
    o = orc()
    case = _case(ndim, LAWS[law])
    nsteps = 2
    M, P, prm, mats = oracle_setup(case)
    n2m, na = o.active_nodes(M)
    d2m, _ = o.active_dofs(n2m, na, ndim, o.BccSet([dirichlet_plane(case, ndim - 1, 3, nsteps)]), 1, nsteps)
    rng = np.random.default_rng(seed)
    dU = AMP[law] * rng.normal(size=na * ndim)
    assert o.compatibility(dU, None, P, M, n2m) == 0 and o.constitutive(P, mats, prm) == 0
    return dict(M=M, P=P, mats=mats, n2m=n2m, d2m=d2m, na=na, ndim=ndim, Mv=o.lumped_mass(P, M, n2m, na))


def linearised_device(ndim, law, seed=13, deterministic=False):
    """The state of test_gpu_tangent_operator._linearised on a handle alone (deterministic: nlps_gpu_set_deterministic)."""
    case = _case(ndim, LAWS[law])
    nsteps = 2
    S = gpu_setup(case, nsteps=nsteps)
    if deterministic:  # (the mode orders the particles in the search: test_gpu_deterministic_implicit.py)
        S.set_deterministic(True)
        S.local_search()
    _, d2m = S.active_masks(nlps().BccSet([dirichlet_plane(case, ndim - 1, 3, nsteps)]), 1)
    na = S.nactive
    S.local_compatibility_conditions(AMP[law] * np.random.default_rng(seed).normal(size=na * ndim))
    S.constitutive_update()
    return dict(S=S, na=na, ndim=ndim, d2m=d2m, Mv=S.compute_nodal_lumped_mass())


# ------------------------------------------------------------------------------------------------ 1. one particle
def one_particle_case(ndim):
    case = _case(ndim, NH, velocity=False)
    case["cloud"] = {k: (np.ascontiguousarray(v[np.array([5])]) if isinstance(v, np.ndarray) else v)
                     for k, v in case["cloud"].items()}
    return case


def _one_particle_dU(ntot):
    return 5e-3 * np.random.default_rng(3).normal(size=ntot)  # test_gpu_tangent_csr.linearise's


def one_particle_oracle(ndim):
    o = orc()
    case = one_particle_case(ndim)
    M, P, prm, mats = oracle_setup(case)
    assert o.local_search(P, M, prm) == 0
    n2m, na = o.active_nodes(M)
    d2m, _ = o.active_dofs(n2m, na, ndim, o.BccSet([]), 0, 2)
    assert o.compatibility(_one_particle_dU(na * ndim), None, P, M, n2m) == 0 and o.constitutive(P, mats, prm) == 0
    return dict(M=M, P=P, mats=mats, n2m=n2m, d2m=d2m, na=na, ndim=ndim, Mv=o.lumped_mass(P, M, n2m, na))


def one_particle_device(ndim):
    S = gpu_setup(one_particle_case(ndim), nsteps=2)
    S.local_search()
    _, d2m = S.active_masks(nlps().BccSet([]), 0)
    assert S.num_particles() == 1
    S.local_compatibility_conditions(_one_particle_dU(S.nactive * ndim))
    S.constitutive_update()
    return dict(S=S, na=S.nactive, ndim=ndim, d2m=d2m, Mv=S.compute_nodal_lumped_mass())


# ------------------------------------------------------------------------------------------------ 2. and 3. eroded clouds
def erosion_case(ndim, law, level):
    """(case, dU, G, Gf): the stretched block of test_eigenerosion_damage_scaling with the oracle's energy release rates G
    at Gf = 0 and a critical rate below all of them (level "all") or at PART_QUANTILE of them (level "part", half way
    between two particles, never on one).  Computed once per (ndim, law)."""
    from test_gpu_eigenerosion import stretch_field
    key = ("erosion", ndim, law)
    if key not in _cache:
        o = orc()
        rng = np.random.default_rng(21)
        mat = {"type": law, "E": 1.0e6, "nu": 0.25, "Ceps": 1.5, "Gf": 0.0}
        if ndim == 2:
            case = make_case(2, [14, 12], [3, 3], [7, 6], material=mat)
        else:
            case = make_case(3, [11, 10, 9], [3, 3, 2], [5, 4, 4], material=mat)
        M, P, prm, mats = oracle_setup(case)
        n2m, na = o.active_nodes(M)
        dU = stretch_field(M, n2m, na, ndim, 0.02, rng)
        beps = o.compute_beps(P, M, mats, initialize=True)
        assert o.compatibility(dU, None, P, M, n2m) == 0 and o.constitutive_eroded(P, mats, prm, np.zeros(P.np)) == 0
        W = P["W"].copy()
        V = P["vol0"] * P["J_n1"]
        G = np.zeros(P.np)
        for p in range(P.np):
            q = beps[1][p, : beps[0][p]]
            G[p] = mat["Ceps"] * case["h"] / (V[p] + V[q].sum()) * (V[p] * W[p] + (V[q] * W[q]).sum())
        assert G.min() > 0.0
        _cache[key] = (dU, G)
    dU, G = _cache[key]
    if level == "all":
        Gf = 0.5 * float(G.min())
    else:
        gs = np.sort(G)
        k = int(PART_QUANTILE * gs.size)
        Gf = 0.5 * float(gs[k - 1] + gs[k])
        assert np.count_nonzero(np.abs(G - Gf) < 1e-9 * Gf) == 0, "no particle may sit on the threshold"
    mat = {"type": law, "E": 1.0e6, "nu": 0.25, "Ceps": 1.5, "Gf": Gf}
    if ndim == 2:
        case = make_case(2, [14, 12], [3, 3], [7, 6], material=mat)
    else:
        case = make_case(3, [11, 10, 9], [3, 3, 2], [5, 4, 4], material=mat)
    return case, dU.copy(), G, Gf


def eroded_oracle(ndim, law, level):
    """The oracle after compatibility, the eroded constitutive stage and the eigenerosion hook; st["damage"] = Damage_n1."""
    o = orc()
    case, dU, G, Gf = erosion_case(ndim, law, level)
    M, P, prm, mats = oracle_setup(case)
    n2m, na = o.active_nodes(M)
    d2m, _ = o.active_dofs(n2m, na, ndim, o.BccSet([]), 0, 2)
    beps = o.compute_beps(P, M, mats, initialize=True)
    damage_n, damage_n1 = np.zeros(P.np), np.zeros(P.np)
    assert o.compatibility(dU, None, P, M, n2m) == 0 and o.constitutive_eroded(P, mats, prm, damage_n) == 0
    assert o.eigenerosion_hook(damage_n1, damage_n, P, mats, beps, case["h"]) == 0
    return dict(M=M, P=P, mats=mats, n2m=n2m, d2m=d2m, na=na, ndim=ndim, Mv=o.lumped_mass(P, M, n2m, na), damage=damage_n1)


def eroded_device(ndim, law, level):
    """A handle with the eigenerosion driver on, after the hook (it runs between the stresses and the forces)."""
    n = nlps()
    case, dU, G, Gf = erosion_case(ndim, law, level)
    params = n.default_params()
    params.driver_eigenerosion = 1
    S = gpu_setup(case, nsteps=2, params=params)
    _, d2m = S.active_masks(n.BccSet([]), 0)
    na = S.nactive
    S.local_compatibility_conditions(dU)
    S.constitutive_update()
    S.nodal_internal_forces(np.zeros(na * ndim))
    return dict(S=S, na=na, ndim=ndim, d2m=d2m, Mv=S.compute_nodal_lumped_mass(), damage=S.download_state()["Damage_n1"])


def block_diagonal(K, ndim):
    na = K.shape[0] // ndim
    return np.stack([K[A * ndim:(A + 1) * ndim, A * ndim:(A + 1) * ndim] for A in range(na)])


def block_pivots(B, kind):
    """What include/nlps_gpu.h's rule looks at, relative to the block's Frobenius norm: the diagonal entries ("jacobi") or
    the pivots of Gauss-Jordan with partial pivoting ("pbjacobi").  A zero block gives zeros."""
    nrm = float(np.sqrt((B * B).sum()))
    if nrm == 0.0:
        return np.zeros(B.shape[0])
    if kind == "jacobi":
        return np.abs(np.diag(B)) / nrm
    a = np.array(B, dtype=np.float64)
    d = a.shape[0]
    piv = np.zeros(d)
    for c in range(d):
        p = c + int(np.argmax(np.abs(a[c:, c])))
        piv[c] = abs(a[p, c])
        if piv[c] == 0.0:
            break
        a[[c, p]] = a[[p, c]]
        a[c] /= a[c, c]
        for r in range(d):
            if r != c:
                a[r] -= a[r, c] * a[c]
    return piv / nrm


def first_refused_node(K, ndim, kind):
    """(the smallest masked node whose diagonal block fails |pivot or entry| <= 1e-14 ||block||_F, or None; the smallest
    relative pivot among the blocks that pass)"""
    bad, margin = None, np.inf
    for A, B in enumerate(block_diagonal(K, ndim)):
        p = block_pivots(B, kind).min()
        if p <= 1e-14:
            bad = A if bad is None else bad
        else:
            margin = min(margin, p)
    return bad, margin


# ------------------------------------------------------------------------------------------------ 4. right-hand sides
def lanczos_steps(ndim):
    """max_it of the Lanczos run on one particle: more steps than dofs (18 in 2-D, 81 in 3-D)"""
    return 64 if ndim == 2 else 128


def rhs(n, seed):
    return np.random.default_rng(seed).normal(size=n)


def dyadic_rhs(n, support, seed):
    """b = +-2^e on 4^k of the dofs in support (k as large as support allows, at most 3), exactly 0 elsewhere; signs, the
    choice of the dofs and e in -3 .. 3 are random.  ||b|| = 2^(k + e), V[0] = b / ||b|| = +-2^-k and V[0] . V[0] = 1 then
    carry no rounding error in ANY order of summation, so a happy first step is happy in the same bits on the device and in
    numpy: with K M^-1 V[0] = V[0] the Gram-Schmidt pass leaves exactly 0, and with K M^-1 = I up to the rounding of
    d * (1 / d) it leaves the same eps-sized vector on both sides.  With normal deviates (fixed_dof_rhs) V[0] . V[0] is 1
    up to a few eps and hn is rounding noise that differs between the two sides (1e-17 ||b|| in numpy, which has no fma;
    1e-31 ||b|| after the device's two fma passes): still happy, but the estimates cannot be compared at 1e-6 of
    1e-12 ||b||."""
    rng = np.random.default_rng(seed)
    support = np.asarray(support)
    assert support.size >= 4
    k = min(3, int(np.log(support.size) / np.log(4.0) + 1e-9))
    b = np.zeros(n)
    b[rng.permutation(support)[: 4 ** k]] = rng.choice([-1.0, 1.0], size=4 ** k) * 2.0 ** int(rng.integers(-3, 4))
    return b


def fixed_dof_rhs(d2m, seed):
    """normal deviates on the dofs with d2m == -1, exactly 0 elsewhere"""
    fixed = np.flatnonzero(d2m == -1)
    b = np.zeros(d2m.shape[0])
    b[fixed] = np.random.default_rng(seed).normal(size=fixed.size)
    return b


# ------------------------------------------------------------------------------------------------ more than 300 free dofs
def wide_case():
    return make_case(2, [40, 30], [3, 3], [32, 20])  # test_gpu_critical_dt.py::test_several_blocks_and_waves's block


def wide_oracle():
    o = orc()
    case = wide_case()
    M, P, prm, mats = oracle_setup(case)
    assert o.local_search(P, M, prm) == 0
    n2m, na = o.active_nodes(M)
    d2m, _ = o.active_dofs(n2m, na, 2, o.BccSet([dirichlet_plane(case, 1, 3, 2)]), 1, 2)
    dU = 2e-2 * np.random.default_rng(3).normal(size=na * 2)
    assert o.compatibility(dU, None, P, M, n2m) == 0 and o.constitutive(P, mats, prm) == 0
    return dict(M=M, P=P, mats=mats, n2m=n2m, d2m=d2m, na=na, ndim=2, Mv=o.lumped_mass(P, M, n2m, na))


def wide_device():
    case = wide_case()
    S = gpu_setup(case, nsteps=2)
    S.local_search()
    _, d2m = S.active_masks(nlps().BccSet([dirichlet_plane(case, 1, 3, 2)]), 1)
    S.local_compatibility_conditions(2e-2 * np.random.default_rng(3).normal(size=S.nactive * 2))
    S.constitutive_update()
    return dict(S=S, na=S.nactive, ndim=2, d2m=d2m, Mv=S.compute_nodal_lumped_mass())


# ------------------------------------------------------------------------------------------------ the reference's conditions
def reference_gmres(K, b, pc, ndim, **kw):
    return krylov_ref.gmres(K, b, krylov_ref.preconditioner(K, pc, ndim), **kw)


def tolerance(info, rtol=1e-5, atol=0.0):
    return max(rtol * info["bnorm"], atol)


def gate_is_clear(info):
    """hn / sqrt(ww) of every Arnoldi step is exactly 0, below 1e-15 or above 1e-12: two decades or more from KSP_HAPPY
    (1e-14) on either side, so that the device's order of summation cannot move a step across the gate."""
    r = info["happy_ratio"]
    return bool(np.all((r == 0.0) | (r < 1e-15) | (r > 1e-12)))


def stop_margin(info, tol):
    """The smallest factor between tol and the estimates that decide the stop: the last entry of the history (it stopped
    the cycle, or the run ended on max_it above it) and the one before (it let the run go on), history[0] included when
    no step was taken.  Infinite where tol or every such entry is 0."""
    h = np.asarray(info["history"], dtype=np.float64)
    deciding = h[-2:]
    deciding = deciding[deciding > 0.0]
    if tol <= 0.0 or deciding.size == 0:
        return np.inf
    f = deciding / tol
    return float(np.maximum(f, 1.0 / f).min())


def rounding_sensitivity(K, b, pc, ndim, window=40, trials=3, **kw):
    """The largest move of the reference's own history (in the measure of the device comparison, over its first `window`
    entries) when every entry of K and b moves by a relative eps, normal deviates of a fixed seed: what two orders of
    summation do to the same iteration.  A case whose history moves by more than a hundredth of the comparison's 1e-6
    says nothing about the device."""
    rng = np.random.default_rng(2024)
    _, ref = reference_gmres(K, b, pc, ndim, **kw)
    h = ref["history"]
    worst = 0.0
    for _ in range(trials):
        Kp = K * (1.0 + 2.220446049250313e-16 * rng.normal(size=K.shape))
        bp = b * (1.0 + 2.220446049250313e-16 * rng.normal(size=b.shape))
        _, p = reference_gmres(Kp, bp, pc, ndim, **kw)
        k = min(window, len(h), len(p["history"]))
        worst = max(worst, float((np.abs(p["history"][:k] - h[:k]) / np.maximum(h[:k], 1e-12 * h[0])).max()))
    return worst
