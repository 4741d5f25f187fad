"""The 2-D implicit kernels against the CPU oracle on clouds that span several tiles.

A 2-D tile is 16 x 16 nodes (TileCfg<2>::TB, window 20 x 20 from tile * 16 - 2) and the other 2-D oracle tests run on grids
of at most 14 cells a side: one tile, one window, one work-list entry.  The two clouds here put the seam between windows
inside the cloud:

  corner  make_case(2, [22, 20], [12, 12], [7, 6]): 168 particles around node (16, 16), closest nodes 12..19 x 12..18, all
          four tiles populated (49 / 49 / 35 / 35), 90 active nodes, last tile column and row partial (23 and 21 nodes);
  strip   make_case(2, [38, 24], [13, 18], [21, 4]): 336 particles, closest nodes 13..34 x 18..22, tiles 3, 4, 5 of a 3 x 2
          tile grid (tile row 0 empty: a compacted, shifted work list), 256 particles in the middle tile, 168 active nodes.

Every comparison is against the oracle (oracle/orc.py: one thread, no tiles, the caller's particle order) or a numpy
reference run on the ORACLE's matrix; where a device result is also held to another device result (CSR against the COO,
block CSR against the CSR arrays) the oracle comparison stands beside it.  Every test first asserts from the downloaded I0
that the intended tiles are populated.  Tolerances are those the project already uses for each quantity (named where
used); none is new."""
import functools

import numpy as np
import pytest

import bsr_ref
import lanczos_ref
import minres_cases as mc
import snes_ref
from newmark import newmark_parameters, newmark_step
from test_gpu_critical_dt import EPS, _free_block
from test_gpu_lagrangian import N_STATE, STATE, TOL, _compare_state, _moved_case, _oracle_residual
from test_gpu_minres import _check_history, _check_rnorm, _reference
from test_gpu_newton_solve import HISTORY_TOL, SOFT, TIGHT, _alpha, _problem, _same_counts, _Step
from test_gpu_parity import _DeviceStages, _OracleStages, compare_search, masks
from test_gpu_tangent_bsr import check_against_csr
from test_gpu_tangent_csr import check_against_coo
from test_gpu_tangent_operator import LAWS, _check_apply, _check_blocks, _coo_dense, _linearised
from test_gpu_tangent_solve import _check_against_reference
from util import DP, NH, assert_close, dirichlet_plane, gpu_setup, make_case, nlps, oracle_setup, orc, relerr

pytestmark = pytest.mark.gpu

TB = 16  # TileCfg<2>::TB
NHK = "neo-hookean"
# plane: the row of grid nodes that is fixed; it runs across the seam(s) between the tile columns
CLOUDS = {"corner": dict(cells=[22, 20], lo=[12, 12], blk=[7, 6], plane=13, tiles={(0, 0), (1, 0), (0, 1), (1, 1)}),
          "strip": dict(cells=[38, 24], lo=[13, 18], blk=[21, 4], plane=19, tiles={(0, 1), (1, 1), (2, 1)})}
THREE_LAWS = [{"type": 0, "E": 2.0e4, "nu": 0.3}, {"type": 1, "E": 1.0e4, "nu": 0.25}, DP]  # test_gpu_lagrangian's
TANGENT_TOL = {NHK: 1e-10, "hencky": 1e-8, "drucker-prager": 1e-8, "von-mises": 1e-8, "matsuoka-nakai": 1e-7}


def cloud(name, material=NH):
    c = CLOUDS[name]
    return make_case(2, c["cells"], c["lo"], c["blk"], material=material, velocity=[1.0, -2.0])


def tile_of(case, node):
    nx = case["grid_n"][0]
    node = np.asarray(node)
    return (node % nx) // TB, (node // nx) // TB


def tile_set(case, nodes):
    tx, ty = tile_of(case, nodes)
    return set(zip(tx.tolist(), ty.tolist()))


def assert_tiles(case, S, name):
    """the closest nodes the DEVICE holds lie in the tiles the cloud is meant to populate, and in no other"""
    I0 = S.download_state()["I0"]
    got = tile_set(case, I0)
    assert got == CLOUDS[name]["tiles"], f"{name}: populated tiles {sorted(got)}, not {sorted(CLOUDS[name]['tiles'])}"
    return I0


def fixed_across_the_seam(case, n2m, d2m):
    """the active nodes with a fixed dof lie in more than one tile column"""
    node = np.nonzero(n2m >= 0)[0]
    fixed = node[(d2m.reshape(-1, 2)[n2m[node]] == -1).any(axis=1)]
    return len({t[0] for t in tile_set(case, fixed)}) > 1


def compare_shapes(S, o, P, M, what):
    """test_gpu_parity.test_shape_functions_level_a's comparison, every particle: N at 1e-11, grad N at 1e-9 of its size"""
    nn, _ = S.download_lists()
    N, dN = S.shape_functions()
    worst_n = worst_d = 0.0
    for p in range(S.np):
        n_ref, d_ref = o.compute_N(P, M, p), o.compute_dN(P, M, p)
        k = n_ref.shape[0]
        assert k == nn[p]
        worst_n = max(worst_n, float(np.max(np.abs(N[p, :k] - n_ref))))
        worst_d = max(worst_d, float(np.max(np.abs(dN[p, :k] - d_ref)) / np.max(np.abs(d_ref))))
        assert not N[p, k:].any() and not dN[p, k:].any()
        assert abs(N[p, :k].sum() - 1.0) < 1e-12
    print(f"{what}: N {worst_n:.3e}, grad N {worst_d:.3e} of its magnitude")
    assert worst_n < 1e-11, f"{what}: N differs by {worst_n:.2e}"
    assert worst_d < 1e-9, f"{what}: dN differs by {worst_d:.2e} of its magnitude"


# ------------------------------------------------------------------------------------------ 1. search and shape functions
@pytest.mark.parametrize("name", ["corner", "strip"])
def test_search_and_shape_functions(name):
    """initialise_shapefun, then the 0.37 h random displacement of _moved_case and local_search: I0, lists (order included),
    beta and both masks bit for bit, lambda at 1e-9, N and grad N of every particle."""
    o = orc()
    nsteps = 2
    case = cloud(name)
    bcs_list = [dirichlet_plane(case, 1, CLOUDS[name]["plane"], nsteps)]
    M, P, prm, mats = oracle_setup(case)
    S = gpu_setup(case, nsteps=nsteps)
    assert_tiles(case, S, name)
    st = compare_search(S, P, M, f"{name}: initialize__LME__")
    print(f"{name}: lambda after initialize__LME__ {relerr(st['lambda'], P['lambda']):.3e}")
    compare_shapes(S, o, P, M, f"{name}: after initialize__LME__")
    n2m, d2m, na = masks(S, M, bcs_list, 1, nsteps)
    assert fixed_across_the_seam(case, n2m, d2m)
    S.close()
    case2, M, P, prm, mats = _moved_case(2, NH, nsteps, np.random.default_rng(7), case=case)
    S = gpu_setup(case2, init=False, nsteps=nsteps)
    assert o.local_search(P, M, prm) == 0
    S.local_search()
    I0 = assert_tiles(case2, S, name)
    assert np.count_nonzero(I0 != case2["cloud"]["I0"]) > 0, "the search must move some closest nodes"
    st = compare_search(S, P, M, f"{name}: local_search__LME__")
    print(f"{name}: lambda after local_search__LME__ {relerr(st['lambda'], P['lambda']):.3e}")
    compare_shapes(S, o, P, M, f"{name}: after local_search__LME__")
    n2m, d2m, na = masks(S, M, bcs_list, 1, nsteps)
    assert fixed_across_the_seam(case2, n2m, d2m)
    S.close()


# ------------------------------------------------------------------------------------------ 2. level-B stages
@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("law", [NHK, "hencky", "drucker-prager"])
def test_level_b_stages(law, deterministic):
    """test_gpu_parity.test_stage_functions on the corner cloud, the fixed row of nodes crossing the seam: lumped mass,
    nodal field, compatibility with the rates, constitutive update, internal forces, roll and kinetics at the project's
    1e-10, with atomics and in deterministic mode against the same oracle."""
    mat = LAWS[law]
    case = cloud("corner", mat)
    rng = np.random.default_rng(7)
    case["cloud"]["acc"][:] = rng.normal(size=case["cloud"]["acc"].shape)
    case["cloud"]["dt_F_n"] = 0.1 * rng.normal(size=(case["cloud"]["x"].shape[0], 5))
    case["cloud"]["dt_F_n"][:, 4] = 0.0
    nsteps = 3
    bcs_list = [dirichlet_plane(case, 1, CLOUDS["corner"]["plane"], nsteps)]
    O, D = _OracleStages(case, nsteps), _DeviceStages(case, nsteps)
    S, P = D.S, O.P
    S.set_deterministic(deterministic)
    assert_tiles(case, S, "corner")
    O.local_search()
    D.local_search()
    compare_search(S, P, O.M, "local_search__LME__")
    n2m, d2m, na = O.masks(bcs_list, 1)
    n2m_g, d2m_g, na_g = D.masks(bcs_list, 1)
    assert na_g == na and np.array_equal(n2m_g, n2m) and np.array_equal(d2m_g, d2m)
    assert fixed_across_the_seam(case, n2m, d2m)
    Mv_o, Mv_g = O.lumped_mass(), D.lumped_mass()
    assert_close(Mv_g, Mv_o, TOL, "lumped mass")
    assert_close(Mv_g.reshape(-1, 2)[:, 0].sum(), P["mass"].sum(), 1e-12, "mass conservation")
    V_o, A_o = O.nodal_field_n(Mv_o)
    V_g, A_g = D.nodal_field_n(Mv_g)
    assert_close(V_g, V_o, TOL, "nodal velocity")
    assert_close(A_g, A_o, TOL, "nodal acceleration")
    dU = (2e-2 if mat["type"] == 2 else 1e-3) * rng.normal(size=na * 2)
    dUdt = 1e-1 * rng.normal(size=na * 2)
    for stages in (O, D):
        stages.compatibility(dU, dUdt)
        stages.constitutive()
    st = S.download_state()
    for k, ok in (("DF", "DF"), ("F_n1", "F_n1"), ("J_n1", "J_n1"), ("dt_DF", "dt_DF"), ("dt_F_n1", "dt_F_n1"),
                  ("Stress", "stress"), ("W", "W"), ("b_e_n1", "b_e_n1"), ("Kappa_n1", "kappa_n1"),
                  ("EPS_n1", "eps_n1"), ("C_ep", "C_ep")):
        if mat["type"] != 2 and k in ("b_e_n1", "Kappa_n1", "EPS_n1", "C_ep"):
            continue
        print(f"{law} {k}: {relerr(st[k], P[ok]):.3e}")
        assert_close(st[k], P[ok], TOL, f"{k} after compatibility+constitutive")
    assert np.abs(P["dt_F_n1"]).max() > 0
    if mat["type"] == 2:
        assert np.count_nonzero(P["eps_n1"] > P["eps_n"]) > 0, "the case must exercise the plastic tangent"
    R_o, R_g = O.internal_forces(), D.internal_forces()
    print(f"{law} internal forces: {relerr(R_g, R_o):.3e}")
    assert_close(R_g, R_o, TOL, "internal forces")
    assert (d2m == -1).any() and np.all(R_g[d2m == -1] == 0.0), "Dirichlet dofs carry exactly 0"
    dV, dA = 1e-2 * rng.normal(size=na * 2), 1e-1 * rng.normal(size=na * 2)
    O.roll()
    D.roll()
    O.update_kinetics(dU, V_o, dV, dA)
    D.update_kinetics(dU, V_g, dV, dA)
    st = S.download_state()
    for k, ok in (("x", "x"), ("dis", "dis"), ("vel", "vel"), ("acc", "acc"), ("F_n", "F_n"), ("J_n", "J_n"), ("rho", "rho"),
                  ("dt_F_n", "dt_F_n")):
        assert_close(st[k], P[ok], TOL, f"{k} after roll+kinetics")
    S.close()


# ------------------------------------------------------------------------------------------ 3. / 4. the fused residual
NSTEPS, STEP, THICKNESS = 3, 1, 0.5


@functools.lru_cache(maxsize=None)
def residual_reference(name, law, layout=None):
    """The oracle's residual and particle state at two dU on the moved cloud, once per (cloud, law, layout).  law: a key of
    LAWS; layout: None (one law), "interleaved" (three laws, p % 3) or "tiles" (one law per tile of the closest node).
    Nothing a test does changes what this returns: the arrays are copies."""
    o = orc()
    rng = np.random.default_rng(11)
    mat = LAWS[law]
    case, M, P, prm, mats = _moved_case(2, mat, NSTEPS, rng, case=cloud(name, mat))
    npart = case["cloud"]["x"].shape[0]
    if layout is not None:
        case["materials"] = THREE_LAWS
        if layout == "interleaved":
            matidx = np.arange(npart) % 3
        else:  # by the tile the moved particle is binned to: the search of the unmixed cloud says which that is
            assert o.local_search(P, M, prm) == 0
            tx, ty = tile_of(case, P["I0"])
            matidx = (tx + 2 * ty) % 3
        case["cloud"]["matidx"] = matidx.astype(np.int32)
        P = o.OracleParticles(case["cloud"])
        mats = o.make_materials(case["materials"])
    bcs_list = [dirichlet_plane(case, 1, CLOUDS[name]["plane"], NSTEPS)]
    assert o.local_search(P, M, prm) == 0
    n2m, na = o.active_nodes(M)
    d2m, _ = o.active_dofs(n2m, na, 2, o.BccSet(bcs_list), STEP, NSTEPS)
    Mv = o.lumped_mass(P, M, n2m, na)
    V, A = o.nodal_field_n(Mv, P, M, n2m, d2m, na)
    a = newmark_parameters(0.25, 0.5, 2.0e-3)
    grav = [0.0, -9.81]
    # contour particles of every populated tile in both load sets
    I0 = P["I0"].copy()
    tx, ty = tile_of(case, I0)
    sets = [[], []]
    for t in sorted(CLOUDS[name]["tiles"]):
        members = rng.permutation(np.nonzero((tx == t[0]) & (ty == t[1]))[0])[:5]
        sets[0] += members[:3].tolist()
        sets[1] += members[3:].tolist()
    d1, d2 = np.ones((2, NSTEPS), dtype=np.int32), np.ones((2, NSTEPS), dtype=np.int32)
    d2[0, STEP] = 0
    loads = [{"nodes": np.asarray(sets[0], dtype=np.int32), "dim": 2, "dir": d1, "value": rng.normal(size=(2, NSTEPS)) * 1e5},
             {"nodes": np.asarray(sets[1], dtype=np.int32), "dim": 2, "dir": d2, "value": rng.normal(size=(2, NSTEPS)) * 1e5}]
    plastic = layout is not None or mat["type"] in (2, 3)
    amps = (2e-2, 1e-2) if plastic else (1e-3, 2e-3)
    dUs, Rs, states = [], [], []
    for amp in amps:
        dU = amp * rng.normal(size=na * 2)
        Rs.append(_oracle_residual(o, P, M, mats, prm, n2m, d2m, na, 2, dU, V, A, Mv, a, grav, loads, STEP, NSTEPS, THICKNESS,
                                   None))
        dUs.append(dU)
        states.append({ok: P[ok].copy() for _, ok in STATE + N_STATE})
    yielded = int(np.count_nonzero(states[0]["eps_n1"] > states[0]["eps_n"]))
    return dict(case=case, mat=mat, bcs_list=bcs_list, n2m=n2m, d2m=d2m, na=na, Mv=Mv, V=V, A=A, grav=grav, loads=loads,
                alpha=[a["a1"], a["a2"], a["a3"], a["a4"], a["a5"], a["a6"]], amps=amps, dU=dUs, R=Rs, state=states, I0=I0,
                yielded=yielded, matidx=case["cloud"]["matidx"].copy())


def check_residuals(name, ref, deterministic, mode=None, mixed=False):
    """One handle in the mode given: mass and nodal field, then the fused residual at the two dU and the separate stages at
    the first, each against the oracle's numbers of `ref` at TOL = 1e-10."""
    n = nlps()
    case = ref["case"]
    S = gpu_setup(case, init=False, nsteps=NSTEPS)
    if mode is not None:
        S.set_law_launch_mode(mode)
    S.set_deterministic(deterministic)
    S.local_search()
    I0 = assert_tiles(case, S, name)
    assert np.array_equal(I0, ref["I0"])
    n2m, d2m = S.active_masks(n.BccSet(ref["bcs_list"]), STEP)
    assert np.array_equal(n2m, ref["n2m"]) and np.array_equal(d2m, ref["d2m"])
    assert fixed_across_the_seam(case, n2m, d2m)
    for ld in ref["loads"]:
        assert tile_set(case, I0[ld["nodes"]]) == CLOUDS[name]["tiles"], "the contour loads sit on every side of the seam"
    tag = f"{name} {'deterministic' if deterministic else 'atomic'}" + (f" mode {mode}" if mode else "")
    Mv = S.compute_nodal_lumped_mass()
    V, A = S.get_nodal_field_n(Mv)
    for got, want, what in ((Mv, ref["Mv"], "lumped mass"), (V, ref["V"], "nodal velocity"), (A, ref["A"], "nodal acceleration")):
        print(f"{tag}: {what} {relerr(got, want):.3e}")
        assert_close(got, want, TOL, f"{tag}: {what}")
    gl = n.BccSet(ref["loads"])
    fixed = ref["d2m"] == -1
    for what, q, flags in (("fused", 0, 0), ("fused, second dU", 1, 0), ("separate stages", 0, S.LAGR_SEPARATE)):
        R = S.lagrangian_evaluation(ref["dU"][q], ref["V"], ref["A"], ref["Mv"], ref["alpha"], ref["grav"], gl, STEP, THICKNESS,
                                    None, flags=flags)
        print(f"{tag} {what}: residual {relerr(R, ref['R'][q]):.3e}")
        assert_close(R, ref["R"][q], TOL, f"{tag} {what}: residual")
        assert fixed.any() and np.all(R[fixed] == 0.0), "Dirichlet dofs carry no residual"
        if not mixed:
            _compare_state(S, ref["state"][q], ref["mat"], f"{tag} {what}", ref["amps"][q])
        else:  # test_lagrangian_evaluation_of_a_cloud_of_three_laws's comparison
            st = S.download_state()
            for k, ok in STATE + N_STATE:
                if k != "W":
                    assert_close(st[k], ref["state"][q][ok], TOL, f"{tag} {what}: {k}",
                                 scale=1e-6 if k in ("EPS_n1", "EPS_n") else None)
    S.close()


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("name,law", [("corner", NHK), ("corner", "hencky"), ("corner", "drucker-prager"),
                                      ("strip", "drucker-prager")])
def test_fused_residual(name, law, deterministic):
    """nlps_gpu_lagrangian_evaluation, fused and with LAGR_SEPARATE, against test_gpu_lagrangian._oracle_residual; the
    deterministic mode against the SAME oracle numbers (not against the atomic run)."""
    ref = residual_reference(name, law)
    if ref["mat"]["type"] == 2:
        assert ref["yielded"] > 0, "the case must yield"
    check_residuals(name, ref, deterministic)


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("layout", ["interleaved", "tiles"])
def test_mixed_cloud(layout, mode, deterministic):
    """Three laws on the corner cloud, interleaved p % 3 or one law per tile (law (tx + 2 ty) % 3: every per-law launch
    sees another set of tiles, and no law is in all four), in both law launch modes."""
    ref = residual_reference("corner", "drucker-prager", layout)
    dp = ref["matidx"] == 2
    assert np.count_nonzero(ref["state"][0]["eps_n1"][dp] > ref["state"][0]["eps_n"][dp]) > 0, "the plastic part must yield"
    assert np.all(ref["state"][0]["eps_n1"][~dp] == 0.0)
    per_law = [tile_set(ref["case"], ref["I0"][ref["matidx"] == m]) for m in range(3)]
    if layout == "tiles":
        assert per_law == [{(0, 0), (1, 1)}, {(1, 0)}, {(0, 1)}], per_law
    else:
        assert all(t == CLOUDS["corner"]["tiles"] for t in per_law)
    check_residuals("corner", ref, deterministic, mode=mode, mixed=True)


# ------------------------------------------------------------------------------------------ 5. the tangent, every form
def crosses_a_seam(case, n2m, K, na):
    """some block (A, B) of K is present whose nodes lie in different tiles"""
    node = np.empty(na, dtype=np.int64)
    act = np.nonzero(n2m >= 0)[0]
    node[n2m[act]] = act
    tx, ty = tile_of(case, node)
    present = np.abs(K.reshape(na, 2, na, 2)).max(axis=(1, 3)) > 0
    other = (tx[:, None] != tx[None, :]) | (ty[:, None] != ty[None, :])
    return bool((present & other).any())


def oracle_error(K, K_o, tol, what):
    err = np.abs(K - K_o).max() / np.abs(K_o).max()
    print(f"{what}: {err:.3e} of max |K_oracle|")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.1e}"


@pytest.mark.parametrize("name,law", [("corner", k) for k in LAWS] + [("strip", NHK), ("strip", "drucker-prager")])
def test_tangent_in_every_form(name, law):
    """The assembled COO, the CSR rows, block CSR (full; upper for Neo-Hookean), K x and the diagonal blocks, each against
    the oracle's tangent_matrix at the tolerances of the assembled tests: 1e-10 (Neo-Hookean), 1e-8 (Hencky, Drucker-Prager,
    Von-Mises), 1e-7 (Matsuoka-Nakai) of max |K_oracle|.  CSR against COO at 1e-11 with the structure exact
    (check_against_coo), block CSR against the rearranged CSR arrays bit for bit (bsr_ref)."""
    s = _linearised(2, law, case=cloud(name, LAWS[law]), plane=CLOUDS[name]["plane"])
    S, o, na, case, rng = s["S"], s["o"], s["na"], cloud(name), s["rng"]
    ntot = na * 2
    assert_tiles(case, S, name)
    assert fixed_across_the_seam(case, s["n2m"], s["d2m"])
    if law in ("drucker-prager", "von-mises"):
        yielded = int((s["P"]["eps_n1"] > s["P"]["eps_n"]).sum())
        print(f"{name} {law}: {yielded} of {s['P'].np} particles yielded")
        assert yielded > 0, "some particles must be plastic"
    tol = TANGENT_TOL[law]
    for alpha_1, mass, dirichlet in ((0.0, None, False), (4.0e4, s["Mv"], True)):
        what = f"{name} {law} (alpha_1={alpha_1}, dirichlet={dirichlet})"
        K_o, _, st = o.tangent_matrix(s["P"], s["M"], s["mats"], s["n2m"], s["d2m"] if dirichlet else None, na, alpha_1, mass,
                                      with_pattern=False)
        assert st == 0
        assert crosses_a_seam(case, s["n2m"], K_o, na), "some row must hold a column of a node in another tile"
        scale = np.abs(K_o).max()
        K_coo = _coo_dense(S, ntot, alpha_1, mass, dirichlet)
        oracle_error(K_coo, K_o, tol, f"{what}: COO")
        K_csr, csr, _ = check_against_coo(S, alpha_1, mass, dirichlet, what)  # (leaves this operator current)
        oracle_error(K_csr, K_o, tol, f"{what}: CSR")
        full = check_against_csr(S, "full", csr, what)
        oracle_error(bsr_ref.dense_of_bsr(*full, 2), K_o, tol, f"{what}: block CSR")
        if law == NHK:
            up = check_against_csr(S, "upper", csr, what)
            oracle_error(bsr_ref.dense_of_bsr(*up, 2, upper=True), K_o, tol, f"{what}: upper block CSR, completed")
        _check_apply(S, K_coo, ntot, rng, what)
        for _ in range(3):
            x = rng.normal(size=ntot)
            y = S.tangent_apply(x)
            print(f"{what}: K x {relerr(y, K_o @ x, scale * np.abs(x).max()):.3e}")
            assert_close(y, K_o @ x, tol, f"{what}: apply vs oracle", scale=scale * np.abs(x).max())
        _check_blocks(S, K_coo, na, 2, what)
        blocks_o = np.stack([K_o[2 * A:2 * A + 2, 2 * A:2 * A + 2] for A in range(na)])
        assert_close(S.tangent_block_diagonal(), blocks_o, tol, f"{what}: block diagonal vs oracle", scale=scale)
    S.close()


# ------------------------------------------------------------------------------------------ 6. solves on the oracle's matrix
def test_linear_solves_and_lambda_max_on_the_strip():
    """Neo-Hookean strip, alpha_1 = 4e4, Dirichlet on.  tangent_solve by GMRES(30) and MINRES with every preconditioner: x
    against np.linalg.solve(K_oracle, b) at 1e-6 of max |x| wherever the numpy reference of the method reaches it on
    K_oracle (GMRES(30) without a preconditioner does not: both stop at max_it = 60, test_gpu_tangent_solve's case),
    iterations and history against krylov_ref / minres_ref on K_oracle (GMRES within 1, MINRES within minres_cases.WIDE's
    margin).  tangent_lambda_max against the largest dense eigenvalue of (K_oracle, M_oracle), the bracket of
    test_gpu_critical_dt.test_against_dense_eigenvalues."""
    s = _linearised(2, NHK, case=cloud("strip"), plane=CLOUDS["strip"]["plane"])
    S, o, na, case = s["S"], s["o"], s["na"], cloud("strip")
    n = na * 2
    assert_tiles(case, S, "strip")
    c = mc.DENSE
    K_o, _, st = o.tangent_matrix(s["P"], s["M"], s["mats"], s["n2m"], s["d2m"], na, c["alpha_1"], s["Mv"], with_pattern=False)
    assert st == 0 and crosses_a_seam(case, s["n2m"], K_o, na)
    S.tangent_operator(c["alpha_1"], s["Mv"], True)
    b = mc.rhs(n, c["seed"])
    xs = np.linalg.solve(K_o, b)
    rtol = c["rtol"]
    for pc in mc.PCS:
        what = f"GMRES(30) pc={pc}"
        max_it = 60 if pc == "none" else 2000
        x, info = S.tangent_solve(b, pc=pc, restart=30, rtol=rtol, max_it=max_it, history=True)
        ir = _check_against_reference(K_o, b, x, info, pc, 30, rtol, 2, what, max_it=max_it)
        print(what, info["iterations"], info["reason_name"], "reference", ir["iterations"], relerr(x, xs))
        assert (ir["reason"] > 0) == (pc != "none")
        if ir["reason"] > 0:
            assert_close(x, xs, 1e-6, f"{what}: x vs np.linalg.solve(K_oracle, b)", scale=np.abs(xs).max())
    S.set_linear_solver("minres")
    for pc in mc.PCS:
        what = f"MINRES pc={pc}"
        kw = dict(rtol=rtol, max_it=c["max_it"][pc])
        x, info = S.tangent_solve(b, pc=pc, history=True, **kw)
        xr, ir = _reference(K_o, b, pc, 2, **kw)
        print(what, info["iterations"], info["reason_name"], "reference", ir["iterations"], relerr(x, xs))
        assert relerr(xr, xs) <= 1e-8, "the reference itself reaches the dense solve on K_oracle"
        assert_close(x, xs, 1e-6, f"{what}: x vs np.linalg.solve(K_oracle, b)", scale=np.abs(xs).max())
        assert info["reason"] == ir["reason"], f"{what}: reason {info['reason_name']} vs reference {ir['reason']}"
        assert abs(info["iterations"] - ir["iterations"]) <= mc.WIDE["margin"], (info["iterations"], ir["iterations"])
        _check_rnorm(K_o, b, x, info, what)
        _check_history(info, ir, what)
    S.set_linear_solver("gmres")
    # lambda_max of (K, M) on the free dofs
    K0, _, st = o.tangent_matrix(s["P"], s["M"], s["mats"], s["n2m"], s["d2m"], na, 0.0, None, with_pattern=False)
    assert st == 0
    S.tangent_operator(0.0, None, True)
    fixed = s["d2m"] == -1
    Aff = _free_block(K0, s["Mv"], fixed)
    lam = np.linalg.eigvalsh(0.5 * (Aff + Aff.T))[-1]
    ref = lanczos_ref.lanczos(K0, s["Mv"], fixed, seed=0, max_it=60, rtol=1e-8)
    info = S.tangent_lambda_max(s["Mv"], seed=0, max_it=60, rtol=1e-8, mode=True)
    print(f"lambda_max {lam:.12e}, lambda_max - theta {lam - info['theta']:.3e}, resid {info['resid']:.3e}, "
          f"{info['iterations']} steps (reference {ref['iterations']})")
    assert info["reason"] == 1 == ref["reason"] and abs(info["iterations"] - ref["iterations"]) <= 1
    assert fixed.any() and not info["mode"][fixed].any(), "exactly 0 on the fixed dofs"
    assert -EPS * len(Aff) * lam <= lam - info["theta"] <= info["resid"] + 1e-12 * lam
    S.close()


class _OracleStep:
    """test_gpu_newton_solve._Step on the oracle: the callables snes_ref wants, from the oracle's residual and tangent"""

    def __init__(self, stages, bcs_list, step, dt, gravity, nsteps):
        self.st, self.step, self.nsteps, self.gravity = stages, step, nsteps, gravity
        self.a = newmark_parameters(0.25, 0.5, dt)
        stages.local_search()
        self.n2m, self.d2m, self.na = stages.masks(bcs_list, step)
        self.M = stages.lumped_mass()
        self.V, self.A = stages.nodal_field_n(self.M)
        self.n = self.na * 2

    def residual(self, x):
        s = self.st
        return _oracle_residual(s.o, s.P, s.M, s.mats, s.prm, self.n2m, self.d2m, self.na, 2, np.asarray(x), self.V, self.A,
                                self.M, self.a, self.gravity, None, self.step, self.nsteps, 1.0, None)

    def tangent(self):
        return self.st.tangent(self.a["a1"], self.M)

    def advance(self, dU):
        a = self.a
        dV = a["a4"] * dU + (a["a5"] - 1) * self.V + a["a6"] * self.A
        dA = a["a1"] * dU - a["a2"] * self.V - (a["a3"] + 1) * self.A
        self.st.roll()
        self.st.update_kinetics(dU, self.V, dV, dA)


@pytest.mark.parametrize("law", [NHK, "drucker-prager"])
def test_newton_solve_and_newmark_step_on_the_corner(law):
    """newton_solve, two time steps, against snes_ref's dense Newton driven by the ORACLE's residual and tangent (counts,
    dU at 1e-8, fnorm_history at test_gpu_newton_solve.HISTORY_TOL, the state the solve leaves at 1e-10), as
    test_against_the_dense_newton does with a second handle; then one newmark_step against tests/newmark.py over the
    oracle's stages (dU and particles at 1e-8, test_implicit_newmark_steps_with_device_stages's bound)."""
    dt = 1.0e-2
    case, bcs, gravity, nsteps = _problem(2, law, case=cloud("corner", SOFT if law == NHK else DP),
                                          plane=CLOUDS["corner"]["plane"])
    bcs_list = [dirichlet_plane(case, 1, CLOUDS["corner"]["plane"], nsteps)]
    alpha = _alpha(dt)
    S = gpu_setup(case, nsteps=nsteps)
    assert_tiles(case, S, "corner")
    stages = _OracleStages(case, nsteps)
    kw = dict(max_it=12, rtol=1e-10, atol=0.0, stol=0.0)
    for step in range(2):
        what = f"{law} step {step}"
        dev = _Step(S, bcs, step, alpha, gravity)
        ref = _OracleStep(stages, bcs_list, step, dt, gravity, nsteps)
        assert dev.n == ref.n and fixed_across_the_seam(case, ref.n2m, ref.d2m)
        assert_tiles(case, S, "corner")
        dU, info = dev.solve(np.zeros(dev.n), linesearch="basic", ksp=TIGHT, **kw)
        xr, ir = snes_ref.newton(ref.residual, ref.tangent, np.zeros(ref.n), linesearch="basic", linear="dense", **kw)
        print(what, "device", info["fnorm_history"], "oracle", ir["fnorm_history"])
        assert info["reason"] == snes_ref.CONVERGED_FNORM_RELATIVE and info["iterations"] >= 2, info
        _same_counts(info, ir, what)
        print(f"{what}: dU {relerr(dU, xr):.3e}")
        assert_close(dU, xr, 1e-8, f"{what}: dU", scale=np.abs(xr).max())
        rn = np.linalg.norm(ref.residual(dU))  # (the oracle's particles are at the device's dU now)
        assert abs(info["fnorm"] - rn) <= 1e-2 * info["fnorm"] + 1e-13 * info["fnorm0"], \
            f"{what}: fnorm {info['fnorm']:.6e} vs the oracle's residual there {rn:.6e}"
        hd, hr = info["fnorm_history"], ir["fnorm_history"]
        big = hr >= 1e-7 * hr[0]
        assert big[:2].all(), f"{what}: the first two entries are above 1e-7 fnorm0: {hr}"
        err = float((np.abs(hd - hr)[big] / hr[big]).max())
        print(what, "fnorm_history: largest relative difference %.3e" % err)
        assert err <= HISTORY_TOL, f"{what}: fnorm_history, relative {err:.3e}\n{hd}\n{hr}"
        st = S.download_state()
        for k, ok in (("DF", "DF"), ("F_n1", "F_n1"), ("J_n1", "J_n1"), ("Stress", "stress"), ("b_e_n1", "b_e_n1")) + \
                ((("Kappa_n1", "kappa_n1"), ("EPS_n1", "eps_n1")) if law != NHK else ()):
            assert_close(st[k], stages.P[ok], 1e-10, f"{what}: state {k}")
        dev.advance(dU)
        ref.advance(dU)
    S.close()
    # one call for the whole step
    S = gpu_setup(case, nsteps=nsteps)
    stages = _OracleStages(case, nsteps)
    dU_o, hist = newmark_step(stages, 2, bcs_list, 0, nsteps, dt, gravity)
    dU_out = np.zeros(S.nnodes * 2)
    info = S.newmark_step(bcs, 0, dt, gravity, dU_out=dU_out, linesearch="basic", ksp=TIGHT, **kw)
    assert_tiles(case, S, "corner")
    print(f"{law} newmark_step: device {info['fnorm_history']} oracle {hist}")
    assert info["reason"] > 0 and info["nactive"] * 2 == dU_o.size and hist[-1] <= 1e-10 * max(1.0, hist[0])
    print(f"{law} newmark_step: dU {relerr(dU_out[: dU_o.size], dU_o):.3e}")
    assert_close(dU_out[: dU_o.size], dU_o, 1e-8, f"{law} newmark_step: dU", scale=np.abs(dU_o).max())
    st = S.download_state()
    for k, ok in (("x", "x"), ("vel", "vel"), ("acc", "acc"), ("F_n", "F_n"), ("Stress", "stress"), ("J_n", "J_n")):
        assert_close(st[k], stages.P[ok], 1e-8, f"{law} after newmark_step: {k}")
    S.close()
