"""GPU parity tests proper: the HIP path (through the C-ABI) against the CPU oracle on the same
seeded inputs.  Bit-exact for index maps (I0, neighbour lists, ActiveNode, Nodes2Mask, dof masks);
FP64 fields to the tolerances of BASELINE.md §4: 1e-10 relative to the field's magnitude for particle
fields, 1e-10 for nodal sums (atomics reorder them)."""
import os

import numpy as np
import pytest

from util import (DP, HENCKY, NH, VM, assert_close, dirichlet_plane, free_port, gpu_setup, make_case, nlps, oracle_setup,
                  orc)

pytestmark = pytest.mark.gpu

TOL = 1e-10


def small_case(ndim, material=NH, velocity=None, **kw):
    if ndim == 2:
        return make_case(2, [14, 12], [3, 3], [7, 6], material=material, velocity=velocity, **kw)
    return make_case(3, [11, 10, 9], [3, 3, 2], [5, 4, 4], material=material, velocity=velocity, **kw)


def lists_equal(nn, a, b):
    """rows compared up to NumberNodes[p] (the oracle keeps stale entries behind the end of a list)"""
    col = np.arange(a.shape[1])[None, :]
    valid = col < nn[:, None]
    return bool(np.all(np.where(valid, a, 0) == np.where(valid, b[:, : a.shape[1]], 0)))


def compare_search(S, P, M, what):
    o = orc()
    st = S.download_state()
    assert np.array_equal(st["I0"], P["I0"]), f"{what}: I0 differs"
    nn, lst = S.download_lists()
    assert np.array_equal(nn, P["nn"]), f"{what}: NumberNodes differs"
    assert lists_equal(nn, lst, P["list"]), f"{what}: ListNodes differ (order included)"
    assert np.array_equal(S.download_active(), M.active()), f"{what}: ActiveNode differs"
    assert np.array_equal(st["beta"], P["beta"]), f"{what}: beta differs"
    assert_close(st["lambda"], P["lambda"], 1e-9, f"{what}: lambda")
    return st


@pytest.mark.parametrize("ndim", [2, 3])
def test_initialize_lme(ndim):
    case = small_case(ndim)
    M, P, prm, mats = oracle_setup(case)
    S = gpu_setup(case)
    compare_search(S, P, M, "initialize__LME__")


@pytest.mark.parametrize("ndim", [2, 3])
def test_initialize_lme_cell_centre_ties(ndim):
    """1 particle per cell at the exact centre: every corner is equidistant, the chain order decides."""
    case = small_case(ndim, jitter=0.0, ppc=1)
    M, P, prm, mats = oracle_setup(case)
    S = gpu_setup(case)
    compare_search(S, P, M, "ties")


@pytest.mark.parametrize("ndim", [2, 3])
def test_grid_boundary_particles(ndim):
    """Particles filling the whole grid: truncated stencils, boundary classes of the order tables."""
    if ndim == 2:
        case = make_case(2, [8, 7], [0, 0], [8, 7])
    else:
        case = make_case(3, [6, 5, 5], [0, 0, 0], [6, 5, 5])
    M, P, prm, mats = oracle_setup(case)
    S = gpu_setup(case)
    compare_search(S, P, M, "boundary")


def masks(S, M, bcs_list, step, nsteps):
    o = orc()
    n = nlps()
    n2m_o, na = o.active_nodes(M)
    ob = o.BccSet(bcs_list)
    d2m_o, nfree = o.active_dofs(n2m_o, na, S.ndim, ob, step, nsteps)
    gb = n.BccSet(bcs_list)
    n2m_g, d2m_g = S.active_masks(gb, step)
    assert S.nactive == na and S.nfree == nfree
    assert np.array_equal(n2m_g, n2m_o), "Nodes2Mask differs"
    assert np.array_equal(d2m_g, d2m_o), "dof mask differs"
    return n2m_o, d2m_o, na


@pytest.mark.parametrize("ndim,material", [(2, NH), (3, NH), (2, HENCKY), (3, HENCKY), (2, DP), (3, DP)])
def test_stage_functions(ndim, material):
    """One pass through the stage functions of U_Newmark_Beta in the order of U-Newmark-beta.c:192-409."""
    o = orc()
    vel = [1.0, -2.0] if ndim == 2 else [1.0, -2.0, 0.5]
    case = small_case(ndim, material=material, velocity=vel)
    rng = np.random.default_rng(7)
    case["cloud"]["acc"][:] = rng.normal(size=case["cloud"]["acc"].shape)
    T = 5 if ndim == 2 else 9
    case["cloud"]["dt_F_n"] = 0.1 * rng.normal(size=(case["cloud"]["x"].shape[0], T))
    if ndim == 2:
        case["cloud"]["dt_F_n"][:, 4] = 0.0
    nsteps = 3
    bcs_list = [dirichlet_plane(case, ndim - 1, 3, nsteps)]
    M, P, prm, mats = oracle_setup(case)
    S = gpu_setup(case, nsteps=nsteps)

    # move the particles a little so that the search does real work
    dx = 0.37 * case["h"] * rng.uniform(-1, 1, size=P["x"].shape)
    P["x"][:] += dx
    P["dis"][:] += dx
    S.close()
    case2 = dict(case)
    cloud2 = dict(case["cloud"])
    cloud2.update(x=P["x"].copy(), dis=P["dis"].copy(), I0=P["I0"].copy(), **{"lambda": P["lambda"].copy()},
                  beta=P["beta"].copy())
    case2["cloud"] = cloud2
    S = gpu_setup(case2, init=False, nsteps=nsteps)

    assert o.local_search(P, M, prm) == 0
    S.local_search()
    compare_search(S, P, M, "local_search__LME__")
    n2m, d2m, na = masks(S, M, bcs_list, 1, nsteps)

    Mv_o = o.lumped_mass(P, M, n2m, na)
    Mv_g = S.compute_nodal_lumped_mass()
    assert_close(Mv_g, Mv_o, TOL, "lumped mass")
    assert_close(Mv_g.reshape(-1, ndim)[:, 0].sum(), P["mass"].sum(), 1e-12, "mass conservation")

    V_o, A_o = o.nodal_field_n(Mv_o, P, M, n2m, d2m, na)
    V_g, A_g = S.get_nodal_field_n(Mv_g)
    assert_close(V_g, V_o, TOL, "nodal velocity")
    assert_close(A_g, A_o, TOL, "nodal acceleration")

    # a dU large enough that the Drucker-Prager particles leave the elastic range (all three tangent branches)
    dU = (2e-2 if material["type"] == 2 else 1e-3) * rng.normal(size=na * ndim)
    dUdt = 1e-1 * rng.normal(size=na * ndim)
    assert o.compatibility(dU, dUdt, P, M, n2m) == 0
    S.local_compatibility_conditions(dU, dUdt)
    assert o.constitutive(P, mats, prm) == 0
    S.constitutive_update()
    st = S.download_state()
    for k, ok in (("DF", "DF"), ("F_n1", "F_n1"), ("J_n1", "J_n1"), ("dt_DF", "dt_DF"), ("dt_F_n1", "dt_F_n1"),
                  ("Stress", "stress"), ("W", "W"), ("b_e_n1", "b_e_n1"), ("Kappa_n1", "kappa_n1"),
                  ("EPS_n1", "eps_n1"), ("C_ep", "C_ep")):
        if material["type"] != 2 and k in ("b_e_n1", "Kappa_n1", "EPS_n1", "C_ep"):
            continue
        assert_close(st[k], P[ok], TOL, f"{k} after compatibility+constitutive")
    assert np.abs(P["dt_F_n1"]).max() > 0
    if material["type"] == 2:
        plastic = np.count_nonzero(P["eps_n1"] > P["eps_n"])
        assert 0 < plastic, "the case must exercise the plastic tangent"
    # without dU_dt the rate tensors stay as they are (U-Static.c passes no rates)
    S.local_compatibility_conditions(dU)
    st2 = S.download_state()
    assert np.array_equal(st2["dt_DF"], st["dt_DF"]) and np.array_equal(st2["F_n1"], st["F_n1"])

    R_o, s = o.internal_forces(P, M, n2m, d2m, na)
    assert s == 0
    R_g = S.nodal_internal_forces(np.zeros(na * ndim))
    assert_close(R_g, R_o, TOL, "internal forces")
    free = d2m != -1
    assert np.all(R_g[~free] == 0.0)

    o.roll_state(P)
    S.update_particles_internal_variables()
    dV = 1e-2 * rng.normal(size=na * ndim)
    dA = 1e-1 * rng.normal(size=na * ndim)
    o.update_kinetics(1.0, dU, V_o, dV, dA, P, M, n2m)
    S.update_particles_kinetics_FLIP_PIC(1.0, dU, V_g, dV, dA)
    st = S.download_state()
    for k, ok in (("x", "x"), ("dis", "dis"), ("vel", "vel"), ("acc", "acc"), ("F_n", "F_n"), ("J_n", "J_n"),
                  ("rho", "rho"), ("dt_F_n", "dt_F_n")):
        assert_close(st[k], P[ok], TOL, f"{k} after roll+kinetics")


@pytest.mark.parametrize("ndim", [2, 3])
def test_masked_numbering_follows_the_mesh_file_order(ndim):
    """get_active_nodes__MeshTools__ hands out the masked index in the order of the mesh FILE's nodes (Nodes-Tools.c:46-66).
    With a file that is not numbered x-fastest (nlps_gpu_set_node_numbering: lattice node of every file node) Nodes2Mask
    comes back indexed by file node with the running index in file order, the dof mask follows the masked node, and every
    masked vector of the stage functions is the oracle's vector for that numbering."""
    o = orc()
    n = nlps()
    case = small_case(ndim, velocity=[1.0, -2.0] if ndim == 2 else [1.0, -2.0, 0.5])
    nsteps = 2
    bcs_list = [dirichlet_plane(case, ndim - 1, 3, nsteps)]
    M, P, prm, mats = oracle_setup(case)
    S = gpu_setup(case, nsteps=nsteps)
    nn = S.nnodes
    rng = np.random.default_rng(5)
    lattice_of_file = rng.permutation(nn).astype(np.int32)
    with pytest.raises(n.NlpsError):
        S.set_node_numbering(np.zeros(nn, dtype=np.int32))  # not a permutation
    S.set_node_numbering(lattice_of_file)
    # the reference's loop, over the file's nodes
    act = S.download_active()
    n2m_file = np.full(nn, -1, dtype=np.int32)
    run = 0
    for A in range(nn):
        if act[lattice_of_file[A]]:
            n2m_file[A] = run
            run += 1
    n2m_lat = np.empty(nn, dtype=np.int32)
    n2m_lat[lattice_of_file] = n2m_file  # the same map, indexed by lattice node: what the oracle's stages take
    d2m_o, nfree = o.active_dofs(n2m_lat, run, ndim, o.BccSet(bcs_list), 1, nsteps)
    n2m_g, d2m_g = S.active_masks(n.BccSet(bcs_list), 1)
    assert S.nactive == run and S.nfree == nfree
    assert np.array_equal(n2m_g, n2m_file), "Nodes2Mask is not the file-order numbering"
    assert np.array_equal(d2m_g, d2m_o), "dof mask differs"
    Mv_o = o.lumped_mass(P, M, n2m_lat, run)
    Mv_g = S.compute_nodal_lumped_mass()
    assert_close(Mv_g, Mv_o, TOL, "lumped mass in file-order numbering")
    V_o, A_o = o.nodal_field_n(Mv_o, P, M, n2m_lat, d2m_o, run)
    V_g, A_g = S.get_nodal_field_n(Mv_g)
    assert_close(V_g, V_o, TOL, "nodal velocity in file-order numbering")
    dU = 1e-3 * rng.normal(size=run * ndim)
    assert o.compatibility(dU, None, P, M, n2m_lat) == 0
    S.local_compatibility_conditions(dU)
    assert o.constitutive(P, mats, prm) == 0
    S.constitutive_update()
    R_o, st = o.internal_forces(P, M, n2m_lat, d2m_o, run)
    assert st == 0
    R_g = S.nodal_internal_forces(np.zeros(run * ndim))
    assert_close(R_g, R_o, TOL, "internal forces in file-order numbering")
    # back to lattice order
    S.set_node_numbering(None)
    masks(S, M, bcs_list, 1, nsteps)
    S.close()


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("stretch", [0.05, 0.01, -0.02])
def test_drucker_prager_return_branches(ndim, stretch):
    """Uniform volumetric stretch fields (LME reproduces them exactly) drive every particle down one branch of
    the return mapping: +5 % ends in the apex return (Drucker-Prager.c:532-590, whose tangent is all zeros
    when the apex iteration backs off), the others in the classical return or the elastic range."""
    o = orc()
    case = small_case(ndim, material=DP)
    M, P, prm, mats = oracle_setup(case)
    S = gpu_setup(case, nsteps=1)
    n2m, d2m, na = masks(S, M, [], 0, 1)
    X = M.coords().reshape(-1, ndim)
    act = np.where(n2m >= 0)[0]
    dU = np.zeros((na, ndim))
    dU[n2m[act]] = stretch * (X[act] - X.mean(0))
    dU = dU.ravel()
    assert o.compatibility(dU, None, P, M, n2m) == 0
    assert o.constitutive(P, mats, prm) == 0
    S.local_compatibility_conditions(dU)
    S.constitutive_update()
    st = S.download_state()
    for k, ok in (("DF", "DF"), ("Stress", "stress"), ("W", "W"), ("b_e_n1", "b_e_n1"), ("Kappa_n1", "kappa_n1"),
                  ("EPS_n1", "eps_n1")):
        assert_close(st[k], P[ok], TOL, f"{k} (stretch {stretch})")
    assert_close(st["C_ep"], P["C_ep"], TOL, "C_ep", scale=DP["E"])
    if stretch == 0.05:
        assert np.all(P["C_ep"] == 0.0) and np.all(st["C_ep"] == 0.0), "apex branch expected"


@pytest.mark.parametrize("ndim,material", [(2, NH), (3, NH), (2, HENCKY), (3, DP), (2, DP)])
def test_explicit_steps(ndim, material):
    """Several fused explicit predictor-corrector steps against the oracle's composition."""
    o = orc()
    n = nlps()
    vel = [0.0, -10.0] if ndim == 2 else [0.0, 0.0, -10.0]
    if material["type"] == 2:
        vel = [v * 0.02 for v in vel]
    case = small_case(ndim, material=material, velocity=vel)
    nsteps = 6
    bcs_list = [dirichlet_plane(case, ndim - 1, 2, nsteps)]
    grav = [0.0] * (ndim - 1) + [-9.81]
    dt = 0.1 * case["h"] / np.sqrt(material["E"] / 1000.0)
    M, P, prm, mats = oracle_setup(case)
    S = gpu_setup(case, nsteps=nsteps)
    stepper = o.ExplicitStepper(P, M, mats, prm, o.BccSet(bcs_list), nsteps, gravity=grav)
    gb = n.BccSet(bcs_list)
    for t in range(nsteps):
        assert stepper.step(t, dt) == 0
        S.explicit_step(gb, t, dt, 0.5, grav)
        nod = S.explicit_nodal()
        assert S.nactive == stepper.out.nactive
        for k in ("mass", "dU", "force", "accel", "reaction"):
            assert_close(nod[k], stepper.nodal(k), 1e-9, f"step {t} nodal {k}")
        st = S.download_state()
        assert np.array_equal(st["I0"], P["I0"]), f"step {t}: I0"
        nn, lst = S.download_lists()
        assert np.array_equal(nn, P["nn"]) and lists_equal(nn, lst, P["list"]), f"step {t}: lists"
        for k, ok in (("x", "x"), ("dis", "dis"), ("vel", "vel"), ("acc", "acc"), ("F_n", "F_n"), ("DF", "DF"),
                      ("Stress", "stress"), ("J_n", "J_n"), ("rho", "rho"), ("W", "W"), ("lambda", "lambda"),
                      ("b_e_n", "b_e_n"), ("Kappa_n", "kappa_n"), ("EPS_n", "eps_n")):
            assert_close(st[k], P[ok], 1e-9, f"step {t} {k}")


@pytest.mark.parametrize("ndim", [2, 3])
def test_long_flight_index_maps(ndim):
    """A soft block thrown through the grid at Mach 1 with a velocity gradient: every particle changes its
    closest node several times, crosses cell mid-planes (the tie rule of Nodes-Tools.c:476-538), the neighbour
    lists are rebuilt around moving I0s and the device re-sorts itself every 7 steps.  I0, NumberNodes, the
    lists in chain order and ActiveNode have to stay bit-identical to the oracle all the way."""
    o = orc()
    n = nlps()
    soft = {"type": 0, "E": 1.0e5, "nu": 0.3}  # celerity 10
    if ndim == 2:
        case = make_case(2, [12, 24], [3, 15], [5, 5], material=soft, velocity=[2.0, -10.0])
    else:
        case = make_case(3, [10, 10, 20], [3, 3, 12], [4, 4, 4], material=soft, velocity=[2.0, -1.0, -10.0])
    x = case["cloud"]["x"]
    xc = x.mean(axis=0)
    case["cloud"]["vel"][:, ndim - 1] *= 1.0 + 0.2 * (x[:, 0] - xc[0]) / 2.5  # shear: real deformation
    nsteps = 40
    bcs_list = [dirichlet_plane(case, ndim - 1, 2, nsteps)]
    dt = 0.25 * case["h"] / 20.0
    M, P, prm, mats = oracle_setup(case)
    I0_start = P["I0"].copy()
    S = gpu_setup(case, nsteps=nsteps)
    S.set_resort_interval(7)
    stepper = o.ExplicitStepper(P, M, mats, prm, o.BccSet(bcs_list), nsteps)
    gb = n.BccSet(bcs_list)
    for t in range(nsteps):
        assert stepper.step(t, dt) == 0, f"oracle failed at step {t}"
        S.explicit_step(gb, t, dt)
        if t % 8 == 7 or t == nsteps - 1:
            st = S.download_state()
            assert np.array_equal(st["I0"], P["I0"]), f"step {t}: I0"
            nn, lst = S.download_lists()
            assert np.array_equal(nn, P["nn"]) and lists_equal(nn, lst, P["list"]), f"step {t}: lists"
            assert np.array_equal(S.download_active(), M.active()), f"step {t}: ActiveNode"
            for k, ok in (("x", "x"), ("vel", "vel"), ("F_n", "F_n"), ("lambda", "lambda")):
                assert_close(st[k], P[ok], 1e-8, f"step {t} {k}")
            assert_close(st["Stress"], P["stress"], 1e-7, f"step {t} stress")
    assert S.status_flags() == 0
    moved = np.abs(M.coords().reshape(-1, ndim)[P["I0"]] - M.coords().reshape(-1, ndim)[I0_start]).max(axis=0)
    assert moved[ndim - 1] >= 4.0, "the block has to travel several cells"


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("ndim", [2, 3])
def test_mixed_materials(ndim, mode):
    """Three laws in one cloud (MatIdx selects the law per particle, Constitutive.c:28-258): mode 2 = the kernel
    compiled for run-time dispatch, mode 1 = one launch per law of the single-law kernels, each compacting its
    particles out of every tile list."""
    o = orc()
    n = nlps()
    vel = [0.0, -2.0] if ndim == 2 else [0.0, 0.0, -2.0]
    soft_nh = {"type": 0, "E": 2.0e4, "nu": 0.3}
    soft_hencky = {"type": 1, "E": 1.0e4, "nu": 0.25}
    case = small_case(ndim, material=DP, velocity=vel)
    case["materials"] = [soft_nh, soft_hencky, DP]
    npart = case["cloud"]["x"].shape[0]
    case["cloud"]["matidx"] = (np.arange(npart) % 3).astype(np.int32)
    nsteps = 8
    bcs_list = [dirichlet_plane(case, ndim - 1, 2, nsteps)]
    grav = [0.0] * (ndim - 1) + [-9.81]
    dt = 0.1 * case["h"] / np.sqrt(2.0e4 / 1000.0)
    M, P, prm, mats = oracle_setup(case)
    S = gpu_setup(case, nsteps=nsteps)
    S.set_law_launch_mode(mode)
    stepper = o.ExplicitStepper(P, M, mats, prm, o.BccSet(bcs_list), nsteps, gravity=grav)
    gb = n.BccSet(bcs_list)
    for t in range(nsteps):
        assert stepper.step(t, dt) == 0
        S.explicit_step(gb, t, dt, 0.5, grav)
    st = S.download_state()
    assert np.array_equal(st["I0"], P["I0"])
    for k, ok in (("x", "x"), ("vel", "vel"), ("F_n", "F_n"), ("Stress", "stress"), ("W", "W"), ("b_e_n", "b_e_n"),
                  ("Kappa_n", "kappa_n"), ("EPS_n", "eps_n"), ("rho", "rho")):
        assert_close(st[k], P[ok], 1e-9, f"mixed laws: {k}")
    for m in range(3):  # every law contributes a visible stress
        assert np.abs(P["stress"][case["cloud"]["matidx"] == m]).max() > 1.0
    # level-B constitutive stage with the same mixed cloud
    n2m, d2m, na = masks(S, M, bcs_list, 0, nsteps)
    rng = np.random.default_rng(3)
    dU = 5e-3 * rng.normal(size=na * ndim)
    assert o.compatibility(dU, None, P, M, n2m) == 0 and o.constitutive(P, mats, prm) == 0
    S.local_compatibility_conditions(dU)
    S.constitutive_update()
    st = S.download_state()
    for k, ok in (("F_n1", "F_n1"), ("Stress", "stress"), ("b_e_n1", "b_e_n1"), ("Kappa_n1", "kappa_n1")):
        assert_close(st[k], P[ok], 1e-9, f"mixed laws, level B: {k}")


@pytest.mark.parametrize("ndim", [2, 3])
def test_tangent_matrix_neo_hookean(ndim):
    """__jacobian_evaluation for Neo-Hookean particles.  The COO triplets of the device, summed
    into a dense matrix, against the oracle's restatement of the reference loop: values, the alpha_1*M diagonal,
    the Dirichlet identity rows and the sparsity pattern (integers: exact)."""
    o = orc()
    if ndim == 2:
        case = make_case(2, [12, 11], [3, 3], [5, 4], material=NH, velocity=[1.0, -2.0])
    else:
        case = make_case(3, [8, 8, 7], [3, 3, 2], [2, 2, 2], material=NH, velocity=[1.0, -2.0, 0.5])
    nsteps = 2
    bcs_list = [dirichlet_plane(case, ndim - 1, 3, nsteps)]
    M, P, prm, mats = oracle_setup(case)
    S = gpu_setup(case, nsteps=nsteps)
    n2m, d2m, na = masks(S, M, bcs_list, 1, nsteps)
    rng = np.random.default_rng(11)
    dU = 2e-2 * rng.normal(size=na * ndim)
    assert o.compatibility(dU, None, P, M, n2m) == 0 and o.constitutive(P, mats, prm) == 0
    S.local_compatibility_conditions(dU)
    S.constitutive_update()
    Mv = o.lumped_mass(P, M, n2m, na)
    ntot = na * ndim
    for alpha_1, mass, dirichlet in ((0.0, None, False), (4.0e4, Mv, True)):
        K_o, pat_o, st = o.tangent_matrix(P, M, mats, n2m, d2m if dirichlet else None, na, alpha_1, mass)
        assert st == 0
        rows, cols, vals = S.jacobian_evaluation(alpha_1, mass, dirichlet)
        assert rows.min() >= 0 and rows.max() < ntot and cols.min() >= 0 and cols.max() < ntot
        K_g = np.zeros((ntot, ntot))
        np.add.at(K_g, (rows, cols), vals)
        assert_close(K_g, K_o, 1e-10, f"tangent matrix (alpha_1={alpha_1}, dirichlet={dirichlet})")
        # every structurally visited entry is present exactly once
        key = rows.astype(np.int64) * ntot + cols
        assert np.unique(key).size == key.size
        assert np.array_equal(S.create_sparsity_pattern(), pat_o), "sparsity pattern"
        assert np.array_equal(np.bincount(rows, minlength=ntot), pat_o), "COO rows vs pattern"
        # triplets written into device arrays by the emit kernel itself: the same triplets, in the same order
        rd, cd, vd = S.jacobian_evaluation(alpha_1, mass, dirichlet, on_device=True)
        assert np.array_equal(rd.cpu().numpy(), rows) and np.array_equal(cd.cpu().numpy(), cols)
        assert_close(vd.cpu().numpy(), vals, 1e-12, "device-resident COO arrays", scale=np.abs(vals).max())
        # a Neo-Hookean cloud assembles the upper half of every row only and mirrors the rest: every pair assembled
        # gives the same triplets (sums in another order)
        S.debug_option("tangent_symmetric", 0)
        rows3, cols3, vals3 = S.jacobian_evaluation(alpha_1, mass, dirichlet)
        S.debug_option("tangent_symmetric", 1)
        assert np.array_equal(rows3, rows) and np.array_equal(cols3, cols)
        assert_close(vals3, vals, 1e-12, "every pair vs upper half + mirror", scale=np.abs(vals).max())
        # the one-wave-per-particle form gives the same matrix
        S.L.nlps_gpu_tangent_set_grouped(S.h, 0)
        rows2, cols2, vals2 = S.jacobian_evaluation(alpha_1, mass, dirichlet)
        S.L.nlps_gpu_tangent_set_grouped(S.h, 1)
        assert np.array_equal(rows2, rows) and np.array_equal(cols2, cols)
        assert_close(vals2, vals, 1e-12, "per-particle vs grouped assembly", scale=np.abs(vals).max())
    assert np.abs(K_o - K_o.T).max() <= 1e-12 * np.abs(K_o).max()


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("law", ["hencky", "drucker-prager"])
def test_tangent_matrix_spectral_laws(ndim, law):
    """The spectral stiffness densities of Hencky (Hencky.c:98-229) and of the elastoplastic laws
    (Elastoplastic-Tangent-Matrix.c:42-163, with the C_ep the Drucker-Prager update left behind), device vs the
    oracle's restatement.  Both divide stress differences by eigenvalue differences of b, so the tolerance is 1e-8
    of the largest entry instead of 1e-10; the reference's formula is not the exact derivative of the internal
    force (checked against finite differences: 2-8 % off at 2 % strain), it is reproduced as it is."""
    o = orc()
    mat = HENCKY if law == "hencky" else DP
    if ndim == 2:
        case = make_case(2, [12, 11], [3, 3], [5, 4], material=mat, velocity=[1.0, -2.0])
    else:
        case = make_case(3, [8, 8, 7], [3, 3, 2], [2, 2, 2], material=mat, velocity=[1.0, -2.0, 0.5])
    nsteps = 2
    bcs_list = [dirichlet_plane(case, ndim - 1, 3, nsteps)]
    M, P, prm, mats = oracle_setup(case)
    S = gpu_setup(case, nsteps=nsteps)
    n2m, d2m, na = masks(S, M, bcs_list, 1, nsteps)
    rng = np.random.default_rng(13)
    dU = (2e-2 if law == "hencky" else 8e-3) * rng.normal(size=na * ndim)
    assert o.compatibility(dU, None, P, M, n2m) == 0 and o.constitutive(P, mats, prm) == 0
    S.local_compatibility_conditions(dU)
    S.constitutive_update()
    if law != "hencky":
        assert (P["eps_n1"] > P["eps_n"]).sum() > 0, "some particles must be plastic"
    Mv = o.lumped_mass(P, M, n2m, na)
    ntot = na * ndim
    K_o, pat_o, st = o.tangent_matrix(P, M, mats, n2m, d2m, na, 2.0e3, Mv)
    assert st == 0
    rows, cols, vals = S.jacobian_evaluation(2.0e3, Mv, True)
    K_g = np.zeros((ntot, ntot))
    np.add.at(K_g, (rows, cols), vals)
    assert_close(K_g, K_o, 1e-8, f"{law} tangent matrix")
    assert np.array_equal(S.create_sparsity_pattern(), pat_o)
    # a physical re-sort (all particle fields gathered into the twin block, level-B ones included) followed by the
    # local search it asks for: the level-B state (C_ep, b_e, stress) has to come through
    S.resort()
    S.local_search()
    assert o.local_search(P, M, prm) == 0
    n2m, d2m, na2 = masks(S, M, bcs_list, 1, nsteps)
    assert na2 == na
    K_o2, _, st2 = o.tangent_matrix(P, M, mats, n2m, d2m, na, 2.0e3, Mv)
    assert st2 == 0
    rows2, cols2, vals2 = S.jacobian_evaluation(2.0e3, Mv, True)
    K_r = np.zeros((ntot, ntot))
    np.add.at(K_r, (rows2, cols2), vals2)
    assert_close(K_r, K_o2, 1e-8, f"{law} tangent matrix after a re-sort")
    if law != "hencky":
        assert_close(S.download_state()["C_ep"], P["C_ep"], 1e-9, "C_ep after a re-sort", scale=mat["E"])


class _OracleStages:
    def __init__(self, case, nsteps):
        self.o = orc()
        self.ndim, self.nsteps = case["ndim"], nsteps
        self.M, self.P, self.prm, self.mats = oracle_setup(case)

    def local_search(self):
        assert self.o.local_search(self.P, self.M, self.prm) == 0

    def masks(self, bcs, step):
        self.n2m, self.na = self.o.active_nodes(self.M)
        self.d2m, _ = self.o.active_dofs(self.n2m, self.na, self.ndim, self.o.BccSet(bcs), step, self.nsteps)
        return self.n2m, self.d2m, self.na

    def lumped_mass(self):
        return self.o.lumped_mass(self.P, self.M, self.n2m, self.na)

    def nodal_field_n(self, Mv):
        return self.o.nodal_field_n(Mv, self.P, self.M, self.n2m, self.d2m, self.na)

    def compatibility(self, dU, dU_dt):
        assert self.o.compatibility(dU, dU_dt, self.P, self.M, self.n2m) == 0

    def constitutive(self):
        assert self.o.constitutive(self.P, self.mats, self.prm) == 0

    def internal_forces(self):
        R, st = self.o.internal_forces(self.P, self.M, self.n2m, self.d2m, self.na)
        assert st == 0
        return R

    def tangent(self, alpha_1, Mv):
        K, _, st = self.o.tangent_matrix(self.P, self.M, self.mats, self.n2m, self.d2m, self.na, alpha_1, Mv,
                                         with_pattern=False)
        assert st == 0
        return K

    def roll(self):
        self.o.roll_state(self.P)

    def update_kinetics(self, dU, Un_dt, dU_dt, dU_dt2):
        self.o.update_kinetics(1.0, dU, Un_dt, dU_dt, dU_dt2, self.P, self.M, self.n2m)


class _DeviceStages:
    def __init__(self, case, nsteps):
        self.n = nlps()
        self.ndim = case["ndim"]
        self.S = gpu_setup(case, nsteps=nsteps)

    def local_search(self):
        self.S.local_search()

    def masks(self, bcs, step):
        n2m, d2m = self.S.active_masks(self.n.BccSet(bcs), step)
        return n2m, d2m, self.S.nactive

    def lumped_mass(self):
        return self.S.compute_nodal_lumped_mass()

    def nodal_field_n(self, Mv):
        return self.S.get_nodal_field_n(Mv)

    def compatibility(self, dU, dU_dt):
        self.S.local_compatibility_conditions(dU, dU_dt)

    def constitutive(self):
        self.S.constitutive_update()

    def internal_forces(self):
        return self.S.nodal_internal_forces(np.zeros(self.S.nactive * self.ndim))

    def form_initial_guess(self, Un_dt, Un_dt2, dt, bcs, step):
        return self.S.form_initial_guess(Un_dt, Un_dt2, dt, self.n.BccSet(bcs), step)

    def kinetic_increments(self, dU, Un_dt, Un_dt2, alpha):
        return self.S.compute_nodal_kinetic_increments(dU, Un_dt, Un_dt2, alpha)

    def inertial_forces(self, R, M, dU, Un_dt, Un_dt2, alpha, gravity):
        return self.S.nodal_inertial_forces(R, M, dU, Un_dt, Un_dt2, alpha, gravity)

    def tangent(self, alpha_1, Mv):
        rows, cols, vals = self.S.jacobian_evaluation(alpha_1, Mv, True)
        ntot = self.S.nactive * self.ndim
        K = np.zeros((ntot, ntot))
        np.add.at(K, (rows, cols), vals)
        return K

    def roll(self):
        self.S.update_particles_internal_variables()

    def update_kinetics(self, dU, Un_dt, dU_dt, dU_dt2):
        self.S.update_particles_kinetics_FLIP_PIC(1.0, dU, Un_dt, dU_dt, dU_dt2)


@pytest.mark.parametrize("ndim", [2, 3])
def test_implicit_newmark_steps_with_device_stages(ndim):
    """The maintained driver's time step (U_Newmark_Beta, U-Newmark-beta.c:192-409) composed from the level-B
    stage calls, the device versions of the per-dof updates (a21: initial guess with Dirichlet values, kinetic
    increments, inertial forces; the oracle side uses the numpy restatement in tests/newmark.py) and the device tangent, three steps with gravity and a fixed floor, against the same host algebra
    (tests/newmark.py) over the oracle.  The Newton iteration must converge quadratically with the device
    tangent, take the same number of iterations and leave the same particles behind."""
    from newmark import newmark_step
    soft = {"type": 0, "E": 2.0e5, "nu": 0.3}
    if ndim == 2:
        case = make_case(2, [12, 11], [3, 3], [5, 4], material=soft, velocity=[0.5, -1.0])
    else:
        case = make_case(3, [8, 8, 7], [3, 3, 2], [2, 2, 2], material=soft, velocity=[0.5, 0.2, -1.0])
    nsteps = 3
    bcs_list = [dirichlet_plane(case, ndim - 1, 3 if ndim == 2 else 2, nsteps)]
    grav = [0.0] * (ndim - 1) + [-9.81]
    dt = 2.0e-2  # 2.8 x the explicit CFL limit h / c: only an implicit step is stable here
    A, B = _OracleStages(case, nsteps), _DeviceStages(case, nsteps)
    for step in range(nsteps):
        dU_o, hist_o = newmark_step(A, ndim, bcs_list, step, nsteps, dt, grav)
        dU_g, hist_g = newmark_step(B, ndim, bcs_list, step, nsteps, dt, grav)
        assert len(hist_o) == len(hist_g) and 2 <= len(hist_g) <= 8, (hist_o, hist_g)
        assert hist_g[-1] <= 1e-10 * max(1.0, hist_g[0]), hist_g
        if len(hist_g) >= 4:  # quadratic tail: the device tangent is the true Jacobian
            assert hist_g[-1] <= 1e-3 * hist_g[-2], hist_g
        assert_close(dU_g, dU_o, 1e-8, f"step {step}: converged dU")
    st = B.S.download_state()
    for k, ok in (("x", "x"), ("vel", "vel"), ("acc", "acc"), ("F_n", "F_n"), ("Stress", "stress"), ("J_n", "J_n")):
        assert_close(st[k], A.P[ok], 1e-8, f"after implicit steps: {k}")
    assert np.abs(A.P["stress"]).max() > 10.0


@pytest.mark.parametrize("nexplicit", [1, 2, 3])
def test_stage_calls_after_explicit_steps(nexplicit):
    """The explicit step rolls F and b_e by renaming their n/n+1 slots; a level-B stage or a download right after an
    odd or even number of such steps must still see the reference's copy semantics (n+1 == n after the roll)."""
    o = orc()
    n = nlps()
    case = small_case(3, material=DP, velocity=[0.0, 0.0, -0.2])
    nsteps = 4
    bcs_list = [dirichlet_plane(case, 2, 2, nsteps)]
    M, P, prm, mats = oracle_setup(case)
    S = gpu_setup(case, nsteps=nsteps)
    stepper = o.ExplicitStepper(P, M, mats, prm, o.BccSet(bcs_list), nsteps, gravity=[0.0, 0.0, -9.81])
    gb = n.BccSet(bcs_list)
    dt = 0.1 * case["h"] / np.sqrt(DP["E"] / 1000.0)
    for t in range(nexplicit):
        assert stepper.step(t, dt) == 0
        S.explicit_step(gb, t, dt, 0.5, [0.0, 0.0, -9.81])
    st = S.download_state()
    for k in ("F_n", "b_e_n"):
        assert_close(st[k], P[k], 1e-10, f"{k} after {nexplicit} explicit steps")
        assert np.array_equal(st[k + "1"], st[k]), f"{k}1 must equal {k} after the roll"
    # level-B stages on top of that state
    assert o.local_search(P, M, prm) == 0
    S.local_search()
    n2m, d2m, na = masks(S, M, bcs_list, nexplicit, nsteps)
    rng = np.random.default_rng(5)
    dU = 2e-3 * rng.normal(size=na * 3)
    assert o.compatibility(dU, None, P, M, n2m) == 0 and o.constitutive(P, mats, prm) == 0
    S.local_compatibility_conditions(dU)
    S.constitutive_update()
    R_o, s = o.internal_forces(P, M, n2m, d2m, na)
    R_g = S.nodal_internal_forces(np.zeros(na * 3))
    assert_close(R_g, R_o, 1e-10, "internal forces after explicit steps")
    st = S.download_state()
    for k, ok in (("F_n1", "F_n1"), ("b_e_n1", "b_e_n1"), ("Stress", "stress"), ("F_n", "F_n"), ("b_e_n", "b_e_n")):
        assert_close(st[k], P[ok], 1e-10, f"{k} after level-B stages on top of {nexplicit} explicit steps")
    # and the explicit scheme continues from there
    o.roll_state(P)
    S.update_particles_internal_variables()
    assert stepper.step(nexplicit, dt) == 0
    S.explicit_step(gb, nexplicit, dt, 0.5, [0.0, 0.0, -9.81])
    st = S.download_state()
    for k, ok in (("x", "x"), ("F_n", "F_n"), ("b_e_n", "b_e_n"), ("Stress", "stress")):
        assert_close(st[k], P[ok], 1e-9, f"{k} after continuing explicitly")


@pytest.mark.parametrize("ndim", [2, 3])
def test_von_mises_law(ndim):
    """SURVEY §8f n4, first item: Von-Mises plasticity (Von-Mises.c:212-392) behind the same switch.  Level-B
    stages (stress, b_e, eps-bar, in-place back stress, C_ep, internal forces, tangent) and fused explicit steps
    against the oracle, with a pre-loaded back stress and enough strain that most particles yield."""
    o = orc()
    n = nlps()
    rng = np.random.default_rng(21)
    vel = [0.0, -0.4] if ndim == 2 else [0.0, 0.0, -0.4]
    case = small_case(ndim, material=VM, velocity=vel)
    npart = case["cloud"]["x"].shape[0]
    back0 = rng.normal(size=(npart, 3))
    back0 -= back0.mean(axis=1, keepdims=True)
    case["cloud"]["back_stress"] = back0.copy()
    nsteps = 6
    bcs_list = [dirichlet_plane(case, ndim - 1, 2, nsteps)]
    M, P, prm, mats = oracle_setup(case)
    S = gpu_setup(case, nsteps=nsteps)
    n2m, d2m, na = masks(S, M, bcs_list, 0, nsteps)
    dU = 1.5e-2 * rng.normal(size=na * ndim)
    assert o.compatibility(dU, None, P, M, n2m) == 0 and o.constitutive(P, mats, prm) == 0
    S.local_compatibility_conditions(dU)
    S.constitutive_update()
    assert (P["eps_n1"] > 0).sum() > npart // 2, "most particles must yield"
    st = S.download_state()
    for k, ok in (("Stress", "stress"), ("W", "W"), ("b_e_n1", "b_e_n1"), ("EPS_n1", "eps_n1"), ("C_ep", "C_ep"),
                  ("Back_stress", "back_stress")):
        assert_close(st[k], P[ok], 1e-10, f"Von-Mises {k}")
    R_o, s = o.internal_forces(P, M, n2m, d2m, na)
    assert_close(S.nodal_internal_forces(np.zeros(na * ndim)), R_o, 1e-10, "internal forces")
    K_o, pat_o, stt = o.tangent_matrix(P, M, mats, n2m, d2m, na)
    assert stt == 0
    rows, cols, vals = S.jacobian_evaluation(0.0, None, True)
    K_g = np.zeros_like(K_o)
    np.add.at(K_g, (rows, cols), vals)
    assert_close(K_g, K_o, 1e-8, "Von-Mises tangent matrix")
    # fused explicit steps from the initial state.  The back stress starts at zero here: upstream stores it per
    # principal direction of the CURRENT trial state, so with F = I (degenerate eigenvalues) a pre-loaded back
    # stress would be assigned to directions by the eigen-solver's tie-breaking, which no second solver shares.
    case["cloud"]["back_stress"] = np.zeros((npart, 3))
    M, P, prm, mats = oracle_setup(case)
    S = gpu_setup(case, nsteps=nsteps)
    stepper = o.ExplicitStepper(P, M, mats, prm, o.BccSet(bcs_list), nsteps, gravity=[0.0] * (ndim - 1) + [-9.81])
    gb = n.BccSet(bcs_list)
    dt = 0.1 * case["h"] / np.sqrt(VM["E"] / 1000.0)
    for t in range(nsteps):
        assert stepper.step(t, dt) == 0
        S.explicit_step(gb, t, dt, 0.5, [0.0] * (ndim - 1) + [-9.81])
    st = S.download_state()
    assert np.array_equal(st["I0"], P["I0"])
    for k, ok in (("x", "x"), ("vel", "vel"), ("F_n", "F_n"), ("Stress", "stress"), ("b_e_n", "b_e_n"), ("EPS_n", "eps_n"),
                  ("Back_stress", "back_stress"), ("rho", "rho")):
        assert_close(st[k], P[ok], 1e-9, f"Von-Mises explicit steps: {k}")
    assert (P["eps_n"] > 0).sum() > 0 and np.abs(P["back_stress"]).max() > 0


def test_device_pointer_nodal_vectors():
    """Nodal Vec arrays may live on the device (torch tensors) as well as on the host."""
    import torch
    o = orc()
    case = small_case(3, velocity=[1.0, 2.0, 3.0])
    M, P, prm, mats = oracle_setup(case)
    S = gpu_setup(case)
    n2m, d2m, na = masks(S, M, [], 0, 1)
    Mt = torch.zeros(na * 3, dtype=torch.float64, device="cuda")
    S.compute_nodal_lumped_mass(out=Mt)
    Mh = S.compute_nodal_lumped_mass()
    torch.cuda.synchronize()
    assert np.array_equal(Mt.cpu().numpy() > 0, Mh > 0)
    assert_close(Mt.cpu().numpy(), Mh, 1e-12, "device vs host output")


def test_failure_is_reported_not_fatal():
    """< d+1 neighbours => EXIT_FAILURE + message (the reference exit()s, LME.c:1087-1092)."""
    n = nlps()
    case = small_case(2)
    # cut-off radius ~ 0 from the second search on (beta = 0 at initialisation => Ra = +inf)
    S = n.Solver(2, case["grid_n"], case["origin"], case["h"], case["cloud"], case["materials"],
                 params=n.Params(3.0, 1.0 - 1e-9, 1e-10, 10, 1e-14, 10))
    S.initialise_shapefun()
    with pytest.raises(n.NlpsError):
        S.local_search()
    assert S.status_flags() & 2


@pytest.mark.parametrize("ndim", [3])
def test_full_size_properties(ndim):
    """BASELINE configs[1] size (1 M particles, 3-D): size-independent properties only."""
    n = nlps()
    case = make_case(3, [60, 60, 60], [5, 5, 5], [50, 50, 50], velocity=[0.0, 0.0, -10.0])
    S = gpu_setup(case, nsteps=4)
    assert S.np == 1_000_000
    gb = n.BccSet([dirichlet_plane(case, 2, 0, 4)])
    cloud = case["cloud"]
    dt = 1e-3
    mass0 = cloud["mass"].sum()
    for t in range(2):
        S.explicit_step(gb, t, dt, 0.5, None)
        nod = S.explicit_nodal()
        # mass conservation: sum_A M_A = sum_p m_p  (partition of unity of the LME basis)
        assert abs(nod["mass"].reshape(-1, 3)[:, 0].sum() / mass0 - 1.0) < 1e-12
        # momentum conservation of the dD projection: sum_A M_A dU_A = sum_p m_p dD_p
        mom_nodes = (nod["mass"] * nod["dU"]).reshape(-1, 3).sum(0)
        v = np.array([0.0, 0.0, -10.0]) if t == 0 else None
        if v is not None:
            assert_close(mom_nodes, mass0 * v * dt, 1e-10, "momentum of dD projection")
        # Newton's third law: internal forces sum to zero
        f = nod["force"].reshape(-1, 3).sum(0)
        assert np.all(np.abs(f) <= 1e-9 * np.abs(nod["force"]).max() * np.sqrt(f.size) + 1e-9)
    st = S.download_state()
    assert np.all(st["J_n"] > 0)
    assert np.allclose(st["Stress"][:, [1, 2, 5]], st["Stress"][:, [3, 6, 7]], rtol=0, atol=1e-6 * np.abs(st["Stress"]).max())
    nn, _ = S.download_lists()
    assert nn.min() >= 4 and nn.max() <= 125
    assert S.status_flags() == 0


def test_long_run_conservation_and_binning():
    """Soak: 125 k particles of a soft block, thrown and spinning, 300 steps with a device re-sort every 25.
    No external force, no Dirichlet node in reach: the particle momentum sum m v is conserved by the scheme (P2G
    partition of unity + internal forces summing to zero), J stays positive, every particle keeps a full
    neighbourhood and the device's own order stays consistent (ids come back exactly once)."""
    n = nlps()
    soft = {"type": 0, "E": 4.0e5, "nu": 0.3}  # celerity 20
    case = make_case(3, [62, 62, 62], [18, 18, 18], [25, 25, 25], material=soft, velocity=[3.0, -2.0, 4.0])
    cloud = case["cloud"]
    xc = cloud["x"].mean(axis=0)
    rel = cloud["x"] - xc
    cloud["vel"][:, 0] += -0.25 * rel[:, 1]      # spin about z
    cloud["vel"][:, 1] += 0.25 * rel[:, 0]
    nsteps = 300
    npart = cloud["x"].shape[0]
    assert npart == 125000
    S = gpu_setup(case, nsteps=1)
    S.set_resort_interval(25)
    gb = n.BccSet([])
    dt = 0.2 * case["h"] / 25.0
    m = cloud["mass"][:, None]
    p0 = (m * cloud["vel"]).sum(axis=0)
    for t in range(nsteps):
        S.explicit_step(gb, 0, dt)
        if t % 100 == 99:
            assert S.status_flags() == 0, f"step {t}: flags {S.status_flags():x}"
    st = S.download_state()
    assert S.status_flags() == 0
    p1 = (m * st["vel"]).sum(axis=0)
    assert np.abs(p1 - p0).max() <= 1e-9 * np.abs(m * cloud["vel"]).sum(), (p0, p1)
    assert np.all(st["J_n"] > 0.5) and np.all(st["J_n"] < 2.0) and np.isfinite(st["Stress"]).all()
    travelled = np.abs(st["x"].mean(axis=0) - xc)
    assert np.all(travelled > 1.0), travelled            # the block moved through several cells ...
    assert np.abs(st["x"] - cloud["x"]).max() > 2.0       # ... and turned
    nn, _ = S.download_lists()
    assert nn.min() >= 20 and nn.max() <= 125
    ids = S.download_ids()
    assert np.array_equal(ids, np.arange(npart))
    assert np.abs(st["rho"] * st["J_n"] * cloud["vol0"] - cloud["mass"]).max() <= 1e-9 * cloud["mass"].max()


def test_halo_callback_and_rccl_on_library_memory():
    """The multi-GPU hook on one GPU: the library hands its nodal arrays (raw device pointers) to the
    halo callback; they are wrapped as torch tensors without a copy and go through RCCL (world size 1
    all-reduce and a self send/recv-free path).  Guards the plumbing bench.py uses for N > 1."""
    import importlib
    import os
    import torch
    import torch.distributed as dist
    n = nlps()
    halo_mod = importlib.import_module("nl-partsol_amd.halo")
    case = small_case(3, velocity=[0.0, 0.0, -10.0])
    stream = torch.cuda.current_stream().cuda_stream
    S = gpu_setup(case, nsteps=3, stream=stream)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(free_port()))
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    seen = []
    gn = case["grid_n"]
    nnodes = gn[0] * gn[1] * gn[2]

    def exchange(dptr, nfield, elem, kind):
        t = halo_mod.device_tensor(torch, dptr, nnodes * nfield, elem)
        before = t.double().sum().item()
        dist.all_reduce(t, op=dist.ReduceOp.SUM if kind == 0 else dist.ReduceOp.MAX)
        after = t.double().sum().item()
        assert before == after
        seen.append((nfield, elem, kind, before))
        return 0

    S.set_halo_exchange(exchange)
    gb = n.BccSet([dirichlet_plane(case, 2, 2, 3)])
    S.explicit_step(gb, 0, 1e-3)
    S.synchronize()
    kinds = [(a, b, c) for a, b, c, _ in seen]
    assert kinds == [(1, 1, 1), (4, 8, 0), (3, 8, 0)], kinds
    # the mass+momentum array the callback saw sums to the particle mass
    mass_total = case["cloud"]["mass"].sum()
    nod = S.explicit_nodal()
    assert abs(nod["mass"].reshape(-1, 3)[:, 0].sum() / mass_total - 1) < 1e-12
    assert seen[0][3] > 0 and S.status_flags() == 0
    # same step without the hook gives the same state
    S2 = gpu_setup(case, nsteps=3)
    S2.explicit_step(gb, 0, 1e-3)
    a, b = S.download_state(), S2.download_state()
    assert_close(a["x"], b["x"], 1e-13, "x with/without halo hook")
    # two-phase form: every exchange is an RCCL all-reduce on a side stream, started behind the boundary tiles and
    # waited for before they need it (ghost bands inside the cloud make both tile classes non-empty)
    S3 = gpu_setup(case, nsteps=3, stream=stream)
    side = torch.cuda.Stream()
    pending, phases = {}, []

    def exchange2(dptr, nfield, elem, kind, phase):
        phases.append(phase)
        t = halo_mod.device_tensor(torch, dptr, nnodes * nfield, elem)
        if phase == 1:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                dist.all_reduce(t, op=dist.ReduceOp.SUM if kind == 0 else dist.ReduceOp.MAX)
                ev = torch.cuda.Event()
                ev.record(side)
            pending[(dptr, kind)] = ev
        elif phase == 2:
            torch.cuda.current_stream().wait_event(pending.pop((dptr, kind)))
        else:
            dist.all_reduce(t, op=dist.ReduceOp.SUM if kind == 0 else dist.ReduceOp.MAX)
        return 0

    S3.set_halo_exchange(exchange2)
    lo, hi = S3.touched_layers()
    S3.set_ghost_bands(lo + 4, hi - 4, True)
    for t in range(3):
        S3.explicit_step(gb, t, 1e-3)
        S2.explicit_step(gb, t, 1e-3) if t > 0 else None
    S3.synchronize()
    assert phases[:6] == [1, 2, 1, 2, 1, 2] and not pending and S3.status_flags() == 0
    c, b = S3.download_state(), S2.download_state()
    for k in ("x", "vel", "Stress", "F_n"):
        assert_close(c[k], b[k], 1e-12, f"{k}: overlapped exchanges vs none")
    assert np.array_equal(c["I0"], b["I0"])
    if created:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,overlap,ndim", [(2, 1, 3), (3, 1, 3), (3, 0, 3), (3, 1, 2)])
def test_multirank_on_one_gpu(world, overlap, ndim):
    """N > 1 rehearsal on the one card of the test box: `world` processes, each with its slab, the halo
    callback (with and without overlapping the exchanges with the interior tiles), the node window and periodic
    re-sorts, against one solver holding the whole cloud
    (tests/mr_gpu_worker.py; gloo with host staging stands in for RCCL, which needs one GPU per rank)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = free_port()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(root, "tests", "mr_gpu_worker.py")]
    env = dict(os.environ, NLPS_OVERLAP=str(overlap), NLPS_NDIM=str(ndim))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert r.returncode == 0 and "MULTIRANK_GPU_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_migration_select_commit_round_trip():
    """One rank: the particles above a layer are selected and packed, then handed straight back as immigrants.
    Nothing may change (matched by global id), capacity is respected, and stepping on is identical to a solver
    that never migrated."""
    n = nlps()
    case = small_case(3, velocity=[1.0, 0.5, -10.0], material=DP)
    nsteps = 6
    gb = n.BccSet([dirichlet_plane(case, 2, 2, nsteps)])
    A, B = gpu_setup(case, nsteps=nsteps), gpu_setup(case, nsteps=nsteps)
    npart = case["cloud"]["x"].shape[0]
    ids = (np.arange(npart) * 7 + 3).astype(np.int32)  # arbitrary distinct global ids
    A.set_particle_ids(ids)
    B.set_particle_ids(ids)
    for t in range(3):
        A.explicit_step(gb, t, 2e-3)
        B.explicit_step(gb, t, 2e-3)
    cut = int(np.median(case["cloud"]["x"][:, 2]))
    n_down, n_up, rw, dptr_down, dptr_up = A.migration_select(0, cut)
    assert n_down == 0 and 0 < n_up < npart and rw > 100
    A.migration_commit(dptr_up, n_up, 0, 0)       # they come straight back
    assert A.num_particles() == npart
    for t in range(3, nsteps):
        A.explicit_step(gb, t, 2e-3)
        B.explicit_step(gb, t, 2e-3)
    a, b = A.download_state(), B.download_state()
    ia, ib = A.download_ids(), B.download_ids()
    assert np.array_equal(ia, np.sort(ids)) and np.array_equal(np.sort(ib), np.sort(ids))
    order_b = np.argsort(ib)
    na, _ = A.download_lists()
    nb, _ = B.download_lists()
    assert np.array_equal(a["I0"], b["I0"][order_b]) and np.array_equal(na, nb[order_b])
    for k in ("x", "vel", "Stress", "F_n", "b_e_n", "Kappa_n", "lambda", "rho"):
        assert_close(a[k], b[k][order_b], 1e-12, f"{k} after select/commit round trip")
    # a real removal: they leave and nobody comes
    n_down, n_up, rw, _, _ = A.migration_select(0, cut)
    A.migration_commit(0, 0, 0, 0)
    assert A.num_particles() == npart - n_up and A.download_ids().size == npart - n_up
    A.explicit_step(gb, nsteps - 1, 2e-3)
    assert A.status_flags() == 0
    # capacity: more immigrants than reserved at create is an error, not a crash
    big = np.zeros(5000 * rw)
    A.migration_select(0, 10 ** 6)
    with pytest.raises(n.NlpsError):
        A.migration_commit(big.ctypes.data, 5000, 0, 0)


@pytest.mark.parametrize("world", [2, 3])
def test_migration_between_ranks_on_one_gpu(world):
    """a block flying along the slab axis changes owner; halo exchange + migration every 4 steps against
    one solver holding everything (tests/mr_gpu_migrate_worker.py)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = free_port()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "tests", "mr_gpu_migrate_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0 and "MIGRATION_GPU_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("scaling", ["weak", "strong"])
def test_bench_multi_rank_path_rehearsal(scaling):
    """bench.py --gpus 2 end to end (slab clouds, shared stream, halo callback with overlap, node window, ghost
    bands, barrier + max-over-ranks timing, JSON line) with two ranks on the one card of the test box; gloo stands
    in for RCCL (NLPS_BENCH_BACKEND), the real launch is the driver's on an 8-GPU node.  strong: ONE cube of 17^3 cells
    split into slabs of 9 and 8 layers (the uneven split of 100 layers over 8 ranks in small)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = free_port()
    extra = ["--cells", "16", "--particles-total", str(8 * 17 ** 3)] + ([] if scaling == "weak" else ["--scaling", "strong"])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4",
           "--warmup", "2", "--full", "--no-cpu-baseline"] + extra
    env = dict(os.environ, NLPS_BENCH_BACKEND="gloo", NLPS_BENCH_DEVICE="0")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 2 and out["scaling"] == scaling and out["value"] > 0
    assert out["config"]["particles_total"] == (2 * 16 ** 3 * 8 if scaling == "weak" else 8 * 17 ** 3)
    # (a) the partitioned-vs-whole check ran over the communicator of the run, before anything was timed
    chk = out["partition_check"]
    assert chk["index_maps_equal"] and chk["max_rel_err"] < 1e-10 and chk["status_flags"] == 0 and chk["particles"] == 2 * 8 ** 3 * 8
    # (b) the overlap form that survived the warm-up is recorded (the gloo stand-in has no single-launch form: 1)
    assert out["config"]["halo_overlap_mode"] == 1 and out["config"]["overlap_forms_tried"][-1]["ok"]
    assert out["config"]["halo_impl"] == "torch" and out["config"]["rccl_nranks"] is None
    # (c) per-rank kernel times and the time the step waited for its exchanges
    rows = out[scaling]["per_rank_kernel_ms"]
    assert len(rows) == 2 and all(r["lists+newton+p2g_mass_mom"] > 0 and r["exchange_wait"] >= 0 for r in rows)
    # (d) the weak AND the strong record in the one line (north_star: strong scaling at 8 M, here --particles-total)
    assert out["weak"]["scaling"] == "weak" and out["strong"]["scaling"] == "strong"
    assert out["weak"]["value"] > 0 and out["strong"]["value"] > 0
    assert out[scaling]["value"] == out["value"] and out[scaling]["ms_per_step"] == out["ms_per_step"]


@pytest.mark.parametrize("ndim", [2, 3])
def test_node_window(ndim):
    """nlps_gpu_set_node_window limits the per-step nodal work to the layers a rank can touch: the same
    steps with a tight window and with the whole grid agree with the oracle and with each other, indices
    bit for bit; a window the particles do not fit in raises status flag 16 instead of corrupting memory."""
    o = orc()
    n = nlps()
    vel = [2.0, -10.0] if ndim == 2 else [2.0, 1.0, -10.0]
    if ndim == 2:
        case = make_case(2, [14, 40], [3, 20], [7, 8], velocity=vel)
    else:
        case = make_case(3, [11, 10, 30], [3, 3, 14], [5, 4, 6], velocity=vel)
    nsteps = 4
    # one Dirichlet plane through the cloud (real deformation) and one outside the window (must be ignored)
    bcs_list = [dirichlet_plane(case, ndim - 1, 21 if ndim == 2 else 15, nsteps),
                dirichlet_plane(case, ndim - 1, 0, nsteps)]
    dt = 0.4 * case["h"] / 100.0
    M, P, prm, mats = oracle_setup(case)
    stepper = o.ExplicitStepper(P, M, mats, prm, o.BccSet(bcs_list), nsteps)
    gb = n.BccSet(bcs_list)
    S = gpu_setup(case, init=False, nsteps=nsteps)
    lo, hi = S.touched_layers()
    assert lo > 0 and hi < case["grid_n"][ndim - 1] - 1
    S.set_node_window(lo, hi)
    S.initialise_shapefun()
    Sf = gpu_setup(case, nsteps=nsteps)
    for t in range(nsteps):
        assert stepper.step(t, dt) == 0
        S.explicit_step(gb, t, dt)
        Sf.explicit_step(gb, t, dt)
    assert S.status_flags() == 0
    a, b = S.download_state(), Sf.download_state()
    assert np.array_equal(a["I0"], P["I0"]) and np.array_equal(a["I0"], b["I0"])
    nn, lst = S.download_lists()
    assert np.array_equal(nn, P["nn"]) and lists_equal(nn, lst, P["list"])
    assert np.array_equal(S.download_active(), M.active())
    for k, ok in (("x", "x"), ("vel", "vel"), ("Stress", "stress"), ("F_n", "F_n")):
        assert_close(a[k], P[ok], 1e-9, f"{k} with node window")
        assert_close(a[k], b[k], 1e-12, f"{k} window vs whole grid")
    na = S.explicit_nodal()
    nb = Sf.explicit_nodal()
    assert S.nactive == Sf.nactive
    assert_close(na["mass"], nb["mass"], 1e-12, "nodal mass window vs whole grid")
    # a window that cuts into the cloud: flagged, and the step still terminates
    S3 = gpu_setup(case, init=False, nsteps=nsteps)
    S3.set_node_window(lo + 4, hi)
    try:
        S3.initialise_shapefun()
        S3.explicit_step(gb, 0, dt)
    except n.NlpsError:
        pass
    assert S3.status_flags() & 16


def test_caller_provided_nonblocking_stream():
    """The handle may run on a stream the caller owns.  torch streams are NON-BLOCKING: nothing orders them with
    the default stream, so an upload that went through the default stream must be complete (and not be wiped by a
    late allocation memset) before the first kernel runs.  Same steps on such a stream and on the library's own
    stream, with a shuffled upload, two materials, uploaded I0/lambda and re-sorts: identical state."""
    import torch
    n = nlps()
    case = small_case(3, velocity=[1.0, 0.5, -10.0])
    rng = np.random.default_rng(4)
    npart = case["cloud"]["x"].shape[0]
    perm = rng.permutation(npart)
    for k, v in list(case["cloud"].items()):
        if isinstance(v, np.ndarray) and v.shape[:1] == (npart,):
            case["cloud"][k] = np.ascontiguousarray(v[perm])
    case["materials"] = [NH, HENCKY]
    case["cloud"]["matidx"] = (np.arange(npart) % 2).astype(np.int32)
    nsteps = 6
    gb = n.BccSet([dirichlet_plane(case, 2, 2, nsteps)])
    out = {}
    prev = torch.cuda.current_stream()
    for kind in ("own", "caller"):
        ts = torch.cuda.Stream()
        if kind == "caller":
            torch.cuda.set_stream(ts)
        S = gpu_setup(case, nsteps=nsteps, stream=ts.cuda_stream if kind == "caller" else None)
        S.set_resort_interval(2)
        for t in range(nsteps):
            S.explicit_step(gb, t, 2e-3)
        out[kind] = (S.download_state(), S.download_lists())
        assert S.status_flags() == 0
        S.close()
    torch.cuda.set_stream(prev)
    (a, (na, la)), (b, (nb, lb)) = out["own"], out["caller"]
    assert np.array_equal(a["I0"], b["I0"]) and np.array_equal(na, nb) and lists_equal(na, la, lb)
    for k in ("x", "vel", "Stress", "F_n", "lambda"):
        assert_close(b[k], a[k], 1e-12, f"{k}: caller's stream vs own stream")
    assert np.abs(a["Stress"]).max() > 1.0


@pytest.mark.parametrize("ndim", [2, 3])
def test_shuffled_upload_and_periodic_resort(ndim):
    """Caller's particle order is arbitrary (shuffled here); the device keeps its own tile-major order,
    re-sorts physically every 2 steps, and every download comes back in the caller's order."""
    o = orc()
    n = nlps()
    vel = [3.0, -10.0] if ndim == 2 else [3.0, 2.0, -10.0]
    case = small_case(ndim, velocity=vel)
    rng = np.random.default_rng(17)
    perm = rng.permutation(case["cloud"]["x"].shape[0])
    for k, v in list(case["cloud"].items()):
        if isinstance(v, np.ndarray) and v.shape[:1] == (len(perm),):
            case["cloud"][k] = np.ascontiguousarray(v[perm])
    nsteps = 7
    bcs_list = [dirichlet_plane(case, ndim - 1, 2, nsteps)]
    dt = 0.4 * case["h"] / 100.0
    M, P, prm, mats = oracle_setup(case)
    S = gpu_setup(case, nsteps=nsteps)
    S.set_resort_interval(2)
    stepper = o.ExplicitStepper(P, M, mats, prm, o.BccSet(bcs_list), nsteps)
    gb = n.BccSet(bcs_list)
    for t in range(nsteps):
        assert stepper.step(t, dt) == 0
        S.explicit_step(gb, t, dt)
        if t == 3:
            S.resort()
    st = S.download_state()
    nn, lst = S.download_lists()
    assert np.array_equal(st["I0"], P["I0"]) and np.array_equal(nn, P["nn"]) and lists_equal(nn, lst, P["list"])
    for k, ok in (("x", "x"), ("vel", "vel"), ("Stress", "stress"), ("F_n", "F_n"), ("lambda", "lambda")):
        assert_close(st[k], P[ok], 1e-9, f"{k} after resorted steps")


def test_periodic_resort_keeps_particles_the_search_could_not_bin():
    """A particle the search flags instead of binning (here: closest node outside the rank's node window, status 16) is
    in no tile list; the periodic re-sort takes the lists as its permutation and must still move the WHOLE cloud: every
    particle comes back once, in the caller's order (the tail of the permutation used to be stale)."""
    n = nlps()
    case = small_case(3, velocity=[0.0, 0.0, -10.0])
    npart = case["cloud"]["x"].shape[0]
    case["cloud"]["mass"] = case["cloud"]["mass"] * (1.0 + 1e-3 * np.arange(npart))  # a tag that survives the steps
    nsteps = 6
    S = gpu_setup(case, nsteps=nsteps)
    st0 = S.download_state(fields=["x_GC", "mass"])
    z = st0["x_GC"][:, 2]
    layer_hi = int(np.floor(0.5 * (z.min() + z.max()) / case["h"]))
    S.set_node_window(0, layer_hi)  # the upper half of the cloud is outside from now on
    S.set_resort_interval(2)
    gb = n.BccSet([dirichlet_plane(case, 2, 2, nsteps)])
    for t in range(nsteps):
        S.explicit_step(gb, t, 1e-4)
    assert S.status_flags() & 16
    st = S.download_state(fields=["x_GC", "mass", "Vol_0"])
    assert np.array_equal(st["mass"], case["cloud"]["mass"]), "particles duplicated / dropped by the re-sort"
    assert np.array_equal(st["Vol_0"], case["cloud"]["vol0"])
    outside = z > (layer_hi - 1.0) * case["h"]  # closest node >= layer_hi - 1: the stencil reaches past the window
    assert outside.any() and not outside.all()
    assert np.array_equal(st["x_GC"][outside], st0["x_GC"][outside]), "a flagged particle is left out of the step"
    assert not np.array_equal(st["x_GC"][~outside], st0["x_GC"][~outside])
    S.close()


def test_periodic_resort_with_particles_flagged_by_the_search_ahead():
    """with the next step's search riding on K5, P.tile[] already belongs to the NEXT lists when a periodic
    re-sort takes the LAST lists as its permutation.  A cloud flying upwards through the top of its node window loses
    particles to status 16 in every step, also in the step right before a re-sort (listed then, flagged now) while others
    were flagged earlier (in no list): every particle must come back exactly once, in the caller's order."""
    n = nlps()
    case = small_case(3, velocity=[0.0, 0.0, 60.0])
    npart = case["cloud"]["x"].shape[0]
    case["cloud"]["mass"] = case["cloud"]["mass"] * (1.0 + 1e-3 * np.arange(npart))  # a tag that survives the steps
    nsteps = 7
    S = gpu_setup(case, nsteps=nsteps)
    z = case["cloud"]["x"][:, 2]
    layer_hi = int(np.floor(z.max() / case["h"])) + 2  # the whole cloud fits at the start ...
    S.set_node_window(0, layer_hi)
    S.set_resort_interval(2)
    S.set_adaptive_resort(0.0)
    gb = n.BccSet([])
    flagged = []
    for t in range(nsteps):  # ... and 0.3 cells per step carry its top layers out, a few more particles every step
        S.explicit_step(gb, t, 5e-3)
        st = S.download_state(fields=["mass", "x_GC"])
        assert np.array_equal(st["mass"], case["cloud"]["mass"]), f"step {t}: particles duplicated / dropped by the re-sort"
        flagged.append(int(np.count_nonzero(st["x_GC"][:, 2] > (layer_hi - 1.5) * case["h"])))
    assert S.status_flags() & 16
    assert flagged[-1] > flagged[1] > 0, flagged
    S.close()


def test_config1_2d_10k_parity():
    """BASELINE configs[0] shape (2-D, 10 000 particles, explicit) on the HIP path against the oracle;
    LME + Hencky stand in for uGIMP / linear-elastic (no runnable reference equivalent)."""
    o = orc()
    n = nlps()
    from util import synth
    case = make_case(2, [60, 60], [5, 5], [50, 50], material=HENCKY, velocity=[1.0, 0.0])
    nsteps = 3
    nodes = synth.plane_nodes(case["grid_n"], 0, 5)
    bc = [{"nodes": nodes, "dim": 2, "dir": np.ones((2, nsteps), dtype=np.int32), "value": np.zeros((2, nsteps))}]
    M, P, prm, mats = oracle_setup(case)
    S = gpu_setup(case, nsteps=nsteps)
    st = o.ExplicitStepper(P, M, mats, prm, o.BccSet(bc), nsteps)
    gb = n.BccSet(bc)
    for t in range(nsteps):
        assert st.step(t, 1e-3) == 0
        S.explicit_step(gb, t, 1e-3)
    d = S.download_state()
    assert np.array_equal(d["I0"], P["I0"])
    for k, ok in (("x", "x"), ("vel", "vel"), ("Stress", "stress"), ("F_n", "F_n"), ("W", "W")):
        assert_close(d[k], P[ok], 1e-9, "config1 " + k)


def test_config3_4m_neo_hookean_column_properties():
    """BASELINE configs[2]: 3-D Neo-Hookean column, 4 M particles (50x50x200 cells x 8), gravity, soft
    material (large-deformation F-update path).  Size-independent properties only."""
    n = nlps()
    case = make_case(3, [60, 60, 210], [5, 5, 5], [50, 50, 200], material={"type": 0, "E": 1.0e5, "nu": 0.3})
    S = gpu_setup(case, nsteps=3)
    assert S.np == 4_000_000
    gb = n.BccSet([dirichlet_plane(case, 2, 5, 3)])
    m0 = case["cloud"]["mass"].sum()
    dt = 0.1 / 10.0
    for t in range(2):
        S.explicit_step(gb, t, dt, 0.5, [0.0, 0.0, -9.81])
    nod = S.explicit_nodal()
    assert abs(nod["mass"].reshape(-1, 3)[:, 0].sum() / m0 - 1.0) < 1e-12
    # free nodes accelerate with g + f/M; with f summing to zero the mass-weighted mean is g on free dofs
    a = nod["accel"].reshape(-1, 3)
    assert np.isfinite(a).all() and a[:, 2].min() < 0
    d = S.download_state()
    assert np.all(d["J_n"] > 0) and np.isfinite(d["Stress"]).all()
    assert d["vel"][:, 2].mean() < 0
    assert S.status_flags() == 0
    # values under the third step (tests/window_oracle.py): a block on the floor, where the column is compressed, and one
    # at mid height, each rebuilt in the oracle from the downloaded state
    from window_oracle import window_step_check
    deep = window_step_check(S, case, gb, [dirichlet_plane(case, 2, 5, 3)], 2, dt, 0.5, [0.0, 0.0, -9.81],
                             [([17, 17, 1], [26, 26, 26]), ([17, 17, 90], [26, 26, 26])], [5, 5, 5], [55, 55, 205], 3,
                             with_lists=False, label="4 M column")
    assert min(deep) >= 1000, deep


def test_config5_drucker_prager_1m_properties():
    """BASELINE configs[4] physics at one GPU's share (1 M particles): Drucker-Prager column under gravity
    (plastic return mapping inside the stress kernel)."""
    n = nlps()
    case = make_case(3, [60, 60, 60], [5, 5, 5], [50, 50, 50], material=DP)
    S = gpu_setup(case, nsteps=6)
    gb = n.BccSet([dirichlet_plane(case, 2, 5, 6)])
    dt = 0.1 / np.sqrt(DP["E"] / 1000.0)
    for t in range(5):
        S.explicit_step(gb, t, dt, 0.5, [0.0, 0.0, -9.81])
    d = S.download_state()
    assert S.status_flags() == 0
    assert np.all(d["J_n"] > 0) and np.isfinite(d["Stress"]).all()
    assert np.all(d["Kappa_n"] >= DP["kappa_0"] - 1e-9) and np.all(d["EPS_n"] >= 0)
    be = d["b_e_n"]
    assert np.allclose(be[:, [1, 2, 5]], be[:, [3, 6, 7]], atol=1e-9)


def _random_cloud_case(ndim, n, seed, cells, lo, hi):
    """Ragged input: n particles at uniformly random positions (0..many per cell), random masses."""
    from util import synth
    rng = np.random.default_rng(seed)
    case = make_case(ndim, cells, [int(v) for v in lo], [1] * ndim)
    x = rng.uniform(lo, hi, size=(n, ndim))
    vol = rng.uniform(0.05, 0.2, size=n)
    case["cloud"] = {
        "ndim": ndim, "x": x, "dis": np.zeros((n, ndim)), "vel": rng.normal(size=(n, ndim)),
        "acc": np.zeros((n, ndim)), "F_n": synth.identity_rows(n, ndim), "b_e_n": synth.identity_rows(n, ndim),
        "J_n": np.ones(n), "rho": np.full(n, 1000.0), "mass": 1000.0 * vol, "vol0": vol,
        "kappa_n": np.zeros(n), "eps_n": np.zeros(n), "matidx": np.zeros(n, dtype=np.int32)}
    return case


@pytest.mark.parametrize("ndim,n", [(2, 1), (2, 37), (3, 1), (3, 5), (3, 333)])
def test_ragged_and_tiny_clouds(ndim, n):
    """Edge cases: a single particle, counts that are no multiple of the wave size, many particles in one
    cell and empty cells in between (uniformly random positions)."""
    o = orc()
    nl = nlps()
    cells = [12, 11] if ndim == 2 else [9, 8, 8]
    lo = np.array([3.2] * ndim)
    hi = np.array([7.7, 6.9] if ndim == 2 else [5.8, 4.9, 4.6])
    case = _random_cloud_case(ndim, n, 100 + n, cells, lo, hi)
    M, P, prm, mats = oracle_setup(case)
    S = gpu_setup(case, nsteps=3)
    compare_search(S, P, M, "ragged init")
    st = o.ExplicitStepper(P, M, mats, prm, o.BccSet([]), 3)
    gb = nl.BccSet([])
    for t in range(3):
        assert st.step(t, 2e-3) == 0
        S.explicit_step(gb, t, 2e-3)
    d = S.download_state()
    assert np.array_equal(d["I0"], P["I0"])
    for k, ok, scale in (("x", "x", None), ("vel", "vel", None), ("Stress", "stress", NH["E"]), ("F_n", "F_n", None)):
        assert_close(d[k], P[ok], 1e-9, "ragged " + k, scale)


def test_empty_particle_set():
    nl = nlps()
    case = _random_cloud_case(2, 0, 1, [8, 8], np.array([3.0, 3.0]), np.array([4.0, 4.0]))
    S = gpu_setup(case, nsteps=2)
    S.explicit_step(nl.BccSet([]), 0, 1e-3)
    assert S.status_flags() == 0 and S.download_state()["x"].shape == (0, 2)
    nod = S.explicit_nodal()
    assert S.nactive == 0 and nod["mass"].size == 0


def test_particle_outside_grid_is_an_error_not_a_crash():
    nl = nlps()
    case = _random_cloud_case(2, 10, 3, [8, 8], np.array([3.0, 3.0]), np.array([4.0, 4.0]))
    case["cloud"]["x"][3] = [-5.0, 2.0]
    S = gpu_setup(case, init=False)
    with pytest.raises(nl.NlpsError):
        S.initialise_shapefun()
    assert S.status_flags() & 2


def test_maximum_size_8m_particles():
    """BASELINE configs[3] total size on ONE GPU (8 M particles, 100^3 cells x 8): capacity and
    size-independent properties (664 B + index data per particle = 5.6 GB of 288 GB)."""
    nl = nlps()
    case = make_case(3, [110, 110, 110], [5, 5, 5], [100, 100, 100], velocity=[0.0, 0.0, -10.0])
    S = gpu_setup(case, nsteps=2)
    assert S.np == 8_000_000
    S.explicit_step(nl.BccSet([dirichlet_plane(case, 2, 0, 2)]), 0, 1e-3)
    nod = S.explicit_nodal()
    assert abs(nod["mass"].reshape(-1, 3)[:, 0].sum() / case["cloud"]["mass"].sum() - 1.0) < 1e-12
    assert S.status_flags() == 0
    nn, _ = S.download_lists()
    assert nn.min() >= 4 and nn.max() <= 125


@pytest.mark.parametrize("ndim", [2, 3])
def test_run_from_gid_mesh_files(tmp_path, ndim):
    """Input side: a command file naming a background mesh with shuffled node numbers, a distorted body
    mesh, a material and a Dirichlet boundary, read by the host helpers of csrc/nlps_io.cpp, drives the HIP path; the
    oracle runs the same arrays.  The Dirichlet nodes are given in FILE numbering and travel through the canon map of
    nlps_host_lattice_from_nodes."""
    import importlib
    import test_gid_io as tg
    gid = importlib.import_module("nl-partsol_amd.gid")
    o = orc()
    n = nlps()
    rng = np.random.default_rng(21)
    cells = [12, 11] if ndim == 2 else [9, 9, 8]
    nn = int(np.prod([c + 1 for c in cells]))
    perm = rng.permutation(nn)
    bg_coords, bg_conn, _ = tg.lattice_mesh(ndim, cells, h=1.0, perm=perm)
    etype = "Quadrilateral" if ndim == 2 else "Hexahedra"
    tg.write_gid(tmp_path / "box.msh", ndim, etype, bg_coords, bg_conn)
    body_cells = [6, 5] if ndim == 2 else [3, 3, 2]
    bc_, bconn, _ = tg.lattice_mesh(ndim, body_cells, h=1.0, origin=[3.0] * ndim)
    bc_ = bc_ + rng.uniform(-0.08, 0.08, size=bc_.shape)
    tg.write_gid(tmp_path / "body.msh", ndim, etype, bc_, bconn)

    # the command file around them: solver, shape function, material, one Dirichlet boundary with constant curves
    nsteps = 4
    plane_file = np.nonzero(bg_coords[:, ndim - 1] == 2.0)[0]  # file numbering, 0-based (File2Chain)
    (tmp_path / "floor.txt").write_text("".join("%d\n" % i for i in plane_file))
    (tmp_path / "zero.txt").write_text("DAT_CURVE NUM#%d\nCONSTANT_CURVE SCALE#0.0\n" % nsteps)
    (tmp_path / "run.nlp").write_text(
        "GramsBox (Type=GID,File=box.msh) {\n  GramsBoundary (File=floor.txt) {\n"
        + "".join("    BcDirichlet V.%s zero.txt\n" % "xyz"[a] for a in range(ndim)) + "  }\n}\n"
        + "One-Phase-Analysis (File=body.msh, GPxElement=%d) {\n}\n" % (4 if ndim == 2 else 8)
        + "GramsShapeFun (Type=LME) {\n  gamma=3.0\n}\n"
        + "NLPS-Solver (Type=NPC-FS) {\n  CFL=0.1\n  Cel=100.0\n  N=%d\n}\n" % nsteps
        + "Define-Material(idx=0,Model=Neo-Hookean-Wriggers)\n{\n  rho=1000.0\n  E=%r\n  nu=%r\n}\n" % (NH["E"], NH["nu"])
        + "GramsInitials (Nodes=body_elements.txt) {\n  Value=[%s]\n}\n" % ",".join(["0.0"] * (ndim - 1) + ["-10.0"]))
    (tmp_path / "body_elements.txt").write_text("".join("%d\n" % e for e in range(len(bconn))))
    deck = gid.read_deck(tmp_path / "run.nlp")
    (_, rho, material), = gid.read_materials(tmp_path / "run.nlp")
    assert (deck["N"], deck["shape_fun"], deck["gamma_lme"], material["type"]) == (nsteps, "LME", 3.0, 0)

    box = gid.read_gid_mesh(deck["box_mesh"])
    h, gn, origin, canon = gid.lattice_from_nodes(box["coords"])
    cloud = gid.cloud_from_mesh(gid.read_gid_mesh(deck["body_mesh"]), deck["gp_per_elem"], rho=rho)
    cloud["vel"] = gid.read_initials(tmp_path / "run.nlp", deck["gp_per_elem"], cloud["vel"])
    assert np.array_equal(cloud["vel"][:, ndim - 1], np.full(len(cloud["vel"]), -10.0))
    case = {"ndim": ndim, "cells": cells, "grid_n": gn, "origin": origin, "h": h, "cloud": cloud,
            "materials": [{k: material[k] for k in ("type", "E", "nu")}]}
    bcs = gid.read_boundaries(tmp_path / "run.nlp", ndim, deck["N"])
    for b in bcs:
        b["nodes"] = np.sort(canon[b["nodes"]]).astype(np.int32)  # file -> library numbering
    assert len(bcs) == 1 and np.array_equal(bcs[0]["nodes"], dirichlet_plane(case, ndim - 1, 2, nsteps)["nodes"])
    assert np.array_equal(bcs[0]["dir"], np.ones((ndim, nsteps))) and not bcs[0]["value"].any()
    dt = 0.1 * h / np.sqrt(NH["E"] / 1000.0)
    M, P, prm, mats = oracle_setup(case)
    S = gpu_setup(case, nsteps=nsteps)
    stepper = o.ExplicitStepper(P, M, mats, prm, o.BccSet(bcs), nsteps)
    gb = n.BccSet(bcs)
    for t in range(nsteps):
        assert stepper.step(t, dt) == 0
        S.explicit_step(gb, t, dt)
    assert S.status_flags() == 0
    st = S.download_state()
    nnb, lst = S.download_lists()
    assert np.array_equal(st["I0"], P["I0"]) and np.array_equal(nnb, P["nn"]) and lists_equal(nnb, lst, P["list"])
    for k, ok in (("x", "x"), ("vel", "vel"), ("F_n", "F_n"), ("Stress", "stress"), ("lambda", "lambda")):
        assert_close(st[k], P[ok], 1e-9, k)
    assert np.abs(st["Stress"]).max() > 1.0


@pytest.mark.parametrize("ndim", [2, 3])
def test_nodal_traction_forces(ndim):
    """__nodal_traction_forces (U-Newmark-beta.c:1376-1500) on the device against the oracle's serial
    restatement: two Neumann contours of particles, the second with one direction switched off (it inherits the first
    contour's traction, as upstream), Dirichlet dofs skipped, accumulated into a residual that already holds the internal
    forces; host and device residual vectors; after a physical re-sort the caller's particle indices still address the
    same particles."""
    o = orc()
    n = nlps()
    if ndim == 2:
        case = make_case(2, [12, 11], [3, 3], [5, 4], material=NH, velocity=[1.0, -2.0])
    else:
        case = make_case(3, [8, 8, 7], [3, 3, 2], [2, 2, 2], material=NH, velocity=[1.0, -2.0, 0.5])
    nsteps, step = 3, 1
    bcs_list = [dirichlet_plane(case, ndim - 1, 3, nsteps)]
    M, P, prm, mats = oracle_setup(case)
    S = gpu_setup(case, nsteps=nsteps)
    n2m, d2m, na = masks(S, M, bcs_list, step, nsteps)
    rng = np.random.default_rng(4)
    npart = case["cloud"]["x"].shape[0]
    pick = rng.choice(npart, size=24, replace=False).astype(np.int32)
    d1, d2 = np.ones((ndim, nsteps), dtype=np.int32), np.ones((ndim, nsteps), dtype=np.int32)
    d2[0, step] = 0
    loads = [{"nodes": pick[:14], "dim": ndim, "dir": d1, "value": rng.normal(size=(ndim, nsteps)) * 1e7},
             {"nodes": pick[14:], "dim": ndim, "dir": d2, "value": rng.normal(size=(ndim, nsteps)) * 1e7}]
    area0 = rng.uniform(0.2, 0.3, size=npart) if ndim == 3 else None
    dU = 1e-2 * rng.normal(size=na * ndim)
    assert o.compatibility(dU, None, P, M, n2m) == 0 and o.constitutive(P, mats, prm) == 0
    S.local_compatibility_conditions(dU)
    S.constitutive_update()
    R_o, st = o.internal_forces(P, M, n2m, d2m, na)
    assert st == 0
    fint = np.abs(R_o).max()
    assert o.nodal_traction_forces(R_o, P, M, n2m, d2m, loads, step, nsteps, 0.5, area0) == 0
    R_g = S.nodal_internal_forces(np.zeros(na * ndim))
    S.nodal_traction_forces(R_g, n.BccSet(loads), step, 0.5, area0)
    assert np.abs(R_o).max() > 2 * fint, "the tractions must matter"
    assert_close(R_g, R_o, 1e-10, "internal + traction forces (host residual)")
    import torch
    R_d = torch.zeros(na * ndim, dtype=torch.float64, device="cuda")
    S.nodal_internal_forces(R_d.data_ptr())
    S.nodal_traction_forces(R_d.data_ptr(), n.BccSet(loads), step, 0.5, area0)
    torch.cuda.synchronize()
    assert_close(R_d.cpu().numpy(), R_o, 1e-10, "device residual")
    S.resort()
    S.local_search()
    assert o.local_search(P, M, prm) == 0
    n2m, d2m, na2 = masks(S, M, bcs_list, step, nsteps)
    R_o2 = np.zeros(na2 * ndim)
    assert o.nodal_traction_forces(R_o2, P, M, n2m, d2m, loads, step, nsteps, 0.5, area0) == 0
    R_g2 = S.nodal_traction_forces(np.zeros(na2 * ndim), n.BccSet(loads), step, 0.5, area0)
    assert_close(R_g2, R_o2, 1e-10, "tractions after a re-sort")


def test_adaptive_resort_only_moves_memory():
    """nlps_gpu_set_adaptive_resort: the search stage counts the particles that left the tile their memory slot was
    sorted into, the step re-sorts when their accumulated share exceeds the budget.  A sheared block (particles cross
    tile boundaries within a few dozen steps): the policy fires (the debt drops back after growing), the status stays
    clean, and the fields agree with the same run without any re-sort to the rounding of the accumulation order --
    a re-sort moves particles in memory, nothing else."""
    n = nlps()
    soft = {"type": 0, "E": 1.0e5, "nu": 0.3}

    def run(budget):
        case = make_case(3, [30, 30, 30], [6, 6, 6], [16, 16, 16], material=soft)
        x = case["cloud"]["x"]
        c = x.mean(axis=0)
        v = np.zeros_like(x)
        v[:, 0] = 10.0 * (x[:, 2] - c[2]) / 8.0
        v[:, 1] = 10.0 * (x[:, 0] - c[0]) / 8.0
        case["cloud"]["vel"] = v
        S = gpu_setup(case, nsteps=1)
        if budget:
            S.set_adaptive_resort(budget, 2)
        else:
            S.set_adaptive_resort(0.0)
            S.set_resort_interval(0)
        gb = n.BccSet([])
        debts = []
        for t in range(60):
            S.explicit_step(gb, 0, 2e-3)
            debts.append(S.debug_displaced()[1])
        assert S.status_flags() == 0
        return S.download_state(), np.array(debts)

    a, debts = run(0.05)
    b, zero = run(0.0)
    assert np.all(zero == 0.0)
    # (the debt is read after the step: the step that crosses the budget re-sorts and is seen at zero again)
    assert debts.max() > 0.0 and np.sum(np.diff(debts) < 0) >= 2, "the adaptive re-sort must have fired"
    assert np.array_equal(a["I0"], b["I0"])
    for k in ("x", "vel", "F_n", "Stress", "rho", "lambda"):
        assert_close(a[k], b[k], 1e-10, f"adaptive re-sort on / off: {k}")


@pytest.mark.parametrize("ndim,material", [(2, DP), (3, NH), (3, DP)])  # (3, DP): the one-material kernels (UMAT) of both forms
def test_folded_step_matches_the_nodal_kernels(ndim, material):
    """Default on one GPU: K3 and K5 make dU and the accelerations of their window nodes themselves (k3_tile_lazy,
    k5_tile_lazy) and the nodal arrays are only made on request.  Same state, same nodal arrays as the form with the
    nodal kernels between the stages (debug option lazy_nodal = 0: what the deterministic path runs), also when
    the request comes late, after a download."""
    nsteps, dt = 5, 1e-4
    v = [0.0, -10.0] if ndim == 2 else [0.0, 0.0, -10.0]
    case = small_case(ndim, material=material, velocity=v)
    n = nlps()
    gb = n.BccSet([dirichlet_plane(case, ndim - 1, 2, nsteps)])
    S = gpu_setup(case, nsteps=nsteps)
    Sn = gpu_setup(case, nsteps=nsteps)
    Sn.debug_option("lazy_nodal", 0)
    grav = [0.0] * (ndim - 1) + [-9.81]
    for t in range(nsteps):
        S.explicit_step(gb, t, dt, gravity=grav)
        Sn.explicit_step(gb, t, dt, gravity=grav)
    assert S.status_flags() == 0 and Sn.status_flags() == 0
    a, b = S.download_state(), Sn.download_state()
    assert np.array_equal(a["I0"], b["I0"])
    for k in ("x", "vel", "acc", "Stress", "F_n", "J_n", "rho"):
        assert_close(a[k], b[k], 1e-11, f"{k}: folded step vs nodal kernels")
    na, nb = S.explicit_nodal(), Sn.explicit_nodal()
    assert S.nactive == Sn.nactive
    for k in ("mass", "dU", "force", "accel", "reaction"):
        assert_close(na[k], nb[k], 1e-10, f"nodal {k}: folded step vs nodal kernels", scale=1e-12)
    assert np.abs(nb["reaction"]).max() > 0.0 and np.abs(nb["dU"]).max() > 0.0


@pytest.mark.parametrize("ndim", [2, 3])
def test_shape_functions_level_a(ndim):
    """compute_N__ShapeFun__ / compute_dN__ShapeFun__ for the LME family (p__LME__, dp__LME__): the values and gradients
    themselves, in the order of every particle's list, after the initial search and again after the cloud has moved
    (new lambda, new masks)."""
    o = orc()
    nsteps, dt = 4, 1e-4
    v = [3.0, -10.0] if ndim == 2 else [3.0, 1.0, -10.0]
    case = small_case(ndim, velocity=v)
    M, P, prm, mats = oracle_setup(case)
    S = gpu_setup(case, nsteps=nsteps)

    def compare(what):
        nn, lst = S.download_lists()
        assert np.array_equal(nn, P["nn"]) and lists_equal(nn, lst, P["list"])
        N, dN = S.shape_functions()
        first = max(0, S.np - 40)
        Nt, dNt = S.shape_functions(first, S.np - first)  # a range that does not start at 0
        assert np.array_equal(Nt, N[first:]) and np.array_equal(dNt, dN[first:])
        worst_n = worst_d = 0.0
        for p in range(0, S.np, 7):
            n_ref, d_ref = o.compute_N(P, M, p), o.compute_dN(P, M, p)
            k = n_ref.shape[0]
            assert k == nn[p]
            worst_n = max(worst_n, float(np.max(np.abs(N[p, :k] - n_ref))))
            worst_d = max(worst_d, float(np.max(np.abs(dN[p, :k] - d_ref)) / np.max(np.abs(d_ref))))
            assert not N[p, k:].any() and not dN[p, k:].any()
            assert abs(N[p, :k].sum() - 1.0) < 1e-12
        assert worst_n < 1e-11, f"{what}: N differs by {worst_n:.2e}"
        assert worst_d < 1e-9, f"{what}: dN differs by {worst_d:.2e} of its magnitude"

    compare("after initialize__LME__")
    n = nlps()
    gb = n.BccSet([dirichlet_plane(case, ndim - 1, 2, nsteps)])
    stepper = o.ExplicitStepper(P, M, mats, prm, o.BccSet([dirichlet_plane(case, ndim - 1, 2, nsteps)]), nsteps)
    for t in range(nsteps):
        assert stepper.step(t, dt) == 0
        S.explicit_step(gb, t, dt)
    o.local_search(P, M, prm)
    S.local_search()
    compare("after four explicit steps and a search")
