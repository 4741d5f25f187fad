"""Matrix-free tangent (nlps_gpu_tangent_operator / _apply / _block_diagonal): y = K x and the diagonal blocks of K
without the assembled matrix, against the assembled COO of the same state (nlps_gpu_tangent_assemble + _coo) and the
oracle's restatement of __jacobian_evaluation (U-Newmark-beta.c:1646-1830)."""
import numpy as np
import pytest

from newmark import newmark_parameters
from test_gpu_parity import masks
from util import DP, HENCKY, NH, VM, assert_close, dirichlet_plane, gpu_setup, make_case, nlps, oracle_setup, orc, synth

pytestmark = pytest.mark.gpu

LAWS = {"neo-hookean": NH, "hencky": HENCKY, "drucker-prager": DP, "von-mises": VM,
        "matsuoka-nakai": synth.matsuoka_nakai_material()}


def _case(ndim, material, velocity=True):
    vel = ([1.0, -2.0] if ndim == 2 else [1.0, -2.0, 0.5]) if velocity else None
    if ndim == 2:
        return make_case(2, [12, 11], [3, 3], [5, 4], material=material, velocity=vel)
    return make_case(3, [8, 8, 7], [3, 3, 2], [2, 2, 2], material=material, velocity=vel)


def _linearised(ndim, law, seed=13, with_oracle=True, case=None, plane=3):
    """Device (and oracle) state after one compatibility + constitutive pass at a random dU, masks at step 1.
    case: another cloud of the law's material than _case's; plane: the row of grid nodes that is fixed."""
    mat = LAWS[law]
    if case is None:
        case = _case(ndim, mat)
    if law == "matsuoka-nakai":
        cl = case["cloud"]
        cl["b_e_n"] = synth.frictional_states(ndim, mat, cl["x"].shape[0], seed=5)
        cl["kappa_n"][:] = mat["kappa_0"]
        cl["eps_n"][:] = mat["eps_0"]
    nsteps = 2
    bcs_list = [dirichlet_plane(case, ndim - 1, plane, nsteps)]
    M, P, prm, mats = oracle_setup(case)
    S = gpu_setup(case, nsteps=nsteps)
    n2m, d2m, na = masks(S, M, bcs_list, 1, nsteps)
    rng = np.random.default_rng(seed)
    amp = {"neo-hookean": 2e-2, "hencky": 2e-2, "drucker-prager": 8e-3, "von-mises": 8e-3, "matsuoka-nakai": 1.5e-4}[law]
    dU = amp * rng.normal(size=na * ndim)
    S.local_compatibility_conditions(dU)
    S.constitutive_update()
    o = None
    if with_oracle:
        o = orc()
        assert o.compatibility(dU, None, P, M, n2m) == 0 and o.constitutive(P, mats, prm) == 0
    Mv = o.lumped_mass(P, M, n2m, na) if with_oracle else S.compute_nodal_lumped_mass()
    return dict(S=S, o=o, M=M, P=P, mats=mats, n2m=n2m, d2m=d2m, na=na, Mv=Mv, dU=dU, rng=rng, mat=mat)


def _coo_dense(S, ntot, alpha_1, mass, dirichlet):
    rows, cols, vals = S.jacobian_evaluation(alpha_1, mass, dirichlet)
    K = np.zeros((ntot, ntot))
    np.add.at(K, (rows, cols), vals)
    return K


def _check_apply(S, K, ntot, rng, what, nvec=3):
    for _ in range(nvec):
        x = rng.normal(size=ntot)
        y = S.tangent_apply(x)
        ref = K @ x
        tol = 1e-11 * np.abs(K).max() * np.abs(x).max() * 125  # |K| |x| over a row of at most 125 member blocks
        assert np.abs(y - ref).max() <= tol, f"{what}: apply vs assembled COO: {np.abs(y - ref).max():.3e} > {tol:.3e}"


def _check_blocks(S, K, na, ndim, what):
    B = S.tangent_block_diagonal()
    ref = np.stack([K[A * ndim:(A + 1) * ndim, A * ndim:(A + 1) * ndim] for A in range(na)])
    assert_close(B, ref, 1e-11, f"{what}: block diagonal", scale=np.abs(K).max())


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("law", ["neo-hookean", "hencky", "drucker-prager", "von-mises", "matsuoka-nakai"])
def test_apply_and_blocks_against_the_assembled_tangent(ndim, law):
    frictional = law == "matsuoka-nakai"
    s = _linearised(ndim, law)
    S, o, na = s["S"], s["o"], s["na"]
    ntot = na * ndim
    if law in ("drucker-prager", "von-mises"):
        assert (s["P"]["eps_n1"] > s["P"]["eps_n"]).sum() > 0, "some particles must be plastic"
    for alpha_1, mass, dirichlet in ((0.0, None, False), (4.0e4, s["Mv"], True)):
        what = f"{law} {ndim}-D (alpha_1={alpha_1}, dirichlet={dirichlet})"
        K = _coo_dense(S, ntot, alpha_1, mass, dirichlet)
        assert np.abs(K).max() > 0
        S.tangent_operator(alpha_1, mass, dirichlet)
        _check_apply(S, K, ntot, s["rng"], what)
        _check_blocks(S, K, na, ndim, what)
        # the oracle's matrix, at the tolerances of the assembled tests (the frictional 3-D tangent has no stable
        # eigenbasis after an elastic step: test_gpu_frictional.py compares it in 2-D only)
        if not (frictional and ndim == 3):
            K_o, _, st = o.tangent_matrix(s["P"], s["M"], s["mats"], s["n2m"], s["d2m"] if dirichlet else None, na, alpha_1,
                                          mass, with_pattern=False)
            assert st == 0
            x = s["rng"].normal(size=ntot)
            tol = 1e-10 if law == "neo-hookean" else (1e-7 if frictional else 1e-8)
            assert_close(S.tangent_apply(x), K_o @ x, tol, f"{what}: apply vs oracle", scale=np.abs(K_o).max() * np.abs(x).max())
    S.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_mixed_materials(ndim):
    """A cloud of Neo-Hookean, Hencky and Drucker-Prager particles interleaved: the law is chosen per particle."""
    case = _case(ndim, DP)  # (the cloud's internal variables start as the Drucker-Prager ones, like test_gpu_parity's)
    npart = case["cloud"]["x"].shape[0]
    case["materials"] = [{"type": 0, "E": 2.0e4, "nu": 0.3}, {"type": 1, "E": 1.0e4, "nu": 0.25}, DP]
    case["cloud"]["matidx"] = (np.arange(npart) % 3).astype(np.int32)
    nsteps = 2
    bcs_list = [dirichlet_plane(case, ndim - 1, 3, nsteps)]
    S = gpu_setup(case, nsteps=nsteps)
    n = nlps()
    S.local_search()
    S.active_masks(n.BccSet(bcs_list), 1)
    na = S.nactive
    ntot = na * ndim
    rng = np.random.default_rng(5)
    S.local_compatibility_conditions(8e-3 * rng.normal(size=ntot))
    S.constitutive_update()
    Mv = S.compute_nodal_lumped_mass()
    for alpha_1, mass, dirichlet in ((0.0, None, False), (3.0e3, Mv, True)):
        K = _coo_dense(S, ntot, alpha_1, mass, dirichlet)
        S.tangent_operator(alpha_1, mass, dirichlet)
        _check_apply(S, K, ntot, rng, f"mixed {ndim}-D")
        _check_blocks(S, K, na, ndim, f"mixed {ndim}-D")
    S.close()


def test_host_and_device_vectors():
    import torch
    s = _linearised(3, "drucker-prager", with_oracle=False)
    S, na = s["S"], s["na"]
    ntot = na * 3
    Mv = s["Mv"]
    S.tangent_operator(2.0e3, torch.from_numpy(np.ascontiguousarray(Mv)).cuda(), True)
    x = s["rng"].normal(size=ntot)
    x0 = x.copy()
    y_h = np.full(ntot, np.nan)
    S.tangent_apply(x, out=y_h)
    assert np.array_equal(x, x0), "x is not touched"
    xd = torch.from_numpy(x).cuda()
    yd = torch.full((ntot,), 7.0, dtype=torch.float64, device="cuda")
    S.tangent_apply(xd, out=yd)
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy(), x0)
    assert_close(yd.cpu().numpy(), y_h, 1e-12, "device vs host y", scale=np.abs(y_h).max())
    assert np.all(np.isfinite(y_h))
    yd2 = S.tangent_apply(xd)
    assert isinstance(yd2, torch.Tensor) and yd2.is_cuda
    B_h = S.tangent_block_diagonal()
    B_d = S.tangent_block_diagonal(on_device=True)
    assert_close(B_d.cpu().numpy(), B_h, 1e-12, "device vs host blocks", scale=np.abs(B_h).max())
    S.close()


def test_snapshot_and_invalidation():
    n = nlps()
    s = _linearised(2, "neo-hookean", with_oracle=False)
    S, na, Mv = s["S"], s["na"], s["Mv"]
    ntot = na * 2
    x = s["rng"].normal(size=ntot)
    with pytest.raises(n.NlpsError, match="nlps_gpu_tangent_operator\\(\\) first"):
        S.tangent_apply(x)
    with pytest.raises(n.NlpsError, match="nlps_gpu_tangent_operator\\(\\) first"):
        S.tangent_block_diagonal()
    K = _coo_dense(S, ntot, 1.0e3, Mv, True)
    S.tangent_operator(1.0e3, Mv, True)
    y0 = S.tangent_apply(x)
    # a line-search trial: a residual at another dU moves DF and the stress, not the operator
    a = newmark_parameters(0.25, 0.5, 1.0e-2)
    alpha = [a["a1"], a["a2"], a["a3"], a["a4"], a["a5"], a["a6"]]
    z = np.zeros(ntot)
    S.lagrangian_evaluation(5e-2 * s["rng"].normal(size=ntot), z, z, Mv, alpha, None)
    y1 = S.tangent_apply(x)
    assert_close(y1, y0, 1e-12, "the operator is a snapshot", scale=np.abs(y0).max())
    _check_apply(S, K, ntot, s["rng"], "after a residual at another dU", nvec=1)
    bcs = n.BccSet([dirichlet_plane(_case(2, NH), 1, 3, 2)])
    for what, call in (("re-sort", S.resort), ("nlps_gpu_local_search", S.local_search),
                       ("nlps_gpu_update_kinetics", lambda: S.update_particles_kinetics_FLIP_PIC(1.0, z, z, z, z)),
                       ("nlps_gpu_roll_state", S.update_particles_internal_variables)):
        S.local_search()
        S.active_masks(bcs, 1)
        S.tangent_operator(1.0e3, Mv, True)
        S.tangent_apply(x)
        call()
        with pytest.raises(n.NlpsError, match="stale: .*" + what):
            S.tangent_apply(x)
        with pytest.raises(n.NlpsError, match="stale"):
            S.tangent_block_diagonal()
    S.close()


@pytest.mark.parametrize("ndim,law", [(2, "neo-hookean"), (3, "neo-hookean"), (3, "drucker-prager")])
def test_newton_krylov_steps(ndim, law):
    """Three implicit Newmark steps (gravity, fixed floor) with the linear solve done by GMRES on the operator,
    preconditioned by the inverted diagonal blocks, against the same steps with a dense solve of the assembled matrix."""
    from scipy.sparse.linalg import LinearOperator, gmres
    n = nlps()
    mat = {"type": 0, "E": 2.0e5, "nu": 0.3} if law == "neo-hookean" else DP
    if ndim == 2:
        case = make_case(2, [12, 11], [3, 3], [5, 4], material=mat, velocity=[0.5, -1.0])
    else:
        case = make_case(3, [8, 8, 7], [3, 3, 2], [2, 2, 2], material=mat, velocity=[0.5, 0.2, -1.0])
    nsteps = 3
    bcs = n.BccSet([dirichlet_plane(case, ndim - 1, 3 if ndim == 2 else 2, nsteps)])
    gravity = [0.0] * (ndim - 1) + [-9.81]
    dt = 1.0e-2
    a = newmark_parameters(0.25, 0.5, dt)
    alpha = [a["a1"], a["a2"], a["a3"], a["a4"], a["a5"], a["a6"]]
    runs = []
    for krylov in (False, True):
        S = gpu_setup(case, nsteps=nsteps)
        its_all, dU_all = [], []
        for step in range(nsteps):
            S.local_search()
            S.active_masks(bcs, step)
            Mv = S.compute_nodal_lumped_mass()
            V, A = S.get_nodal_field_n(Mv)
            ntot = S.nactive * ndim
            dU = np.zeros(ntot)
            R = S.lagrangian_evaluation(dU, V, A, Mv, alpha, gravity)
            r0 = np.linalg.norm(R)
            its, norms = 0, [r0]
            while np.linalg.norm(R) > 1e-10 * max(r0, 1e-30) and its < 12:
                if krylov:
                    S.tangent_operator(a["a1"], Mv, True)
                    B = S.tangent_block_diagonal()
                    Binv = np.linalg.inv(B)
                    Kop = LinearOperator((ntot, ntot), matvec=lambda v: S.tangent_apply(np.ascontiguousarray(v)))
                    Pre = LinearOperator((ntot, ntot), matvec=lambda v: np.einsum("aij,aj->ai", Binv, v.reshape(-1, ndim)).ravel())
                    try:
                        d, info = gmres(Kop, -R, rtol=1e-12, atol=0.0, M=Pre, restart=200, maxiter=50)
                    except TypeError:  # older scipy
                        d, info = gmres(Kop, -R, tol=1e-12, atol=0.0, M=Pre, restart=200, maxiter=50)
                    assert info == 0, f"GMRES did not converge (info={info})"
                else:
                    K = _coo_dense(S, ntot, a["a1"], Mv, True)
                    d = np.linalg.solve(K, -R)
                dU = dU + d
                R = S.lagrangian_evaluation(dU, V, A, Mv, alpha, gravity)
                its += 1
                norms.append(np.linalg.norm(R))
            assert np.linalg.norm(R) <= 1e-10 * max(r0, 1e-30), f"step {step}: Newton did not converge: {norms}"
            its_all.append(its)
            dU_all.append(dU.copy())
            if law == "neo-hookean" and len(norms) >= 4:  # quadratic tail
                assert norms[-2] <= 1e-3 * norms[-3] or norms[-2] < 1e-8 * r0, norms
            dV = a["a4"] * dU + (a["a5"] - 1) * V + a["a6"] * A
            dA = a["a1"] * dU - a["a2"] * V - (a["a3"] + 1) * A
            S.update_particles_internal_variables()
            S.update_particles_kinetics_FLIP_PIC(1.0, dU, V, dV, dA)
        runs.append((its_all, dU_all))
        S.close()
    assert runs[0][0] == runs[1][0], f"Newton iterations: dense {runs[0][0]} vs Krylov {runs[1][0]}"
    for s_ in range(nsteps):
        assert_close(runs[1][1][s_], runs[0][1][s_], 1e-8, f"step {s_}: converged dU", scale=np.abs(runs[0][1][s_]).max())


def test_finite_differences_symmetry_and_bytes():
    """1 M particles (the bench cube), Neo-Hookean, fused residual: K x against central differences of the residual (the
    Neo-Hookean tangent is the exact derivative), symmetry of K, the bytes of the header's formula."""
    import os
    import sys
    from util import ROOT
    sys.path.insert(0, ROOT)
    import bench
    n = nlps()
    ndim = 3
    case = bench.build_case(0, 1, 50)
    nsteps = 2
    bcs = n.BccSet([dirichlet_plane(case, 2, case["block_lo"][2], nsteps)])
    S = gpu_setup(case, nsteps=nsteps)
    S.local_search()
    _, d2m = S.active_masks(bcs, 0)
    Mv = S.compute_nodal_lumped_mass()
    V, A = S.get_nodal_field_n(Mv)
    na = S.nactive
    ntot = na * ndim
    a = newmark_parameters(0.25, 0.5, 1.0e-2)
    alpha = [a["a1"], a["a2"], a["a3"], a["a4"], a["a5"], a["a6"]]
    rng = np.random.default_rng(7)
    dU = 1e-3 * rng.normal(size=ntot)
    S.lagrangian_evaluation(dU, V, A, Mv, alpha, None)
    nb = S.tangent_operator(a["a1"], Mv, True)
    npart = S.num_particles()
    assert npart == 1000000
    nnodes = int(np.prod(case["grid_n"]))
    assert nb == 8 * (ndim ** 4 * npart + ntot + ndim * ndim * nnodes), "bytes vs the header's formula"
    fixed = d2m == -1
    x = rng.normal(size=ntot)
    y = S.tangent_apply(x)
    assert fixed.any() and np.array_equal(y[fixed], x[fixed]), "identity rows on the fixed dofs"
    x[fixed] = 0.0  # (the residual moves with the fixed dofs too; the operator's identity columns ignore them)
    y = S.tangent_apply(x)
    eps = 1e-6
    Rp = S.lagrangian_evaluation(dU + eps * x, V, A, Mv, alpha, None)
    Rm = S.lagrangian_evaluation(dU - eps * x, V, A, Mv, alpha, None)
    fd = (Rp - Rm) / (2 * eps)
    assert_close(y[~fixed], fd[~fixed], 1e-6, "K x vs central differences of the residual", scale=np.abs(fd).max())
    x2 = rng.normal(size=ntot)
    y2 = S.tangent_apply(x2)
    assert abs(x2 @ y - x @ y2) <= 1e-12 * np.abs(y).max() * np.abs(x2).sum(), "symmetry"
    S.close()


def test_two_ranks_on_one_gpu():
    """Two ranks on the one card (gloo and host staging behind the halo callback, as test_multirank_on_one_gpu), NH in
    3-D: each rank's y = K x and diagonal blocks on its active nodes equal the whole cloud's at those nodes
    (tests/mr_gpu_tangent_worker.py)."""
    import os
    import subprocess
    import sys
    from util import ROOT, free_port
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "tests", "mr_gpu_tangent_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "MULTIRANK_TANGENT_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("ndim,law", [(2, 0), (3, 0), (3, 1)])
def test_eigenerosion_damage_scaling(ndim, law):
    """With the eigenerosion driver on, the tangent of a particle scales with (1 - Damage_n1) (U-Newmark-beta.c:1757-1764):
    apply and blocks against the assembled COO of the same damaged state (setup of test_gpu_eigenerosion.py)."""
    from test_gpu_eigenerosion import stretch_field
    o = orc()
    n = nlps()
    rng = np.random.default_rng(21)
    mat = {"type": law, "E": 1.0e6, "nu": 0.25, "Ceps": 1.5, "Gf": 0.0}
    if ndim == 2:
        case = make_case(2, [14, 12], [3, 3], [7, 6], material=mat)
    else:
        case = make_case(3, [11, 10, 9], [3, 3, 2], [5, 4, 4], material=mat)
    M, P, prm, mats = oracle_setup(case)
    n2m, na = o.active_nodes(M)
    dU = stretch_field(M, n2m, na, ndim, 0.02, rng)
    # the oracle's energy release rates at Gf = 0 give a Gf that fails about half of the cloud
    beps = o.compute_beps(P, M, mats, initialize=True)
    assert o.compatibility(dU, None, P, M, n2m) == 0 and o.constitutive_eroded(P, mats, prm, np.zeros(P.np)) == 0
    W = P["W"].copy()
    V = P["vol0"] * P["J_n1"]
    G = np.zeros(P.np)
    for p in range(P.np):
        q = beps[1][p, : beps[0][p]]
        G[p] = mat["Ceps"] * case["h"] / (V[p] + V[q].sum()) * (V[p] * W[p] + (V[q] * W[q]).sum())
    mat["Gf"] = float(np.median(G))
    case["materials"] = [mat]
    M, P, prm, mats = oracle_setup(case)
    params = n.default_params()
    params.driver_eigenerosion = 1
    S = gpu_setup(case, nsteps=2, params=params)
    n2m, d2m, na = masks(S, M, [], 0, 2)
    S.local_compatibility_conditions(dU)
    S.constitutive_update()
    S.nodal_internal_forces(np.zeros(na * ndim))  # (the eigenerosion hook runs between the stresses and the forces)
    dmg = S.download_state()["Damage_n1"]
    assert 0 < np.count_nonzero(dmg) < dmg.size, "part of the cloud must be damaged"
    ntot = na * ndim
    Mv = S.compute_nodal_lumped_mass()
    for alpha_1, mass, dirichlet in ((0.0, None, False), (2.0e3, Mv, True)):
        K = _coo_dense(S, ntot, alpha_1, mass, dirichlet)
        S.tangent_operator(alpha_1, mass, dirichlet)
        _check_apply(S, K, ntot, rng, f"eigenerosion {ndim}-D law {law}")
        _check_blocks(S, K, na, ndim, f"eigenerosion {ndim}-D law {law}")
    S.close()
