"""The tangent in CSR, assembled row by row without float atomics (nlps_gpu_tangent_csr_pattern / nlps_gpu_tangent_csr,
DESIGN.md 5o).  References, never the code under test: the assembled COO of the same state (Solver.jacobian_evaluation,
the atomic path, densified with np.add.at) and the oracle's tangent_matrix.

Tolerances: 1e-11 of max |K| between the CSR and the COO matrix, the project's bound between two summation orders of the
same blocks (test_gpu_tangent_operator.py::_check_blocks); against the oracle those of the assembled tests, 1e-10
(Neo-Hookean), 1e-8 (spectral laws), 1e-7 (Matsuoka-Nakai, 2-D only).  Structure, counts and replays are exact."""
import numpy as np
import pytest

from test_gpu_deterministic_damage import Handle as DamageHandle
from test_gpu_deterministic_damage import erosion_problem
from test_gpu_fluid import _Case as FluidCase
from test_gpu_newton_solve import _alpha
from test_gpu_tangent_operator import _case, _linearised
from util import DP, NH, dirichlet_plane, gpu_setup, make_case, nlps, oracle_setup

pytestmark = pytest.mark.gpu

TOL_COO = 1e-11


def csr_bytes(ndim, npart, nnodes, nactive):
    """the formula of include/nlps_gpu.h"""
    w = 12 if ndim == 3 else 2
    return 8 * npart * (ndim ** 4 + 6 * ndim + 2) + 4 * (nnodes + 1) + 8 * w * nnodes + 8 * (nactive + 1)


def dense_of_csr(row_ptr, cols, vals, ntot):
    K = np.zeros((ntot, ntot))
    rows = np.repeat(np.arange(ntot), np.diff(row_ptr))
    np.add.at(K, (rows, cols), vals)
    return K, rows


def ascending(row_ptr, cols):
    """columns strictly ascending inside every row"""
    if cols.size < 2:
        return True
    inside = np.ones(cols.size - 1, dtype=bool)
    ends = row_ptr[1:-1]
    ends = ends[(ends > 0) & (ends < cols.size)]
    inside[ends - 1] = False  # (the step from one row's last column to the next row's first)
    return bool((np.diff(cols.astype(np.int64))[inside] > 0).all())


def check_against_coo(S, alpha_1, mass, dirichlet, what):
    """The CSR matrix of (alpha_1, mass, dirichlet) at the current state against the assembled COO: values, structure,
    counts, order.  Returns (K_csr, (row_ptr, cols, vals), bytes)."""
    ndim, ntot = S.ndim, S.nactive * S.ndim
    r, c, v = S.jacobian_evaluation(alpha_1, mass, dirichlet)
    nnz_coo = r.size
    pattern = S.create_sparsity_pattern()
    K_coo = np.zeros((ntot, ntot))
    np.add.at(K_coo, (r, c), v)
    S.tangent_operator(alpha_1, mass, dirichlet)
    nnz, nb = S.tangent_csr_pattern()
    row_ptr, cols, vals = S.tangent_csr()
    assert nnz == nnz_coo, f"{what}: nnz {nnz} vs nlps_gpu_tangent_assemble's {nnz_coo}"
    assert row_ptr.shape == (ntot + 1,) and cols.shape == (nnz,) and vals.shape == (nnz,)
    assert row_ptr[0] == 0 and row_ptr[-1] == nnz
    assert np.array_equal(np.diff(row_ptr), pattern), f"{what}: row lengths vs nlps_gpu_sparsity_pattern"
    assert cols.size == 0 or (cols.min() >= 0 and cols.max() < ntot)
    assert ascending(row_ptr, cols), f"{what}: columns are not strictly ascending in every row"
    K, rows = dense_of_csr(row_ptr, cols, vals, ntot)
    lin_coo = np.unique(r.astype(np.int64) * ntot + c)
    lin_csr = rows.astype(np.int64) * ntot + cols
    assert np.array_equal(lin_csr, lin_coo), f"{what}: the set of (row, col) differs from the COO's"
    scale = np.abs(K_coo).max()
    err = np.abs(K - K_coo).max()
    print(f"{what}: nnz {nnz}, |K_csr - K_coo| = {err:.3e}, max |K| = {scale:.3e}")
    assert scale > 0 and np.isfinite(vals).all()
    assert err <= TOL_COO * scale, f"{what}: CSR vs COO {err:.3e} > {TOL_COO * scale:.3e}"
    if dirichlet:  # identity rows and columns, structurally present
        fixed = np.nonzero(K_coo.diagonal() == 1.0)[0]
        fixed = [i for i in fixed if np.count_nonzero(K_coo[i]) == 1]
        for i in fixed[:8]:
            assert np.count_nonzero(K[i]) == 1 and K[i, i] == 1.0 and np.count_nonzero(K[:, i]) == 1
            assert row_ptr[i + 1] - row_ptr[i] == pattern[i] > 1, "the zeroed entries of a Dirichlet row stay in the structure"
    return K, (row_ptr, cols, vals), nb


# ------------------------------------------------------------------------------------------------ 1. values and structure
@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("law", ["neo-hookean", "hencky", "drucker-prager", "von-mises", "matsuoka-nakai"])
def test_values_and_structure(ndim, law):
    frictional = law == "matsuoka-nakai"
    s = _linearised(ndim, law)
    S, o, na = s["S"], s["o"], s["na"]
    if law in ("drucker-prager", "von-mises"):
        assert (s["P"]["eps_n1"] > s["P"]["eps_n"]).sum() > 0, "some particles must be plastic"
    for alpha_1, mass, dirichlet in ((0.0, None, False), (4.0e4, s["Mv"], True)):
        what = f"{law} {ndim}-D (alpha_1={alpha_1}, dirichlet={dirichlet})"
        K, _, _ = check_against_coo(S, alpha_1, mass, dirichlet, what)
        if not (frictional and ndim == 3):
            K_o, _, st = o.tangent_matrix(s["P"], s["M"], s["mats"], s["n2m"], s["d2m"] if dirichlet else None, na, alpha_1,
                                          mass, with_pattern=False)
            assert st == 0
            tol = 1e-10 if law == "neo-hookean" else (1e-7 if frictional else 1e-8)
            err = np.abs(K - K_o).max() / np.abs(K_o).max()
            print(f"{what}: vs the oracle {err:.3e}")
            assert err <= tol, f"{what}: CSR vs the oracle {err:.3e} > {tol:.1e}"
    S.close()


# ------------------------------------------------------------------------------------------------ 2. the fluid law
@pytest.mark.parametrize("ndim", [2, 3])
def test_fluid_law(ndim):
    c = FluidCase(ndim)
    S = c.S
    dU = 1e-3 * c.rng.normal(size=c.ntot)
    c.residual_gpu(dU)
    S.set_tangent_alpha4(c.a["a4"])
    for alpha_1, mass, dirichlet in ((0.0, None, False), (c.a["a1"], c.Mv, True)):
        K, _, _ = check_against_coo(S, alpha_1, mass, dirichlet, f"fluid {ndim}-D (alpha_1={alpha_1})")
        if mass is None:
            assert np.abs(K - K.T).max() > 1e-4 * np.abs(K).max(), "the fluid's blocks are not symmetric"
    c.close()


# ------------------------------------------------------------------------------------------------ 3. the mixed cloud
@pytest.mark.parametrize("ndim", [2, 3])
def test_mixed_cloud(ndim):
    case = _case(ndim, DP)
    npart = case["cloud"]["x"].shape[0]
    case["materials"] = [{"type": 0, "E": 2.0e4, "nu": 0.3}, {"type": 1, "E": 1.0e4, "nu": 0.25}, DP]
    case["cloud"]["matidx"] = (np.arange(npart) % 3).astype(np.int32)
    S = gpu_setup(case, nsteps=2)
    S.local_search()
    S.active_masks(nlps().BccSet([dirichlet_plane(case, ndim - 1, 3, 2)]), 1)
    ntot = S.nactive * ndim
    S.local_compatibility_conditions(8e-3 * np.random.default_rng(5).normal(size=ntot))
    S.constitutive_update()
    Mv = S.compute_nodal_lumped_mass()
    for alpha_1, mass, dirichlet in ((0.0, None, False), (3.0e3, Mv, True)):
        check_against_coo(S, alpha_1, mass, dirichlet, f"mixed {ndim}-D")
    S.close()


# ------------------------------------------------------------------------------------------------ 4. the damage cloud
def damaged(name, det):
    case, driver, dU = erosion_problem(name)
    M_o = oracle_setup(case)[0]
    return case, driver, dU, M_o, [DamageHandle(case, driver, M_o, det) for _ in range(2 if det else 1)]


@pytest.mark.parametrize("name", ["2-D Neo-Hookean", "3-D Neo-Hookean"])
def test_damage_cloud(name):
    case, driver, dU, M_o, (h,) = damaged(name, False)
    h.residual(dU)
    dmg = h.S.download_state()["Damage_n1"]
    assert 0 < np.count_nonzero(dmg) < dmg.size, "part of the cloud must be damaged"
    for alpha_1, mass, dirichlet in ((0.0, None, False), (h.alpha[0], h.M, True)):
        check_against_coo(h.S, alpha_1, mass, dirichlet, f"eigenerosion {name}")
    h.close()


# ------------------------------------------------------------------------------------------------ 5. shapes of the row walk
def linearise(case, seed=3, amp=5e-3, bcs_list=(), numbering=None):
    """searched, masked (step 0), one compatibility + constitutive pass at a random dU; returns (S, M)"""
    S = gpu_setup(case, nsteps=2)
    if numbering is not None:
        S.set_node_numbering(numbering)
    S.local_search()
    S.n2m_last, _ = S.active_masks(nlps().BccSet(list(bcs_list)), 0)
    ntot = S.nactive * case["ndim"]
    S.local_compatibility_conditions(amp * np.random.default_rng(seed).normal(size=ntot))
    S.constitutive_update()
    return S, S.compute_nodal_lumped_mass()


STAGED = {2: 4, 3: 8}  # particles the row kernel stages per pass (CsrCfg::CH)


def dense_cloud(ndim, per_axis):
    """a block of 3 x 3 (x 2) cells with per_axis[a] particles along axis a of every cell: 20 per cell in 2-D, 27 in 3-D"""
    if ndim == 2:
        case = make_case(2, [11, 10], [4, 3], [3, 3], material=NH, ppc=1)
    else:
        case = make_case(3, [9, 9, 8], [3, 3, 3], [3, 3, 2], material=NH, ppc=1)
    cl = case["cloud"]
    k = int(np.prod(per_axis))
    sub = np.stack(np.meshgrid(*[(np.arange(m) + 0.5) / m - 0.5 for m in per_axis], indexing="ij"), axis=-1).reshape(-1, ndim)
    centre = np.floor(cl["x"] / case["h"]) * case["h"] + 0.5 * case["h"]
    rng = np.random.default_rng(9)
    x = (centre[:, None, :] + case["h"] * sub[None, :, :]).reshape(-1, ndim)
    x = x + rng.uniform(-0.02, 0.02, size=x.shape) * case["h"]
    out = {}
    for key, v in cl.items():
        out[key] = np.repeat(v, k, axis=0) if isinstance(v, np.ndarray) else v
    out["x"] = np.ascontiguousarray(x)
    out["vol0"] = out["vol0"] / k
    out["mass"] = out["mass"] / k
    case["cloud"] = out
    return case, k


@pytest.mark.parametrize("ndim", [2, 3])
def test_long_node_runs(ndim):
    """27 particles per cell in 3-D, 5 x 4 in 2-D: the run of a closest node is far longer than one staging pass"""
    case, k = dense_cloud(ndim, [5, 4] if ndim == 2 else [3, 3, 3])
    assert k == (20 if ndim == 2 else 27)
    S, Mv = linearise(case)
    I0 = S.download_state()["I0"]
    longest = int(np.bincount(I0).max())
    print(f"{ndim}-D: longest node run {longest}")
    assert longest > 2 * STAGED[ndim], "a node run must take more than two staging passes"
    check_against_coo(S, 2.0e3, Mv, False, f"{k} particles per cell, {ndim}-D")
    S.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_cloud_against_the_grid_boundary(ndim):
    """the block sits in the corner of the grid: column offsets of the boundary rows fall off the grid"""
    if ndim == 2:
        case = make_case(2, [9, 8], [0, 0], [4, 3], material=NH)
    else:
        case = make_case(3, [7, 6, 6], [0, 0, 0], [3, 2, 2], material=NH)
    S, Mv = linearise(case, bcs_list=[dirichlet_plane(case, ndim - 1, 0, 2)])
    check_against_coo(S, 1.0e3, Mv, True, f"corner cloud {ndim}-D")
    S.close()


def subset(case, keep):
    case["cloud"] = {k: (np.ascontiguousarray(v[keep]) if isinstance(v, np.ndarray) else v) for k, v in case["cloud"].items()}
    return case


@pytest.mark.parametrize("ndim", [2, 3])
def test_ragged_cloud(ndim):
    """two thirds of the particles removed at random: active nodes that are members of lists but nobody's closest node"""
    case = _case(ndim, DP, velocity=False)
    npart = case["cloud"]["x"].shape[0]
    keep = np.sort(np.random.default_rng(17).permutation(npart)[: npart // 3])
    subset(case, keep)
    S, Mv = linearise(case, bcs_list=[dirichlet_plane(case, ndim - 1, 3, 2)])
    I0 = S.download_state()["I0"]
    assert S.nactive > np.unique(I0).size, "some active nodes are nobody's closest node"
    check_against_coo(S, 1.0e3, Mv, True, f"ragged cloud {ndim}-D")
    S.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_single_particle(ndim):
    case = subset(_case(ndim, NH, velocity=False), np.array([5]))
    S, Mv = linearise(case)
    assert S.num_particles() == 1
    _, (row_ptr, _, _), _ = check_against_coo(S, 0.0, None, False, f"one particle {ndim}-D")
    members = np.count_nonzero(np.diff(row_ptr)) // ndim
    assert row_ptr[-1] == (members * ndim) ** 2, "one particle: every pair of its member nodes"
    S.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_no_particles(ndim):
    case = subset(_case(ndim, NH, velocity=False), np.zeros(0, dtype=np.int64))
    S = gpu_setup(case, nsteps=2)
    assert S.np == 0
    S.local_search()
    S.active_masks(nlps().BccSet([]), 0)
    S.tangent_operator(0.0, None, False)
    nnz, nb = S.tangent_csr_pattern()
    assert nnz == 0
    row_ptr, cols, vals = S.tangent_csr()
    assert row_ptr.shape == (S.nactive * ndim + 1,) and not row_ptr.any() and cols.size == 0 and vals.size == 0
    S.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_permuted_node_numbering(ndim):
    """a caller's numbering that does not ascend with the grid order: the columns are sorted per row"""
    case = _case(ndim, NH, velocity=False)
    nn = int(np.prod(case["grid_n"]))
    perm = np.random.default_rng(23).permutation(nn).astype(np.int32)
    S, Mv = linearise(case, bcs_list=[dirichlet_plane(case, ndim - 1, 3, 2)], numbering=perm)
    n2m_lat = np.empty(nn, dtype=np.int32)
    n2m_lat[perm] = S.n2m_last  # (Nodes2Mask comes back indexed by file node)
    act = n2m_lat[n2m_lat >= 0]
    assert (np.diff(act) < 0).any(), "the masked numbers must not ascend with the grid order"
    check_against_coo(S, 1.0e3, Mv, True, f"permuted numbering {ndim}-D")
    S.close()


# ------------------------------------------------------------------------------------------------ 6. replay
def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a, b), f"{what}: not bit-identical"


def test_two_calls_on_one_linearisation():
    s = _linearised(3, "drucker-prager", with_oracle=False)
    S = s["S"]
    S.tangent_operator(2.0e3, s["Mv"], True)
    S.tangent_csr_pattern()
    a = S.tangent_csr()
    S.jacobian_evaluation(2.0e3, s["Mv"], True)  # (the atomic path shares the sort buffers: the CSR path keeps its own list)
    b = S.tangent_csr()
    for x, y, k in zip(a, b, ("row_ptr", "cols", "vals")):
        same(x, y, f"second call: {k}")
    S.close()


def det_run(ndim, law):
    """a fresh handle in deterministic mode: residual -> operator -> pattern -> CSR"""
    case = _case(ndim, {"nh": NH, "dp": DP}[law])
    S = gpu_setup(case, nsteps=3)
    S.set_deterministic(True)
    S.local_search()
    S.active_masks(nlps().BccSet([dirichlet_plane(case, ndim - 1, 3, 3)]), 0)
    M = S.compute_nodal_lumped_mass()
    V, A = S.get_nodal_field_n(M)
    alpha = _alpha(1.0e-2)
    dU = (2e-2 if law == "nh" else 8e-3) * np.random.default_rng(7).normal(size=S.nactive * ndim)
    S.lagrangian_evaluation(dU, V, A, M, alpha, [0.0] * (ndim - 1) + [-9.81])
    S.tangent_operator(alpha[0], M, True)
    S.tangent_csr_pattern()
    out = S.tangent_csr()
    S.close()
    return out


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("law", ["nh", "dp"])
def test_deterministic_replay(ndim, law):
    a, b = det_run(ndim, law), det_run(ndim, law)
    assert a[2].size > 0 and np.abs(a[2]).max() > 0
    for x, y, k in zip(a, b, ("row_ptr", "cols", "vals")):
        same(x, y, f"{law} {ndim}-D, two fresh handles: {k}")


@pytest.mark.parametrize("name", ["2-D Neo-Hookean", "3-D Neo-Hookean"])
def test_deterministic_replay_of_a_damage_cloud(name):
    case, driver, dU, M_o, hs = damaged(name, True)
    out = []
    for h in hs:
        h.residual(dU)
        h.S.tangent_operator(h.alpha[0], h.M, True)
        h.S.tangent_csr_pattern()
        out.append(h.S.tangent_csr())
    dmg = hs[0].S.download_state()["Damage_n1"]
    assert 0 < np.count_nonzero(dmg) < dmg.size
    for x, y, k in zip(out[0], out[1], ("row_ptr", "cols", "vals")):
        same(x, y, f"damage cloud {name}, two handles: {k}")
    for h in hs:
        h.close()


# ------------------------------------------------------------------------------------------------ 7. destinations
def test_host_and_device_destinations():
    import torch
    s = _linearised(3, "hencky", with_oracle=False)
    S = s["S"]
    S.tangent_operator(2.0e3, s["Mv"], True)
    nnz, _ = S.tangent_csr_pattern()
    host = S.tangent_csr()
    dev = S.tangent_csr(on_device=True)
    torch.cuda.synchronize()
    for x, y, k in zip(host, dev, ("row_ptr", "cols", "vals")):
        assert isinstance(y, torch.Tensor) and y.is_cuda
        same(x, y.cpu().numpy(), f"device destination: {k}")
    S.close()


# ------------------------------------------------------------------------------------------------ 8. bytes
def test_bytes_formula_and_no_stencil_array():
    s = _linearised(2, "neo-hookean", with_oracle=False)
    S = s["S"]
    S.tangent_operator(0.0, None, False)
    _, nb = S.tangent_csr_pattern()
    assert nb == csr_bytes(2, S.num_particles(), int(np.prod(_case(2, NH)["grid_n"])), S.nactive)
    S.close()
    # a 3-D block inside a grid of 40^3 nodes: the atomic path would clear a stencil array of 8 * 9 * 729 * nnodes bytes
    case = make_case(3, [39, 39, 39], [17, 17, 17], [4, 4, 4], material=NH)
    S, Mv = linearise(case)
    nnodes = 40 ** 3
    assert int(np.prod(case["grid_n"])) == nnodes
    S.tangent_operator(1.0e3, Mv, False)
    nnz, nb = S.tangent_csr_pattern()
    assert nb == csr_bytes(3, S.num_particles(), nnodes, S.nactive)
    stencil = 8 * 9 * 729 * nnodes
    print(f"CSR path keeps {nb} bytes, the stencil array of the atomic path {stencil}: {nb / stencil:.4%}")
    assert nb < 0.01 * stencil
    row_ptr, cols, vals = S.tangent_csr()
    assert row_ptr[-1] == nnz > 0 and ascending(row_ptr, cols) and np.isfinite(vals).all()
    S.close()


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals():
    import ctypes as C
    n = nlps()
    s = _linearised(2, "neo-hookean", with_oracle=False)
    S, Mv = s["S"], s["Mv"]
    ntot = s["na"] * 2
    z = np.zeros(ntot)
    with pytest.raises(n.NlpsError, match="nlps_gpu_tangent_csr_pattern: call nlps_gpu_tangent_operator\\(\\) first"):
        S.tangent_csr_pattern()
    with pytest.raises(n.NlpsError, match="nlps_gpu_tangent_csr: call nlps_gpu_tangent_operator\\(\\) first"):
        S.tangent_csr()
    S.tangent_operator(1.0e3, Mv, True)
    with pytest.raises(n.NlpsError, match="nlps_gpu_tangent_csr: call nlps_gpu_tangent_csr_pattern\\(\\)"):
        S.tangent_csr()
    nnz, _ = S.tangent_csr_pattern()
    S.tangent_csr()
    # a new linearisation needs a new pattern
    S.tangent_operator(1.0e3, Mv, True)
    with pytest.raises(n.NlpsError, match="nlps_gpu_tangent_csr: call nlps_gpu_tangent_csr_pattern\\(\\)"):
        S.tangent_csr()
    S.tangent_csr_pattern()
    # NULL destinations
    row_ptr, cols, vals = np.zeros(ntot + 1, dtype=np.int32), np.zeros(nnz, dtype=np.int32), np.zeros(nnz)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for args in ((None, cols, vals), (row_ptr, None, vals), (row_ptr, cols, None)):
        assert S.L.nlps_gpu_tangent_csr(S.h, *[vp(a) for a in args]) == 1
        assert "row_ptr, cols and vals are required" in S.L.nlps_gpu_last_error(S.h).decode()
    # a halo callback attached
    S.set_halo_exchange(lambda dptr, nfield, elem, kind: 0)
    for call in (S.tangent_csr_pattern, S.tangent_csr):
        with pytest.raises(n.NlpsError, match="one rank.*halo callback"):
            call()
    S.set_halo_exchange(None)
    S.tangent_csr()
    # stale after a search, the kinetics update and the roll
    bcs = n.BccSet([dirichlet_plane(_case(2, NH), 1, 3, 2)])
    for what, call in (("nlps_gpu_local_search", S.local_search),
                       ("nlps_gpu_update_kinetics", lambda: S.update_particles_kinetics_FLIP_PIC(1.0, z, z, z, z)),
                       ("nlps_gpu_roll_state", S.update_particles_internal_variables)):
        S.local_search()
        S.active_masks(bcs, 1)
        S.tangent_operator(1.0e3, Mv, True)
        S.tangent_csr_pattern()
        S.tangent_csr()
        call()
        with pytest.raises(n.NlpsError, match="nlps_gpu_tangent_csr: .*stale: .*" + what):
            S.tangent_csr()
        with pytest.raises(n.NlpsError, match="nlps_gpu_tangent_csr_pattern: .*stale: .*" + what):
            S.tangent_csr_pattern()
    S.close()
