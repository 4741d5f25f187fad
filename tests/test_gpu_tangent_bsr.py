"""The tangent in block CSR, every block or the upper blocks of a symmetric tangent (nlps_gpu_tangent_bsr_pattern /
nlps_gpu_tangent_bsr).  The reference is never the code under test: the CSR arrays of the same
linearisation (nlps_gpu_tangent_csr, held to the COO matrix and the oracle by tests/test_gpu_tangent_csr.py) rearranged
by numpy (tests/bsr_ref.py, checked alone in tests/test_bsr_ref.py).  Structure and values are compared exactly: a kept
block is the same sum in the same order.  The completed upper form against the dense COO matrix: TOL_COO, the project's
bound between two summation orders of the same blocks."""
import numpy as np
import pytest

import bsr_ref
from test_gpu_tangent_csr import (TOL_COO, DamageHandle, FluidCase, check_against_coo, damaged, dense_cloud, linearise, same,
                                  subset)
from test_gpu_tangent_operator import _case, _linearised
from util import DP, NH, dirichlet_plane, gpu_setup, nlps

pytestmark = pytest.mark.gpu

SETTINGS = ((0.0, None, False), (4.0e4, "Mv", True))  # (alpha_1, mass, dirichlet) of the operator


def bsr_bytes(ndim, npart, nnodes, nactive):
    """the formula of include/nlps_gpu.h"""
    w = 12 if ndim == 3 else 2
    csr = 8 * npart * (ndim ** 4 + 6 * ndim + 2) + 4 * (nnodes + 1) + 8 * w * nnodes + 8 * (nactive + 1)
    return csr + 8 * (nactive + 1) + 4


def csr_now(S):
    S.tangent_csr_pattern()
    return S.tangent_csr()


def check_against_csr(S, kind, csr, what, layouts=(False, True)):
    """pattern + emit of `kind` on the current linearisation against the rearranged CSR arrays, bit for bit, in both block
    layouts; returns the row-major arrays"""
    d = S.ndim
    upper = kind == "upper"
    ref = bsr_ref.bsr_from_csr(*csr, d, upper=upper)
    nblocks, nbytes = S.tangent_bsr_pattern(kind)
    assert nblocks == ref[1].size, f"{what} {kind}: nblocks {nblocks} vs {ref[1].size}"
    if not upper:
        assert nblocks * d * d == csr[1].size, f"{what}: nblocks d^2 vs the nnz of the CSR pattern"
    out = None
    for col_major in layouts:
        brow_ptr, bcols, vals = S.tangent_bsr(col_major=col_major)
        assert brow_ptr.shape == (S.nactive + 1,) and bcols.shape == (nblocks,) and vals.shape == (nblocks, d, d)
        assert np.array_equal(brow_ptr, ref[0]), f"{what} {kind}: brow_ptr"
        assert np.array_equal(bcols, ref[1]), f"{what} {kind}: bcols"
        assert bsr_ref.ascending(brow_ptr, bcols), f"{what} {kind}: bcols do not ascend in every block row"
        got = vals.transpose(0, 2, 1) if col_major else vals
        assert np.array_equal(got, ref[2]), f"{what} {kind} (col_major={col_major}): values differ from the CSR entries"
        if upper:
            assert all((bcols[a:b] >= A).all() for A, (a, b) in enumerate(zip(brow_ptr[:-1], brow_ptr[1:])))
        if not col_major:
            out = (brow_ptr, bcols, vals)
    return out


def check_both_kinds(S, csr, what):
    """full and upper against the CSR arrays, and the count identity FULL = 2 UPPER - diagonal blocks"""
    full = check_against_csr(S, "full", csr, what)
    up = check_against_csr(S, "upper", csr, what)
    diag = bsr_ref.diagonal_blocks(up[0], up[1])
    assert diag == bsr_ref.diagonal_blocks(full[0], full[1])
    assert full[1].size == 2 * up[1].size - diag, f"{what}: FULL = 2 UPPER - diagonal blocks"
    return full, up


# ------------------------------------------------------------------------------------------------ 1. full, every law
@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("law", ["neo-hookean", "hencky", "drucker-prager", "von-mises", "matsuoka-nakai"])
def test_full_form_of_every_law(ndim, law):
    s = _linearised(ndim, law, with_oracle=False)
    S = s["S"]
    for alpha_1, mass, dirichlet in SETTINGS:
        S.tangent_operator(alpha_1, s["Mv"] if mass else None, dirichlet)
        check_against_csr(S, "full", csr_now(S), f"{law} {ndim}-D (alpha_1={alpha_1})")
    S.close()


# ------------------------------------------------------------------------------------------------ 2. upper, Neo-Hookean
def check_upper_against_coo(S, alpha_1, mass, dirichlet, what):
    K_coo_like, csr, _ = check_against_coo(S, alpha_1, mass, dirichlet, what)  # (leaves this linearisation current)
    r, c, v = S.jacobian_evaluation(alpha_1, mass, dirichlet)
    ntot = S.nactive * S.ndim
    K_coo = np.zeros((ntot, ntot))
    np.add.at(K_coo, (r, c), v)
    _, up = check_both_kinds(S, csr, what)
    K_up = bsr_ref.dense_of_bsr(*up, S.ndim, upper=True)
    scale = np.abs(K_coo).max()
    err = np.abs(K_up - K_coo).max()
    print(f"{what}: completed upper form against the COO matrix {err:.3e}, max |K| = {scale:.3e}")
    assert err <= TOL_COO * scale, f"{what}: completed upper form vs COO {err:.3e} > {TOL_COO * scale:.3e}"


@pytest.mark.parametrize("ndim", [2, 3])
def test_upper_form_of_a_neo_hookean_cloud(ndim):
    s = _linearised(ndim, "neo-hookean", with_oracle=False)
    for alpha_1, mass, dirichlet in SETTINGS:
        check_upper_against_coo(s["S"], alpha_1, s["Mv"] if mass else None, dirichlet, f"neo-hookean {ndim}-D (alpha_1={alpha_1})")
    s["S"].close()


@pytest.mark.parametrize("name", ["2-D Neo-Hookean", "3-D Neo-Hookean"])
def test_upper_form_of_a_damage_cloud(name):
    case, driver, dU, M_o, (h,) = damaged(name, False)
    h.residual(dU)
    dmg = h.S.download_state()["Damage_n1"]
    assert 0 < np.count_nonzero(dmg) < dmg.size, "part of the cloud must be damaged"
    for alpha_1, mass, dirichlet in ((0.0, None, False), (h.alpha[0], h.M, True)):
        check_upper_against_coo(h.S, alpha_1, mass, dirichlet, f"eigenerosion {name}")
    h.close()


# ------------------------------------------------------------------------------------------------ 3. upper refused
def refused_then_full(S, Mv, law_word, what):
    n = nlps()
    S.tangent_operator(2.0e3, Mv, True)
    with pytest.raises(n.NlpsError, match="nlps_gpu_tangent_bsr_pattern: NLPS_BSR_UPPER.*" + law_word):
        S.tangent_bsr_pattern("upper")
    check_against_csr(S, "full", csr_now(S), what)


@pytest.mark.parametrize("law,word", [("hencky", "Hencky"), ("drucker-prager", "Drucker-Prager")])
def test_upper_refused_for_an_unsymmetric_law(law, word):
    s = _linearised(3, law, with_oracle=False)
    refused_then_full(s["S"], s["Mv"], word, law)
    s["S"].close()


def test_upper_refused_for_the_fluid_law():
    c = FluidCase(2)
    c.residual_gpu(1e-3 * c.rng.normal(size=c.ntot))
    c.S.set_tangent_alpha4(c.a["a4"])
    refused_then_full(c.S, c.Mv, "Newtonian-Fluid", "fluid")
    c.close()


def test_upper_refused_for_a_mixed_cloud():
    case = _case(2, DP)
    npart = case["cloud"]["x"].shape[0]
    case["materials"] = [{"type": 0, "E": 2.0e4, "nu": 0.3}, {"type": 1, "E": 1.0e4, "nu": 0.25}, DP]
    case["cloud"]["matidx"] = (np.arange(npart) % 3).astype(np.int32)
    S = gpu_setup(case, nsteps=2)
    S.local_search()
    S.active_masks(nlps().BccSet([dirichlet_plane(case, 1, 3, 2)]), 1)
    S.local_compatibility_conditions(8e-3 * np.random.default_rng(5).normal(size=S.nactive * 2))
    S.constitutive_update()
    refused_then_full(S, S.compute_nodal_lumped_mass(), "Hencky, Drucker-Prager", "mixed")
    S.close()


# ------------------------------------------------------------------------------------------------ 4. numbering and shapes
def both_kinds_of(S, Mv, alpha_1, dirichlet, what):
    S.tangent_operator(alpha_1, Mv if alpha_1 else None, dirichlet)
    return check_both_kinds(S, csr_now(S), what)


@pytest.mark.parametrize("ndim", [2, 3])
def test_permuted_node_numbering(ndim):
    """upper is decided by the masked numbers, which do not ascend with the grid order here, and bcols ascend"""
    case = _case(ndim, NH, velocity=False)
    nn = int(np.prod(case["grid_n"]))
    perm = np.random.default_rng(23).permutation(nn).astype(np.int32)
    S, Mv = linearise(case, bcs_list=[dirichlet_plane(case, ndim - 1, 3, 2)], numbering=perm)
    n2m_lat = np.empty(nn, dtype=np.int32)
    n2m_lat[perm] = S.n2m_last
    act = n2m_lat[n2m_lat >= 0]
    assert (np.diff(act) < 0).any(), "the masked numbers must not ascend with the grid order"
    both_kinds_of(S, Mv, 1.0e3, True, f"permuted numbering {ndim}-D")
    S.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_long_node_runs(ndim):
    case, k = dense_cloud(ndim, [5, 4] if ndim == 2 else [3, 3, 3])
    S, Mv = linearise(case)
    both_kinds_of(S, Mv, 2.0e3, False, f"{k} particles per cell, {ndim}-D")
    S.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_cloud_against_the_grid_boundary(ndim):
    from util import make_case
    if ndim == 2:
        case = make_case(2, [9, 8], [0, 0], [4, 3], material=NH)
    else:
        case = make_case(3, [7, 6, 6], [0, 0, 0], [3, 2, 2], material=NH)
    S, Mv = linearise(case, bcs_list=[dirichlet_plane(case, ndim - 1, 0, 2)])
    both_kinds_of(S, Mv, 1.0e3, True, f"corner cloud {ndim}-D")
    S.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_ragged_cloud(ndim):
    case = _case(ndim, NH, velocity=False)
    npart = case["cloud"]["x"].shape[0]
    subset(case, np.sort(np.random.default_rng(17).permutation(npart)[: npart // 3]))
    S, Mv = linearise(case, bcs_list=[dirichlet_plane(case, ndim - 1, 3, 2)])
    both_kinds_of(S, Mv, 1.0e3, True, f"ragged cloud {ndim}-D")
    S.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_single_particle(ndim):
    S, Mv = linearise(subset(_case(ndim, NH, velocity=False), np.array([5])))
    assert S.num_particles() == 1
    full, up = both_kinds_of(S, Mv, 0.0, False, f"one particle {ndim}-D")
    members = np.count_nonzero(np.diff(full[0]))
    assert full[1].size == members ** 2 and up[1].size == members * (members + 1) // 2
    S.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_no_particles(ndim):
    S = gpu_setup(subset(_case(ndim, NH, velocity=False), np.zeros(0, dtype=np.int64)), nsteps=2)
    S.local_search()
    S.active_masks(nlps().BccSet([]), 0)
    S.tangent_operator(0.0, None, False)
    for kind in ("full", "upper"):
        nblocks, _ = S.tangent_bsr_pattern(kind)
        assert nblocks == 0
        brow_ptr, bcols, vals = S.tangent_bsr()
        assert brow_ptr.shape == (S.nactive + 1,) and not brow_ptr.any() and bcols.size == 0 and vals.size == 0
    brow_ptr = np.ones(S.nactive + 1, dtype=np.int32)
    import ctypes as C
    assert S.L.nlps_gpu_tangent_bsr(S.h, 0, brow_ptr.ctypes.data_as(C.c_void_p), None, None) == 0 and not brow_ptr.any()
    S.close()


# ------------------------------------------------------------------------------------------------ 5. replays
def test_two_calls_destinations_and_both_patterns_on_one_linearisation():
    import torch
    s = _linearised(3, "neo-hookean", with_oracle=False)
    S = s["S"]
    S.tangent_operator(2.0e3, s["Mv"], True)
    # a CSR pattern first, then the block pattern: _bsr works; then _csr still returns its arrays
    csr = csr_now(S)
    for kind in ("full", "upper"):
        a = check_against_csr(S, kind, csr, "after csr_pattern", layouts=(False,))
        for x, y, k in zip(csr, S.tangent_csr(), ("row_ptr", "cols", "vals")):
            same(x, y, f"tangent_csr after tangent_bsr_pattern({kind}): {k}")
        S.jacobian_evaluation(2.0e3, s["Mv"], True)  # (the atomic path shares the sort buffers)
        b = S.tangent_bsr()
        dev = S.tangent_bsr(on_device=True)
        torch.cuda.synchronize()
        for x, y, z, k in zip(a, b, dev, ("brow_ptr", "bcols", "vals")):
            same(x, y, f"{kind}, second call: {k}")
            assert isinstance(z, torch.Tensor) and z.is_cuda
            same(x, z.cpu().numpy(), f"{kind}, device destination: {k}")
    # a new linearisation, the block pattern first: the records are built by it, and a CSR pattern made after it
    # leaves it valid
    S.tangent_operator(2.0e3, s["Mv"], True)
    S.tangent_bsr_pattern("upper")
    first = S.tangent_bsr()
    csr2 = csr_now(S)
    for x, y, k in zip(csr, csr2, ("row_ptr", "cols", "vals")):
        same(x, y, f"tangent_csr after a block pattern built the records: {k}")
    for x, y, k in zip(first, S.tangent_bsr(), ("brow_ptr", "bcols", "vals")):
        same(x, y, f"tangent_bsr after tangent_csr_pattern: {k}")
    S.close()


def det_run(ndim, kind):
    """a fresh handle in deterministic mode: residual -> operator -> pattern -> block CSR"""
    from test_gpu_newton_solve import _alpha
    case = _case(ndim, NH)
    S = gpu_setup(case, nsteps=3)
    S.set_deterministic(True)
    S.local_search()
    S.active_masks(nlps().BccSet([dirichlet_plane(case, ndim - 1, 3, 3)]), 0)
    M = S.compute_nodal_lumped_mass()
    V, A = S.get_nodal_field_n(M)
    alpha = _alpha(1.0e-2)
    dU = 2e-2 * np.random.default_rng(7).normal(size=S.nactive * ndim)
    S.lagrangian_evaluation(dU, V, A, M, alpha, [0.0] * (ndim - 1) + [-9.81])
    S.tangent_operator(alpha[0], M, True)
    S.tangent_bsr_pattern(kind)
    out = S.tangent_bsr()
    S.close()
    return out


@pytest.mark.parametrize("ndim,kind", [(2, "upper"), (3, "upper"), (3, "full")])
def test_deterministic_replay(ndim, kind):
    a, b = det_run(ndim, kind), det_run(ndim, kind)
    assert a[2].size > 0 and np.abs(a[2]).max() > 0
    for x, y, k in zip(a, b, ("brow_ptr", "bcols", "vals")):
        same(x, y, f"{kind} {ndim}-D, two fresh handles: {k}")


def test_deterministic_replay_of_a_damage_cloud():
    case, driver, dU, M_o, hs = damaged("3-D Neo-Hookean", True)
    out = []
    for h in hs:
        h.residual(dU)
        h.S.tangent_operator(h.alpha[0], h.M, True)
        h.S.tangent_bsr_pattern("upper")
        out.append(h.S.tangent_bsr())
    for x, y, k in zip(out[0], out[1], ("brow_ptr", "bcols", "vals")):
        same(x, y, f"damage cloud, two handles: {k}")
    for h in hs:
        h.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_each_followed_by_a_good_call():
    import ctypes as C
    n = nlps()
    s = _linearised(2, "neo-hookean", with_oracle=False)
    S, Mv = s["S"], s["Mv"]
    with pytest.raises(n.NlpsError, match="nlps_gpu_tangent_bsr_pattern: call nlps_gpu_tangent_operator\\(\\) first"):
        S.tangent_bsr_pattern()
    with pytest.raises(n.NlpsError, match="nlps_gpu_tangent_bsr: call nlps_gpu_tangent_operator\\(\\) first"):
        S.tangent_bsr()
    S.tangent_operator(1.0e3, Mv, True)
    with pytest.raises(n.NlpsError, match="nlps_gpu_tangent_bsr: call nlps_gpu_tangent_bsr_pattern\\(\\)"):
        S.tangent_bsr()
    csr = csr_now(S)
    with pytest.raises(n.NlpsError, match="nlps_gpu_tangent_bsr: call nlps_gpu_tangent_bsr_pattern\\(\\)"):
        S.tangent_bsr()  # (a CSR pattern is no block pattern)
    check_against_csr(S, "upper", csr, "after the refusals")
    # an unknown kind: refused, and no pattern is left behind
    with pytest.raises(n.NlpsError, match="nlps_gpu_tangent_bsr_pattern: kind 2 "):
        S.tangent_bsr_pattern(2)
    with pytest.raises(n.NlpsError, match="nlps_gpu_tangent_bsr: call nlps_gpu_tangent_bsr_pattern\\(\\)"):
        S.tangent_bsr()
    nblocks, _ = S.tangent_bsr_pattern("full")
    # NULL destinations
    brow_ptr, bcols, vals = np.zeros(S.nactive + 1, dtype=np.int32), np.zeros(nblocks, dtype=np.int32), np.zeros(nblocks * 4)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for args in ((None, bcols, vals), (brow_ptr, None, vals), (brow_ptr, bcols, None)):
        assert S.L.nlps_gpu_tangent_bsr(S.h, 0, *[vp(a) for a in args]) == 1
        assert "brow_ptr, bcols and vals are required" in S.L.nlps_gpu_last_error(S.h).decode()
    check_against_csr(S, "full", csr, "after NULL destinations")
    # a halo callback attached
    S.set_halo_exchange(lambda dptr, nfield, elem, kind: 0)
    for call in (S.tangent_bsr_pattern, S.tangent_bsr):
        with pytest.raises(n.NlpsError, match="one rank.*halo callback"):
            call()
    S.set_halo_exchange(None)
    check_against_csr(S, "full", csr, "after the halo callback")
    # a new linearisation needs a new pattern; stale after a search
    S.tangent_operator(1.0e3, Mv, True)
    with pytest.raises(n.NlpsError, match="nlps_gpu_tangent_bsr: call nlps_gpu_tangent_bsr_pattern\\(\\)"):
        S.tangent_bsr()
    S.tangent_bsr_pattern("upper")
    S.tangent_bsr()
    S.local_search()
    with pytest.raises(n.NlpsError, match="nlps_gpu_tangent_bsr: .*stale: .*nlps_gpu_local_search"):
        S.tangent_bsr()
    with pytest.raises(n.NlpsError, match="nlps_gpu_tangent_bsr_pattern: .*stale: .*nlps_gpu_local_search"):
        S.tangent_bsr_pattern("upper")
    S.active_masks(n.BccSet([dirichlet_plane(_case(2, NH), 1, 3, 2)]), 1)
    S.tangent_operator(1.0e3, Mv, True)
    check_both_kinds(S, csr_now(S), "after the stale refusal")
    S.close()


# ------------------------------------------------------------------------------------------------ 7. bytes
def test_bytes_formula_shared_records_and_no_stencil_array():
    from util import make_case
    case = make_case(3, [39, 39, 39], [17, 17, 17], [4, 4, 4], material=NH)
    S, Mv = linearise(case)
    nnodes = 40 ** 3
    S.tangent_operator(1.0e3, Mv, False)
    expect = bsr_bytes(3, S.num_particles(), nnodes, S.nactive)
    _, nb_upper = S.tangent_bsr_pattern("upper")
    _, nb_csr = S.tangent_csr_pattern()
    _, nb_full = S.tangent_bsr_pattern("full")
    assert nb_upper == expect == nb_full, "the bytes do not grow with the other kind or with a CSR pattern beside it"
    assert nb_full - nb_csr == 8 * (S.nactive + 1) + 4, "beside the CSR path's bytes only the counts of the block rows"
    stencil = 8 * 9 * 729 * nnodes
    print(f"block-CSR path keeps {nb_full} bytes, a stencil array 8 d^2 9^d nnodes {stencil}: {nb_full / stencil:.4%}")
    assert nb_full < 0.01 * stencil
    S.close()
