"""tests/bsr_ref.py (the numpy reference of tests/test_gpu_tangent_bsr.py) alone, on the oracle's dense tangents of the
states test_gpu_tangent_operator._linearised builds: the round trip is exact, FULL = 2 UPPER - diagonal blocks, the
completed upper form of a Neo-Hookean tangent is K within 1e-14 max|K| (the oracle's own asymmetry there is 1.3e-16 in
2-D and 3.6e-17 in 3-D, 2.7e-17 and 6.1e-18 with alpha_1 M and the Dirichlet rows), and the Hencky tangent (1.8e-3) does
not pass that check: an upper form of it is not the matrix."""
import numpy as np
import pytest

import bsr_ref
from test_gpu_tangent_operator import LAWS, _case
from util import dirichlet_plane, oracle_setup, orc

AMP = {"neo-hookean": 2e-2, "hencky": 2e-2}
SYM_TOL = 1e-14
_cache = {}


def oracle_tangents(ndim, law, seed=13):
    """[K(0, no mass, no Dirichlet), K(4e4, M, Dirichlet)] of the oracle at _linearised's state, computed once per case"""
    if (ndim, law) not in _cache:
        o = orc()
        case = _case(ndim, LAWS[law])
        nsteps = 2
        M, P, prm, mats = oracle_setup(case)
        n2m, na = o.active_nodes(M)
        d2m, _ = o.active_dofs(n2m, na, ndim, o.BccSet([dirichlet_plane(case, ndim - 1, 3, nsteps)]), 1, nsteps)
        dU = AMP[law] * np.random.default_rng(seed).normal(size=na * ndim)
        assert o.compatibility(dU, None, P, M, n2m) == 0 and o.constitutive(P, mats, prm) == 0
        Mv = o.lumped_mass(P, M, n2m, na)
        Ks = []
        for alpha_1, mass, d in ((0.0, None, None), (4.0e4, Mv, d2m)):
            K, _, st = o.tangent_matrix(P, M, mats, n2m, d, na, alpha_1, mass, with_pattern=False)
            assert st == 0
            K.setflags(write=False)
            Ks.append(K)
        _cache[(ndim, law)] = Ks
    return _cache[(ndim, law)]


CASES = [(2, "neo-hookean"), (3, "neo-hookean"), (2, "hencky")]


@pytest.mark.parametrize("ndim,law", CASES)
def test_round_trip_and_counts(ndim, law):
    for K in oracle_tangents(ndim, law):
        row_ptr, cols, vals = bsr_ref.csr_of_dense(K, ndim)
        assert vals.size % (ndim * ndim) == 0 and vals.size > 0
        full = bsr_ref.bsr_from_csr(row_ptr, cols, vals, ndim)
        up = bsr_ref.bsr_from_csr(row_ptr, cols, vals, ndim, upper=True)
        nb = K.shape[0] // ndim
        for brow_ptr, bcols, bvals in (full, up):
            assert brow_ptr.shape == (nb + 1,) and brow_ptr[-1] == bcols.size == bvals.shape[0]
            assert bvals.shape[1:] == (ndim, ndim) and bsr_ref.ascending(brow_ptr, bcols)
        assert full[1].size * ndim * ndim == vals.size
        assert np.array_equal(bsr_ref.dense_of_bsr(*full, ndim), K), "the round trip of the full form is exact"
        swapped = np.ascontiguousarray(full[2].transpose(0, 2, 1))
        assert np.array_equal(bsr_ref.dense_of_bsr(full[0], full[1], swapped, ndim, col_major=True), K)
        # the structure is symmetric: every block above the diagonal has its mirror below it
        diag = bsr_ref.diagonal_blocks(full[0], full[1])
        assert diag == bsr_ref.diagonal_blocks(up[0], up[1]) == nb
        assert full[1].size == 2 * up[1].size - diag
        Ku = bsr_ref.dense_of_bsr(*up, ndim, upper=True)
        assert np.array_equal(np.triu(Ku, ndim), np.triu(K, ndim)), "the kept blocks are K's, bit for bit"
        assert all(np.array_equal(Ku[i:i + ndim, i:i + ndim], K[i:i + ndim, i:i + ndim]) for i in range(0, nb * ndim, ndim))


@pytest.mark.parametrize("ndim", [2, 3])
def test_completed_upper_form_of_a_neo_hookean_tangent(ndim):
    for K in oracle_tangents(ndim, "neo-hookean"):
        up = bsr_ref.bsr_from_csr(*bsr_ref.csr_of_dense(K, ndim), ndim, upper=True)
        err = np.abs(bsr_ref.dense_of_bsr(*up, ndim, upper=True) - K).max() / np.abs(K).max()
        print(f"Neo-Hookean {ndim}-D: completed upper form against K {err:.3e}")
        assert err <= SYM_TOL


def test_hencky_tangent_is_not_its_upper_form():
    for K in oracle_tangents(2, "hencky"):
        up = bsr_ref.bsr_from_csr(*bsr_ref.csr_of_dense(K, 2), 2, upper=True)
        err = np.abs(bsr_ref.dense_of_bsr(*up, 2, upper=True) - K).max() / np.abs(K).max()
        print(f"Hencky 2-D: completed upper form against K {err:.3e}")
        assert err > 1e-4, "the helper must not hide an unsymmetric tangent"


def test_empty():
    brow_ptr, bcols, bvals = bsr_ref.bsr_from_csr(np.zeros(7, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0), 3)
    assert brow_ptr.shape == (3,) and not brow_ptr.any() and bcols.size == 0 and bvals.shape == (0, 3, 3)
    assert not bsr_ref.dense_of_bsr(brow_ptr, bcols, bvals, 3).any()
