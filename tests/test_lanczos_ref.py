"""The numpy Lanczos of tests/lanczos_ref.py (the reference of nlps_gpu_tangent_lambda_max) against dense eigenvalues of
S K S on the free block, on the oracle's tangents of the states test_gpu_tangent_operator._linearised builds: Neo-Hookean
in 2-D and 3-D (symmetric), Hencky and Drucker-Prager in 3-D (assembled tangent not symmetric)."""
import numpy as np
import pytest

import lanczos_ref
from test_gpu_tangent_operator import LAWS, _case
from util import dirichlet_plane, oracle_setup, orc

CASES = [(2, "neo-hookean"), (3, "neo-hookean"), (3, "hencky"), (3, "drucker-prager")]
AMP = {"neo-hookean": 2e-2, "hencky": 2e-2, "drucker-prager": 8e-3}
EIGVALSH_ERR = 2.220446049250313e-16  # per row: the dense eigenvalue itself is good to n eps ||A||
_cache = {}


def oracle_pencil(ndim, law, seed=13):
    """(K, M, fixed) of the oracle at _linearised's state: one compatibility + constitutive pass at a random dU, masks at
    step 1, the floor fixed; K without mass term, Dirichlet rows as the identity.  Computed once per case."""
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
        K, _, st = o.tangent_matrix(P, M, mats, n2m, d2m, na, 0.0, None, with_pattern=False)
        assert st == 0
        fixed = d2m == -1
        assert fixed.any() and not fixed.all()
        for a in (K, Mv, fixed):
            a.setflags(write=False)
        _cache[(ndim, law)] = (K, Mv, fixed)
    return _cache[(ndim, law)]


def free_block(K, Mv, fixed):
    A, _ = lanczos_ref.scaled_operator(K, Mv, fixed)
    return A[np.ix_(~fixed, ~fixed)]


def test_hash_vector_is_reproducible_and_in_range():
    v = lanczos_ref.hash_vector(7, 1000)
    assert np.array_equal(v, lanczos_ref.hash_vector(7, 1000))
    assert np.array_equal(v[:10], lanczos_ref.hash_vector(7, 10)), "counter based: component i does not depend on n"
    assert not np.array_equal(v, lanczos_ref.hash_vector(8, 1000))
    assert v.min() >= -1.0 and v.max() < 1.0 and abs(v.mean()) < 0.1 and 0.5 < v.std() < 0.65
    # the first output of the splitmix64 stream seeded with 0 is 0xE220A8397B1DCDAF
    assert lanczos_ref.hash_vector(0, 1)[0] == 2.0 * ((0xE220A8397B1DCDAF >> 11) * 2.0 ** -53) - 1.0


@pytest.mark.parametrize("ndim,law", CASES)
def test_against_dense_eigenvalues(ndim, law):
    K, Mv, fixed = oracle_pencil(ndim, law)
    symmetric = law == "neo-hookean"
    r = lanczos_ref.lanczos(K, Mv, fixed, seed=0, max_it=200, rtol=1e-8)
    assert r["reason"] == lanczos_ref.CONVERGED and r["iterations"] <= 40, (r["reason"], r["iterations"])
    assert len(r["history"]) == r["iterations"] and r["history"][-1] == r["theta"]
    Aff = free_block(K, Mv, fixed)
    asym_K = np.abs(K - K.T).max() / np.abs(K).max()
    mode = r["mode"]
    assert not mode[fixed].any() and abs(mode @ (Mv * mode) - 1.0) <= 1e-12
    if symmetric:
        lam = np.linalg.eigvalsh(0.5 * (Aff + Aff.T))[-1]
        print(f"{law} {ndim}-D: {r['iterations']} steps, lambda_max {lam:.9e}, lambda_max - theta {lam - r['theta']:.3e}, "
              f"resid {r['resid']:.3e}, asymmetry {r['asymmetry']:.3e}, 2/omega {2 / np.sqrt(lam):.4e}")
        assert asym_K < 1e-12
        # (eigvalsh's own error, n eps lambda_max, on the lower side: a converged theta equals lambda_max to the last
        # bits and the difference came out at -3.6e-16 lambda_max in 3-D)
        assert -EIGVALSH_ERR * len(Aff) * lam <= lam - r["theta"] <= r["resid"] + 1e-12 * lam
        assert np.all(np.diff(r["history"]) >= -1e-13 * lam), "theta_j does not decrease"
        assert r["asymmetry"] < 1e-10
    else:
        lam = np.linalg.eigvals(Aff).real.max()
        lam_s = np.linalg.eigvalsh(0.5 * (Aff + Aff.T))[-1]
        print(f"{law} {ndim}-D: {r['iterations']} steps, max Re eig {lam:.9e}, |theta - max Re eig| / . "
              f"{abs(r['theta'] - lam) / lam:.3e}, |theta - lambda_max(sym A)| / . {abs(r['theta'] - lam_s) / lam_s:.3e}, "
              f"asymmetry {r['asymmetry']:.3e}, max|K - K^T| / max|K| {asym_K:.3e}")
        assert asym_K > 1e-4, "the case must have an unsymmetric tangent"
        # the skew part of A moves an eigenvalue of its symmetric part at second order only: well inside its own size
        assert abs(r["theta"] - lam) <= asym_K * lam and abs(r["theta"] - lam_s) <= asym_K * lam_s
        assert 1e-6 < r["asymmetry"] < 10 * asym_K


@pytest.mark.parametrize("ndim,law", CASES[:2])
def test_start_vectors_stopping_rules_and_empty(ndim, law):
    K, Mv, fixed = oracle_pencil(ndim, law)
    n = K.shape[0]
    lam = np.linalg.eigvalsh(free_block(K, Mv, fixed))[-1]
    a = lanczos_ref.lanczos(K, Mv, fixed, seed=3, max_it=60, rtol=1e-8)
    b = lanczos_ref.lanczos(K, Mv, fixed, v0=lanczos_ref.hash_vector(3, n), max_it=60, rtol=1e-8)
    assert a["iterations"] == b["iterations"] and np.array_equal(a["history"], b["history"]), "seed == its own vector as v0"
    c = lanczos_ref.lanczos(K, Mv, fixed, v0=np.random.default_rng(1).normal(size=n), max_it=60, rtol=1e-8)
    assert c["reason"] == lanczos_ref.CONVERGED and abs(c["theta"] - lam) <= 1e-10 * lam
    d = lanczos_ref.lanczos(K, Mv, fixed, max_it=5, rtol=0.0)
    assert d["reason"] == lanczos_ref.DIVERGED_ITS and d["iterations"] == 5 and len(d["history"]) == 5
    assert -EIGVALSH_ERR * n * lam <= lam - d["theta"] <= d["resid"] + 1e-12 * lam, "the bracket holds for a run that did not converge"
    e = lanczos_ref.lanczos(K, Mv, np.ones(n, dtype=bool))
    assert e["reason"] == lanczos_ref.EMPTY and e["iterations"] == 0
    v0 = np.zeros(n)
    v0[fixed] = 1.0
    assert lanczos_ref.lanczos(K, Mv, fixed, v0=v0)["reason"] == lanczos_ref.EMPTY, "P v0 == 0"
    # the shift: (K + alpha_1 M, M) has the eigenvalues of (K, M) moved by alpha_1
    s = lanczos_ref.lanczos(K + 4.0e4 * np.diag(Mv), Mv, fixed, seed=3, max_it=60, rtol=1e-8)
    assert abs(s["theta"] - a["theta"] - 4.0e4) <= s["resid"] + a["resid"] + 1e-12 * s["theta"]
