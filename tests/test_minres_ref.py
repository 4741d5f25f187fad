"""The numpy MINRES (tests/minres_ref.py) on the CPU oracle's Neo-Hookean tangents: no GPU.  tests/test_gpu_minres.py holds
the device to this reference; this file holds the reference to a dense solve and asserts the CONDITIONS those
comparisons rest on (tests/minres_cases.py describes the cases once for both files):
  * the 3-D quasi-static tangent really is indefinite while its diagonal blocks are positive definite;
  * for the chosen seed the reference GMRES(30) is still above tol after twice the MINRES count plus its margin;
  * the recorded iteration-count margins cover max(2, 3 x spread) of the reference's own counts on nine copies of K and b
    that differ by one relative eps;
  * the histories compared over their first ten entries move by less than 1e-8 under that perturbation;
  * the negative-alpha_1 operator makes the Jacobi preconditioner negative on every free dof."""
import functools

import numpy as np
import pytest

import krylov_ref
import minres_cases as mc
import minres_ref
import solver_exit_cases as sx

EPS = 2.220446049250313e-16
LAW = "neo-hookean"


@functools.lru_cache(maxsize=None)
def _linearised(ndim):
    return sx.linearised_oracle(ndim, LAW)


@functools.lru_cache(maxsize=None)
def _wide():
    return sx.wide_oracle()


def _matrix(st, alpha_1):
    K = sx.oracle_matrix(st, alpha_1, st["Mv"] if alpha_1 != 0.0 else None, True)
    assert np.abs(K - K.T).max() <= 1e-14 * np.abs(K).max(), "the Neo-Hookean tangent is symmetric"
    return K


def _minres(K, b, pc, ndim, **kw):
    return minres_ref.minres(K, b, krylov_ref.preconditioner(K, pc, ndim), **kw)


def perturbed_counts(K, b, pc, ndim, copies=8, **kw):
    """(the reference's counts on K, b and `copies` one-eps neighbours (symmetric ones); the largest move of the first ten
    history entries among them): the construction of solver_exit_cases.rounding_sensitivity"""
    rng = np.random.default_rng(2024)
    _, ref = _minres(K, b, pc, ndim, **kw)
    counts, move = [ref["iterations"]], 0.0
    for _ in range(copies):
        Kp = K * (1.0 + EPS * rng.normal(size=K.shape))
        Kp = np.triu(Kp) + np.triu(Kp, 1).T
        bp = b * (1.0 + EPS * rng.normal(size=b.shape))
        _, p = _minres(Kp, bp, pc, ndim, **kw)
        assert p["reason"] == ref["reason"]
        counts.append(p["iterations"])
        move = max(move, mc.history_error(p["history"], ref["history"]))
    return counts, move


def _check_margin(case, counts, what):
    spread = max(counts) - min(counts)
    assert max(2, 3 * spread) <= case["margin"], f"{what}: counts {counts}: the recorded margin {case['margin']} is too small"


# ------------------------------------------------------------------------------------------------ against a dense solve
@pytest.mark.parametrize("pc", mc.PCS)
@pytest.mark.parametrize("ndim", [2, 3])
def test_dynamic_regime_against_a_dense_solve(ndim, pc):
    st = _linearised(ndim)
    K = _matrix(st, mc.DENSE["alpha_1"])
    b = mc.rhs(K.shape[0], mc.DENSE["seed"])
    xs = np.linalg.solve(K, b)
    x, info = _minres(K, b, pc, ndim, rtol=mc.DENSE["rtol"], max_it=mc.DENSE["max_it"][pc])
    assert np.abs(x - xs).max() <= 1e-8 * np.abs(xs).max()
    assert abs(info["rnorm"] - np.linalg.norm(b - K @ x)) <= 1e-12 * info["bnorm"]
    assert len(info["history"]) == info["iterations"] + 1
    if pc == "none":
        assert info["reason"] == minres_ref.DIVERGED_ITS and info["iterations"] == mc.DENSE["max_it"][pc]
    else:
        assert info["reason"] == minres_ref.CONVERGED_RTOL and info["iterations"] < 20 and 1 <= info["confirmations"] <= 3
        assert info["rnorm"] <= mc.DENSE["rtol"] * info["bnorm"]
    counts, move = perturbed_counts(K, b, pc, ndim, copies=4, rtol=mc.DENSE["rtol"], max_it=mc.DENSE["max_it"][pc])
    assert max(counts) == min(counts), f"'within 1' needs a count that does not move: {counts}"
    assert move < 1e-8, f"the first ten history entries move by {move:.2e}"


def test_quasi_static_2d_against_a_dense_solve_and_gmres():
    st = _linearised(2)
    K = _matrix(st, 0.0)
    b = mc.rhs(K.shape[0], mc.DENSE["seed"])
    xs = np.linalg.solve(K, b)
    x, info = _minres(K, b, "pbjacobi", 2, rtol=1e-8)
    assert info["reason"] == minres_ref.CONVERGED_RTOL and np.abs(x - xs).max() <= 1e-6 * np.abs(xs).max()
    _, g = sx.reference_gmres(K, b, "pbjacobi", 2, rtol=1e-8, restart=30, max_it=2000)
    assert g["iterations"] > 2 * info["iterations"], (g["iterations"], info["iterations"])


# ------------------------------------------------------------------------------------------------ the conditions
def test_the_quasi_static_tangent_is_indefinite_with_definite_blocks():
    st = _linearised(3)
    K = _matrix(st, 0.0)
    Ks = 0.5 * (K + K.T)
    ev = np.linalg.eigvalsh(Ks)
    assert ev[0] < -1e-3 and ev[-1] > 1e6, f"eigenvalues {ev[0]:.3e} .. {ev[-1]:.3e} (measured -3.2e-2 .. 4.3e6)"
    blocks = min(float(np.linalg.eigvalsh(B).min()) for B in sx.block_diagonal(Ks, 3))
    assert blocks > 0.5, f"smallest block eigenvalue {blocks:.3e} (measured 0.80)"


@pytest.mark.parametrize("pc", mc.INDEFINITE["pcs"])
def test_indefinite_case_converges_and_its_margin(pc):
    c = mc.INDEFINITE
    st = _linearised(3)
    K = _matrix(st, c["alpha_1"])
    b = K @ mc.rhs(K.shape[0], c["seed"])
    x, info = _minres(K, b, pc, 3, rtol=c["rtol"])
    assert info["reason"] == minres_ref.CONVERGED_RTOL and info["confirmations"] <= 3
    assert np.linalg.norm(b - K @ x) <= c["rtol"] * np.linalg.norm(b)
    counts, _ = perturbed_counts(K, b, pc, 3, rtol=c["rtol"])
    _check_margin(c, counts, f"indefinite, {pc}")


@pytest.mark.parametrize("pc", mc.GAP["pcs"])
def test_gmres_gap_and_its_margin(pc):
    c = mc.GAP
    st = _linearised(3)
    K = _matrix(st, c["alpha_1"])
    b = mc.rhs(K.shape[0], c["seed"])
    x, info = _minres(K, b, pc, 3, rtol=c["rtol"])
    xs = np.linalg.solve(K, b)
    assert info["reason"] == minres_ref.CONVERGED_RTOL and np.abs(x - xs).max() <= 1e-5 * np.abs(xs).max()
    counts, _ = perturbed_counts(K, b, pc, 3, rtol=c["rtol"])
    _check_margin(c, counts, f"gap, {pc}")
    # GMRES(30) given twice the largest count the device may take: still a factor 2 above tol
    most = 2 * (max(counts) + c["margin"])
    _, g = sx.reference_gmres(K, b, pc, 3, rtol=c["rtol"], restart=30, max_it=most)
    assert g["reason"] == krylov_ref.DIVERGED_ITS and g["rnorm"] > 2.0 * c["rtol"] * g["bnorm"], g


@pytest.mark.parametrize("pc", mc.WIDE["pcs"])
def test_wide_case_and_its_margin(pc):
    c = mc.WIDE
    st = _wide()
    K = _matrix(st, c["alpha_1"])
    b = mc.rhs(K.shape[0], c["seed"])
    assert K.shape[0] == 1610
    x, info = _minres(K, b, pc, 2, rtol=c["rtol"])
    xs = np.linalg.solve(K, b)
    assert info["reason"] == minres_ref.CONVERGED_RTOL and np.abs(x - xs).max() <= 1e-6 * np.abs(xs).max()
    assert abs(info["iterations"] - c["counts"][pc]) <= c["margin"], info["iterations"]
    counts, _ = perturbed_counts(K, b, pc, 2, copies=8, rtol=c["rtol"])
    _check_margin(c, counts, f"wide, {pc}")


# ------------------------------------------------------------------------------------------------ the exits
def test_exits_ahead_of_the_first_step():
    st = _linearised(2)
    K = _matrix(st, mc.ALPHA_DYNAMIC)
    n = K.shape[0]
    b = mc.rhs(n, 3)
    xs = np.linalg.solve(K, b)
    x, i = _minres(K, b, "jacobi", 2, x0=xs, rtol=1e-8)
    assert i["reason"] == minres_ref.CONVERGED_RTOL and i["iterations"] == 0 and np.array_equal(x, xs)
    x, i = _minres(K, np.zeros(n), "jacobi", 2, x0=xs)
    assert i["reason"] == minres_ref.CONVERGED_BZERO and not x.any() and i["history"][0] == 0.0
    x, i = _minres(K, b, "jacobi", 2, rtol=1e-12, atol=2.0 * np.linalg.norm(b))
    assert i["reason"] == minres_ref.CONVERGED_ATOL and i["iterations"] == 0
    x, i = _minres(K, b, "jacobi", 2, rtol=1e-12, dtol=0.5)
    assert i["reason"] == minres_ref.DIVERGED_DTOL and i["iterations"] == 0
    x, i = _minres(K, b, "jacobi", 2, rtol=1e-12, max_it=2)
    assert i["reason"] == minres_ref.DIVERGED_ITS and i["iterations"] == 2 and len(i["history"]) == 3 and i["confirmations"] == 1
    assert abs(i["rnorm"] - np.linalg.norm(b - K @ x)) <= 1e-12 * i["bnorm"]
    for bad in (np.nan, np.inf):
        bb = b.copy()
        bb[n // 2] = bad
        x, i = _minres(K, bb, "jacobi", 2)
        assert i["reason"] == minres_ref.DIVERGED_NANORINF and i["iterations"] == 0 and not x.any()


def test_a_negative_jacobi_preconditioner_is_reported():
    st = _linearised(3)
    K = _matrix(st, mc.NEGATIVE_ALPHA)
    free = st["d2m"] != -1
    d = np.diag(K)
    assert np.all(d[free] < 0.0) and np.all(d[~free] == 1.0)
    b = mc.free_dof_rhs(st["d2m"], mc.SEED_INDEFINITE_PC)
    x, i = _minres(K, b, "jacobi", 3)
    assert i["reason"] == minres_ref.DIVERGED_INDEFINITE_PC and i["iterations"] == 0 and not x.any()
    assert i["rnorm"] == i["history"][0] == i["bnorm"]
    # far from the gate: r0 . M^-1 r0 is a sum of negative terms only
    assert float(b @ (b / d)) < 0.0 and np.all((b * b / d) <= 0.0)
