"""The numpy references (tests/krylov_ref.py, tests/lanczos_ref.py, tests/snes_ref.py) on the CPU oracle's matrices of the
constructions of tests/solver_exit_cases.py: no GPU.  tests/test_gpu_solver_exits.py holds the device to the same
references on the same states; this file asserts what makes that comparison mean something:
  * every rare exit is reached by the reference (the reasons, the step at which it stops);
  * at every Arnoldi step of a happy or singular case hn / sqrt(ww) is exactly 0, below 1e-15 or above 1e-12, two decades or
    more from KSP_HAPPY on either side (the device and numpy sum in different orders);
  * where the device must stop on the very same step (an exact zero, a non-finite value, a test made before the first
    step) every estimate that decides the stop is a factor 10 or more from tol;
  * where the issue's "within one" applies (a stop reached by iterating: the estimate falls by less than a decade per step,
    so an entry within a factor 10 of tol cannot be avoided) the deciding estimates are 5 % or more from tol, 5e4 times the
    1e-6 to which the histories must agree, and the reference's own history moves by less than 1e-8 under a one-eps
    perturbation of K and b (solver_exit_cases.rounding_sensitivity).
A case that fails a condition is re-seeded here; nothing is loosened on the device side.  The eroded tangents are the
oracle's with 1 - Damage_n1 (orc.set_tangent_damage), the scaling of U-Newmark-beta.c:1757-1764."""
import functools

import numpy as np
import pytest

import krylov_ref
import lanczos_ref
import snes_ref
import solver_exit_cases as sx
from test_snes_ref import oracle_problem

ALPHA_1 = sx.ALPHA_1
EPS = 2.220446049250313e-16


@functools.lru_cache(maxsize=None)
def _linearised(ndim, law):
    return sx.linearised_oracle(ndim, law)


@functools.lru_cache(maxsize=None)
def _eroded(ndim, law, level):
    return sx.eroded_oracle(ndim, law, level)


@functools.lru_cache(maxsize=None)
def _one_particle(ndim):
    return sx.one_particle_oracle(ndim)


@functools.lru_cache(maxsize=None)
def _wide():
    return sx.wide_oracle()


# ------------------------------------------------------------------------------------------------ GMRES
@pytest.mark.parametrize("pc", ["none", "pbjacobi"])
@pytest.mark.parametrize("guess", [False, True])
def test_happy_breakdown_on_the_fixed_dofs(pc, guess):
    st = _linearised(2, "neo-hookean")
    K = sx.oracle_matrix(st, ALPHA_1, st["Mv"], True)
    n = K.shape[0]
    b = sx.dyadic_rhs(n, np.flatnonzero(st["d2m"] == -1), sx.SEED_FIXED)
    assert np.count_nonzero(b) == 16 and not b[st["d2m"] != -1].any() and np.array_equal(K @ b, b)
    x, info = sx.reference_gmres(K, b, pc, 2, rtol=1e-10, x0=-b if guess else None)
    assert info["reason"] == krylov_ref.CONVERGED_RTOL and info["iterations"] == 1
    assert info["history"][1] == 0.0 and info["happy_ratio"][0] == 0.0 and np.array_equal(x, b)
    assert info["refinements"] == 1, "the first pass leaves exactly 0, which is below half of w . w: the second pass runs"
    # normal deviates: happy all the same, on rounding noise (solver_exit_cases.dyadic_rhs says why the device is not held to it)
    bn = sx.fixed_dof_rhs(st["d2m"], sx.SEED_FIXED)
    xn, noisy = sx.reference_gmres(K, bn, pc, 2, rtol=1e-10)
    assert noisy["iterations"] == 1 and noisy["reason"] > 0 and sx.gate_is_clear(noisy)
    assert noisy["history"][1] <= 32 * EPS * noisy["bnorm"] and np.abs(xn - bn).max() <= 1e-15 * np.abs(bn).max()


@pytest.mark.parametrize("ndim,law", sx.ERODED)
def test_happy_breakdown_of_a_diagonal_operator(ndim, law):
    st = _eroded(ndim, law, "all")
    assert np.all(st["damage"] == 1.0)
    K = sx.oracle_matrix(st, ALPHA_1, st["Mv"], True)
    n = K.shape[0]
    assert np.array_equal(K, np.diag(ALPHA_1 * st["Mv"])), "exactly alpha_1 M: every particle's volume is V0 (1 - 1)"
    b = sx.dyadic_rhs(n, np.arange(n), sx.SEED_DIAGONAL)
    x, info = sx.reference_gmres(K, b, "jacobi", ndim, rtol=1e-10)
    assert info["reason"] == krylov_ref.CONVERGED_RTOL and info["iterations"] == 1, info
    assert sx.gate_is_clear(info) and info["happy_ratio"][0] <= 1e-15
    assert sx.stop_margin(info, sx.tolerance(info, 1e-10)) >= 10.0
    assert np.abs(x - b / np.diag(K)).max() <= 1e-14 * np.abs(x).max()


@pytest.mark.parametrize("restart", [30, 256])
@pytest.mark.parametrize("pc", ["none", "pbjacobi"])
@pytest.mark.parametrize("ndim", [2, 3])
def test_fewer_dofs_than_the_restart(ndim, pc, restart):
    st = _one_particle(ndim)
    K = sx.oracle_matrix(st, ALPHA_1, st["Mv"], False)
    n = K.shape[0]
    assert n == (18 if ndim == 2 else 81), "9 members in 2-D, 27 in 3-D"
    b = sx.rhs(n, sx.SEED_ONE_PARTICLE)
    kw = dict(restart=restart, rtol=1e-12, max_it=100)
    x, info = sx.reference_gmres(K, b, pc, ndim, **kw)
    tol = sx.tolerance(info, 1e-12)
    print(f"{ndim}-D {pc} restart {restart}: reason {info['reason']}, {info['iterations']} steps, rnorm / bnorm "
          f"{info['rnorm'] / info['bnorm']:.3e}, margin {sx.stop_margin(info, tol):.3g}")
    if (ndim, pc, restart) == (3, "none", 30):
        # 81 dofs against GMRES(30): NOT fewer dofs than the restart.  The reference stagnates over its restarts and ends
        # on max_it; its second cycle moves by 1e-5 .. 5e-4 under a one-eps perturbation, so the device is held to its
        # first cycle, the reason and the count only (test_gpu_solver_exits.py)
        assert info["reason"] == krylov_ref.DIVERGED_ITS and info["iterations"] == 100
        assert sx.rounding_sensitivity(K, b, pc, ndim, window=31, **kw) <= 1e-8
        assert sx.rounding_sensitivity(K, b, pc, ndim, window=41, **kw) > 1e-6
        return
    assert info["reason"] == krylov_ref.CONVERGED_RTOL and info["iterations"] <= n
    assert np.abs(x - np.linalg.solve(K, b)).max() <= 1e-9 * np.abs(x).max()
    assert sx.stop_margin(info, tol) >= 1.05 and sx.rounding_sensitivity(K, b, pc, ndim, **kw) <= 1e-8
    if ndim == 2 and pc == "none":
        assert info["iterations"] == n and info["happy_ratio"][-1] <= 1e-15 and sx.gate_is_clear(info), "the space runs out at step n"
        assert sx.stop_margin(info, tol) >= 10.0


@pytest.mark.parametrize("ndim,law", sx.ERODED)
def test_singular_step(ndim, law):
    st = _eroded(ndim, law, "all")
    K = sx.oracle_matrix(st)
    assert not K.any(), "the operator is exactly zero"
    n = K.shape[0]
    b = sx.rhs(n, sx.SEED_SINGULAR)
    x, info = sx.reference_gmres(K, b, "none", ndim)
    assert info["reason"] == krylov_ref.DIVERGED_BREAKDOWN and info["iterations"] == 1 and not x.any()
    assert info["rnorm"] == info["bnorm"] and info["history"][1] == 0.0 and info["happy_ratio"][0] == 0.0
    assert info["refinements"] == 0, "0 < 0 / 2 is false: no second pass"
    guess = sx.rhs(n, sx.SEED_SINGULAR + 1)
    xg, ig = sx.reference_gmres(K, b, "none", ndim, x0=guess)
    assert ig["reason"] == krylov_ref.DIVERGED_BREAKDOWN and ig["iterations"] == 1 and np.array_equal(xg, guess)


@pytest.mark.parametrize("ndim,law", sx.ERODED)
def test_preconditioner_refusal(ndim, law):
    st = _eroded(ndim, law, "part")
    assert 0 < np.count_nonzero(st["damage"]) < st["damage"].size
    K = sx.oracle_matrix(st)
    n = K.shape[0]
    B = sx.block_diagonal(K, ndim)
    dead = np.array([not blk.any() for blk in B])
    assert dead.any() and not dead.all(), "at least one exactly zero diagonal block and one that is not"
    for A in np.flatnonzero(dead):
        assert not K[A * ndim:(A + 1) * ndim].any() and not K[:, A * ndim:(A + 1) * ndim].any(), "a node that lost every particle"
    for kind in ("jacobi", "pbjacobi"):
        bad, margin = sx.first_refused_node(K, ndim, kind)
        assert bad == int(np.flatnonzero(dead)[0]), "only the zero blocks fail the rule"
        assert margin >= 1e-11, f"{kind}: every other block passes by three decades or more ({margin:.3e})"
    b = K @ sx.rhs(n, sx.SEED_REFUSAL)
    kw = sx.REFUSAL_KSP  # (one cycle: over a restart this singular system's history moves by 2e-3 under a one-eps perturbation)
    x, info = sx.reference_gmres(K, b, "none", ndim, **kw)
    print(f"{ndim}-D law {law}: consistent b, no preconditioner: reason {info['reason']}, {info['iterations']} steps")
    assert info["reason"] == krylov_ref.DIVERGED_ITS and info["iterations"] == 40
    assert info["history"].min() >= 1.05 * sx.tolerance(info, 1e-5), "max_it decides, not the estimate"
    assert sx.rounding_sensitivity(K, b, "none", ndim, **kw) <= 1e-8
    Kd = sx.oracle_matrix(st, ALPHA_1, st["Mv"], True)
    assert sx.first_refused_node(Kd, ndim, "pbjacobi")[0] is None
    xd, idyn = sx.reference_gmres(Kd, b, "pbjacobi", ndim, rtol=1e-10)
    assert idyn["reason"] > 0 and np.abs(xd - np.linalg.solve(Kd, b)).max() <= 1e-6 * np.abs(xd).max()


def test_converged_atol_and_diverged_dtol():
    st = _linearised(3, "hencky")
    K = sx.oracle_matrix(st, ALPHA_1, st["Mv"], True)
    n = K.shape[0]
    b = sx.rhs(n, sx.SEED_ATOL)
    bn = float(np.linalg.norm(b))
    kw = dict(rtol=0.0, atol=1e-6 * bn)
    x, info = sx.reference_gmres(K, b, "pbjacobi", 3, **kw)
    print("atol:", info["iterations"], "steps, history / bnorm", info["history"] / bn)
    assert info["reason"] == krylov_ref.CONVERGED_ATOL and 1 < info["iterations"] < 30
    assert sx.stop_margin(info, 1e-6 * bn) >= 1.05 and sx.rounding_sensitivity(K, b, "pbjacobi", 3, **kw) <= 1e-8
    x, info = sx.reference_gmres(K, b, "pbjacobi", 3, rtol=0.0, atol=10.0 * bn)
    assert info["reason"] == krylov_ref.CONVERGED_ATOL and info["iterations"] == 0 and not x.any()
    assert sx.stop_margin(info, 10.0 * bn) >= 10.0
    guess = 1e8 * sx.rhs(n, sx.SEED_ATOL + 1)
    x, info = sx.reference_gmres(K, b, "pbjacobi", 3, x0=guess)
    assert info["reason"] == krylov_ref.DIVERGED_DTOL and info["iterations"] == 0 and np.array_equal(x, guess)
    assert info["rnorm"] >= 10.0 * 1e5 * bn
    x, info = sx.reference_gmres(K, b, "pbjacobi", 3, dtol=0.5)
    assert info["reason"] == krylov_ref.DIVERGED_DTOL and info["iterations"] == 0 and not x.any()


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_nanorinf(value):
    st = _linearised(3, "hencky")
    K = sx.oracle_matrix(st, ALPHA_1, st["Mv"], True)
    n = K.shape[0]
    b = sx.rhs(n, sx.SEED_NAN)
    b[n // 3] = value
    x, info = sx.reference_gmres(K, b, "pbjacobi", 3)
    assert info["reason"] == krylov_ref.DIVERGED_NANORINF and info["iterations"] == 0 and not x.any()
    guess = sx.rhs(n, sx.SEED_NAN + 1)
    x, info = sx.reference_gmres(K, b, "pbjacobi", 3, x0=guess)
    assert info["reason"] == krylov_ref.DIVERGED_NANORINF and info["iterations"] == 0 and np.array_equal(x, guess)


def test_restart_1_and_restart_256():
    st = _wide()
    n = st["na"] * 2
    assert np.count_nonzero(st["d2m"] != -1) > 300
    b = sx.rhs(n, sx.SEED_WIDE)
    K = sx.oracle_matrix(st, ALPHA_1, st["Mv"], True)
    kw = dict(restart=1, max_it=40)
    x, info = sx.reference_gmres(K, b, "pbjacobi", 2, **kw)
    print("restart 1:", info["reason"], info["iterations"], info["history"] / info["bnorm"])
    assert info["iterations"] >= 5, "several cycles of one step"
    assert sx.stop_margin(info, sx.tolerance(info)) >= 1.05 and sx.rounding_sensitivity(K, b, "pbjacobi", 2, **kw) <= 1e-8
    K = sx.oracle_matrix(st, *sx.WIDE_256_OPERATOR[:1], st["Mv"], sx.WIDE_256_OPERATOR[1])
    kw = dict(restart=256, max_it=300, rtol=1e-14)
    x, info = sx.reference_gmres(K, b, "none", 2, **kw)
    h = info["history"] / info["bnorm"]
    print("restart 256:", info["reason"], info["iterations"], "history / bnorm at 1, 40, 200, 255 .. 258, 300:", h[[1, 40, 200, 255, 256, 257, 258, 300]],
          "refinements", info["refinements"])
    assert info["reason"] == krylov_ref.DIVERGED_ITS and info["iterations"] == 300, "a full cycle of 256 and 44 steps of a second one"
    assert h[1:].min() >= 1e-6, "no entry near the floor of the comparison, where the estimate is rounding noise"
    assert sx.rounding_sensitivity(K, b, "none", 2, window=301, **kw) <= 1e-8
    assert info["refinements"] >= 256, "DGKS: (nearly) every step of the long cycle takes the second pass"


# ------------------------------------------------------------------------------------------------ Lanczos
@pytest.mark.parametrize("ndim,law", sx.ERODED)
def test_lanczos_on_the_zero_and_the_diagonal_operator(ndim, law):
    st = _eroded(ndim, law, "all")
    Mv = st["Mv"]
    r = lanczos_ref.lanczos(sx.oracle_matrix(st), Mv, None, seed=sx.SEED_LANCZOS)
    assert r["reason"] == lanczos_ref.CONVERGED and r["iterations"] == 1 and r["theta"] == 0.0
    assert r["resid"] == 0.0 and r["asymmetry"] == 0.0 and np.isfinite(r["mode"]).all() and r["mode"].any()
    assert abs(r["mode"] @ (Mv * r["mode"]) - 1.0) <= 1e-12
    r = lanczos_ref.lanczos(sx.oracle_matrix(st, ALPHA_1, Mv, False), Mv, None, seed=sx.SEED_LANCZOS)
    assert r["reason"] == lanczos_ref.CONVERGED and r["iterations"] == 1
    assert abs(r["theta"] - ALPHA_1) <= 1e-15 * ALPHA_1, "A = S (alpha_1 M) S = alpha_1 I up to the rounding of m / sqrt(m)^2"


@pytest.mark.parametrize("ndim", [2, 3])
def test_lanczos_with_fewer_dofs_than_steps(ndim):
    st = _one_particle(ndim)
    Mv = st["Mv"]
    K = sx.oracle_matrix(st, ALPHA_1, Mv, False)
    n = K.shape[0]
    fixed = np.zeros(n, dtype=bool)
    max_it = sx.lanczos_steps(ndim)
    r = lanczos_ref.lanczos(K, Mv, fixed, seed=sx.SEED_LANCZOS, max_it=max_it, rtol=1e-10)
    lam = np.linalg.eigvalsh(lanczos_ref.scaled_operator(K, Mv, fixed)[0])[-1]
    print(f"{ndim}-D: {r['iterations']} steps of {n} dofs, theta {r['theta']:.12e}, lambda_max - theta {lam - r['theta']:.3e}")
    assert r["reason"] == lanczos_ref.CONVERGED and r["iterations"] <= n < max_it
    assert -EPS * n * lam <= lam - r["theta"] <= r["resid"] + 1e-12 * lam


# ------------------------------------------------------------------------------------------------ Newton
def test_newton_reasons():
    residual, tangent, n = oracle_problem([0.5, -1.0], 1.0e-2)
    kw = dict(linear="dense", linesearch="basic")
    z = np.zeros(n)
    x, info = snes_ref.newton(residual, tangent, z, rtol=0.0, atol=0.0, stol=sx.SNES_STOL, **kw)
    assert info["reason"] == snes_ref.CONVERGED_SNORM_RELATIVE and info["iterations"] == 2
    assert info["snorm"] <= 1e-2 * sx.SNES_STOL * info["xnorm"], "far below stol at iterate 2 (and snorm == xnorm at iterate 1)"
    for ls in ("basic", "bt"):
        x, info = snes_ref.newton(residual, tangent, z, rtol=1e-10, atol=0.0, stol=0.0, max_funcs=2, linear="dense", linesearch=ls)
        assert info["reason"] == snes_ref.DIVERGED_FUNCTION_COUNT and info["iterations"] == 2 and info["function_evaluations"] == 3
    start = z.copy()
    start[7] = np.nan
    x, info = snes_ref.newton(residual, tangent, start, **kw)
    assert info["reason"] == snes_ref.DIVERGED_FNORM_NAN and info["iterations"] == 0 and info["function_evaluations"] == 1
    residual, tangent, n = oracle_problem([5.0, -40.0], 5.0e-2)
    x, free = snes_ref.newton(residual, tangent, np.zeros(n), rtol=1e-8, atol=0.0, stol=0.0, max_it=1, **kw)
    ratio = free["fnorm_history"][1] / free["fnorm0"]
    assert ratio > 4.0, "the full first step of the violent start raises the norm"
    x, info = snes_ref.newton(residual, tangent, np.zeros(n), rtol=1e-8, atol=0.0, stol=0.0, divtol=np.sqrt(ratio), **kw)
    assert info["reason"] == snes_ref.DIVERGED_DTOL and info["iterations"] == 1


def test_no_finite_start_brings_a_nan_into_a_line_search_trial():
    """Starts ten and a hundred times as violent as the one that backtracks, and a time step ten times as long, never show
    a non-finite norm in six iterates of either line search: a trial that crushes particles has a large but finite
    residual.  The branch that halves lambda on a non-finite trial therefore has no device test
    (test_gpu_solver_exits.py says so)."""
    for velocity, dt in (([50.0, -400.0], 5.0e-2), ([500.0, -4000.0], 5.0e-2), ([5.0, -40.0], 0.5)):
        residual, tangent, n = oracle_problem(velocity, dt)
        for ls in ("basic", "bt"):
            x, info = snes_ref.newton(residual, tangent, np.zeros(n), rtol=1e-8, atol=0.0, stol=0.0, max_it=6, linear="dense",
                                      linesearch=ls)
            assert info["reason"] != snes_ref.DIVERGED_FNORM_NAN and np.isfinite(info["fnorm_history"]).all()
