"""The device GMRES, Lanczos and Newton solves (nlps_gpu_tangent_solve, nlps_gpu_tangent_lambda_max, nlps_gpu_newton_solve,
nlps_gpu_newmark_step) down the exits their own tests never take: happy and singular Arnoldi steps, fewer dofs than the
restart, a refused preconditioner, every stopping test ahead of the first step, restarts of 1 and of 256 vectors, zero and
diagonal operators under Lanczos, and the Newton reasons reached on the CPU only so far.  Device side: the call.  Reference
side: tests/krylov_ref.py, tests/lanczos_ref.py and tests/snes_ref.py on the dense matrix of the SAME state, the assembled
COO of the handle (another code path than the matrix-free product, itself held to the oracle).  The constructions are
tests/solver_exit_cases.py's; tests/test_solver_exits_ref.py holds the references to the conditions under which a
comparison step by step means something, on the CPU.

Every GMRES case: reason equal; iterations equal where an exact zero, a non-finite value or a test ahead of the first step
decides (exact=True), else within one; the history entry by entry to 1e-6 (the measure of
test_gpu_tangent_solve.py::_check_against_reference) over its first 40 entries; x against the reference's to 1e-5.

Which test asserts which reason of include/nlps_gpu.h:
  NLPS_KSP_CONVERGED_BZERO 1       test_singular_step (b = 0 on the zero operator)
  NLPS_KSP_CONVERGED_RTOL 2        test_happy_breakdown_on_the_fixed_dofs, test_fewer_dofs_than_the_restart
  NLPS_KSP_CONVERGED_ATOL 3        test_converged_atol_and_diverged_dtol
  NLPS_KSP_DIVERGED_ITS -3         test_preconditioner_refusal (the solve that follows), test_restart_256
  NLPS_KSP_DIVERGED_DTOL -4        test_converged_atol_and_diverged_dtol
  NLPS_KSP_DIVERGED_BREAKDOWN -5   test_singular_step
  NLPS_KSP_DIVERGED_NANORINF -9    test_nanorinf
  NLPS_EIG_CONVERGED 1             test_lanczos_on_the_zero_and_the_diagonal_operator, test_lanczos_with_fewer_dofs_than_steps
  NLPS_EIG_EMPTY 2                 test_lanczos_on_the_zero_and_the_diagonal_operator (v0 = 0)
  NLPS_EIG_DIVERGED_ITS -3         test_lanczos_with_fewer_dofs_than_steps (two steps, rtol 0)
  NLPS_EIG_DIVERGED_NANORINF -9    test_lanczos_with_fewer_dofs_than_steps (a NaN in v0)
  NLPS_SNES_CONVERGED_FNORM_ABS 2, _FNORM_RELATIVE 3, _SNORM_RELATIVE 4, NLPS_SNES_DIVERGED_FUNCTION_COUNT -2,
  _LINEAR_SOLVE -3, _FNORM_NAN -4, _MAX_IT -5     test_newton_exits_of_the_mild_start
  NLPS_SNES_DIVERGED_LINE_SEARCH -6, _DTOL -9     test_newton_exits_of_the_violent_start
  NLPS_SNES_DIVERGED_FUNCTION_COUNT through nlps_gpu_newmark_step    test_newmark_step_passes_the_reason_through
The DGKS second pass: the reference counts its second passes (krylov_ref.gmres's "refinements"); test_singular_step is
the case that never refines (0 of 1 step), test_restart_256 the one that does (299 of 300 steps), and the device's history
matches in both.  On systems this well conditioned the history alone cannot tell whether the device took the pass (the
reference without it moves by 4e-11 on the 300 steps).  What can is the happy step on normal deviates in
test_happy_breakdown_on_the_fixed_dofs: one pass leaves eps ||b||, two leave eps^2 ||b||, and the test bounds it between."""
import re

import numpy as np
import pytest

import krylov_ref
import lanczos_ref
import snes_ref
import solver_exit_cases as sx
from test_gpu_critical_dt import EPS, HIST_TOL, _check_reference
from test_gpu_newton_solve import DRIVER, HISTORY_TOL, TIGHT, _alpha, _problem, _same_counts, _Step
from test_gpu_tangent_operator import _check_blocks, _coo_dense
from util import assert_close, gpu_setup, nlps

pytestmark = pytest.mark.gpu

ALPHA_1 = sx.ALPHA_1


def _operator(s, alpha_1, mass, dirichlet):
    """The operator on the device and the dense matrix of the same state."""
    S = s["S"]
    K = _coo_dense(S, s["na"] * s["ndim"], alpha_1, mass, dirichlet)
    S.tangent_operator(alpha_1, mass, dirichlet)
    return K


def _history_error(hd, hr, lo, hi):
    hi = min(hi, len(hd), len(hr))
    if hi <= lo:
        return 0.0
    return float((np.abs(hd[lo:hi] - hr[lo:hi]) / np.maximum(hr[lo:hi], 1e-12 * hr[0])).max())


def _solve_and_check(s, K, b, what, exact, x0=None, window=40, around=None, **kw):
    """One device solve beside the reference GMRES of the same settings on K; returns (x, info, xr, ir)."""
    S, ndim = s["S"], s["ndim"]
    b0 = b.copy()
    x, info = S.tangent_solve(b, x=None if x0 is None else x0.copy(), history=True, **kw)
    assert np.array_equal(b, b0, equal_nan=True), "b is not touched"
    ref_kw = {k: v for k, v in kw.items() if k != "pc"}
    xr, ir = sx.reference_gmres(K, b, kw.get("pc", "pbjacobi"), ndim, x0=x0, **ref_kw)
    hd, hr = info["history"], ir["history"]
    err = _history_error(hd, hr, 0, window)
    print(f"{what}: reason {info['reason']} ({ir['reason']}), iterations {info['iterations']} ({ir['iterations']}), history vs "
          f"reference {err:.3e} over {min(window, len(hd), len(hr))} entries, whole {_history_error(hd, hr, 0, 1 << 30):.3e}, "
          f"rnorm / bnorm {info['rnorm'] / info['bnorm']:.3e}, reference refinements {ir['refinements']}")
    assert info["reason"] == ir["reason"], f"{what}: reason {info['reason']} vs reference {ir['reason']}"
    slack = 0 if exact else 1
    assert abs(info["iterations"] - ir["iterations"]) <= slack, f"{what}: iterations {info['iterations']} vs {ir['iterations']}"
    assert len(hd) == info["iterations"] + 1
    assert abs(info["bnorm"] - ir["bnorm"]) <= 1e-12 * ir["bnorm"]
    assert err <= 1e-6, f"{what}: history vs reference, relative {err:.3e}:\n{hd[:window]}\n{hr[:window]}"
    if around is not None:
        assert len(hd) > around[1] and len(hr) > around[1]
        e2 = _history_error(hd, hr, around[0], around[1])
        print(f"{what}: history entries {around[0]} .. {around[1] - 1} vs reference {e2:.3e}")
        assert e2 <= 1e-6, f"{what}: history around the restart:\n{hd[around[0]:around[1]]}\n{hr[around[0]:around[1]]}"
    if ir["reason"] > 0:
        assert_close(x, xr, 1e-5, f"{what}: x vs reference GMRES", scale=np.abs(xr).max())
    return x, info, xr, ir


# ------------------------------------------------------------------------------------------------ GMRES
@pytest.mark.parametrize("pc", ["none", "pbjacobi"])
def test_happy_breakdown_on_the_fixed_dofs(pc):
    """b on the fixed dofs, K b = b: V[1] = K M^-1 V[0] - V[0] is exactly 0, hn == 0 (k_ksp_scale is a no-op, V[1] is no
    unit vector), one step, the estimate exactly 0, x = b; the same over a guess that lives on the fixed dofs."""
    s = sx.linearised_device(2, "neo-hookean")
    S = s["S"]
    K = _operator(s, ALPHA_1, s["Mv"], True)
    n = K.shape[0]
    b = sx.dyadic_rhs(n, np.flatnonzero(s["d2m"] == -1), sx.SEED_FIXED)
    assert np.count_nonzero(b) == 16 and np.array_equal(K @ b, b)
    for guess in (None, -b):
        what = f"happy, pc={pc}, guess={guess is not None}"
        x, info, xr, ir = _solve_and_check(s, K, b, what, True, x0=guess, pc=pc, rtol=1e-10)
        assert ir["happy_ratio"][0] == 0.0
        assert info["iterations"] == 1 and info["history"][1] == 0.0 and info["reason"] > 0, info
        assert np.abs(x - b).max() <= 1e-15 * np.abs(b).max()
    # normal deviates on the same dofs: h = V[0] . V[0] = 1 + d with |d| <= 16 eps (16 terms).  The first Gram-Schmidt pass
    # leaves w = -d V[0] (one fma per entry, its rounding eps |d|), below half of w . w, so the DGKS pass runs and leaves
    # d^2 V[0]: hn <= (17 eps)^2 = 1.4e-29.  Without the second pass hn = |d| >= eps / 2 = 1.1e-16 unless d is exactly 0.
    # 1e-24 ||b|| lies five decades from either.  numpy has no fma and keeps eps-sized noise, so no history comparison.
    bn = sx.fixed_dof_rhs(s["d2m"], sx.SEED_FIXED)
    x, info = S.tangent_solve(bn, pc=pc, rtol=1e-10, history=True)
    print(f"normal deviates, pc={pc}: history {info['history']}")
    assert info["iterations"] == 1 and info["reason"] == krylov_ref.CONVERGED_RTOL and info["history"][1] <= 1e-24 * info["bnorm"]
    assert np.abs(x - bn).max() <= 1e-15 * np.abs(bn).max()
    S.close()


@pytest.mark.parametrize("ndim,law", sx.ERODED)
def test_happy_breakdown_of_a_diagonal_operator(ndim, law):
    """Every particle failed: K = alpha_1 M exactly, K M^-1 = I up to the rounding of d (1 / d) with PCJACOBI."""
    s = sx.eroded_device(ndim, law, "all")
    S = s["S"]
    assert np.all(s["damage"] == 1.0), "Gf below every particle's G: all of them fail in the hook"
    K = _operator(s, ALPHA_1, s["Mv"], True)
    n = K.shape[0]
    d = np.diag(K).copy()
    assert np.array_equal(K, np.diag(d)) and np.abs(d - ALPHA_1 * s["Mv"]).max() <= 4 * EPS * d.max()
    b = sx.dyadic_rhs(n, np.arange(n), sx.SEED_DIAGONAL)
    x, info, xr, ir = _solve_and_check(s, K, b, f"diagonal operator {ndim}-D", True, pc="jacobi", rtol=1e-10)
    assert sx.gate_is_clear(ir) and ir["happy_ratio"][0] <= 1e-15
    assert info["iterations"] == 1 and info["reason"] == krylov_ref.CONVERGED_RTOL
    assert np.abs(x - b / d).max() <= 1e-14 * np.abs(x).max()
    S.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_fewer_dofs_than_the_restart(ndim):
    """One particle, 18 dofs in 2-D and 81 in 3-D, with the mass term: GMRES(30) and GMRES(256) (the largest small state
    on the smallest vector, one mostly empty block of KSP_TILE) end within n steps.  The exception is 3-D without
    preconditioner under GMRES(30): 81 dofs are NOT fewer than that restart, the reference stagnates to max_it = 100 with x
    1.6e-4 off, and its second cycle moves by 1e-5 .. 5e-4 under a one-eps perturbation (test_solver_exits_ref.py): there
    the reason, the count (max_it decides: exact) and the first cycle's 31 entries are compared."""
    s = sx.one_particle_device(ndim)
    S = s["S"]
    K = _operator(s, ALPHA_1, s["Mv"], False)
    n = K.shape[0]
    assert n == (18 if ndim == 2 else 81)
    b = sx.rhs(n, sx.SEED_ONE_PARTICLE)
    sol = np.linalg.solve(K, b)
    for pc in ("none", "pbjacobi"):
        for restart in (30, 256):
            what = f"one particle {ndim}-D, pc={pc}, restart={restart}"
            stagnates = (ndim, pc, restart) == (3, "none", 30)
            x, info, xr, ir = _solve_and_check(s, K, b, what, stagnates, window=31 if stagnates else 40, pc=pc, restart=restart,
                                               rtol=1e-12, max_it=100)
            if stagnates:
                assert info["reason"] == krylov_ref.DIVERGED_ITS and info["iterations"] == 100
                continue
            assert info["reason"] == krylov_ref.CONVERGED_RTOL and info["iterations"] <= n, info
            assert_close(x, sol, 1e-9, f"{what}: x vs np.linalg.solve", scale=np.abs(sol).max())
            nb = (n + 511) // 512
            expect = 8 * ((restart + 3) * n + (restart + 2) * nb + 6 * (restart + 2) + 8 + restart * (restart + 1) +
                          (s["na"] * ndim * ndim if pc != "none" else 0))
            assert nb == 1 and info["bytes"] == expect
    S.close()


@pytest.mark.parametrize("ndim,law", sx.ERODED)
def test_singular_step(ndim, law):
    """The operator is exactly zero: w = 0, r = 0 in the rotation (KSP_FLAG_SINGULAR), column 0 stays out of the update,
    x comes back as it went in and the reason is the breakdown.  The reference takes no DGKS second pass here."""
    s = sx.eroded_device(ndim, law, "all")
    S = s["S"]
    assert np.all(s["damage"] == 1.0)
    K = _operator(s, 0.0, None, False)
    assert not K.any(), "tangent_vol = V0 (1 - 1) = 0 exactly"
    n = K.shape[0]
    b = sx.rhs(n, sx.SEED_SINGULAR)
    x, info, xr, ir = _solve_and_check(s, K, b, f"zero operator {ndim}-D", True, pc="none")
    assert ir["refinements"] == 0 and ir["happy_ratio"][0] == 0.0
    assert info["reason"] == krylov_ref.DIVERGED_BREAKDOWN and info["iterations"] == 1
    assert not x.any() and info["rnorm"] == info["bnorm"] and info["history"][1] == 0.0
    guess = sx.rhs(n, sx.SEED_SINGULAR + 1)
    xg, ig, _, _ = _solve_and_check(s, K, b, f"zero operator {ndim}-D over a guess", True, x0=guess, pc="none")
    assert ig["reason"] == krylov_ref.DIVERGED_BREAKDOWN and ig["iterations"] == 1
    assert np.array_equal(xg, guess), "x is bit-identical to the guess"
    xz, iz = S.tangent_solve(np.zeros(n), x=guess, pc="none")
    assert iz["reason"] == krylov_ref.CONVERGED_BZERO and iz["iterations"] == 0 and not xz.any()
    S.close()


@pytest.mark.parametrize("ndim,law", sx.ERODED)
def test_preconditioner_refusal(ndim, law):
    """Some active nodes lost every particle: their rows of the quasi-static tangent are exactly zero.  Both Jacobi
    preconditioners are refused, naming the SMALLEST masked node whose dense block fails the rule; the handle stays
    usable: a solve without preconditioner, the diagonal blocks, and point-block Jacobi on a new operator with mass."""
    n_ = nlps()
    s = sx.eroded_device(ndim, law, "part")
    S, na = s["S"], s["na"]
    assert 0 < np.count_nonzero(s["damage"]) < s["damage"].size
    K = _operator(s, 0.0, None, False)
    n = K.shape[0]
    dead = np.array([not blk.any() for blk in sx.block_diagonal(K, ndim)])
    assert dead.any() and not dead.all(), "at least one exactly zero diagonal block and one that is not"
    b = K @ sx.rhs(n, sx.SEED_REFUSAL)
    for kind in ("jacobi", "pbjacobi", "jacobi"):
        bad, margin = sx.first_refused_node(K, ndim, kind)
        assert bad == int(np.flatnonzero(dead)[0]) and margin >= 1e-11
        with pytest.raises(n_.NlpsError, match="does not invert") as e:
            S.tangent_solve(b, pc=kind)
        named = int(re.search(r"masked node (\d+)", str(e.value)).group(1))
        assert named == bad, f"{kind}: the message names node {named}, the first block that fails the rule is {bad}"
    # the same handle, no new operator
    x, info, xr, ir = _solve_and_check(s, K, b, f"after the refusal, {ndim}-D", False, pc="none", **sx.REFUSAL_KSP)
    assert info["reason"] == krylov_ref.DIVERGED_ITS and info["iterations"] == 40
    _check_blocks(S, K, na, ndim, "after the refusal")
    Kd = _operator(s, ALPHA_1, s["Mv"], True)
    assert sx.first_refused_node(Kd, ndim, "pbjacobi")[0] is None
    xd, idyn, _, _ = _solve_and_check(s, Kd, b, f"a new operator with mass, {ndim}-D", False, pc="pbjacobi", rtol=1e-10)
    assert idyn["reason"] == krylov_ref.CONVERGED_RTOL
    sol = np.linalg.solve(Kd, b)
    assert_close(xd, sol, 1e-6, "pbjacobi on the new operator vs np.linalg.solve", scale=np.abs(sol).max())
    S.close()


def test_converged_atol_and_diverged_dtol():
    s = sx.linearised_device(3, "hencky")
    S = s["S"]
    K = _operator(s, ALPHA_1, s["Mv"], True)
    n = K.shape[0]
    b = sx.rhs(n, sx.SEED_ATOL)
    bn = float(np.linalg.norm(b))
    x, info, xr, ir = _solve_and_check(s, K, b, "atol 1e-6 ||b||", False, pc="pbjacobi", rtol=0.0, atol=1e-6 * bn)
    assert info["reason"] == krylov_ref.CONVERGED_ATOL and info["iterations"] > 1
    x, info, xr, ir = _solve_and_check(s, K, b, "atol 10 ||b||", True, pc="pbjacobi", rtol=0.0, atol=10.0 * bn)
    assert info["reason"] == krylov_ref.CONVERGED_ATOL and info["iterations"] == 0 and not x.any()
    guess = 1e8 * sx.rhs(n, sx.SEED_ATOL + 1)
    x, info, xr, ir = _solve_and_check(s, K, b, "a guess of 1e8", True, x0=guess, pc="pbjacobi")
    assert info["reason"] == krylov_ref.DIVERGED_DTOL and info["iterations"] == 0
    assert np.array_equal(x, guess), "x is bit-identical to the guess"
    x, info, xr, ir = _solve_and_check(s, K, b, "dtol 0.5", True, pc="pbjacobi", dtol=0.5)
    assert info["reason"] == krylov_ref.DIVERGED_DTOL and info["iterations"] == 0 and not x.any()
    S.close()


@pytest.mark.parametrize("deterministic", [False, True])
def test_nanorinf(deterministic):
    """One NaN or one +Inf in b, host and device vectors: the call returns 0 with reason -9 ahead of the first step, x is
    zeros or the guess; nothing of it stays on the handle: the next solve is a fresh handle's, bit for bit in deterministic
    mode.  (NaN data through arithmetic, as test_gpu_critical_dt.py's start vector.)"""
    import torch
    s = sx.linearised_device(3, "hencky", deterministic=deterministic)
    S = s["S"]
    K = _operator(s, ALPHA_1, s["Mv"], True)
    n = K.shape[0]
    good = sx.rhs(n, sx.SEED_NAN)
    guess = sx.rhs(n, sx.SEED_NAN + 1)
    for value in (np.nan, np.inf):
        b = good.copy()
        b[n // 3] = value
        for where in ("host", "device"):
            for x0 in (None, guess):
                bb = b if where == "host" else torch.from_numpy(b).cuda()
                xx = x0 if x0 is None or where == "host" else torch.from_numpy(x0).cuda()
                x, info = S.tangent_solve(bb, x=xx, pc="pbjacobi", history=True)  # (NlpsError unless the call returns 0)
                xr, ir = sx.reference_gmres(K, b, "pbjacobi", 3, x0=x0)
                x = x if where == "host" else x.cpu().numpy()
                assert info["reason"] == ir["reason"] == krylov_ref.DIVERGED_NANORINF and info["iterations"] == ir["iterations"] == 0
                assert np.array_equal(x, np.zeros(n) if x0 is None else guess), f"{value} {where}: x is zeros, or the guess"
                assert len(info["history"]) == 1 and not np.isfinite(info["history"][0])
    x, info, xr, ir = _solve_and_check(s, K, good, "after the non-finite right-hand sides", False, pc="pbjacobi", rtol=1e-10)
    assert info["reason"] == krylov_ref.CONVERGED_RTOL
    S.close()
    f = sx.linearised_device(3, "hencky", deterministic=deterministic)
    f["S"].tangent_operator(ALPHA_1, f["Mv"], True)
    xf, inf_ = f["S"].tangent_solve(good, pc="pbjacobi", rtol=1e-10, history=True)
    f["S"].close()
    assert info["iterations"] == inf_["iterations"] and info["reason"] == inf_["reason"]
    if deterministic:
        assert np.array_equal(x, xf) and np.array_equal(info["history"], inf_["history"]) and info["rnorm"] == inf_["rnorm"]
    else:
        assert_close(x, xf, 1e-12, "the next solve vs a fresh handle's", scale=np.abs(xf).max())
        assert_close(info["history"], inf_["history"], 1e-12, "the next solve's history", scale=inf_["history"][0])


def test_restart_1():
    """GMRES(1): every cycle is one step, one true residual and one update (col, red, the R stride at their smallest)."""
    s = sx.wide_device()
    S = s["S"]
    assert np.count_nonzero(s["d2m"] != -1) > 300
    K = _operator(s, ALPHA_1, s["Mv"], True)
    b = sx.rhs(K.shape[0], sx.SEED_WIDE)
    x, info, xr, ir = _solve_and_check(s, K, b, "restart 1", False, pc="pbjacobi", restart=1, max_it=40)
    assert info["iterations"] >= 5
    S.close()


def test_restart_256():
    """GMRES(NLPS_KSP_MAX_RESTART) over more than 300 free dofs: the first cycle fills all 256 columns (k_ksp_finish over 257
    blocks, col[258], the R stride of 257), the second starts and max_it = 300 ends it.  The history over its first 40
    entries and around the restart; the reference takes the DGKS second pass on 299 of the 300 steps."""
    s = sx.wide_device()
    S = s["S"]
    alpha_1, dirichlet = sx.WIDE_256_OPERATOR
    K = _operator(s, alpha_1, s["Mv"], dirichlet)
    b = sx.rhs(K.shape[0], sx.SEED_WIDE)
    x, info, xr, ir = _solve_and_check(s, K, b, "restart 256", True, around=(250, 263), pc="none", restart=256, max_it=300,
                                       rtol=1e-14)
    assert ir["refinements"] >= 256
    assert info["reason"] == krylov_ref.DIVERGED_ITS and info["iterations"] == 300
    assert np.isfinite(x).all() and abs(info["rnorm"] - ir["rnorm"]) <= 1e-6 * ir["rnorm"]
    S.close()


# ------------------------------------------------------------------------------------------------ Lanczos
@pytest.mark.parametrize("ndim,law", sx.ERODED)
def test_lanczos_on_the_zero_and_the_diagonal_operator(ndim, law):
    s = sx.eroded_device(ndim, law, "all")
    S, Mv = s["S"], s["Mv"]
    n = s["na"] * ndim
    K = _operator(s, 0.0, None, False)
    assert not K.any()
    info = S.tangent_lambda_max(Mv, seed=sx.SEED_LANCZOS, mode=True, history=True)
    ref = lanczos_ref.lanczos(K, Mv, None, seed=sx.SEED_LANCZOS)
    print("zero operator:", {k: info[k] for k in ("reason", "iterations", "theta", "resid", "asymmetry")})
    assert info["reason"] == ref["reason"] == lanczos_ref.CONVERGED and info["iterations"] == ref["iterations"] == 1
    assert info["theta"] == 0.0 and np.array_equal(info["history"], [0.0]) and info["asymmetry"] == 0.0
    assert np.isfinite(info["resid"]) and info["resid"] == ref["resid"] == 0.0
    assert_close(info["mode"], ref["mode"], 1e-13, "zero operator: the mode is the scaled start vector", scale=np.abs(ref["mode"]).max())
    assert nlps().critical_dt(info["theta"] + info["resid"]) == np.inf
    empty = S.tangent_lambda_max(Mv, v0=np.zeros(n), mode=True)
    assert empty["reason"] == lanczos_ref.EMPTY and empty["iterations"] == 0 and not empty["mode"].any()
    K = _operator(s, ALPHA_1, Mv, False)
    assert np.array_equal(K, np.diag(np.diag(K)))
    info = S.tangent_lambda_max(Mv, seed=sx.SEED_LANCZOS, mode=True, history=True)
    ref = lanczos_ref.lanczos(K, Mv, None, seed=sx.SEED_LANCZOS)
    _check_reference(info, ref, f"A = alpha_1 I, {ndim}-D")
    assert info["reason"] == lanczos_ref.CONVERGED and info["iterations"] == 1
    assert abs(info["theta"] - ALPHA_1) <= 1e-15 * ALPHA_1, f"theta {info['theta']!r}"
    S.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_lanczos_with_fewer_dofs_than_steps(ndim):
    """One particle with the mass term: A = alpha_1 I + a stiffness of rank 4 (2-D), so the Krylov space runs out after a
    handful of steps, long before max_it (more steps than there are dofs)."""
    s = sx.one_particle_device(ndim)
    S, Mv = s["S"], s["Mv"]
    K = _operator(s, ALPHA_1, Mv, False)
    n = K.shape[0]
    fixed = np.zeros(n, dtype=bool)
    max_it = sx.lanczos_steps(ndim)
    assert max_it > n
    info = S.tangent_lambda_max(Mv, seed=sx.SEED_LANCZOS, max_it=max_it, rtol=1e-10, mode=True, history=True)
    ref = lanczos_ref.lanczos(K, Mv, fixed, seed=sx.SEED_LANCZOS, max_it=max_it, rtol=1e-10)
    _check_reference(info, ref, f"one particle {ndim}-D")
    assert info["reason"] == lanczos_ref.CONVERGED and info["iterations"] <= n
    lam = np.linalg.eigvalsh(lanczos_ref.scaled_operator(K, Mv, fixed)[0])[-1]
    assert -EPS * n * lam <= lam - info["theta"] <= info["resid"] + 1e-12 * lam
    two = S.tangent_lambda_max(Mv, seed=sx.SEED_LANCZOS, max_it=2, rtol=0.0, history=True)
    assert two["reason"] == lanczos_ref.DIVERGED_ITS and two["iterations"] == 2
    assert np.abs(two["history"] - ref["history"][:2]).max() <= HIST_TOL * ref["history"][1]
    v0 = np.ones(n)
    v0[n // 2] = np.nan
    bad = S.tangent_lambda_max(Mv, v0=v0, mode=True)
    assert bad["reason"] == lanczos_ref.DIVERGED_NANORINF and bad["iterations"] == 0 and not bad["mode"].any()
    S.close()


# ------------------------------------------------------------------------------------------------ Newton
COMMITTED = ("x", "dis", "vel", "acc", "F_n", "J_n", "b_e_n", "mass")


def _newton_pair(dev, ref, start, what, **kw):
    """nlps_gpu_newton_solve beside snes_ref.newton over the twin handle (its linear solve krylov_ref's GMRES at the same
    settings), to the tolerances of test_gpu_newton_solve.py."""
    dU, info = dev.solve(start.copy(), ksp=TIGHT, **kw)
    xr, ir = snes_ref.newton(ref.residual, ref.tangent, start.copy(), linear="gmres", ksp=TIGHT, ndim=dev.S.ndim, **kw)
    print(what, "device", info["reason"], info["fnorm_history"], info["ksp_iterations"], "reference", ir["reason"],
          ir["fnorm_history"], ir["ksp_iterations"])
    _same_counts(info, ir, what)
    # Arnoldi steps: one entry per ACCEPTED iterate on the device; the reference also lists the iterate whose search failed
    kd, kr = info["ksp_iterations"], ir["ksp_iterations"]
    assert len(kd) == info["iterations"] and len(kr) - len(kd) == (1 if ir["reason"] == snes_ref.DIVERGED_LINE_SEARCH else 0)
    assert np.all(np.abs(kd - kr[: len(kd)]) <= 1), (kd, kr)
    assert abs(info["linear_iterations"] - ir["linear_iterations"]) <= len(kr) and info["linear_iterations"] >= kd.sum()
    hd, hr = info["fnorm_history"], ir["fnorm_history"]
    assert len(hd) == len(hr)
    big = hr >= 1e-7 * hr[0]  # (below that the entries are summation noise of the residual's atomics)
    err = float((np.abs(hd - hr)[big] / hr[big]).max())
    assert err <= HISTORY_TOL, f"{what}: fnorm_history, relative {err:.3e}\n{hd}\n{hr}"
    if np.isfinite(xr).all():
        assert_close(dU, xr, 1e-8, f"{what}: dU", scale=max(np.abs(xr).max(), 1e-300))
    return dU, info, xr, ir


def test_newton_exits_of_the_mild_start():
    case, bcs, gravity, nsteps = _problem(2)
    alpha = _alpha(1.0e-2)
    S, S2 = gpu_setup(case, nsteps=nsteps), gpu_setup(case, nsteps=nsteps)
    dev, ref = _Step(S, bcs, 0, alpha, gravity), _Step(S2, bcs, 0, alpha, gravity)
    z = np.zeros(dev.n)
    # snorm < stol xnorm: at iterate 1 snorm == xnorm (the start is 0), at iterate 2 their ratio is 3e-5
    dU, info, xr, ir = _newton_pair(dev, ref, z, "stol", rtol=0.0, atol=0.0, stol=sx.SNES_STOL, linesearch="basic")
    assert info["reason"] == snes_ref.CONVERGED_SNORM_RELATIVE and info["iterations"] == 2
    assert info["snorm"] <= 1e-2 * sx.SNES_STOL * info["xnorm"]
    # the count of evaluations is tested ahead of the relative norm, which iterate 2 meets as well
    for ls in ("basic", "bt"):
        dU, info, xr, ir = _newton_pair(dev, ref, z, f"max_funcs, {ls}", rtol=1e-10, atol=0.0, stol=0.0, max_funcs=2, linesearch=ls)
        assert info["reason"] == snes_ref.DIVERGED_FUNCTION_COUNT and info["iterations"] == 2 and info["function_evaluations"] == 3
    # one NaN in the start vector: no iterate, one evaluation, the committed particle state as before the call
    before = S.download_state()
    start = z.copy()
    start[7] = np.nan
    dU, info = dev.solve(start.copy(), ksp=TIGHT, linesearch="basic")
    xr, ir = snes_ref.newton(ref.residual, ref.tangent, start.copy(), linear="gmres", ksp=TIGHT, ndim=2, linesearch="basic")
    _same_counts(info, ir, "a NaN in the start vector")
    assert info["reason"] == snes_ref.DIVERGED_FNORM_NAN and info["iterations"] == 0 and info["function_evaluations"] == 1
    assert np.array_equal(dU, start, equal_nan=True) and np.isnan(info["fnorm"]) and len(info["fnorm_history"]) == 1
    after = S.download_state()
    for k in COMMITTED:
        assert np.array_equal(after[k], before[k]), f"a NaN in the start vector: {k} moved"
    assert np.isnan(after["F_n1"]).any(), "the state is the one of the evaluation at the returned dU (include/nlps_gpu.h)"
    # and nothing of it stays: the same handle converges from zeros as the reference does
    dU, info, xr, ir = _newton_pair(dev, ref, z, "after the NaN", rtol=1e-10, atol=0.0, stol=0.0, max_it=12, linesearch="basic")
    assert info["reason"] == snes_ref.CONVERGED_FNORM_RELATIVE
    fnorm0 = info["fnorm0"]
    # the remaining reasons of this start, each beside the reference
    dU, info, xr, ir = _newton_pair(dev, ref, z, "atol", rtol=0.0, atol=10.0 * fnorm0, stol=0.0, linesearch="basic")
    assert info["reason"] == snes_ref.CONVERGED_FNORM_ABS and info["iterations"] == 0
    dU, info, xr, ir = _newton_pair(dev, ref, z, "max_it", rtol=1e-10, atol=0.0, stol=0.0, max_it=1, linesearch="basic")
    assert info["reason"] == snes_ref.DIVERGED_MAX_IT and info["iterations"] == 1
    short = dict(pc="pbjacobi", restart=30, max_it=1, rtol=1e-12)
    dU, info = dev.solve(z.copy(), ksp=short, rtol=1e-10, atol=0.0, stol=0.0)
    xr, ir = snes_ref.newton(ref.residual, ref.tangent, z.copy(), linear="gmres", ksp=short, ndim=2, rtol=1e-10, atol=0.0, stol=0.0)
    _same_counts(info, ir, "a linear solve of one step")
    assert info["reason"] == snes_ref.DIVERGED_LINEAR_SOLVE and info["ksp_reason"] == krylov_ref.DIVERGED_ITS
    S.close()
    S2.close()


def test_newton_exits_of_the_violent_start():
    """The start of test_backtracking_and_a_failed_line_search: the full first step raises the norm sevenfold.  With the
    basic line search and a divtol between 1 and that ratio (its square root, from the reference's own history) the solve
    diverges at iterate 1; with bt and no backtracking allowed the search fails.

    No case brings a NaN into a line-search trial from a finite start: the reference stays finite from starts a hundred
    times as violent and a step ten times as long (test_solver_exits_ref.py), so the branch that halves lambda on a
    non-finite trial is not reached here."""
    case, bcs, gravity, nsteps = _problem(2, violent=True)
    alpha = _alpha(5.0e-2)
    S, S2 = gpu_setup(case, nsteps=nsteps), gpu_setup(case, nsteps=nsteps)
    dev, ref = _Step(S, bcs, 0, alpha, gravity), _Step(S2, bcs, 0, alpha, gravity)
    z = np.zeros(dev.n)
    kw = dict(rtol=1e-8, atol=0.0, stol=0.0, linesearch="basic")
    _, free = snes_ref.newton(ref.residual, ref.tangent, z.copy(), linear="gmres", ksp=TIGHT, ndim=2, max_it=1, **kw)
    ratio = free["fnorm_history"][1] / free["fnorm0"]
    assert ratio > 4.0, f"the full first step must raise the norm: {ratio}"
    dU, info, xr, ir = _newton_pair(dev, ref, z, "divtol", divtol=float(np.sqrt(ratio)), **kw)
    assert info["reason"] == snes_ref.DIVERGED_DTOL and info["iterations"] == 1
    dU, info, xr, ir = _newton_pair(dev, ref, z, "no backtracking", rtol=1e-8, atol=0.0, stol=0.0, linesearch="bt", ls_max_it=0)
    assert info["reason"] == snes_ref.DIVERGED_LINE_SEARCH and info["iterations"] == 0 and np.array_equal(dU, z)
    S.close()
    S2.close()


def test_newmark_step_passes_the_reason_through():
    """max_funcs = 2 through nlps_gpu_newmark_step: the reason of the solve comes back, and the step is not committed."""
    case, bcs, gravity, nsteps = _problem(2)
    dt = 2.0e-2
    alpha = _alpha(dt)
    kw = dict(max_it=50, atol=1e-8, rtol=1e-10, stol=1e-8, linesearch="bt", ksp=DRIVER, max_funcs=2)
    S, S2 = gpu_setup(case, nsteps=nsteps), gpu_setup(case, nsteps=nsteps)
    before = S.download_state()
    info = S.newmark_step(bcs, 0, dt, gravity, **kw)
    sep = _Step(S2, bcs, 0, alpha, gravity)
    guess = S2.form_initial_guess(sep.V, sep.A, dt, bcs, 0)
    dU, ir = sep.solve(guess, **kw)
    print("newmark_step", info["reason"], info["fnorm_history"], "the separate calls", ir["reason"], ir["fnorm_history"])
    assert info["reason"] == ir["reason"] == snes_ref.DIVERGED_FUNCTION_COUNT
    for k in ("iterations", "function_evaluations", "linear_iterations"):
        assert info[k] == ir[k], f"{k} {info[k]} vs {ir[k]}"
    after = S.download_state()
    assert np.array_equal(after["x"], before["x"]) and np.array_equal(after["F_n"], before["F_n"])
    assert np.abs(after["F_n1"] - before["F_n"]).max() > 0.0, "the last evaluated state is there"
    S.close()
    S2.close()
