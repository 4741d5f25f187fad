"""Reference Newton solve for nlps_gpu_newton_solve (tests only): the algorithm of include/nlps_gpu.h -- SNES NEWTONLS
with SNESConvergedDefault's tests and the basic or bt line search -- restated in numpy over two callables:
    residual(x) -> F      evaluates the residual at x (and leaves whatever state the tangent is linearised at)
    tangent()   -> K      the dense tangent at the state the last residual left
The linear solve K Y = F is np.linalg.solve (linear="dense") or tests/krylov_ref.py's GMRES (linear="gmres", x0 = 0).
It never calls the code under test; it plays the role krylov_ref.py plays for the linear solve."""
import numpy as np

import krylov_ref

CONVERGED_FNORM_ABS, CONVERGED_FNORM_RELATIVE, CONVERGED_SNORM_RELATIVE = 2, 3, 4
DIVERGED_FUNCTION_COUNT, DIVERGED_LINEAR_SOLVE, DIVERGED_FNORM_NAN = -2, -3, -4
DIVERGED_MAX_IT, DIVERGED_LINE_SEARCH, DIVERGED_DTOL = -5, -6, -9


def _clamp(lt, lam):
    if lt > 0.5 * lam:
        return 0.5 * lam
    if lt <= 0.1 * lam:
        return 0.1 * lam
    return lt


def newton(residual, tangent, x0, max_it=50, max_funcs=10000, atol=1e-8, rtol=1e-10, stol=1e-8, divtol=1e4,
           linesearch="bt", ls_alpha=1e-4, ls_steptol=1e-12, ls_maxstep=1e8, ls_max_it=40, linear="dense", ksp=None,
           ndim=None):
    """Returns (x, info) with info's keys as nlps.Solver.newton_solve's.  ksp: dict(pc, restart, max_it, rtol, atol, dtol)
    for linear="gmres" (ndim: the block size of "pbjacobi")."""
    nf = [0]

    def evaluate(x):
        nf[0] += 1
        F = np.array(residual(x), dtype=np.float64)
        return F, float(np.linalg.norm(F))

    kw = dict(pc="jacobi", restart=30, max_it=10000, rtol=1e-5, atol=0.0, dtol=1e5)
    kw.update(ksp or {})
    X = np.array(x0, dtype=np.float64)
    F, fnorm = evaluate(X)
    fnorm0 = fnorm
    fhist, lhist, khist = [fnorm], [], []
    its, snorm, xnorm, reason = 0, 0.0, 0.0, 0
    if not np.isfinite(fnorm):
        reason = DIVERGED_FNORM_NAN
    elif fnorm < atol:
        reason = CONVERGED_FNORM_ABS
    while not reason and its < max_it:
        K = tangent()
        if linear == "dense":
            Y = np.linalg.solve(K, F)
            khist.append(0)
        else:
            pc = krylov_ref.preconditioner(K, kw["pc"], ndim)
            Y, ki = krylov_ref.gmres(K, F, pc, restart=kw["restart"], max_it=kw["max_it"], rtol=kw["rtol"],
                                     atol=kw["atol"], dtol=kw["dtol"])
            khist.append(ki["iterations"])
            if ki["reason"] < 0:
                reason = DIVERGED_LINEAR_SOLVE
                break
        lam = 1.0
        ynorm = float(np.linalg.norm(Y))
        accepted = True
        if linesearch == "basic":
            W = X - Y
            G, gnorm = evaluate(W)
        else:
            s = float(F @ (K @ Y))
            ratio = float(np.max(np.abs(Y) / np.maximum(np.abs(X), 1.0))) if Y.size else 0.0
            W = X - Y
            G, gnorm = evaluate(W)
            if ynorm > ls_maxstep:  # (the full step is evaluated before ||Y|| is known; it counts, the scaled one follows)
                sc = ls_maxstep / ynorm
                Y, s, ratio, ynorm = sc * Y, sc * s, sc * ratio, ls_maxstep
                W = X - Y
                G, gnorm = evaluate(W)
            if s > 0.0:
                s = -s
            if s == 0.0:
                s = -1.0
            with np.errstate(divide="ignore"):
                minlam = ls_steptol / ratio if ratio > 0.0 else np.inf
            f2 = fnorm * fnorm

            def accept(g, lam_):
                return bool(np.isfinite(g) and 0.5 * g * g <= 0.5 * f2 + ls_alpha * lam_ * s)

            if ynorm != 0.0 and not accept(gnorm, lam):
                accepted = False
                if ls_max_it > 0:
                    g2 = gnorm * gnorm
                    lprev, g2prev = lam, g2
                    lam = _clamp(-s / (g2 - f2 - 2.0 * lam * s), lam) if np.isfinite(g2) else 0.5 * lam
                    W = X - lam * Y
                    G, gnorm = evaluate(W)
                    accepted = accept(gnorm, lam)
                    for _ in range(ls_max_it):
                        if accepted or lam < minlam:
                            break
                        g2 = gnorm * gnorm
                        lt = 0.5 * lam
                        if np.isfinite(g2) and np.isfinite(g2prev):
                            t1 = 0.5 * (g2 - f2) - lam * s
                            t2 = 0.5 * (g2prev - f2) - lprev * s
                            a = (t1 / (lam * lam) - t2 / (lprev * lprev)) / (lam - lprev)
                            b = (-lprev * t1 / (lam * lam) + lam * t2 / (lprev * lprev)) / (lam - lprev)
                            d = max(b * b - 3.0 * a * s, 0.0)
                            lt = -s / (2.0 * b) if a == 0.0 else (-b + np.sqrt(d)) / (3.0 * a)
                            lt = _clamp(lt, lam)
                        lprev, g2prev = lam, g2
                        lam = lt
                        W = X - lam * Y
                        G, gnorm = evaluate(W)
                        accepted = accept(gnorm, lam)
        if not accepted:
            F, fnorm = evaluate(X)  # the state goes back to X
            reason = DIVERGED_LINE_SEARCH
            break
        X, F, fnorm = W, G, gnorm
        its += 1
        snorm = lam * ynorm
        xnorm = float(np.linalg.norm(X))
        fhist.append(fnorm)
        lhist.append(lam)
        if not np.isfinite(fnorm):
            reason = DIVERGED_FNORM_NAN
        elif fnorm < atol:
            reason = CONVERGED_FNORM_ABS
        elif nf[0] > max_funcs:
            reason = DIVERGED_FUNCTION_COUNT
        elif fnorm <= rtol * fnorm0:
            reason = CONVERGED_FNORM_RELATIVE
        elif snorm < stol * xnorm:
            reason = CONVERGED_SNORM_RELATIVE
        elif fnorm > divtol * fnorm0:
            reason = DIVERGED_DTOL
    if not reason:
        reason = DIVERGED_MAX_IT
    return X, dict(reason=reason, iterations=its, function_evaluations=nf[0], linear_iterations=int(sum(khist)),
                   fnorm0=fnorm0, fnorm=fnorm, snorm=snorm, xnorm=xnorm, fnorm_history=np.array(fhist),
                   lambda_history=np.array(lhist), ksp_iterations=np.array(khist, dtype=np.int64))
