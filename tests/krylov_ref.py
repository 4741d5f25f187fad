"""Reference GMRES for nlps_gpu_tangent_solve (tests only): right-preconditioned restarted GMRES(m) in numpy on a dense K,
classical Gram-Schmidt with the same DGKS second pass (when ||w|| drops below 1/sqrt 2 of its value), Givens rotations,
and the same stopping rules: the estimate |g[j+1]| ends a cycle, the true residual b - K x at the end of every cycle
confirms it or starts the next one.  history[0] = ||b - K x0||, history[k] = the estimate after Arnoldi step k.
Beside the device's outputs the returned dict says what the device cannot: refined[k] whether step k + 1 took the DGKS second
pass (refinements: how many did) and happy_ratio[k] = hn / sqrt(w . w), what the happy-breakdown gate compares with HAPPY."""
import numpy as np

CONVERGED_BZERO, CONVERGED_RTOL, CONVERGED_ATOL = 1, 2, 3
DIVERGED_ITS, DIVERGED_DTOL, DIVERGED_BREAKDOWN, DIVERGED_NANORINF = -3, -4, -5, -9
HAPPY = 1e-14


def preconditioner(K, kind, ndim):
    """M^-1 as a function: "none", "jacobi" (reciprocal diagonal) or "pbjacobi" (inverted d x d diagonal blocks)."""
    n = K.shape[0]
    if kind == "none":
        return lambda v: v.copy()
    if kind == "jacobi":
        dinv = 1.0 / np.diag(K)
        return lambda v: dinv * v
    na = n // ndim
    B = np.stack([K[A * ndim:(A + 1) * ndim, A * ndim:(A + 1) * ndim] for A in range(na)])
    Binv = np.linalg.inv(B)
    return lambda v: np.einsum("aij,aj->ai", Binv, v.reshape(na, ndim)).ravel()


def gmres(K, b, Minv, restart=30, max_it=10000, rtol=1e-5, atol=0.0, dtol=1e5, x0=None):
    n = b.shape[0]
    bnorm = float(np.linalg.norm(b))
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    if bnorm == 0.0:
        return np.zeros(n), dict(iterations=0, reason=CONVERGED_BZERO, rnorm=0.0, bnorm=0.0, history=np.zeros(1),
                                 refinements=0, refined=np.zeros(0, dtype=bool), happy_ratio=np.zeros(0))
    r = b - K @ x
    rnorm = float(np.linalg.norm(r))
    tol = max(rtol * bnorm, atol)
    hist = [rnorm]
    its, broke, reason = 0, False, 0
    refined, ratio = [], []  # per Arnoldi step: did the DGKS second pass run, and hn / sqrt(ww) (what the happy gate sees)
    m = restart
    while True:
        if not (np.isfinite(rnorm) and np.isfinite(bnorm)):
            reason = DIVERGED_NANORINF
        elif rnorm <= tol:
            reason = CONVERGED_ATOL if rnorm < atol else CONVERGED_RTOL
        elif rnorm > dtol * bnorm:
            reason = DIVERGED_DTOL
        elif its >= max_it:
            reason = DIVERGED_ITS
        elif broke:
            reason = DIVERGED_BREAKDOWN
        if reason:
            break
        V = np.zeros((m + 1, n))
        V[0] = r / rnorm
        R = np.zeros((m, m))
        cs, sn, g = np.zeros(m), np.zeros(m), np.zeros(m + 1)
        g[0] = rnorm
        k, nonfinite = 0, False
        for j in range(m):
            w = K @ Minv(V[j])
            h = V[: j + 1] @ w
            ww = w @ w
            w = w - V[: j + 1].T @ h
            wn2 = w @ w
            refined.append(bool(wn2 < 0.5 * ww))
            if wn2 < 0.5 * ww:  # DGKS: one more pass
                h2 = V[: j + 1] @ w
                w = w - V[: j + 1].T @ h2
                wn2 = w @ w
                h = h + h2
            hn = np.sqrt(wn2)
            ratio.append(hn / np.sqrt(ww) if ww > 0.0 else 0.0)
            col = np.append(h, hn)
            for i in range(j):
                a, bb = col[i], col[i + 1]
                col[i] = cs[i] * a + sn[i] * bb
                col[i + 1] = -sn[i] * a + cs[i] * bb
            a = col[j]
            rr = np.sqrt(a * a + hn * hn)
            singular = not rr > 0.0
            c, s = (a / rr, hn / rr) if not singular else (1.0, 0.0)
            cs[j], sn[j] = c, s
            gj = g[j]
            g[j], g[j + 1] = c * gj, -s * gj
            R[: j, j] = col[:j]
            R[j, j] = rr
            est = abs(g[j + 1])
            its += 1
            hist.append(est)
            if not (np.isfinite(est) and np.isfinite(rr) and np.isfinite(col[: j + 1]).all()):
                nonfinite = True
                break
            if singular:
                broke = True
                break
            if hn > 0.0:
                V[j + 1] = w / hn
            k = j + 1
            if est <= tol or hn <= HAPPY * np.sqrt(ww) or its >= max_it:
                break
        if nonfinite:
            reason = DIVERGED_NANORINF
            break
        if k > 0:
            y = np.zeros(k)
            for i in range(k - 1, -1, -1):
                y[i] = (g[i] - R[i, i + 1:k] @ y[i + 1:k]) / R[i, i]
            x = x + Minv(V[:k].T @ y)
        r = b - K @ x
        rnorm = float(np.linalg.norm(r))
    return x, dict(iterations=its, reason=reason, rnorm=rnorm, bnorm=bnorm, history=np.array(hist),
                   refinements=int(np.sum(refined)), refined=np.array(refined, dtype=bool), happy_ratio=np.array(ratio))
