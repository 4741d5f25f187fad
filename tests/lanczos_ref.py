"""Reference Lanczos for nlps_gpu_tangent_lambda_max (tests only): the algorithm of include/nlps_gpu.h in numpy on a dense K.
A = P S K S P with S = diag(M^-1/2) and P the projection off the fixed dofs; q_1 = P v0 / ||P v0|| (v0 None: the splitmix64
hash vector of seed); per step w = A q_j, alpha_j = q_j . w, classical Gram-Schmidt against every q_i with the DGKS second
pass, beta_j = ||w||, the largest eigenpair (theta_j, s) of T_j, est_j = beta_j |s_j|, history[j-1] = theta_j; the stopping
rules in the header's order; y = Q s, resid = ||A y - theta y|| from one more product, mode = S y."""
import numpy as np

CONVERGED, EMPTY, DIVERGED_ITS, DIVERGED_NANORINF = 1, 2, -3, -9
_M64 = (1 << 64) - 1


def hash_vector(seed, n):
    """Component i: output i + 1 of the splitmix64 stream seeded with seed, top 53 bits as u in [0, 1), 2 u - 1."""
    with np.errstate(over="ignore"):
        i = np.arange(1, n + 1, dtype=np.uint64)
        z = np.uint64(seed & _M64) + i * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return 2.0 * ((z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53) - 1.0


def scaled_operator(K, M, fixed):
    """A = P S K S P as a dense matrix and ps = the diagonal of P S (0 on the fixed dofs)."""
    fixed = np.zeros(K.shape[0], dtype=bool) if fixed is None else np.asarray(fixed, dtype=bool)
    ps = np.zeros(K.shape[0])
    ps[~fixed] = 1.0 / np.sqrt(np.asarray(M, dtype=np.float64)[~fixed])
    return ps[:, None] * K * ps[None, :], ps


def lanczos(K, M, fixed=None, v0=None, seed=0, max_it=64, rtol=1e-6):
    """dict(reason, iterations, theta, resid, asymmetry, history, mode, y)"""
    n = K.shape[0]
    A, ps = scaled_operator(K, M, fixed)
    q = hash_vector(seed, n) if v0 is None else np.array(v0, dtype=np.float64)
    q = np.where(ps != 0.0, q, 0.0)
    n2 = float(q @ q)
    out = dict(reason=0, iterations=0, theta=0.0, resid=0.0, asymmetry=0.0, history=np.zeros(0), mode=np.zeros(n), y=np.zeros(n))
    if n == 0 or n2 == 0.0:
        out["reason"] = EMPTY
        return out
    if not np.isfinite(n2):
        out.update(reason=DIVERGED_NANORINF, resid=float("nan"))
        return out
    Q =np.zeros((max_it + 1, n))
    Q[0] = q / np.sqrt(n2)
    alpha, beta, hist = np.zeros(max_it), np.zeros(max_it), []
    asym, theta, s, reason, its = 0.0, 0.0, None, 0, 0
    for j in range(max_it):
        w = A @ Q[j]
        alpha[j] = Q[j] @ w
        h1 = Q[: j + 1] @ w
        ww = w @ w
        w = w - Q[: j + 1].T @ h1
        wn2 = w @ w
        if wn2 < 0.5 * ww:  # DGKS: one more pass
            w = w - Q[: j + 1].T @ (Q[: j + 1] @ w)
            wn2 = w @ w
        beta[j] = np.sqrt(wn2)
        T = np.diag(alpha[: j + 1]) + np.diag(beta[:j], 1) + np.diag(beta[:j], -1)
        if not np.isfinite(T).all():
            reason, its = DIVERGED_NANORINF, j + 1
            break
        lam, vec = np.linalg.eigh(T)
        theta, s = float(lam[-1]), vec[:, -1]
        est = beta[j] * abs(s[-1])
        hist.append(theta)
        its = j + 1
        if j > 0:
            t = h1[:j].copy()
            t[j - 1] -= beta[j - 1]
            asym = max(asym, float(np.sqrt(t @ t)) / abs(theta))
        if not (np.isfinite(theta) and np.isfinite(est) and np.isfinite(asym)):
            reason = DIVERGED_NANORINF
        elif est <= rtol * abs(theta) or beta[j] == 0.0:
            reason = CONVERGED
        elif its == max_it:
            reason = DIVERGED_ITS
        if reason:
            break
        Q[j + 1] = w / beta[j]
    out.update(reason=reason, iterations=its, theta=theta, asymmetry=asym, history=np.array(hist))
    if reason != DIVERGED_NANORINF:
        y = Q[:its].T @ s
        out.update(resid=float(np.linalg.norm(A @ y - theta * y)), y=y, mode=ps * y)
    else:
        out["resid"] = float("nan")
    return out
