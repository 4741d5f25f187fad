"""Reference MINRES for nlps_gpu_tangent_solve with NLPS_KSP_TYPE_MINRES (tests only): the preconditioned MINRES of
include/nlps_gpu.h in numpy on a dense symmetric K, statement by statement.  The Lanczos vectors v carry their M^-1 norm g
(q = M^-1 v / g is the normalised direction), the QR of the tridiagonal goes by one rotation per step, and the estimate
est = scale |eta| is the preconditioned residual norm calibrated to the true one: at r0 and at every confirmation that
did not end the solve.  A confirmation is one product, b - K x, and leaves the recurrence alone.
history[0] = ||b - K x0||, history[k] = est after step k.  Returns what krylov_ref.gmres does (x, dict(iterations, reason,
rnorm, bnorm, history)) plus confirmations, the number of true residuals taken inside the loop."""
import numpy as np

CONVERGED_BZERO, CONVERGED_RTOL, CONVERGED_ATOL = 1, 2, 3
DIVERGED_ITS, DIVERGED_DTOL, DIVERGED_BREAKDOWN, DIVERGED_INDEFINITE_PC, DIVERGED_NANORINF = -3, -4, -5, -8, -9


def minres(K, b, Minv, max_it=10000, rtol=1e-5, atol=0.0, dtol=1e5, x0=None):
    n = b.shape[0]
    bnorm = float(np.linalg.norm(b))
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)

    def done(reason, its, rnorm, hist, conf):
        return x, dict(iterations=its, reason=reason, rnorm=rnorm, bnorm=bnorm, history=np.array(hist), confirmations=conf)

    if bnorm == 0.0:
        x = np.zeros(n)
        return done(CONVERGED_BZERO, 0, 0.0, [0.0], 0)
    r0 = b - K @ x if x0 is not None else b.copy()
    rnorm = float(np.linalg.norm(r0))
    tol = max(rtol * bnorm, atol)
    hist = [rnorm]
    if not (np.isfinite(rnorm) and np.isfinite(bnorm)):
        return done(DIVERGED_NANORINF, 0, rnorm, hist, 0)
    if rnorm <= tol:
        return done(CONVERGED_ATOL if rnorm < atol else CONVERGED_RTOL, 0, rnorm, hist, 0)
    if rnorm > dtol * bnorm:
        return done(DIVERGED_DTOL, 0, rnorm, hist, 0)
    if max_it == 0:
        return done(DIVERGED_ITS, 0, rnorm, hist, 0)
    v_prev, v = np.zeros(n), r0
    z = Minv(v)
    vz = float(v @ z)
    if vz <= 0.0:
        return done(DIVERGED_INDEFINITE_PC, 0, rnorm, hist, 0)
    if not np.isfinite(vz):
        return done(DIVERGED_NANORINF, 0, rnorm, hist, 0)
    g = np.sqrt(vz)
    g_prev, eta, scale = 1.0, g, rnorm / g
    c_prev = c = 1.0
    s_prev = s = 0.0
    w_prev, w = np.zeros(n), np.zeros(n)
    its, conf = 0, 0

    def early(reason):  # (the true residual of the x that is returned)
        return done(reason, its, float(np.linalg.norm(b - K @ x)), hist, conf)

    with np.errstate(all="ignore"):
        while True:
            k = its + 1
            q = z / g
            p = K @ q
            d = float(p @ q)
            v_new = p - (d / g) * v - (g / g_prev) * v_prev
            z_new = Minv(v_new)
            gg = float(v_new @ z_new)
            if gg < 0.0:
                return early(DIVERGED_INDEFINITE_PC)
            if not (np.isfinite(d) and np.isfinite(gg)):
                return early(DIVERGED_NANORINF)
            g_new = np.sqrt(gg)
            a0 = c * d - c_prev * s * g
            a1 = np.sqrt(a0 * a0 + gg)
            a2 = s * d + c_prev * c * g
            a3 = s_prev * g
            if a1 == 0.0:
                return early(DIVERGED_BREAKDOWN)
            c_prev, c = c, a0 / a1
            s_prev, s = s, g_new / a1
            w_new = (q - a3 * w_prev - a2 * w) / a1
            x = x + (c * eta) * w_new
            eta = -s * eta
            v_prev, v, z, g_prev, g, w_prev, w = v, v_new, z_new, g, g_new, w, w_new
            its = k
            est = scale * abs(eta)
            hist.append(est)
            if not np.isfinite(est):
                return early(DIVERGED_NANORINF)
            if est <= tol or k == max_it or g_new == 0.0:
                conf += 1
                rnorm = float(np.linalg.norm(b - K @ x))
                if not np.isfinite(rnorm):
                    return done(DIVERGED_NANORINF, its, rnorm, hist, conf)
                if rnorm <= tol:
                    return done(CONVERGED_ATOL if rnorm < atol else CONVERGED_RTOL, its, rnorm, hist, conf)
                if rnorm > dtol * bnorm:
                    return done(DIVERGED_DTOL, its, rnorm, hist, conf)
                if k == max_it:
                    return done(DIVERGED_ITS, its, rnorm, hist, conf)
                if g_new == 0.0:
                    return done(DIVERGED_BREAKDOWN, its, rnorm, hist, conf)
                scale = rnorm / abs(eta)
