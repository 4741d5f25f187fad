// Device MINRES on the matrix-free tangent (nlps_gpu_tangent_solve with NLPS_KSP_TYPE_MINRES): the preconditioned
// short recurrence of include/nlps_gpu.h for a symmetric K and a symmetric positive definite M^-1, around y = K x of
// nlps_tangent_operator.hpp.  Per step, beside the product:
//   k_minres_dot      the partial sums of p . q                                        (elements, KSP_TILE per block)
//   k_minres_lanczos  d = p . q, v_new = p - (d / g) v - (g / g_prev) v_prev over v_prev, z = M^-1 v_new and the partial
//                     sums of v_new . z                                                (one masked node per thread)
//   k_minres_rotate   one wave: gg, the rotation, the step's coefficients into the small device state, |eta| and the
//                     flags into the host word
//   k_minres_update   w_new over w_prev, x += c eta w_new, q = z / g_new                (elements)
// Seven vectors: two v, z, q, p (also the K x of a confirmation) and two w; the pairs rotate by pointer on the host.
// Sums as in nlps_krylov.hpp: one partial per block, added in a fixed order, no float atomics.  The coefficients never
// leave the device; a step that must not touch x (MINRES_SKIP) turns k_minres_update into a no-op.
#pragma once

enum { MINRES_FLAG_INDEFINITE = 8, MINRES_FLAG_GZERO = 16 };  // beside KSP_FLAG_NONFINITE and KSP_FLAG_SINGULAR (a1 == 0)

// the small device state (doubles)
enum {
  MINRES_D = 0,   // p . q of the step
  MINRES_G,       // g: the M^-1 norm of v
  MINRES_GP,      // g_prev
  MINRES_ETA,
  MINRES_C,
  MINRES_CP,
  MINRES_S,
  MINRES_SP,
  MINRES_A1,      // the step's column of the rotated tridiagonal
  MINRES_A2,
  MINRES_A3,
  MINRES_TAU,     // c eta: the step of x along w_new
  MINRES_SKIP,    // 1.0: the step's update is not applied
  MINRES_SMALL = 16
};

// partial sums of p . q
__global__ __launch_bounds__(KSP_NT) void k_minres_dot(int n, const double* __restrict__ p, const double* __restrict__ q,
                                                       double* __restrict__ partials) {
  __shared__ double red4[KSP_NT / 64];
  const int base = blockIdx.x * KSP_TILE + threadIdx.x;
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < KSP_EPT; e++) {
    const int i = base + e * KSP_NT;
    if (i < n) s = fma(p[i], q[i], s);
  }
  s = ksp_block_sum(s, red4);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// The Lanczos step on the masked nodes, one node per thread.  Every block adds the nbd partials of p . q in the same
// fixed order (block 0 leaves d in the state for k_minres_rotate).  first: v_new = p (= r0, already where v lives).
// vio holds v_prev on entry and v_new on return.
template <int ND>
__global__ __launch_bounds__(KSP_NT) void k_minres_lanczos(int nA, int kind, const double* __restrict__ Minv, int first,
                                                           const double* __restrict__ p, const double* __restrict__ v,
                                                           double* __restrict__ vio, double* __restrict__ z,
                                                           const double* __restrict__ dpart, int nbd,
                                                           double* __restrict__ s, double* __restrict__ partials) {
  __shared__ double red4[KSP_NT / 64];
  double cv = 0.0, cp = 0.0;
  if (!first) {
    double a = 0.0;
    for (int i = threadIdx.x; i < nbd; i += KSP_NT) a += dpart[i];
    const double d = ksp_block_sum(a, red4);
    __syncthreads();  // (red4 serves the second sum below)
    const double g = s[MINRES_G];
    cv = d / g;
    cp = g / s[MINRES_GP];
    if (blockIdx.x == 0 && threadIdx.x == 0) s[MINRES_D] = d;
  }
  const int m = blockIdx.x * KSP_NT + threadIdx.x;
  double acc = 0.0;
  if (m < nA) {
    double vn[ND], zz[ND];
#pragma unroll
    for (int f = 0; f < ND; f++) {
      const size_t i = (size_t)m * ND + f;
      vn[f] = first ? p[i] : fma(-cp, vio[i], fma(-cv, v[i], p[i]));
    }
    ksp_pc_node<ND>(kind, Minv, m, vn, zz);
#pragma unroll
    for (int f = 0; f < ND; f++) {
      const size_t i = (size_t)m * ND + f;
      if (!first) vio[i] = vn[f];
      z[i] = zz[f];
      acc = fma(vn[f], zz[f], acc);
    }
  }
  acc = ksp_block_sum(acc, red4);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// One wave: gg = the sum of the nb partials of v_new . z in a fixed order, then lane 0 alone.  first: g = sqrt(v . z)
// and the start of the recurrence.  Otherwise the step's rotation and the shift of (g, c, s, eta).  The host word gets
// |eta| (first: g) and the flags; the host scales |eta| to the estimate.
__global__ __launch_bounds__(64) void k_minres_rotate(int first, const double* __restrict__ partials, int nb,
                                                      double* __restrict__ s, KspHost* __restrict__ hw) {
  double gg = 0.0;
  for (int i = threadIdx.x; i < nb; i += 64) gg += partials[i];
  gg = ksp_wave_sum(gg);
  if (threadIdx.x != 0) return;
  int flags = 0;
  if (first) {
    if (gg <= 0.0) flags = MINRES_FLAG_INDEFINITE;
    else if (!isfinite(gg)) flags = KSP_FLAG_NONFINITE;
    const double g = sqrt(gg);
    s[MINRES_G] = g;
    s[MINRES_GP] = 1.0;
    s[MINRES_ETA] = g;
    s[MINRES_C] = s[MINRES_CP] = 1.0;
    s[MINRES_S] = s[MINRES_SP] = 0.0;
    s[MINRES_SKIP] = flags ? 1.0 : 0.0;
    hw->est = g;
    hw->flags = flags;
    return;
  }
  const double d = s[MINRES_D], g = s[MINRES_G], c = s[MINRES_C], cp = s[MINRES_CP], sn = s[MINRES_S], sp = s[MINRES_SP];
  double eta = s[MINRES_ETA];
  if (gg < 0.0) {
    flags = MINRES_FLAG_INDEFINITE;
  } else if (!isfinite(d) || !isfinite(gg)) {
    flags = KSP_FLAG_NONFINITE;
  } else {
    const double gn = sqrt(gg);
    const double a0 = c * d - cp * sn * g;
    const double a1 = sqrt(a0 * a0 + gg);
    const double a2 = sn * d + cp * c * g;
    const double a3 = sp * g;
    if (a1 == 0.0) {
      flags = KSP_FLAG_SINGULAR;
    } else {
      const double cn = a0 / a1, snn = gn / a1;
      s[MINRES_A1] = a1;
      s[MINRES_A2] = a2;
      s[MINRES_A3] = a3;
      s[MINRES_TAU] = cn * eta;
      eta = -snn * eta;
      s[MINRES_ETA] = eta;
      s[MINRES_CP] = c;
      s[MINRES_C] = cn;
      s[MINRES_SP] = sn;
      s[MINRES_S] = snn;
      s[MINRES_GP] = g;
      s[MINRES_G] = gn;
      if (gn == 0.0) flags = MINRES_FLAG_GZERO;
    }
  }
  s[MINRES_SKIP] = (flags & ~MINRES_FLAG_GZERO) ? 1.0 : 0.0;
  hw->est = fabs(eta);
  hw->flags = flags;
}

// w_new = (q - a3 w_prev - a2 w) / a1 over w_prev, x += c eta w_new, and the next step's q = z / g_new (kept when
// g_new == 0: the solve ends there).  first: only q = z / g.
__global__ __launch_bounds__(KSP_NT) void k_minres_update(int n, int first, const double* __restrict__ s,
                                                          const double* __restrict__ z, double* __restrict__ q,
                                                          double* __restrict__ wio, const double* __restrict__ w,
                                                          double* __restrict__ x) {
  if (s[MINRES_SKIP] != 0.0) return;
  const double gn = s[MINRES_G];
  const double a1 = s[MINRES_A1], a2 = s[MINRES_A2], a3 = s[MINRES_A3], tau = s[MINRES_TAU];
  const int base = blockIdx.x * KSP_TILE + threadIdx.x;
#pragma unroll
  for (int e = 0; e < KSP_EPT; e++) {
    const int i = base + e * KSP_NT;
    if (i >= n) continue;
    if (!first) {
      const double wn = fma(-a2, w[i], fma(-a3, wio[i], q[i])) / a1;
      wio[i] = wn;
      x[i] = fma(tau, wn, x[i]);
    }
    if (gn > 0.0) q[i] = z[i] / gn;
  }
}
