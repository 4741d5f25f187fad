// Device Lanczos on the matrix-free tangent (nlps_gpu_tangent_lambda_max): the largest Ritz value of the pencil (K, M) on
// the free dofs, the bound on the explicit step's stable time step (include/nlps_gpu.h states the algorithm; this file
// and tests/lanczos_ref.py restate it).
//
// A = P S K S P with S = diag(M^-1/2) and P the projection off the Dirichlet dofs of the operator's snapshot.  Both live
// in ONE masked array ps: ps[i] = 1 / sqrt(M[i]) on a free dof, 0 on a fixed one.  k_eig_expand folds x = ps q into the
// product's gather array (as k_ksp_pc_expand folds the preconditioner), k_eig_nodal is the nodal epilogue
// w = ps (K x) with the partial sums of alpha = q . w.  The orthogonalisation is the GMRES's (k_ksp_mdot / k_ksp_maxpy /
// k_ksp_finish / k_ksp_scale of nlps_krylov.hpp), so are the vector layout and the fixed-order sums: no float atomics here.
//
// The small state of a run lives in one device array of doubles (EigSmall offsets).  k_eig_ritz (one wave) appends
// alpha_j, beta_j to T, finds T's largest eigenpair and leaves theta, est and the flags in the host-visible word EigHost.
#pragma once

enum { EIG_FLAG_NONFINITE = 1 };

// what the host reads after a step (a pinned word the kernels write through its device alias)
struct EigHost {
  double theta;  // largest eigenvalue of T_j
  double est;    // beta_j |s_j|
  double asym;   // the running maximum of the asymmetry measure
  double n2;     // ||P v0||^2
  double rn2;    // ||A y - theta y||^2
  int flags;     // EIG_FLAG_*
  int bad;       // first masked node with an unusable mass on a free dof (>= N_A: none)
};

// offsets into the small device array of a run of at most m steps
struct EigSmall {
  int m;
  __host__ __device__ int h1() const { return 0; }               // [m + 2] pass 1: Q^T w, then w.w at [j + 1]
  __host__ __device__ int h2() const { return (m + 2); }         // [m + 2] pass 2 (DGKS refinement)
  __host__ __device__ int alpha() const { return 2 * (m + 2); }  // [m + 2] diagonal of T
  __host__ __device__ int beta() const { return 3 * (m + 2); }   // [m + 2] off-diagonal of T, beta[j] = ||w|| of step j
  __host__ __device__ int s() const { return 4 * (m + 2); }      // [m + 2] the Ritz vector of the last step in T's basis
  __host__ __device__ int wn2() const { return 5 * (m + 2); }    // ||w||^2 after the latest multi-axpy
  __host__ __device__ int refine() const { return 5 * (m + 2) + 1; }  // 1.0: the second pass runs
  __host__ __device__ int aj() const { return 5 * (m + 2) + 2; }      // q_j . w of the step (the nodal epilogue's)
  __host__ __device__ int n2() const { return 5 * (m + 2) + 3; }      // ||P v0||^2
  __host__ __device__ int theta() const { return 5 * (m + 2) + 4; }   // theta of the last step
  __host__ __device__ int asym() const { return 5 * (m + 2) + 5; }    // running maximum
  __host__ __device__ size_t size() const { return (size_t)5 * (m + 2) + 8; }
};

// component i of the default start vector: output i + 1 of the splitmix64 stream seeded with seed, its top 53 bits
// as a fraction u in [0, 1), mapped to 2 u - 1 in [-1, 1)
__host__ __device__ __forceinline__ double eig_hash(unsigned long long seed, unsigned long long i) {
  unsigned long long z = seed + (i + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return 2.0 * ((double)(z >> 11) * 0x1.0p-53) - 1.0;
}

// ps = P S from the mass and the Dirichlet mask (d2m == NULL: P = I), the unnormalised start vector q = P v0 (v0 == NULL:
// the hash) and the partial sums of ||q||^2.  A mass that is not positive and finite on a free dof lowers *bad to its
// masked node and leaves ps = 0 there.
__global__ __launch_bounds__(KSP_NT) void k_eig_start(int n, int nd, const int* __restrict__ d2m,
                                                      const double* __restrict__ mass, const double* __restrict__ v0,
                                                      unsigned long long seed, double* __restrict__ ps,
                                                      double* __restrict__ q, double* __restrict__ partials,
                                                      int* __restrict__ bad) {
  __shared__ double red4[KSP_NT / 64];
  const int base = blockIdx.x * KSP_TILE + threadIdx.x;
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < KSP_EPT; e++) {
    const int i = base + e * KSP_NT;
    if (i < n) {
      double p = 0.0;
      if (!(d2m && d2m[i] == -1)) {
        const double mi = mass[i];
        if (mi > 0.0 && isfinite(mi)) p = 1.0 / sqrt(mi);
        else atomicMin(bad, i / nd);
      }
      const double v = p != 0.0 ? (v0 ? v0[i] : eig_hash(seed, (unsigned long long)i)) : 0.0;
      ps[i] = p;
      q[i] = v;
      s = fma(v, v, s);
    }
  }
  s = ksp_block_sum(s, red4);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// The product's input with the scaling and the projection folded in: x = ps q on the masked node (kept in xs: the mass
// term of the nodal epilogue reads it), xg = x in grid numbering (0 on inactive nodes) and the zeroed accumulator yg.
template <int ND>
__global__ void k_eig_expand(int nnodes, const int* __restrict__ n2m, const double* __restrict__ ps,
                             const double* __restrict__ q, double* __restrict__ xs, double* __restrict__ xg,
                             double* __restrict__ yg) {
  const int A = blockIdx.x * blockDim.x + threadIdx.x;
  if (A >= nnodes) return;
  const int m = n2m[A];
#pragma unroll
  for (int f = 0; f < ND; f++) {
    const size_t i = (size_t)m * ND + f;
    double x = 0.0;
    if (m >= 0) {
      const double p = ps[i];
      x = p != 0.0 ? p * q[i] : 0.0;
      xs[i] = x;
    }
    xg[(size_t)A * ND + f] = x;
    yg[(size_t)A * ND + f] = 0.0;
  }
}

// The nodal epilogue w = ps (K x + alpha_1 M x) (0 on the fixed dofs) with the partial sums of q . w, one per block
// (q == NULL: only w).  Every thread reaches the block sum.
template <int ND>
__global__ __launch_bounds__(KSP_NT) void k_eig_nodal(int nnodes, const int* __restrict__ n2m, const double* __restrict__ yg,
                                                      const double* __restrict__ xs, const double* __restrict__ aM,
                                                      const double* __restrict__ ps, const double* __restrict__ q,
                                                      double* __restrict__ w, double* __restrict__ partials) {
  __shared__ double red4[KSP_NT / 64];
  const int A = blockIdx.x * KSP_NT + threadIdx.x;
  const int m = A < nnodes ? n2m[A] : -1;
  double s = 0.0;
  if (m >= 0) {
#pragma unroll
    for (int f = 0; f < ND; f++) {
      const size_t i = (size_t)m * ND + f;
      const double p = ps[i];
      double v = 0.0;
      if (p != 0.0) {
        v = yg[(size_t)A * ND + f];
        if (aM) v = fma(aM[i], xs[i], v);
        v *= p;
      }
      w[i] = v;
      if (q) s = fma(q[i], v, s);
    }
  }
  if (!partials) return;  // (uniform)
  s = ksp_block_sum(s, red4);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__device__ __forceinline__ double eig_wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  return v;  // (every lane)
}
__device__ __forceinline__ double eig_wave_min(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ double eig_wave_allsum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// One Lanczos step's small work, one wave, k = j + 1 rows of T (j counts from 0):
//   * appends alpha[j] = q_j . w (the nodal epilogue's) and beta[j] = sqrt(wn2) to T;
//   * the asymmetry measure of the step from the first Gram-Schmidt pass h1 (lanes stride the row);
//   * theta = the largest eigenvalue of T_k by multisection on Sturm counts: every lane counts the negative pivots of
//     T - x I at its own x, 64 points per round, the bracket shrinks 65 times per round (9 rounds to one ulp);
//   * its eigenvector by the twisted factorisation: lane 0 the pivots from the top, lane 1 those from the bottom in the
//     same instructions, the twist at the smallest |gamma|, then the two substitutions away from it;
//   * est = beta[j] |s[k - 1]|, theta, the flags and the running asymmetry into the host word.
// T, the pivots and s sit in LDS.  Every barrier is reached by all 64 lanes; the shuffles sit in uniform control flow.
__global__ __launch_bounds__(64) void k_eig_ritz(EigSmall L, double* __restrict__ sm, int j, EigHost* __restrict__ hw) {
  __shared__ double a[KSP_MAXK], b[KSP_MAXK], b2[KSP_MAXK], dp[KSP_MAXK], dm[KSP_MAXK], z[KSP_MAXK];
  const int lane = threadIdx.x, k = j + 1;
  const double aj = sm[L.aj()], bj = sqrt(sm[L.wn2()]);
  const double bprev = j > 0 ? sm[L.beta() + j - 1] : 0.0;
  double amax = -INFINITY, gl = INFINITY, gu = -INFINITY, bmax = 0.0, asq = 0.0;
  for (int i = lane; i < k; i += 64) {
    const double ai = i < j ? sm[L.alpha() + i] : aj;
    const double bi = i < j ? sm[L.beta() + i] : 0.0;  // (beta[j] couples to row k, not part of T_k)
    const double bl = i > 0 ? fabs(sm[L.beta() + i - 1]) : 0.0;
    a[i] = ai;
    b[i] = bi;
    b2[i] = bi * bi;
    amax = fmax(amax, fabs(ai));
    bmax = fmax(bmax, bi * bi);
    gl = fmin(gl, ai - bl - fabs(bi));
    gu = fmax(gu, ai + bl + fabs(bi));
    if (i < j) {
      double t = sm[L.h1() + i];
      if (i == j - 1) t -= bprev;
      asq = fma(t, t, asq);
    }
  }
  asq = eig_wave_allsum(asq);
  gl = eig_wave_min(gl);
  gu = eig_wave_max(gu);
  bmax = eig_wave_max(bmax);
  amax = eig_wave_max(amax);
  __syncthreads();
  const double pivmin = 2.2250738585072014e-308 * fmax(1.0, bmax);
  const double tnorm = fmax(fabs(gl), fabs(gu));
  const bool finite = isfinite(tnorm) && isfinite(bj) && isfinite(asq);
  double theta = a[0];
  if (k > 1 && finite) {
    const double eps = 2.220446049250313e-16;
    double lo = gl - (2.0 * eps * tnorm * k + 2.0 * pivmin), hi = gu + (2.0 * eps * tnorm * k + 2.0 * pivmin);
    for (int it = 0; it < 64; it++) {
      const double wd = hi - lo;
      if (!(wd > 2.0 * eps * fmax(fabs(lo), fabs(hi)) + 2.0 * pivmin)) break;
      const double x = lo + wd * ((lane + 1) * (1.0 / 65.0));
      double d = a[0] - x;
      int cnt = d < 0.0;
      for (int i = 1; i < k; i++) {
        if (fabs(d) < pivmin) d = -pivmin;
        d = (a[i] - x) - b2[i - 1] / d;
        cnt += d < 0.0;
      }
      const unsigned long long full = __ballot(cnt == k);  // x above every eigenvalue
      const int f = full ? __ffsll((long long)full) - 1 : 64;
      const double xl = __shfl(x, f > 0 ? f - 1 : 0), xh = __shfl(x, f < 64 ? f : 63);
      const double nlo = f > 0 ? xl : lo, nhi = f < 64 ? xh : hi;
      if (!(nhi - nlo < wd)) break;  // (rounding: the points no longer separate)
      lo = nlo;
      hi = nhi;
    }
    theta = 0.5 * (lo + hi);
  }
  // the eigenvector of theta
  if (lane < 2 && finite) {
    const bool up = lane == 1;
    double d = a[up ? k - 1 : 0] - theta;
    (up ? dm : dp)[up ? k - 1 : 0] = d;
    for (int i = 0; i + 1 < k; i++) {
      if (fabs(d) < pivmin) d = -pivmin;
      const int r = up ? k - 2 - i : i + 1, c = up ? k - 2 - i : i;
      d = (a[r] - theta) - b2[c] / d;
      (up ? dm : dp)[r] = d;
    }
  }
  __syncthreads();
  double gbest = INFINITY;
  int rbest = 0;
  if (finite)
    for (int i = lane; i < k; i += 64) {
      const double g = fabs(dp[i] + dm[i] - (a[i] - theta));
      if (g < gbest) gbest = g, rbest = i;
    }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double g2 = __shfl_xor(gbest, off);
    const int r2 = __shfl_xor(rbest, off);
    if (g2 < gbest || (g2 == gbest && r2 < rbest)) gbest = g2, rbest = r2;
  }
  if (lane == 0) z[rbest] = 1.0;
  __syncthreads();
  if (finite && lane == 0) {
    double v = 1.0;
    for (int i = rbest - 1; i >= 0; i--) {
      const double d = fabs(dp[i]) < pivmin ? -pivmin : dp[i];
      v = -(b[i] / d) * v;
      z[i] = v;
    }
  } else if (finite && lane == 1) {
    double v = 1.0;
    for (int i = rbest; i + 1 < k; i++) {
      const double d = fabs(dm[i + 1]) < pivmin ? -pivmin : dm[i + 1];
      v = -(b[i] / d) * v;
      z[i + 1] = v;
    }
  }
  __syncthreads();
  double zz = 0.0;
  if (finite)
    for (int i = lane; i < k; i += 64) zz = fma(z[i], z[i], zz);
  zz = eig_wave_allsum(zz);
  const double zs = zz > 0.0 ? 1.0 / sqrt(zz) : 0.0;
  if (finite)
    for (int i = lane; i < k; i += 64) sm[L.s() + i] = zs * z[i];
  if (lane == 0) {
    const double slast = finite ? zs * z[k - 1] : 0.0;
    const double est = bj * fabs(slast);
    double as = j > 0 ? sm[L.asym()] : 0.0;
    if (j > 0) as = fmax(as, sqrt(asq) / fabs(theta));
    sm[L.alpha() + j] = aj;
    sm[L.beta() + j] = bj;
    sm[L.theta()] = theta;
    sm[L.asym()] = as;
    hw->theta = theta;
    hw->est = est;
    hw->asym = as;
    hw->flags = (finite && isfinite(theta) && isfinite(est) && isfinite(as) && isfinite(amax)) ? 0 : EIG_FLAG_NONFINITE;
  }
}

// y = Q s over the first k basis vectors (the Ritz vector, unit norm), KSP tiling
__global__ __launch_bounds__(KSP_NT) void k_eig_ritzvec(int n, const double* __restrict__ Q, size_t ld, int k,
                                                        const double* __restrict__ s, double* __restrict__ y) {
  const int base = blockIdx.x * KSP_TILE + threadIdx.x;
  double acc[KSP_EPT];
#pragma unroll
  for (int e = 0; e < KSP_EPT; e++) acc[e] = 0.0;
  for (int c = 0; c < k; c++) {
    const double sc = s[c];
    const double* __restrict__ v = Q + (size_t)c * ld;
#pragma unroll
    for (int e = 0; e < KSP_EPT; e++) {
      const int i = base + e * KSP_NT;
      if (i < n) acc[e] = fma(sc, v[i], acc[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < KSP_EPT; e++) {
    const int i = base + e * KSP_NT;
    if (i < n) y[i] = acc[e];
  }
}

// the partial sums of ||t - theta y||^2 (t = A y) and, with mode != NULL, mode = ps y (= S y, exactly 0 on the fixed dofs)
__global__ __launch_bounds__(KSP_NT) void k_eig_resid(int n, const double* __restrict__ t, const double* __restrict__ y,
                                                      const double* __restrict__ theta, const double* __restrict__ ps,
                                                      double* __restrict__ mode, double* __restrict__ partials) {
  __shared__ double red4[KSP_NT / 64];
  const int base = blockIdx.x * KSP_TILE + threadIdx.x;
  const double th = *theta;
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < KSP_EPT; e++) {
    const int i = base + e * KSP_NT;
    if (i < n) {
      const double yi = y[i], r = fma(-th, yi, t[i]);
      s = fma(r, r, s);
      if (mode) {
        const double p = ps[i];
        mode[i] = p != 0.0 ? p * yi : 0.0;
      }
    }
  }
  s = ksp_block_sum(s, red4);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}
