// Device GMRES(m) on the matrix-free tangent (nlps_gpu_tangent_solve): the Krylov loop of the implicit driver's KSP
// around y = K x of nlps_tangent_operator.hpp.  Right preconditioning, K M^-1 u = b, x = M^-1 u, so the residual of the
// Arnoldi recurrence is the true residual b - K x.
//
// Vectors are the masked [N_A d] arrays of the operator.  The streaming kernels give every thread KSP_EPT elements at a
// stride of KSP_NT (a block covers KSP_TILE consecutive elements) and leave one partial sum per block and column,
// partials[col][block]; k_ksp_finish adds a column's partials in a fixed order.  No float atomics: a solve adds no
// run-to-run noise of its own (the product's f64 atomics still do).  Sums inside a block: per-wave shuffle, then the
// waves' sums from LDS in wave order.
//
// The small state of a cycle lives in one device array of doubles (KspSmall offsets): the Hessenberg column of the
// step in two Gram-Schmidt passes, the Givens rotations, the rotated right-hand side g, the R factor (column-major,
// R[c][i] at c * (m + 1) + i) and y.  k_ksp_arnoldi (one wave) turns the column into the next R column and leaves the
// residual estimate |g[j+1]| and the step's flags in the host-visible word KspHost.
#pragma once

static constexpr int KSP_NT = 256;                     // threads of the streaming kernels (4 waves)
static constexpr int KSP_EPT = 2;                      // elements per thread (873 blocks at 1 M particles: 3.4 per CU)
static constexpr int KSP_TILE = KSP_NT * KSP_EPT;      // elements per block
static constexpr int KSP_MAXK = 256;                   // largest restart (LDS of the multi-dot: (KSP_MAXK + 2) x 4 doubles)
static constexpr double KSP_PIVOT = 1e-14;             // a PC block or diagonal does not invert: |pivot| <= 1e-14 ||block||_F
static constexpr double KSP_HAPPY = 1e-14;             // happy breakdown: ||w|| after Gram-Schmidt <= 1e-14 ||K M^-1 v_j||

enum { KSP_FLAG_NONFINITE = 1, KSP_FLAG_HAPPY = 2, KSP_FLAG_SINGULAR = 4 };

// what the host reads after a step (a pinned word the kernels write through its device alias)
struct KspHost {
  double est;    // |g[j+1]|: the residual estimate after the step
  double bn2;    // ||b||^2
  double rn2;    // ||b - K x||^2 (the true residual)
  int flags;     // KSP_FLAG_*
  int pad;
};

// offsets into the small device array of a restart m
struct KspSmall {
  int m;
  __host__ __device__ int h1() const { return 0; }                  // [m + 2] pass 1: V^T w, then w.w at [j + 1]
  __host__ __device__ int h2() const { return (m + 2); }            // [m + 2] pass 2 (DGKS refinement)
  __host__ __device__ int cs() const { return 2 * (m + 2); }        // [m + 2]
  __host__ __device__ int sn() const { return 3 * (m + 2); }        // [m + 2]
  __host__ __device__ int g() const { return 4 * (m + 2); }         // [m + 2]
  __host__ __device__ int y() const { return 5 * (m + 2); }         // [m + 2]
  __host__ __device__ int wn2() const { return 6 * (m + 2); }       // ||w||^2 after the latest multi-axpy
  __host__ __device__ int refine() const { return 6 * (m + 2) + 1; }  // 1.0: the second pass runs
  __host__ __device__ int hnorm() const { return 6 * (m + 2) + 2; }   // H[j+1][j] of the last step
  __host__ __device__ int R() const { return 6 * (m + 2) + 8; }     // [m][m + 1]
  __host__ __device__ size_t size() const { return (size_t)6 * (m + 2) + 8 + (size_t)m * (m + 1); }
};

__device__ __forceinline__ double ksp_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  return v;  // (lane 0 holds the sum)
}

// the block's sum of v (every thread passes one value), in a fixed order; valid in thread 0
__device__ __forceinline__ double ksp_block_sum(double v, double* red4) {
  v = ksp_wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red4[wave] = v;
  __syncthreads();
  return red4[0] + red4[1] + red4[2] + red4[3];
}

// h[c] = V[c] . w for c < ncol and, with ww, h[ncol] = w . w (the DGKS reference norm): w is read once into registers,
// every basis vector once.  skip: a device word; 0.0 there makes the launch a no-op (the second pass when DGKS says no).
__global__ __launch_bounds__(KSP_NT) void k_ksp_mdot(int n, const double* __restrict__ V, size_t ld, int ncol, int ww,
                                                     const double* __restrict__ w, double* __restrict__ partials, int nb,
                                                     const double* __restrict__ skip) {
  if (skip && *skip == 0.0) return;
  __shared__ double red[KSP_MAXK + 2][KSP_NT / 64];
  const int base = blockIdx.x * KSP_TILE + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double wr[KSP_EPT];
#pragma unroll
  for (int e = 0; e < KSP_EPT; e++) {
    const int i = base + e * KSP_NT;
    wr[e] = i < n ? w[i] : 0.0;
  }
  const int ntot = ncol + (ww ? 1 : 0);
  for (int c = 0; c < ntot; c++) {
    double s = 0.0;
    if (c < ncol) {
      const double* __restrict__ v = V + (size_t)c * ld;
#pragma unroll
      for (int e = 0; e < KSP_EPT; e++) {
        const int i = base + e * KSP_NT;
        s = fma(i < n ? v[i] : 0.0, wr[e], s);
      }
    } else {
#pragma unroll
      for (int e = 0; e < KSP_EPT; e++) s = fma(wr[e], wr[e], s);
    }
    s = ksp_wave_sum(s);
    if (lane == 0) red[c][wave] = s;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < ntot; c += KSP_NT)
    partials[(size_t)c * nb + blockIdx.x] = ((red[c][0] + red[c][1]) + red[c][2]) + red[c][3];
}

// w -= sum_c h[c] V[c] (c < ncol), fused with the partial sums of ||w||^2 (column 0 of partials)
__global__ __launch_bounds__(KSP_NT) void k_ksp_maxpy(int n, const double* __restrict__ V, size_t ld, int ncol,
                                                      const double* __restrict__ hc, double* __restrict__ w,
                                                      double* __restrict__ partials, const double* __restrict__ skip) {
  if (skip && *skip == 0.0) return;
  __shared__ double red4[KSP_NT / 64];
  const int base = blockIdx.x * KSP_TILE + threadIdx.x;
  double wr[KSP_EPT];
#pragma unroll
  for (int e = 0; e < KSP_EPT; e++) {
    const int i = base + e * KSP_NT;
    wr[e] = i < n ? w[i] : 0.0;
  }
#pragma unroll 4
  for (int c = 0; c < ncol; c++) {
    const double a = hc[c];
    const double* __restrict__ v = V + (size_t)c * ld;
#pragma unroll
    for (int e = 0; e < KSP_EPT; e++) {
      const int i = base + e * KSP_NT;
      if (i < n) wr[e] = fma(-a, v[i], wr[e]);
    }
  }
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < KSP_EPT; e++) {
    const int i = base + e * KSP_NT;
    if (i < n) w[i] = wr[e];
    s = fma(wr[e], wr[e], s);
  }
  s = ksp_block_sum(s, red4);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// r = b - y (y may be NULL: r = b; r may be NULL: only the norm), with the partial sums of ||r||^2
__global__ __launch_bounds__(KSP_NT) void k_ksp_resid(int n, const double* __restrict__ b, const double* __restrict__ y,
                                                      double* __restrict__ r, double* __restrict__ partials) {
  __shared__ double red4[KSP_NT / 64];
  const int base = blockIdx.x * KSP_TILE + threadIdx.x;
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < KSP_EPT; e++) {
    const int i = base + e * KSP_NT;
    if (i < n) {
      const double v = y ? b[i] - y[i] : b[i];
      if (r) r[i] = v;
      s = fma(v, v, s);
    }
  }
  s = ksp_block_sum(s, red4);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// one block per column: out[c] = the sum of partials[c][0..nb) in a fixed order (and host[c] when host != NULL).
// refine != NULL (column 0, the norm after the first multi-axpy of a step): also sets the refine word, 1.0 when
// ||w||^2 < ||w_before||^2 / 2 (the norm ratio below 1/sqrt 2: DGKS), else 0.0; a step refines at most once.
__global__ __launch_bounds__(KSP_NT) void k_ksp_finish(const double* __restrict__ partials, int nb, double* __restrict__ out,
                                                       double* __restrict__ host, const double* __restrict__ skip,
                                                       double* __restrict__ refine, const double* __restrict__ before) {
  if (skip && *skip == 0.0) return;
  __shared__ double red4[KSP_NT / 64];
  const int c = blockIdx.x;
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += KSP_NT) s += partials[(size_t)c * nb + i];
  s = ksp_block_sum(s, red4);
  if (threadIdx.x == 0) {
    if (out) out[c] = s;
    if (host) host[c] = s;
    if (refine) *refine = (before && s < 0.5 * *before) ? 1.0 : 0.0;
  }
}

// v_dst = a v_src, a = 1 / sqrt(*n2) when n2 is a device word (no-op unless that norm is positive and finite), else a
__global__ __launch_bounds__(KSP_NT) void k_ksp_scale(int n, const double* __restrict__ src, double* __restrict__ dst,
                                                      double a, const double* __restrict__ n2) {
  if (n2) {
    const double v = *n2;
    if (!(v > 0.0) || !isfinite(v)) return;
    a = 1.0 / sqrt(v);
  }
  const int base = blockIdx.x * KSP_TILE + threadIdx.x;
#pragma unroll
  for (int e = 0; e < KSP_EPT; e++) {
    const int i = base + e * KSP_NT;
    if (i < n) dst[i] = a * src[i];
  }
}

// One Arnoldi step's small work, one wave, lane 0: the column H[0..j+1][j] = h1 (+ h2 after a refinement), sqrt(wn2);
// the previous rotations on it, the new rotation, g; R column j; the estimate |g[j+1]| and the flags into the host word.
// j == 0 starts the cycle: g = (beta, 0, ...).
__global__ __launch_bounds__(64) void k_ksp_arnoldi(KspSmall L, double* __restrict__ s, int j, double beta,
                                                    KspHost* __restrict__ hw) {
  __shared__ double col[KSP_MAXK + 2];
  if (threadIdx.x != 0) return;
  double* __restrict__ cs = s + L.cs();
  double* __restrict__ sn = s + L.sn();
  double* __restrict__ g = s + L.g();
  const double* __restrict__ h1 = s + L.h1();
  const double* __restrict__ h2 = s + L.h2();
  const bool ref = s[L.refine()] != 0.0;
  if (j == 0) {
    g[0] = beta;
    g[1] = 0.0;
  }
  for (int i = 0; i <= j; i++) col[i] = ref ? h1[i] + h2[i] : h1[i];
  const double hn = sqrt(s[L.wn2()]);
  for (int i = 0; i < j; i++) {
    const double a = col[i], b = col[i + 1];
    col[i] = cs[i] * a + sn[i] * b;
    col[i + 1] = -sn[i] * a + cs[i] * b;
  }
  const double a = col[j];
  const double r = sqrt(a * a + hn * hn);
  int flags = 0;
  double c = 1.0, sg = 0.0;
  if (r > 0.0) {
    c = a / r;
    sg = hn / r;
  } else {
    flags |= KSP_FLAG_SINGULAR;
  }
  cs[j] = c;
  sn[j] = sg;
  const double gj = g[j];
  g[j] = c * gj;
  g[j + 1] = -sg * gj;
  double* __restrict__ R = s + L.R() + (size_t)j * (L.m + 1);
  bool finite = isfinite(r) && isfinite(hn) && isfinite(gj);
  for (int i = 0; i < j; i++) {
    R[i] = col[i];
    finite = finite && isfinite(col[i]);
  }
  R[j] = r;
  if (!finite) flags |= KSP_FLAG_NONFINITE;
  if (hn <= KSP_HAPPY * sqrt(h1[j + 1])) flags |= KSP_FLAG_HAPPY;
  s[L.hnorm()] = hn;
  hw->est = fabs(g[j + 1]);
  hw->flags = flags;
}

// y = R^-1 g over the first k columns (back substitution, one lane)
__global__ __launch_bounds__(64) void k_ksp_hsolve(KspSmall L, double* __restrict__ s, int k) {
  __shared__ double ys[KSP_MAXK];
  if (threadIdx.x != 0) return;
  const double* __restrict__ R = s + L.R();
  const double* __restrict__ g = s + L.g();
  const size_t ldr = (size_t)L.m + 1;
  for (int i = k - 1; i >= 0; i--) {
    double acc = g[i];
    for (int c = i + 1; c < k; c++) acc = fma(-R[c * ldr + i], ys[c], acc);
    ys[i] = acc / R[i * ldr + i];
  }
  double* __restrict__ y = s + L.y();
  for (int i = 0; i < k; i++) y[i] = ys[i];
}

// M^-1 applied to the d values of one masked node: kind 1 (JACOBI) the reciprocal diagonal kept on the block's
// diagonal, kind 2 (PBJACOBI) the inverted block, row-major d x d per node
template <int ND>
__device__ __forceinline__ void ksp_pc_node(int kind, const double* __restrict__ Minv, int m, const double* v, double* z) {
  constexpr int E = ND * ND;
  if (kind == 2) {
#pragma unroll
    for (int i = 0; i < ND; i++) {
      double a = 0.0;
#pragma unroll
      for (int j = 0; j < ND; j++) a = fma(Minv[(size_t)m * E + i * ND + j], v[j], a);
      z[i] = a;
    }
  } else if (kind == 1) {
#pragma unroll
    for (int i = 0; i < ND; i++) z[i] = Minv[(size_t)m * E + i * ND + i] * v[i];
  } else {
#pragma unroll
    for (int i = 0; i < ND; i++) z[i] = v[i];
  }
}

// The product's input with the preconditioner folded in: z = M^-1 v on the masked node, then what k_tanop_expand
// writes (xg = z in grid numbering, 0 on fixed dofs and inactive nodes) and the zeroed accumulator yg of the apply.
// kind 0: no preconditioner, z is not written (the nodal epilogue reads v).
template <int ND>
__global__ void k_ksp_pc_expand(int nnodes, const int* __restrict__ n2m, const int* __restrict__ d2m, int kind,
                                const double* __restrict__ Minv, const double* __restrict__ v, double* __restrict__ z,
                                double* __restrict__ xg, double* __restrict__ yg) {
  const int A = blockIdx.x * blockDim.x + threadIdx.x;
  if (A >= nnodes) return;
  const int m = n2m[A];
  double vv[ND], zz[ND];
#pragma unroll
  for (int f = 0; f < ND; f++) vv[f] = m >= 0 ? v[(size_t)m * ND + f] : 0.0;
  ksp_pc_node<ND>(kind, Minv, m >= 0 ? m : 0, vv, zz);
#pragma unroll
  for (int f = 0; f < ND; f++) {
    const size_t i = (size_t)m * ND + f;
    if (m >= 0 && kind) z[i] = zz[f];
    xg[(size_t)A * ND + f] = (m >= 0 && !(d2m && d2m[i] == -1)) ? zz[f] : 0.0;
    yg[(size_t)A * ND + f] = 0.0;
  }
}

// x += M^-1 (V y) over the first k basis vectors, one thread per masked node
template <int ND>
__global__ void k_ksp_update(int nA, int kind, const double* __restrict__ Minv, const double* __restrict__ V, size_t ld,
                             int k, const double* __restrict__ y, double* __restrict__ x) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= nA) return;
  double u[ND], z[ND];
#pragma unroll
  for (int f = 0; f < ND; f++) u[f] = 0.0;
  for (int c = 0; c < k; c++) {
    const double yc = y[c];
#pragma unroll
    for (int f = 0; f < ND; f++) u[f] = fma(yc, V[(size_t)c * ld + (size_t)m * ND + f], u[f]);
  }
  ksp_pc_node<ND>(kind, Minv, m, u, z);
#pragma unroll
  for (int f = 0; f < ND; f++) x[(size_t)m * ND + f] += z[f];
}

// The preconditioner from the masked diagonal blocks (k_tanop_bdiag + k_tanop_bdiag_nodal), in place.  kind 2: every
// block inverted (Gauss-Jordan, partial pivoting with the row swaps as selects: no indexed registers, no scratch);
// kind 1: the diagonal entries replaced by their reciprocals.  A pivot (kind 2) or a diagonal entry (kind 1) at or
// below KSP_PIVOT ||block||_F leaves the block as it is and lowers *bad to the masked node index.
template <int ND>
__global__ void k_ksp_pc_build(int nA, int kind, double* __restrict__ B, int* __restrict__ bad) {
  constexpr int E = ND * ND;
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= nA) return;
  double a[E], inv[E];
  double nrm = 0.0;
#pragma unroll
  for (int q = 0; q < E; q++) {
    a[q] = B[(size_t)m * E + q];
    nrm = fma(a[q], a[q], nrm);
  }
  const double tol = KSP_PIVOT * sqrt(nrm);
  if (kind == 1) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < ND; i++) ok = ok && fabs(a[i * ND + i]) > tol;
    if (!ok) {
      atomicMin(bad, m);
      return;
    }
#pragma unroll
    for (int i = 0; i < ND; i++) B[(size_t)m * E + i * ND + i] = 1.0 / a[i * ND + i];
    return;
  }
#pragma unroll
  for (int q = 0; q < E; q++) inv[q] = (q % (ND + 1) == 0) ? 1.0 : 0.0;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < ND; c++) {
    double best = fabs(a[c * ND + c]);
    int p = c;
#pragma unroll
    for (int r = c + 1; r < ND; r++)
      if (fabs(a[r * ND + c]) > best) {
        best = fabs(a[r * ND + c]);
        p = r;
      }
    ok = ok && best > tol;
#pragma unroll
    for (int r = c + 1; r < ND; r++) {
      const bool sw = p == r;
#pragma unroll
      for (int q = 0; q < ND; q++) {
        const double t = a[c * ND + q], u = a[r * ND + q];
        a[c * ND + q] = sw ? u : t;
        a[r * ND + q] = sw ? t : u;
        const double ti = inv[c * ND + q], ui = inv[r * ND + q];
        inv[c * ND + q] = sw ? ui : ti;
        inv[r * ND + q] = sw ? ti : ui;
      }
    }
    const double piv = ok ? 1.0 / a[c * ND + c] : 0.0;
#pragma unroll
    for (int q = 0; q < ND; q++) {
      a[c * ND + q] *= piv;
      inv[c * ND + q] *= piv;
    }
#pragma unroll
    for (int r = 0; r < ND; r++) {
      if (r == c) continue;
      const double f = a[r * ND + c];
#pragma unroll
      for (int q = 0; q < ND; q++) {
        a[r * ND + q] = fma(-f, a[c * ND + q], a[r * ND + q]);
        inv[r * ND + q] = fma(-f, inv[c * ND + q], inv[r * ND + q]);
      }
    }
  }
  if (!ok) {
    atomicMin(bad, m);
    return;
  }
#pragma unroll
  for (int q = 0; q < E; q++) B[(size_t)m * E + q] = inv[q];
}
