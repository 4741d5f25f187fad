// Device side of the Newton solve (nlps_gpu_newton_solve): the vector work SNES NEWTONLS and its bt line search do
// between a residual evaluation, a linearisation and a linear solve.  Streaming kernels in the shape of nlps_krylov.hpp
// (KSP_NT threads, KSP_EPT elements each at a stride of KSP_NT, one partial per block and column, partials[col][block]);
// k_snes_finish combines a column's partials in a fixed order and leaves the scalar in the host-visible word.  No float
// atomics: the solve adds no summation noise of its own.  The host takes every scalar decision (accept, next lambda,
// stopping tests) from that word after the one synchronisation that ends a residual evaluation.
#pragma once

// the scalars the host reads (a pinned array of doubles the kernels write through its device alias)
enum {
  SNES_H_FF = 0,     // F . F of the latest residual
  SNES_H_FT = 1,     // F . (K Y): the initial slope of the bt line search
  SNES_H_WW = 2,     // W . W of the latest trial point
  SNES_H_YY = 3,     // Y . Y
  SNES_H_RATIO = 4,  // max_i |y_i| / max(|x_i|, 1)
  SNES_H_N = 5
};

// the block's sum of a and b and the maximum of c (every thread passes one value each), fixed order; valid in thread 0
__device__ __forceinline__ void snes_block_reduce(double& a, double& b, double& c, double (*red)[KSP_NT / 64]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off);
    b += __shfl_down(b, off);
    c = fmax(c, __shfl_down(c, off));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wave] = a;
    red[1][wave] = b;
    red[2][wave] = c;
  }
  __syncthreads();
  a = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
  b = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  c = fmax(fmax(red[2][0], red[2][1]), fmax(red[2][2], red[2][3]));
}

// The trial point W = X - lambda Y, fused with the partial sums of W . W (column 0) and Y . Y (column 1) and the block
// maxima of |y_i| / max(|x_i|, 1) (column 2: what bounds the smallest step of the line search)
__global__ __launch_bounds__(KSP_NT) void k_snes_trial(int n, const double* __restrict__ X, const double* __restrict__ Y,
                                                       double lambda, double* __restrict__ W, double* __restrict__ partials,
                                                       int nb) {
  __shared__ double red[3][KSP_NT / 64];
  const int base = blockIdx.x * KSP_TILE + threadIdx.x;
  double ww = 0.0, yy = 0.0, ratio = 0.0;
#pragma unroll
  for (int e = 0; e < KSP_EPT; e++) {
    const int i = base + e * KSP_NT;
    if (i < n) {
      const double x = X[i], y = Y[i];
      const double w = x - lambda * y;
      W[i] = w;
      ww = fma(w, w, ww);
      yy = fma(y, y, yy);
      ratio = fmax(ratio, fabs(y) / fmax(fabs(x), 1.0));
    }
  }
  snes_block_reduce(ww, yy, ratio, red);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = ww;
    partials[(size_t)nb + blockIdx.x] = yy;
    partials[(size_t)2 * nb + blockIdx.x] = ratio;
  }
}

// F . F (column 0) and, with T != NULL, F . T (column 1) in one pass over F
__global__ __launch_bounds__(KSP_NT) void k_snes_dots(int n, const double* __restrict__ F, const double* __restrict__ T,
                                                      double* __restrict__ partials, int nb) {
  __shared__ double red[3][KSP_NT / 64];
  const int base = blockIdx.x * KSP_TILE + threadIdx.x;
  double ff = 0.0, ft = 0.0, unused = 0.0;
#pragma unroll
  for (int e = 0; e < KSP_EPT; e++) {
    const int i = base + e * KSP_NT;
    if (i < n) {
      const double f = F[i];
      ff = fma(f, f, ff);
      if (T) ft = fma(f, T[i], ft);
    }
  }
  snes_block_reduce(ff, ft, unused, red);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = ff;
    if (T) partials[(size_t)nb + blockIdx.x] = ft;
  }
}

// one block per column: host[c] = the sum (c == maxcol: the maximum) of partials[c][0..nb) in a fixed order
__global__ __launch_bounds__(KSP_NT) void k_snes_finish(const double* __restrict__ partials, int nb, int maxcol,
                                                        double* __restrict__ host) {
  __shared__ double red[3][KSP_NT / 64];
  const int c = blockIdx.x;
  double s = 0.0, unused = 0.0, m = 0.0;
  for (int i = threadIdx.x; i < nb; i += KSP_NT) {
    const double v = partials[(size_t)c * nb + i];
    s += v;
    m = fmax(m, v);
  }
  snes_block_reduce(s, unused, m, red);
  if (threadIdx.x == 0) host[c] = c == maxcol ? m : s;
}
