// Assembled tangent in block CSR, every block or the upper blocks only (nlps_gpu_tangent_bsr_pattern /
// nlps_gpu_tangent_bsr): the matrix of nlps_tangent_csr.hpp with one column index and d^2 contiguous doubles per node
// pair -- what MatCreateSeqBAIJWithArrays / MatCreateSeqSBAIJWithArrays take.
//
// The records per particle, the runs and the visited-offset masks are those of nlps_tangent_csr.hpp (k_tancsr_setup,
// k_tancsr_runs, k_tancsr_pattern), built once per linearisation whichever form asks first.  Every kept block is summed
// by tancsr_walk, the function k_tancsr_rows calls, so its d^2 values are the bits of the CSR entries.  This file holds
// what the block forms add to it: the count of the upper blocks, the store of a block, and the kernel.
//
// Upper form, HALF = true (masked numbers that ascend with the grid order: the default numbering).  B >= A is then the
// lexicographic order of the offset B - A.  Inside the run of C, with A the member sA of C's stencil, the kept members
// are the codes sA .. 5^d - 1: a dense range.  They are dealt to the lanes from 0, and a run with few of them uses
// narrower worker groups and fewer waves (the waves without a member skip the run's passes).  The owners hold the
// accumulators of the offsets >= 0 only: 365 of 729 (41 of 81), two per thread instead of three (BsrCfg).  The order
// of a sum belongs to the block, not to the lane: dealing members and offsets to other lanes changes no sum.
// Under a caller's numbering "upper" follows the masked numbers, not the offsets: HALF = false walks every member like
// the full form and keeps, ranked by masked number, the blocks with B >= A (`upper` != 0).
#pragma once

// the upper form: blocks B >= A of every masked node's block row, and whether "B >= A" is the order of the offsets on
// every row (*mixed stays 0)
template <int ND>
__global__ __launch_bounds__(256) void k_tanbsr_count(GridD g, const u64* __restrict__ mask, const int* __restrict__ n2m,
                                                       int* __restrict__ cntb, int* __restrict__ mixed) {
  constexpr int S = CsrCfg<ND>::S, MW = CsrCfg<ND>::MW, SC = BsrCfg<ND>::SC;
  const int lane = threadIdx.x & 63;
  const int A = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (A >= g.nnodes) return;  // (whole waves)
  const int mA = n2m[A];
  if (mA < 0) return;
  int cnt = 0, odd = 0;
#pragma unroll
  for (int t = 0; t < MW; t++) {
    const u64 word = mask[(size_t)A * MW + t];
    const int s = 64 * t + lane;
    bool keep = s < S && ((word >> lane) & 1ull) != 0ull;
    if (keep) {
      // (a visited offset is a node pair of one particle's list: B is a node of the grid)
      const int mB = n2m[A + (s % 9 - 4) + g.n[0] * (((s / 9) % 9 - 4) + g.n[1] * (ND == 3 ? s / 81 - 4 : 0))];
      keep = mB >= mA;
      odd |= keep != (s >= SC);
    }
    cnt += (int)__popcll(__ballot(keep));
  }
  if (__any(odd) && lane == 0) atomicOr(mixed, 1);
  if (lane == 0) cntb[mA] = cnt;
}

// one column index and d^2 contiguous values per block, row-major or (col_major) transposed
template <int ND>
struct EmitBsr {
  int col_major;
  int* __restrict__ bcols;
  double* __restrict__ vals;
  __device__ __forceinline__ void operator()(size_t base, int, int pos, int mB, const double (&o)[ND * ND]) const {
    constexpr int E = ND * ND;
    const size_t at = base + (size_t)pos;
    bcols[at] = mB;
    // (the layout picks the value, not the address: the d^2 stores stay at fixed offsets and merge into wide ones)
#pragma unroll
    for (int c = 0; c < E; c++) vals[at * E + c] = col_major ? o[(c % ND) * ND + c / ND] : o[c];
  }
};

// the block row of row node A, one workgroup per row node
// (the upper form in 3-D holds 18 accumulators instead of 27: asked to fit 4 waves per SIMD, which it does without scratch;
// 0 = no request for the other instances, which then compile like k_tancsr_rows)
template <int ND, bool HALF>
__global__ __launch_bounds__(CsrCfg<ND>::NT, (HALF && ND == 3) ? 4 : 0) void k_tanbsr_rows(
    GridD g, const int* __restrict__ run, const double* __restrict__ Ep, const double* __restrict__ Fp,
    const u64* __restrict__ Mk, const u64* __restrict__ mask, const int* __restrict__ n2m, const int* __restrict__ d2m,
    const double* __restrict__ aM, const int* __restrict__ cntb, const int* __restrict__ offb, int upper, int col_major,
    int* __restrict__ bcols, double* __restrict__ vals) {
  tancsr_walk<ND, HALF>(g, run, Ep, Fp, Mk, mask, n2m, d2m, aM, cntb, offb, upper, EmitBsr<ND>{col_major, bcols, vals});
}
