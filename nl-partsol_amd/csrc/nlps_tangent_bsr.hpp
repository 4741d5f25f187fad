// Assembled tangent in block CSR, every block or the upper blocks only (nlps_gpu_tangent_bsr_pattern /
// nlps_gpu_tangent_bsr): the matrix of nlps_tangent_csr.hpp with one column index and d^2 contiguous doubles per node
// pair -- what MatCreateSeqBAIJWithArrays / MatCreateSeqSBAIJWithArrays take.
//
// The records per particle, the runs and the visited-offset masks are those of nlps_tangent_csr.hpp (k_tancsr_setup,
// k_tancsr_runs, k_tancsr_pattern), built once per linearisation whichever form asks first.  Every kept block is the sum
// k_tancsr_rows forms for it, in the same order -- closest nodes C around the row node A in grid order, the particles of
// a run by ascending slot, one thread per (member, component) sum, the run's sums added to the owner's accumulator with
// one plain add per run -- so its d^2 values are the bits of the CSR entries.  The order belongs to the block, not to
// the lane: the upper form deals members and offsets to other lanes and changes no sum.
//
// Upper form, HALF = true (masked numbers that ascend with the grid order: the default numbering).  B >= A is then the
// lexicographic order of the offset B - A.  Inside the run of C, with A the member sA of C's stencil, the kept members
// are the codes sA .. 5^d - 1: a dense range.  They are dealt to the lanes from 0, and a run with few of them uses
// narrower worker groups and fewer waves (the waves without a member skip the run's passes).  The owners hold the
// accumulators of the offsets >= 0 only: 365 of 729 (41 of 81), two per thread instead of three.
// Under a caller's numbering "upper" follows the masked numbers, not the offsets: HALF = false walks every member like
// the full form and keeps, ranked by masked number, the blocks with B >= A (`upper` != 0).
#pragma once

template <int ND>
struct BsrCfg {
  using C = CsrCfg<ND>;
  static constexpr int SC = (C::S - 1) / 2;                  // the centre offset: 40 / 364
  static constexpr int SH = C::S - SC;                       // offsets >= 0: 41 / 365
  static constexpr int OPTH = (SH + C::NT - 1) / C::NT;      // offsets an owner holds in the upper form: 1 / 2
  // worker groups of a run with few kept members: 4 groups of 16 lanes (one wave) / 3 groups of 64 lanes (three waves)
  static constexpr int GSS = (ND == 3) ? 64 : 16;
  static constexpr int NGS = (ND == 3) ? 3 : 4;
  static constexpr int LGS = (ND == 3) ? 6 : 4;              // log2 GSS, and of CsrCfg::GS
  static constexpr int LG = (ND == 3) ? 7 : 5;
  static_assert((1 << LGS) == GSS && (1 << LG) == C::GS, "worker groups are powers of two");
};

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

// (the upper form in 3-D holds 18 accumulators instead of 27: asked to fit 4 waves per SIMD, which it does without scratch;
// 0 = no request for the other instances, which then compile like k_tancsr_rows)
template <int ND, bool HALF>
__global__ __launch_bounds__(CsrCfg<ND>::NT, (HALF && ND == 3) ? 4 : 0) void k_tanbsr_rows(GridD g, const int* __restrict__ run,
                                                                 const double* __restrict__ Ep, const double* __restrict__ Fp,
                                                                 const u64* __restrict__ Mk, const u64* __restrict__ mask,
                                                                 const int* __restrict__ n2m, const int* __restrict__ d2m,
                                                                 const double* __restrict__ aM, const int* __restrict__ cntb,
                                                                 const int* __restrict__ offb, int upper, int col_major,
                                                                 int* __restrict__ bcols, double* __restrict__ vals) {
  using Cfg = CsrCfg<ND>;
  using Bfg = BsrCfg<ND>;
  constexpr int S = Cfg::S, NT = Cfg::NT, MW = Cfg::MW, E = Cfg::E, E4 = Cfg::E4, NWV = Cfg::NWV, NF = Cfg::NF,
                NFX = Cfg::NFX, CH = Cfg::CH, MAXM = Cfg::MAXM, NPT = Cfg::NPT, NC = (ND == 3) ? 125 : 25,
                S0 = HALF ? Bfg::SC : 0, OPT = HALF ? Bfg::OPTH : Cfg::OPT;
  // (the staging of k_tancsr_rows: two buffers, one barrier per pass)
  __shared__ double sh_w[2][CH][NWV];     // w[b][ij] = N_A sum_a l_A[a] E[a][b][ij]
  __shared__ double sh_f[2][CH][2 * NF];  // factors (x, y, z), then l per axis and stencil index
  __shared__ u64 sh_m[2][CH][2];
  __shared__ int sh_p[2][CH];             // 1 = staged and holds A
  __shared__ int sh_run[NC][2];           // the runs of the closest nodes around A (empty where the grid ends)
  __shared__ double sh_part[MAXM][E];     // the blocks of one closest node's run, by member of its stencil
  __shared__ u64 sh_mask[MW];
  __shared__ int sh_pref[MW + 1];
  __shared__ int sh_key[S];               // masked node of the q-th listed offset
  const int A = blockIdx.x, t = threadIdx.x;
  const int mA = n2m[A];
  if (mA < 0) return;  // (uniform)
  const int cnt = cntb[mA];
  if (cnt == 0) return;
  const int Ai[3] = {A % g.n[0], (A / g.n[0]) % g.n[1], ND == 3 ? A / (g.n[0] * g.n[1]) : 0};
  // owner role: the column offsets S0 + t + k NT of this thread, each axis 0 .. 8 in one byte of dofp (a register each)
  int dofp[OPT];
  double acc[OPT][E];
#pragma unroll
  for (int k = 0; k < OPT; k++) {
    const int s = S0 + t + k * NT;
    dofp[k] = s % 9 | ((s / 9) % 9) << 8 | (ND == 3 ? s / 81 : 4) << 16;
#pragma unroll
    for (int ij = 0; ij < E; ij++) acc[k][ij] = 0.0;
  }
#define TANBSR_DOF(k, ax) ((int)((dofp[k] >> (8 * (ax))) & 0xff) - 4)
  int buf = 0;
  if (t < NC) {
    const int Cc[3] = {Ai[0] + t % 5 - 2, Ai[1] + (t / 5) % 5 - 2, ND == 3 ? Ai[2] + t / 25 - 2 : 0};
    const bool in = Cc[0] >= 0 && Cc[0] < g.n[0] && Cc[1] >= 0 && Cc[1] < g.n[1] && (ND == 2 || (Cc[2] >= 0 && Cc[2] < g.n[2]));
    const int C = Cc[0] + g.n[0] * (Cc[1] + g.n[1] * Cc[2]);
    sh_run[t][0] = in ? run[C] : 0;
    sh_run[t][1] = in ? run[C + 1] : 0;
  }
  __syncthreads();
#pragma unroll 1
  for (int ec = 0; ec < NC; ec++) {
    const int r0 = sh_run[ec][0], r1 = sh_run[ec][1];
    if (r0 >= r1) continue;
    const int e[3] = {ec % 5 - 2, (ec / 5) % 5 - 2, ND == 3 ? ec / 25 - 2 : 0};
    const int Cc[3] = {Ai[0] + e[0], Ai[1] + e[1], Ai[2] + e[2]};
    const int a[3] = {2 - e[0], 2 - e[1], ND == 3 ? 2 - e[2] : 0};  // stencil index of A around C
    const int sA = a[0] + 5 * a[1] + 25 * a[2];
    // worker role: member wm of the closest node's stencil, components ij = wg + n ng of its block.  The kept members
    // are first .. NC - 1; few of them take the narrow groups (uniform over the workgroup: sA is)
    const int first = HALF ? sA : 0;
    const bool narrow = HALF && NC - first <= Bfg::GSS;
    const int lg = narrow ? Bfg::LGS : Bfg::LG, ng = narrow ? Bfg::NGS : Cfg::NG;
    const int wg = t >> lg, wm = first + (t & ((1 << lg) - 1));
    const bool worker = wg < ng && wm < NC;
    const int wb[3] = {wm % 5, (wm / 5) % 5, ND == 3 ? (wm / 25) % 5 : 0};
    double part[NPT];
#pragma unroll
    for (int n = 0; n < NPT; n++) part[n] = 0.0;
#pragma unroll 1
    for (int c0 = r0; c0 < r1; c0 += CH) {
      // staging: every role reads what it needs from memory itself (no barrier between the roles)
      if (t < CH) {
        int on = 0;
        if (c0 + t < r1) {
          const u64 lo = Mk[2 * (size_t)(c0 + t)], hi = Mk[2 * (size_t)(c0 + t) + 1];
          on = tancsr_bit(lo, hi, sA) ? 1 : 0;
          sh_m[buf][t][0] = lo;
          sh_m[buf][t][1] = hi;
        }
        sh_p[buf][t] = on;
      }
      if (t < CH * NF) {
        const int q = t / NF, f = t - q * NF;
        if (c0 + q < r1) {
          const int ax = f / 5, i = f - 5 * ax;
          const double* fp = Fp + (size_t)(c0 + q) * NFX;
          sh_f[buf][q][f] = fp[f];
          // (Lme::geom: l = x_p - (origin + h * lattice index), evaluated like the host mesh builder does)
          sh_f[buf][q][NF + f] = fp[NF + ax] - (g.o[ax] + g.h * (double)(Cc[ax] + i - 2));
        }
      }
      {
        const int q = t >> 5, cw = t & 31;
        if (c0 + q < r1 && cw < NWV) {  // (also for a particle that does not hold A: nobody reads its w)
          const double* f = Fp + (size_t)(c0 + q) * NFX;
          double NA = f[a[0]] * f[5 + a[1]];
          if (ND == 3) NA *= f[(10 + a[2]) % NF];
          double lA[3];  // x_p - x_A
#pragma unroll
          for (int ax = 0; ax < ND; ax++) lA[ax] = f[NF + ax] - (g.o[ax] + g.h * (double)Ai[ax]);
          const double* ep = Ep + (size_t)(c0 + q) * E4 + cw;
          double w = lA[0] * ep[0];
          w = fma(lA[1], ep[NWV], w);
          if (ND == 3) w = fma(lA[2 % ND], ep[(2 * NWV) % E4], w);
          sh_w[buf][q][cw] = NA * w;
        }
      }
      __syncthreads();
      if (worker) {
#pragma unroll 1
        for (int q = 0; q < CH; q++) {
          if (!sh_p[buf][q]) continue;
          if (!tancsr_bit(sh_m[buf][q][0], sh_m[buf][q][1], wm)) continue;
          const double* f = sh_f[buf][q];
          double NB = f[wb[0]] * f[5 + wb[1]];
          if (ND == 3) NB *= f[(10 + wb[2]) % NF];
          const double l0 = f[NF + wb[0]], l1 = f[NF + 5 + wb[1]];
          const double l2 = ND == 3 ? f[(NF + 10 + wb[2]) % (2 * NF)] : 0.0;
          const double* w = sh_w[buf][q];
#pragma unroll
          for (int n = 0; n < NPT; n++) {
            const int ij = wg + n * ng;
            if (ij < E) {
              double v = l0 * w[ij];
              v = fma(l1, w[E + ij], v);
              if (ND == 3) v = fma(l2, w[(2 * E + ij) % NWV], v);
              part[n] = fma(NB, v, part[n]);
            }
          }
        }
      }
      buf ^= 1;
    }
    // the run's blocks go from the member that summed them to the thread that owns the column offset.  (sh_part is
    // rewritten behind at least one more barrier, the next run's first pass, which every thread reaches after these
    // reads.)  Every kept member of the run is written, also one no particle holds (a zero, as in k_tancsr_rows); an
    // owner of the upper form reads kept members only: offset >= 0 is member code >= sA
    if (worker) {
#pragma unroll
      for (int n = 0; n < NPT; n++) {
        const int ij = wg + n * ng;
        if (ij < E) sh_part[wm][ij] = part[n];
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < OPT; k++) {
      const int b0 = TANBSR_DOF(k, 0) + a[0], b1 = TANBSR_DOF(k, 1) + a[1], b2 = ND == 3 ? TANBSR_DOF(k, 2) + a[2] : 0;
      if (S0 + t + k * NT < S && (unsigned)b0 < 5u && (unsigned)b1 < 5u && (unsigned)b2 < 5u) {
        const double* src = sh_part[b0 + 5 * b1 + 25 * b2];
#pragma unroll
        for (int ij = 0; ij < E; ij++) acc[k][ij] += src[ij];
      }
    }
  }
  // the visited offsets in lexicographic order; listed position of an offset = visited offsets from S0 before it
  __syncthreads();
  if (t < MW) sh_mask[t] = mask[(size_t)A * MW + t];
  __syncthreads();
  if (t == 0) {
    int s = 0;
    for (int w = 0; w <= MW; w++) {
      sh_pref[w] = s;
      if (w < MW) s += (int)__popcll(sh_mask[w]);
    }
  }
  __syncthreads();
  const int skip = HALF ? sh_pref[S0 >> 6] + (int)__popcll(sh_mask[S0 >> 6] & ((1ull << (S0 & 63)) - 1ull)) : 0;
  const int listed = sh_pref[MW] - skip;  // (cnt, but for the walk of every member with `upper`: then cnt <= listed)
  int pos[OPT], mB[OPT];
#pragma unroll
  for (int k = 0; k < OPT; k++) {
    const int s = S0 + t + k * NT;
    pos[k] = -1;
    mB[k] = -1;
    if (s < S && ((sh_mask[s >> 6] >> (s & 63)) & 1ull)) {
      pos[k] = sh_pref[s >> 6] + (int)__popcll(sh_mask[s >> 6] & ((1ull << (s & 63)) - 1ull)) - skip;
      mB[k] = n2m[A + TANBSR_DOF(k, 0) + g.n[0] * (TANBSR_DOF(k, 1) + g.n[1] * TANBSR_DOF(k, 2))];
      sh_key[pos[k]] = mB[k];
    }
  }
  __syncthreads();
  // masked numbers that ascend with the grid order leave the columns ascending as they stand; otherwise the row's keys
  // are ranked in LDS (keys of one row are distinct), among the keys >= mA where the upper blocks are picked by number
  const int least = (!HALF && upper) ? mA : -1;
  int bad = (!HALF && upper) ? 1 : 0;
  for (int q = t; q + 1 < listed; q += NT) bad |= sh_key[q] >= sh_key[q + 1];
  if (__syncthreads_or(bad)) {
#pragma unroll
    for (int k = 0; k < OPT; k++) {
      if (pos[k] < 0) continue;
      int rk = 0;
      for (int q = 0; q < listed; q++) rk += sh_key[q] >= least && sh_key[q] < mB[k];
      pos[k] = mB[k] >= least ? rk : -1;
    }
  }
  const size_t base = (size_t)offb[mA];
#pragma unroll
  for (int k = 0; k < OPT; k++) {
    if (pos[k] < 0) continue;
    const bool centre = dofp[k] == 0x040404;
    const size_t at = base + (size_t)pos[k];
    bcols[at] = mB[k];
    double o[E];
#pragma unroll
    for (int i = 0; i < ND; i++) {
      const int ra = mA * ND + i;
#pragma unroll
      for (int j = 0; j < ND; j++) {
        const int cb = mB[k] * ND + j;
        double v = acc[k][i * ND + j];
        if (centre && i == j && aM) v += aM[ra];
        if (d2m && (d2m[ra] == -1 || d2m[cb] == -1)) v = (ra == cb) ? 1.0 : 0.0;
        o[i * ND + j] = v;
      }
    }
    // (the layout picks the value, not the address: the d^2 stores stay at fixed offsets and merge into wide ones)
#pragma unroll
    for (int c = 0; c < E; c++) vals[at * E + c] = col_major ? o[(c % ND) * ND + c / ND] : o[c];
  }
}
#undef TANBSR_DOF
