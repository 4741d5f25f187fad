// Assembled tangent in CSR, row by row and without float atomics (nlps_gpu_tangent_csr_pattern / nlps_gpu_tangent_csr).
//
// With the per-particle tensor Dh of k_tanop_setup (nlps_tangent_operator.hpp) and gn_B = -N_B Jm1 l_B every block is
//   K_AB[i][j] = N_A N_B sum_ab l_A[a] l_B[b] E[a][b][i][j],   E[a][b][i][j] = sum_mn Jm1[m][a] Jm1[n][b] Dh[m][n][i][j]
// (k_tanop_bdiag is this formula for B = A).  Every matrix entry has ONE owner: the workgroup of row node A holds the
// d x d accumulators of A's 9^d column offsets in registers, one thread per offset (three in 3-D), and walks the
// particles that hold A -- the runs of the closest nodes C with |C - A| <= 2 per axis, in lexicographic order of C and
// ascending memory slot inside a run.  Inside one run every particle has the same stencil, so the run is summed by
// MEMBER: thread (member B, component group) adds its share of the particles' blocks in registers -- all 5^d members
// are column nodes of the row, no lane idles on an offset outside the stencil --, the finished run passes through LDS
// as plain stores and each offset's owner adds it to its accumulator.  Every sum has one thread and one order; the
// finished rows are written once.  No kernel of this file holds a float atomic, so the matrix repeats bit for bit
// whenever the particle arrays do.  That walk is tancsr_walk below; k_tancsr_rows stores its blocks as scalar CSR rows,
// k_tanbsr_rows (nlps_tangent_bsr.hpp) stores the same blocks as block CSR.
//
// Kept per linearisation (nlps_gpu_tangent_csr_pattern, counted in its `bytes`), one record per particle IN THE ORDER BY
// CLOSEST NODE, so that a row reads its runs as contiguous memory at addresses that depend on the run starts alone (no
// load waits for an index another load fetches): E [np][d^4] (consecutive lanes consecutive doubles); the 5 d separable
// LME factors, Z^-1 folded into the x factors, and the position [np][6 d] (regenerating the factors costs 3 d + 1
// exponentials and the moments of 5^d members for each of the up to 5^d rows that visit the particle); the membership
// mask [np][2].  Per node: the run starts [nnodes + 1] and the visited-offset bit mask of every row node
// [nnodes][2 | 12] words; block counts and their scan per masked node.  Nothing of the order 9^d nnodes doubles: the
// dense stencil array of the atomic path is not used.
#pragma once

template <int ND>
struct CsrCfg {
  static constexpr int S = TanCfg<ND>::S;            // 81 / 729 column offsets of a row node
  static constexpr int NT = (ND == 3) ? 256 : 128;   // threads of a row workgroup
  static constexpr int OPT = (S + NT - 1) / NT;      // offsets a thread owns: 1 / 3
  static constexpr int MW = (S + 63) / 64;           // 64-bit words of a row's visited mask: 2 / 12
  static constexpr int E = ND * ND, E4 = E * E;
  static constexpr int NWV = ND * E;                 // w[b][ij] of one (row, particle) visit: 8 / 27 values
  static constexpr int NF = 5 * ND;                  // separable factors of a particle
  static constexpr int NFX = NF + ND;                // a particle's record: the factors, then its position
  static constexpr int CH = NT / 32;                 // particles staged per pass (32 threads form one particle's w)
  static constexpr int MAXM = TanCfg<ND>::MAXM;      // members of a particle's stencil: 25 / 125
  static constexpr int GS = (ND == 3) ? 128 : 32;    // threads of a worker group: one per member
  static constexpr int NG = NT / GS;                 // worker groups, each sums its share of a block's d^2 components: 4 / 2
  static constexpr int NPT = (E + NG - 1) / NG;      // components per worker: 1 / 5
};

// how the walk deals offsets and members where it keeps the upper blocks only (tancsr_walk<ND, true>)
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

__device__ __forceinline__ bool tancsr_bit(u64 lo, u64 hi, int b) {
  return b < 64 ? ((lo >> b) & 1ull) != 0ull : ((hi >> (b - 64)) & 1ull) != 0ull;
}

// E and the factors of one particle (zeros without a neighbourhood or with a singular J: flagged like the operator does)
template <int ND>
__global__ __launch_bounds__(64) void k_tancsr_setup(PView P, GridD g, const double* __restrict__ Dh, int ld,
                                                      const int* __restrict__ sorted, double* __restrict__ Ep,
                                                      double* __restrict__ Fp, u64* __restrict__ Mk,
                                                      int* __restrict__ gstatus) {
  constexpr int E = ND * ND, E4 = E * E, NF = 5 * ND, NFX = CsrCfg<ND>::NFX;
  const int pos = blockIdx.x * blockDim.x + threadIdx.x;  // position in the order by closest node: the records' order
  if (pos >= P.np) return;
  const int p = sorted[pos];
  Lme<ND> c;
  double lam[ND], beta;
  bool ok = load_lme<ND>(P, g, p, c, lam, beta);
  double Zinv = 0.0, r[ND], J[E], Jm1[E];
  if (ok) {
    lme_moments_h<ND>(c, Zinv, r, J);
    if (!inverse<ND>(Jm1, J)) {
      atomicOr(&P.status[p], ST_NEWTON);
      atomicOr(gstatus, ST_NEWTON);
      ok = false;
    }
  }
  double* const ep = Ep + (size_t)pos * E4;
  double* const fp = Fp + (size_t)pos * NFX;
  Mk[2 * (size_t)pos] = c.mlo;
  Mk[2 * (size_t)pos + 1] = c.mhi;
#pragma unroll
  for (int a = 0; a < ND; a++) fp[NF + a] = PF(P, F_X + a, p);
  if (!ok) {
    for (int e = 0; e < E4; e++) ep[e] = 0.0;
    for (int f = 0; f < NF; f++) fp[f] = 0.0;
    return;
  }
#pragma unroll
  for (int i = 0; i < 5; i++) {
    fp[i] = Zinv * c.ex[i];
    fp[5 + i] = c.ey[i];
    if (ND == 3) fp[(10 + i) % NF] = c.ez[i % Lme<ND>::KN];
  }
#pragma unroll
  for (int ij = 0; ij < E; ij++) {
    double Dm[E], X[E];  // slice Dh[.][.][ij], then Jm1^T slice Jm1
#pragma unroll
    for (int mn = 0; mn < E; mn++) Dm[mn] = Dh[(size_t)(mn * E + ij) * ld + p];
#pragma unroll
    for (int a = 0; a < ND; a++)
#pragma unroll
      for (int n = 0; n < ND; n++) {
        double v = 0.0;
#pragma unroll
        for (int mm = 0; mm < ND; mm++) v = fma(Jm1[mm * ND + a], Dm[mm * ND + n], v);
        X[a * ND + n] = v;
      }
#pragma unroll
    for (int a = 0; a < ND; a++)
#pragma unroll
      for (int b = 0; b < ND; b++) {
        double v = 0.0;
#pragma unroll
        for (int n = 0; n < ND; n++) v = fma(X[a * ND + n], Jm1[n * ND + b], v);
        ep[(a * ND + b) * E + ij] = v;
      }
  }
}

// run[n] = first position of the (I0, p)-sorted particle list whose closest node is >= n
__global__ void k_tancsr_runs(int np, int nnodes, const unsigned long long* __restrict__ keys, int* __restrict__ run) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= np) return;
  // (a key that is no node of the grid counts as `nnodes`: such particles sit behind every run)
  const unsigned long long top = (unsigned long long)nnodes;
  const int k = (int)min(keys[s], top), prev = s > 0 ? (int)min(keys[s - 1], top) : -1;
  for (int n = prev + 1; n <= k; n++) run[n] = s;
  if (s == np - 1)
    for (int n = k + 1; n <= nnodes; n++) run[n] = np;
}

// visited column offsets of every row node: one wave per row node ORs the membership of the particles that hold it
template <int ND>
__global__ __launch_bounds__(256) void k_tancsr_pattern(GridD g, const int* __restrict__ run, const u64* __restrict__ Mk,
                                                         const int* __restrict__ n2m, u64* __restrict__ mask,
                                                         int* __restrict__ cntm) {
  constexpr int S = CsrCfg<ND>::S, MW = CsrCfg<ND>::MW;
  const int lane = threadIdx.x & 63;
  const int A = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (A >= g.nnodes) return;  // (whole waves)
  const int mA = n2m[A];
  unsigned fl = 0u;  // bit t: offset 64 t + lane is visited
  if (mA >= 0) {
    const int Ai[3] = {A % g.n[0], (A / g.n[0]) % g.n[1], ND == 3 ? A / (g.n[0] * g.n[1]) : 0};
#pragma unroll 1
    for (int ec = 0; ec < (ND == 3 ? 125 : 25); ec++) {
      const int e[3] = {ec % 5 - 2, (ec / 5) % 5 - 2, ND == 3 ? ec / 25 - 2 : 0};
      const int Cc[3] = {Ai[0] + e[0], Ai[1] + e[1], Ai[2] + e[2]};
      if (Cc[0] < 0 || Cc[0] >= g.n[0] || Cc[1] < 0 || Cc[1] >= g.n[1]) continue;
      if (ND == 3 && (Cc[2] < 0 || Cc[2] >= g.n[2])) continue;
      const int C = Cc[0] + g.n[0] * (Cc[1] + g.n[1] * Cc[2]);
      const int r0 = run[C], r1 = run[C + 1];
      if (r0 >= r1) continue;
      const int a[3] = {2 - e[0], 2 - e[1], ND == 3 ? 2 - e[2] : 0};  // stencil code of A around C
      const int sA = a[0] + 5 * a[1] + 25 * a[2];
#pragma unroll 1
      for (int pos = r0; pos < r1; pos++) {
        const u64 lo = Mk[2 * (size_t)pos], hi = Mk[2 * (size_t)pos + 1];
        if (!tancsr_bit(lo, hi, sA)) continue;
#pragma unroll
        for (int t = 0; t < MW; t++) {
          const int s = 64 * t + lane;
          const int b0 = s % 9 - 4 + a[0], b1 = (s / 9) % 9 - 4 + a[1], b2 = ND == 3 ? s / 81 - 4 + a[2] : 0;
          const bool in = s < S && (unsigned)b0 < 5u && (unsigned)b1 < 5u && (unsigned)b2 < 5u;
          if (in && tancsr_bit(lo, hi, b0 + 5 * b1 + 25 * b2)) fl |= 1u << t;
        }
      }
    }
  }
  int cnt = 0;
#pragma unroll
  for (int t = 0; t < MW; t++) {
    const u64 word = __ballot((fl >> t) & 1u);
    if (lane == 0) mask[(size_t)A * MW + t] = word;
    cnt += (int)__popcll(word);
  }
  if (lane == 0 && mA >= 0) cntm[mA] = cnt;
}

// row_ptr of the N_A d dof rows from the block counts of the masked nodes and their exclusive scan
template <int ND>
__global__ void k_tancsr_rowptr(int nactive, const int* __restrict__ cntm, const int* __restrict__ off, int* __restrict__ row_ptr) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx > nactive * ND) return;
  if (idx == nactive * ND) {
    row_ptr[idx] = off[nactive] * ND * ND;
    return;
  }
  const int m = idx / ND, i = idx - m * ND;
  row_ptr[idx] = off[m] * ND * ND + i * cntm[m] * ND;
}

// axis `ax` of a column offset packed by tancsr_walk: 0 .. 8 in one byte each, here as -4 .. 4
__device__ __forceinline__ int tancsr_dof(int packed, int ax) { return (int)((packed >> (8 * ax)) & 0xff) - 4; }

// The walk of row node A = blockIdx.x by one workgroup of CsrCfg::NT threads: the blocks K_AB of A's visited column
// offsets, summed as the header says, finished (alpha_1 M on the diagonal, Dirichlet rows and columns) and handed to
// emit(off[mA], cntm[mA], pos, mB, o) by the thread that owns the offset: pos is the block's place among the row's kept
// blocks in ascending order of masked number, mB its masked column node, o its d^2 values row-major.  Every form of the
// assembled tangent is this function with another emit, so every form stores the same bits.  HALF and `upper` (cntm
// and off are then those of the kept blocks): nlps_tangent_bsr.hpp.
template <int ND, bool HALF, class Emit>
__device__ __forceinline__ void tancsr_walk(
    const GridD& g, const int* __restrict__ run, const double* __restrict__ Ep, const double* __restrict__ Fp,
    const u64* __restrict__ Mk, const u64* __restrict__ mask, const int* __restrict__ n2m, const int* __restrict__ d2m,
    const double* __restrict__ aM, const int* __restrict__ cntm, const int* __restrict__ off, int upper, const Emit& emit) {
  using Cfg = CsrCfg<ND>;
  using Bfg = BsrCfg<ND>;
  constexpr int S = Cfg::S, NT = Cfg::NT, MW = Cfg::MW, E = Cfg::E, E4 = Cfg::E4, NWV = Cfg::NWV, NF = Cfg::NF,
                NFX = Cfg::NFX, CH = Cfg::CH, MAXM = Cfg::MAXM, NPT = Cfg::NPT, NC = (ND == 3) ? 125 : 25,
                S0 = HALF ? Bfg::SC : 0, OPT = HALF ? Bfg::OPTH : Cfg::OPT;
  // the staged particles, in two buffers (a pass fills one while slower waves still read the other: one barrier per pass)
  __shared__ double sh_w[2][CH][NWV];     // w[b][ij] = N_A sum_a l_A[a] E[a][b][ij]
  __shared__ double sh_f[2][CH][2 * NF];  // factors (x, y, z), then l per axis and stencil index
  __shared__ u64 sh_m[2][CH][2];
  __shared__ int sh_p[2][CH];             // 1 = staged and holds A
  __shared__ int sh_run[NC][2];           // the runs of the closest nodes around A (empty where the grid ends)
  __shared__ double sh_part[MAXM][E];     // the blocks of one closest node's run, by member of its stencil
  __shared__ u64 sh_mask[MW];
  __shared__ int sh_pref[MW];
  __shared__ int sh_key[S];               // masked node of the q-th listed offset
  const int A = blockIdx.x, t = threadIdx.x;
  const int mA = n2m[A];
  if (mA < 0) return;  // (uniform)
  const int cnt = cntm[mA];
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
      // (the records lie in run order: every load below depends on the position alone)
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
    // reads.)  Every kept member of the run is written, also one no particle holds (a zero); an owner of the upper
    // form reads kept members only: offset >= 0 is member code >= sA
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
      const int b0 = tancsr_dof(dofp[k], 0) + a[0], b1 = tancsr_dof(dofp[k], 1) + a[1];
      const int b2 = ND == 3 ? tancsr_dof(dofp[k], 2) + a[2] : 0;
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
    for (int w = 0; w < MW; w++) {
      sh_pref[w] = s;
      s += (int)__popcll(sh_mask[w]);
    }
  }
  __syncthreads();
  const int skip = HALF ? sh_pref[S0 >> 6] + (int)__popcll(sh_mask[S0 >> 6] & ((1ull << (S0 & 63)) - 1ull)) : 0;
  // (cnt, but for the walk of every member with `upper`: then cnt <= listed)
  const int listed = sh_pref[MW - 1] + (int)__popcll(sh_mask[MW - 1]) - skip;
  int pos[OPT], mB[OPT];
#pragma unroll
  for (int k = 0; k < OPT; k++) {
    const int s = S0 + t + k * NT;
    pos[k] = -1;
    mB[k] = -1;
    if (s < S && ((sh_mask[s >> 6] >> (s & 63)) & 1ull)) {
      pos[k] = sh_pref[s >> 6] + (int)__popcll(sh_mask[s >> 6] & ((1ull << (s & 63)) - 1ull)) - skip;
      mB[k] = n2m[A + tancsr_dof(dofp[k], 0) + g.n[0] * (tancsr_dof(dofp[k], 1) + g.n[1] * tancsr_dof(dofp[k], 2))];
      sh_key[pos[k]] = mB[k];
    }
  }
  __syncthreads();
  // masked numbers that ascend with the grid order (the default numbering) leave the columns ascending as they stand;
  // under a caller's numbering the row's keys are ranked in LDS (keys of one row are distinct), among the keys >= mA
  // where the upper blocks are picked by number
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
  const size_t base = (size_t)off[mA];
#pragma unroll
  for (int k = 0; k < OPT; k++) {
    if (pos[k] < 0) continue;
    const bool centre = dofp[k] == 0x040404;
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
    emit(base, cnt, pos[k], mB[k], o);
  }
}

// scalar CSR: the d rows of the row node lie behind one another, each with the row's cnt d columns
template <int ND>
struct EmitCsr {
  int* __restrict__ cols;
  double* __restrict__ vals;
  __device__ __forceinline__ void operator()(size_t base, int cnt, int pos, int mB, const double (&o)[ND * ND]) const {
#pragma unroll
    for (int i = 0; i < ND; i++) {
      const size_t at = base * (ND * ND) + (size_t)i * cnt * ND + (size_t)pos * ND;
#pragma unroll
      for (int j = 0; j < ND; j++) {
        cols[at + j] = mB * ND + j;
        vals[at + j] = o[i * ND + j];
      }
    }
  }
};

// the d rows of row node A: columns and values, one workgroup per row node
template <int ND>
__global__ __launch_bounds__(CsrCfg<ND>::NT) void k_tancsr_rows(
    GridD g, const int* __restrict__ run, const double* __restrict__ Ep, const double* __restrict__ Fp,
    const u64* __restrict__ Mk, const u64* __restrict__ mask, const int* __restrict__ n2m, const int* __restrict__ d2m,
    const double* __restrict__ aM, const int* __restrict__ cntm, const int* __restrict__ off, int* __restrict__ cols,
    double* __restrict__ vals) {
  tancsr_walk<ND, false>(g, run, Ep, Fp, Mk, mask, n2m, d2m, aM, cntm, off, 0, EmitCsr<ND>{cols, vals});
}
