// nlps_gpu.hip — MI355X (gfx950) kernels and C-ABI host code for NL-PartSol's particle<->grid +
// stress-update hot path.  See include/nlps_gpu.h for the boundary and DESIGN.md for the layout.
//
// Layout in HBM
//   particles : SoA, one contiguous run of `npad` doubles per scalar component (enum below), physically
//               sorted (tile of the closest node I0, corner type, I0) at upload and by the periodic device
//               re-sort; lane p of a wave reads consecutive doubles of every component => coalesced
//               512-B wave loads.
//   nodes     : AoS per node in GRID numbering (x fastest, slab axis slowest): nm[node][1+d] =
//               {mass, momentum}, dU[node][d], force[node][d], accel[node][d]; a slab halo is one
//               contiguous byte range.  active[node], seed[node], fixed[node][d] are bytes.
// One lane = one particle.  All LME quantities (15 separable exp factors, Z, r, J, J^-1, DF, tau)
// live in that lane's registers; no MFMA (<=3x3 contractions).  The particle<->grid kernels work per tile of
// closest nodes with the tile's node window in LDS (nlps_tile_kernels.hpp); this file holds the search, the
// nodal kernels, the per-particle level-B kernels and the C-ABI host code.
#include <hip/hip_runtime.h>
#include <unistd.h>
#include <thread>
#include <hipcub/hipcub.hpp>

#include <dlfcn.h>
#include <rccl/rccl.h>  // types and prototypes only: the library is dlopen()ed when a communicator is attached

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/nlps_gpu.h"
#include "nlps_device.hpp"
#include "nlps_tables.hpp"
#include "nlps_host_mem.hpp"

// one kernel name per dimension, the same arguments: the 2-D or the 3-D one on the handle's stream
#define LAUNCH_ND_BLK(kern2, kern3, grid, block, ...)                                              \
  do {                                                                                             \
    if (h->nd == 2) { hipLaunchKernelGGL(kern2, dim3(grid), dim3(block), 0, h->stream, __VA_ARGS__); } \
    else { hipLaunchKernelGGL(kern3, dim3(grid), dim3(block), 0, h->stream, __VA_ARGS__); }        \
  } while (0)
#define LAUNCH_ND(kern2, kern3, grid, ...) LAUNCH_ND_BLK(kern2, kern3, grid, BLK, __VA_ARGS__)

using namespace nlps;

// Run-time values as template arguments: f is a generic lambda, called with a std::integral_constant, and names its
// kernel through CT(arg).  Only the values a helper can pass are instantiated, so a kernel that exists for a part of
// the laws is dispatched with with_law_in<LO, HI> over exactly that part.
template <int V>
using ic = std::integral_constant<int, V>;
#define CT(x) (decltype(x)::value)
template <class F>
static void with_nd(int nd, F&& f) {
  if (nd == 2) f(ic<2>{});
  else f(ic<3>{});
}
template <class F>
static void with_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}
// law in LO .. HI; anything else goes to HI, as the last `else` of the ladders this replaces did (the handle only holds
// kernel laws 0 .. NLPS_KLAW_FRICTIONAL, klaw_of): a law out of range launches the last kernel, never nothing
template <int LO, int HI, class F>
static void with_law_in(int law, F&& f) {
  if constexpr (LO < HI) {
    if (law == LO) f(ic<LO>{});
    else with_law_in<LO + 1, HI>(law, f);
  } else {
    f(ic<HI>{});
  }
}
template <class F>
static void with_law(int law, F&& f) {
  with_law_in<0, NLPS_KLAW_FRICTIONAL>(law, f);
}
// the laws of a cloud of several (law_present of the handle), ascending: f(law, is it the last one)
template <class F>
static void for_each_law_present(unsigned mask, F&& f) {
  for (int l = 0; l <= NLPS_KLAW_FLUID; l++)
    if (mask & (1u << l)) f(l, (mask >> (l + 1)) == 0);
}

// ------------------------------------------------------------------------------------------------
// particle component table
// ------------------------------------------------------------------------------------------------
enum {
  F_X = 0, F_DIS = 3, F_VEL = 6, F_ACC = 9, F_DDIS = 12,
  F_FN = 15, F_FN1 = 24, F_DF = 33, F_TAU = 42, F_BEN = 51, F_BEN1 = 60,
  F_JN = 69, F_JN1 = 70, F_RHO = 71, F_MASS = 72, F_VOL0 = 73, F_W = 74,
  F_KN = 75, F_KN1 = 76, F_EN = 77, F_EN1 = 78, F_LAM = 79, F_BETA = 82,
  F_LAMP = 83,  // lambda of the previous step (Newton start extrapolation)
  F_BACK = 86,  // principal back stress (Von-Mises), 3 components
  // rho * J, the invariant of the explicit density update rho <- rho / det DF (U-Verlet.c:630-632: det DF = J_n+1 / J_n):
  // the fused step leaves rho alone and k_copy_n_to_n1 returns rho = (rho J) / J_n when somebody asks (k_init_rhoj)
  F_RHOJ = 89,
  F_CEP = 90,   // C_ep[ndim*ndim] (Drucker-Prager / Von-Mises tangent moduli, implicit driver only)
  F_DTFN = 99, F_DTFN1 = 108, F_DTDF = 117,  // rate tensors (level-B compatibility with dU_dt)
  F_DMG = 126, F_DMG1 = 127,                 // Damage_n, Damage_n1 (eigenerosion / eigensoftening, level B only)
  F_STRF = 128, F_STRF1 = 129,               // Strain_f_n, Strain_f_n1 (eigensoftening)
  // eigenerosion: position and closest node of every particle when the epsilon-neighbourhoods were initialised
  // (compute_Beps__Constitutive__(.., true), U-Newmark-beta.c:182-183): what the FROZEN list of a particle that has
  // not moved since is made of (Beps.c:30-36).  The closest node travels as a double like any other field.
  F_X0 = 130, F_I00 = 133,
  NFD = 134
};

struct PView {
  int np;
  size_t npad;
  double* d;  // [NFD][npad]
  int* I0;
  int* I0n;  // closest node for the position the last explicit step wrote (k5_tile's search ahead); = I0 otherwise.  I0
             // itself stays the node of the last search until the next one adopts I0n (downloads, migration see I0)
  int* mat;
  int* nn;
  int* status;
  u64* mlo;
  u64* mhi;
  int* tile;  // tile of I0 (per-step binning)
  int* rank;  // arrival rank inside the tile
  int flip;   // 1: the n / n+1 slots of F and b_e are swapped (the explicit step rolls them by renaming)
  int erosion;  // Driver_EigenErosion or Driver_EigenSoftening: the damage hooks of the level-B stages are on
  int softening;  // ... with Eigensoftening__Constitutive__ (Driver_EigenSoftening and not Driver_EigenErosion)
};
#define PF(P, f, p) ((P).d[(size_t)(f) * (P).npad + (size_t)(p)])
// first component of F_n, F_n+1, b_e,n, b_e,n+1 under the current renaming
__host__ __device__ __forceinline__ int fFN(const PView& P) { return P.flip ? F_FN1 : F_FN; }
__host__ __device__ __forceinline__ int fFN1(const PView& P) { return P.flip ? F_FN : F_FN1; }
__host__ __device__ __forceinline__ int fBEN(const PView& P) { return P.flip ? F_BEN1 : F_BEN; }
__host__ __device__ __forceinline__ int fBEN1(const PView& P) { return P.flip ? F_BEN : F_BEN1; }

struct NView {
  unsigned char* active;  // [nnodes]
  unsigned char* seed;    // [nnodes] 1 where some particle has this node as I0 (dilate_node turns it into `active`)
  const double* h_avg;    // [nnodes]
  // [nnodes] {beta, T2, Ra, -}: beta__LME__ of a particle whose closest node this is (gamma / h_avg^2, LME.c:177-185),
  // the cut-off radius Ra of the NEXT list built with that beta (LME.c:1052) and its exact squared form T2 =
  // max{t : fl(sqrt(t)) <= Ra}; functions of the node alone, made once at create by the device functions K2 would
  // otherwise call per particle and step (two divisions and three or more square roots)
  const double4* beta_t2;
  double* nm;             // [nnodes][1+ND]
  double* dU;             // [nnodes][ND]
  double* force;          // [nnodes][ND]
  double* accel;          // [nnodes][ND]
  double* reaction;       // [nnodes][ND]
  unsigned char* fixed;   // [nnodes][ND]
};

#define ST_NEWTON 1
#define ST_CONNECT 2
#define ST_JACOBIAN 4
#define ST_CONSTITUTIVE 8
#define ST_HALO 16

static constexpr int BLK = 256;

struct TileCnt {
  int nt[3];
  int* count;       // [ntiles] particles per tile, nullptr = no binning
  int tile0, ntw;   // tiles of the node window (nlps_gpu_set_node_window); default: all
  int win_lo, win_hi, plane;  // node layers (slowest axis) of the window, nodes per layer
  int* gstatus;
  // adaptive re-sort (nlps_gpu_set_adaptive_resort), nullptr = off: home[slot] = tile of the particle in that memory
  // slot at the first search after the last re-sort (rehome != 0: this search records it); foreign = 64 counters,
  // 128 B apart, of the particles found in another tile than their slot's home
  int* home;
  int rehome;
  int* foreign;
  // canonical tile lists without a per-tile sort (k_fill_order): node_cnt[node] counts the particles of every closest
  // node, nrank[p] = the rank of p inside its node (arrival order of the atomic); nullptr = off
  int* node_cnt;
  int* nrank;
  // defer != 0 (the search that rides on k5_tile, canonical lists on): only COUNT here -- the tile and node counters by
  // atomics whose result nobody waits for -- and leave the ranks (positions inside the tile list and inside the node) to
  // k_fill_orders of the next step, which takes them from cursors at full occupancy.  K5 runs three waves per SIMD: a
  // returning atomic there is a stall nothing covers (+20 us of K5's 110 at 1 M particles).
  // (The host sets it for every riding search outside the deterministic mode; the field goes with a later change of
  // the kernels that read it.)
  int defer;
};
template <int ND>
struct TileCfg;
template <int ND>
__device__ __forceinline__ int tile_of_node(const GridD& g, const int* nt, int I0);

__device__ __forceinline__ void atomic_add_f64(double* addr, double v) { unsafeAtomicAdd(addr, v); }

// Bins a particle to the tile of its I0.  Wave-aggregated: one returning atomic per (wave, tile); the
// lanes of a wave that share a tile get CONSECUTIVE slots in lane order, so order[] keeps runs of 64
// memory-consecutive particles together (coalesced loads in the tile kernels).  Every lane of the wave
// must call this (invalid lanes pass valid = false).
template <int ND>
__device__ __forceinline__ void bin_particle(const PView& P, const GridD& g, const TileCnt& tc, int p, int I0,
                                             bool valid) {
  if (!tc.count) return;
  int t = valid ? tile_of_node<ND>(g, tc.nt, I0) : -1;
  if (valid) {  // the 5^d stencil of I0 must stay inside this rank's node window
    const int layer = I0 / tc.plane, nl = g.n[ND - 1];
    const int s_lo = layer - 2 < 0 ? 0 : layer - 2, s_hi = layer + 2 > nl - 1 ? nl - 1 : layer + 2;
    if (s_lo < tc.win_lo || s_hi > tc.win_hi) {
      // flagged AND left out of the lists: its stencil holds nodes nothing of this rank resets or exchanges (the per-node
      // counters of the canonical lists among them), so no kernel may take it; it keeps its state, the re-sort keeps it
      // (k_append_unlisted), a migration hands it on
      atomicOr(&P.status[p], ST_HALO);
      atomicOr(tc.gstatus, ST_HALO);
      t = -1;
      valid = false;
    }
    if (valid && (t < tc.tile0 || t >= tc.tile0 + tc.ntw)) {  // not binned: its tile is never launched
      t = -1;
      valid = false;
    }
  }
  const int lane = threadIdx.x & 63;
  if (tc.defer) {  // count only (see TileCnt::defer)
    bool todo_l = valid;
    while (true) {
      const u64 todo = __ballot(todo_l);
      if (!todo) break;
      const int leader = __ffsll((unsigned long long)todo) - 1;
      const int t0 = __shfl(t, leader);
      const bool mine = todo_l && (t == t0);
      const u64 same = __ballot(mine);
      if (lane == leader) atomicAdd(&tc.count[t0], (int)__popcll(same));  // (no result wanted: no wait)
      if (mine) todo_l = false;
    }
    if (p < P.np) {
      P.tile[p] = t;
      if (tc.node_cnt && valid) atomicAdd(&tc.node_cnt[I0], 1);
    }
  } else {
  // groups of lanes that share a tile: leader lane, group size and the lane's place in its group, by ballots alone ...
  int rank = 0;
  {
    int my_leader = lane, my_off = 0, my_cnt = 0;
    bool todo_l = valid;
    while (true) {
      const u64 todo = __ballot(todo_l);
      if (!todo) break;
      const int leader = __ffsll((unsigned long long)todo) - 1;
      const int t0 = __shfl(t, leader);
      const bool mine = todo_l && (t == t0);
      const u64 same = __ballot(mine);
      if (mine) {
        my_leader = leader;
        my_off = (int)__popcll(same & ((1ull << lane) - 1ull));
        my_cnt = (int)__popcll(same);
        todo_l = false;
      }
    }
    // ... then ONE returning atomic per group, all groups of the wave in the same instruction: one round trip to the
    // counters however many tiles the wave's particles are in (a loop with the atomic inside paid one per tile: K5 of a
    // stirred cloud 0.226 ms, of which 0.07 waiting here)
    int base = 0;
    if (valid && lane == my_leader) base = atomicAdd(&tc.count[t], my_cnt);
    base = __shfl(base, my_leader);
    if (valid) rank = base + my_off;
  }
  if (p < P.np) {
    P.tile[p] = t;  // -1: not binned (failed element search or outside the node window)
    P.rank[p] = rank;
    // (the lanes of a wave mostly hold distinct closest nodes -- the memory order is the canonical one -- so these
    // atomics spread over the node array)
    if (tc.node_cnt) tc.nrank[p] = valid ? atomicAdd(&tc.node_cnt[I0], 1) : 0;
  }
  }
  if (tc.home) {
    bool away = false;
    if (p < P.np) {
      if (tc.rehome) tc.home[p] = t;
      else away = t != tc.home[p];
    }
    const u64 m = __ballot(away);
    if (lane == 0 && m) atomicAdd(&tc.foreign[32 * ((blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) & 63)], (int)__popcll(m));
  }
}

template <int ND>
__device__ __forceinline__ int class3_of(const GridD& g, const int* ijk) {
  int c = 0, mul = 1;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    int ca = (a < ND) ? (ijk[a] == 0 ? 0 : (ijk[a] == g.n[a] - 1 ? 2 : 1)) : 1;
    c += ca * mul;
    mul *= 3;
  }
  return c;
}

// ------------------------------------------------------------------------------------------------
// S1a: closest-node update (LME.c:913-945, Nodes-Tools.c:476-538) + 1-ring activation (LME.c:949-960)
// ------------------------------------------------------------------------------------------------
// One launch instead of five hipMemsetAsync (each of which costs one or two 5-us fill kernels): resets the
// search seeds and tile counters and, for the fused explicit step, the nodal accumulators of the node window.
template <int ND>
__global__ void k_step_clear(int n0, int nnodes, NView N, int* __restrict__ tile_count, int ntiles, int nodal,
                             int* __restrict__ node_cnt, int bins) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (bins && t < ntiles) tile_count[t] = 0;
  if (t >= nnodes) return;
  const size_t A = (size_t)n0 + t;
  if (bins) {  // (not when the last step's k5_tile has done this step's search: its seeds and counters are the input)
    N.seed[A] = 0;  // Shape-Functions.c:38-46
    if (node_cnt) node_cnt[A] = 0;
  }
  if (nodal) {
#pragma unroll
    for (int a = 0; a < 1 + ND; a++) N.nm[A * (1 + ND) + a] = 0.0;
#pragma unroll
    for (int a = 0; a < ND; a++) {
      N.force[A * ND + a] = 0.0;
      N.fixed[A * ND + a] = 0;
    }
  }
}

// 1-ring activation (LME.c:949-960): the particles only mark their I0 (one byte store each instead of 3^d
// scattered ones); node n is active iff some I0 lies in its 1-ring.
template <int ND>
__device__ __forceinline__ void dilate_node(int A, const GridD& g, const NView& N) {
  const int i0 = A % g.n[0], j0 = (A / g.n[0]) % g.n[1], k0 = A / (g.n[0] * g.n[1]);
  unsigned any = 0u;
#pragma unroll
  for (int dk = (ND == 3 ? -1 : 0); dk <= (ND == 3 ? 1 : 0); dk++)
#pragma unroll
    for (int dj = -1; dj <= 1; dj++)
#pragma unroll
      for (int di = -1; di <= 1; di++) {
        const int i = i0 + di, j = j0 + dj, k = k0 + dk;
        const bool ok = i >= 0 && i < g.n[0] && j >= 0 && j < g.n[1] && (ND == 2 || (k >= 0 && k < g.n[2]));
        if (ok) any |= N.seed[i + g.n[0] * (j + g.n[1] * k)];
      }
  N.active[A] = any ? 1 : 0;
}

// The closest-node update of local_search__LME__ (LME.c:924-930): argmin of the distance over the 1-ring of the
// PREVIOUS closest node, ties by chain position (get_closest_node__MeshTools__, Nodes-Tools.c:476-538).
template <int ND>
__device__ __forceinline__ int closest_node_update(const GridD& g, const uint8_t* __restrict__ rank1, const double* x, int I0) {
  int ijk[3] = {I0 % g.n[0], (I0 / g.n[0]) % g.n[1], I0 / (g.n[0] * g.n[1])};
  const uint8_t* rk = rank1 + 27 * class3_of<ND>(g, ijk);
  // Of the 3^d candidates only those that can be the minimum are evaluated.  Along an axis where the particle is
  // clearly closer to the old node's plane than to either neighbouring plane (|d| <= 0.49 h) a step to a neighbouring
  // plane adds at least 0.02 h^2 to the squared distance -- orders of magnitude beyond rounding -- and along any axis
  // the step AWAY from the particle adds more than h^2: such candidates lose in the reference's loop as well.  What is
  // left is the old node and, per axis with |d| > 0.49 h, its neighbour on the particle's side: at most 2^d nodes,
  // usually one.  Their squared distances are summed like point_distance__MeshTools__ (Nodes-Tools.c:397-420:
  // DIST += pow(d,2) in axis order), the winner is the reference's: lexicographic minimum of (sqrt(D), chain position)
  // = first strict minimum of the chain walk (Nodes-Tools.c:476-538).
  int sgn[3] = {0, 0, 0};
#pragma unroll
  for (int a = 0; a < ND; a++) {
    const double d = x[a] - (g.o[a] + g.h * (double)ijk[a]);
    if (fabs(d) > 0.49 * g.h) sgn[a] = d > 0.0 ? 1 : -1;
  }
  double best = 0.0;
  int bestrank = 256, bi = ijk[0], bj = ijk[1], bk = ijk[2];
#pragma unroll
  for (int q = 0; q < (1 << ND); q++) {
    const int di = (q & 1) ? sgn[0] : 0, dj = (q & 2) ? sgn[1] : 0, dk = (ND == 3 && (q & 4)) ? sgn[2] : 0;
    // a combination that asks for a step along an axis that has none repeats another one
    const bool dup = ((q & 1) && sgn[0] == 0) || ((q & 2) && sgn[1] == 0) || (ND == 3 && (q & 4) && sgn[2] == 0);
    const int i = ijk[0] + di, j = ijk[1] + dj, k = ijk[2] + dk;
    const bool ok = !dup && i >= 0 && i < g.n[0] && j >= 0 && j < g.n[1] && (ND == 2 || (k >= 0 && k < g.n[2]));
    if (ok) {
      double Dc = 0.0, t;
      t = x[0] - (g.o[0] + g.h * (double)i);
      Dc += t * t;
      t = x[1] - (g.o[1] + g.h * (double)j);
      Dc += t * t;
      if (ND == 3) {
        t = x[ND - 1] - (g.o[2] + g.h * (double)k);
        Dc += t * t;
      }
      const double d = sqrt(Dc);
      const int rank = rk[(di + 1) + 3 * (dj + 1) + 9 * (dk + 1)];
      if (bestrank == 256 || d < best || (d == best && rank < bestrank)) {
        best = d;
        bestrank = rank;
        bi = i;
        bj = j;
        bk = k;
      }
    }
  }
  return bi + g.n[0] * (bj + g.n[1] * bk);
}

// update != 0: the search proper.  update == 0: seeds and bins only, with the closest nodes as they are -- the last
// kernel of the fused explicit step (k5_tile) has already updated them for the positions it wrote, and a second update
// would start from the new node's 1-ring instead of the old one's (LME.c:927-929).
template <int ND>
__global__ __launch_bounds__(BLK) void k_search(PView P, GridD g, NView N, const uint8_t* __restrict__ rank1, TileCnt tc,
                                                int update) {
  const int p = blockIdx.x * BLK + threadIdx.x;
  const bool valid = p < P.np;
  int I0 = 0;
  if (valid) {
    I0 = P.I0[p];
    if (update) {
      double x[ND], aux = 0.0;
#pragma unroll
      for (int a = 0; a < ND; a++) {
        x[a] = PF(P, F_X + a, p);
        aux += dsqr(PF(P, F_DIS + a, p));
      }
      if (sqrt(aux) > 0.0) {  // norm__MatrixLib__(dis_p,2) > 0, LME.c:924
        I0 = closest_node_update<ND>(g, rank1, x, I0);
        P.I0[p] = I0;
      }
      P.I0n[p] = I0;
    } else {  // adopt the update the last explicit step made for the position it wrote
      const int In = P.I0n[p];
      if (In != I0) P.I0[p] = In;
      I0 = In;
    }
  }
  bin_particle<ND>(P, g, tc, p, I0, valid);
  // (only a particle that is in a tile list activates nodes: one left out -- outside the node window -- takes no part)
  if (valid && (!tc.count || P.tile[p] >= 0)) N.seed[I0] = 1;
}

// The search that rides on k5_tile as a kernel of its own, launched between K3 and K5 of the folded one-rank step (async
// lists, nlps_gpu_explicit_step): closest-node update, seed and full-rank binning of the NEXT step from the position K5
// is about to write, x + d_dis, with the additions of k5_body (so I0n is the same number, bit for bit).  It visits what
// K5 visits -- the particles of this step's lists, P.tile[] >= 0 -- and moves what K5 moves (load_lme: a particle
// without a neighbourhood stays where it is and keeps its node).  I0n is written for EVERY particle (= I0 for one that is
// in no list), so the host can adopt the whole array by exchanging the two pointers.
//
// The deferred move (nlps_gpu::move_pending).  In the deferred form K5 (k5_tile_lazy<., ., false, true>) leaves x and dis
// alone, and this kernel records per particle, in moved[], the predicate it has formed anyway: "K5 moves this particle".
// K2 of the next step applies x += d_dis, dis += d_dis to every marked particle of its lists and clears the mark
// (k2_body); k_materialise_move does it for every marked particle when somebody else wants x first.
// Particles the next lists leave out (moved by this step, then outside the node window: status 16, P.tile < 0) are
// visited by no K2.  The rule: a mark that is still set when the NEXT k_search_ahead comes by -- it visits every
// particle, behind K2 of its step -- is applied here, before the new predicate is formed; K3 and K5 of that step never
// touch an unlisted particle, so d_dis is still the one the mark was made for.  A materialise in between takes them like
// any other mark.  record = 0 (the step keeps the in-place K5): the stale marks are applied, none is made.
template <int ND>
__device__ __forceinline__ void apply_move(const PView& P, int p, double* x) {  // the additions of k5_body
#pragma unroll
  for (int a = 0; a < ND; a++) {
    const double dd = PF(P, F_DDIS + a, p);
    x[a] = PF(P, F_X + a, p) + dd;
    PF(P, F_X + a, p) = x[a];
    PF(P, F_DIS + a, p) = PF(P, F_DIS + a, p) + dd;
  }
}
template <int ND>
__global__ __launch_bounds__(BLK) void k_materialise_move(PView P, unsigned char* __restrict__ moved) {
  const int p = blockIdx.x * BLK + threadIdx.x;
  if (p >= P.np || !moved[p]) return;
  double x[ND];
  apply_move<ND>(P, p, x);
  moved[p] = 0;
}
template <int ND>
__global__ __launch_bounds__(BLK) void k_search_ahead(PView P, GridD g, NView N, const uint8_t* __restrict__ rank1, TileCnt tc,
                                                      unsigned char* __restrict__ moved, int record) {
  const int p = blockIdx.x * BLK + threadIdx.x;
  int I0n = 0;
  bool binned = false;
  if (p < P.np) {
    I0n = P.I0[p];
    binned = P.tile[p] >= 0;
    const bool moves = binned && (P.mlo[p] | P.mhi[p]) != 0ull;
    if (moved) {
      if (moved[p]) {  // left out of this step's lists: see above
        double x[ND];
        apply_move<ND>(P, p, x);
      }
      moved[p] = (record && moves) ? 1 : 0;
    }
    if (moves) {
      double xn[ND], dn2 = 0.0;
#pragma unroll
      for (int a = 0; a < ND; a++) {
        const double dd = PF(P, F_DDIS + a, p);
        xn[a] = PF(P, F_X + a, p) + dd;
        const double dn = PF(P, F_DIS + a, p) + dd;
        dn2 += dsqr(dn);
      }
      if (sqrt(dn2) > 0.0) I0n = closest_node_update<ND>(g, rank1, xn, I0n);  // LME.c:924
    }
    P.I0n[p] = I0n;
  }
  bin_particle<ND>(P, g, tc, binned ? p : P.np, I0n, binned);
  if (binned && P.tile[p] >= 0) N.seed[I0n] = 1;
}

// the closest nodes k5_tile found ahead become THE closest nodes (paths whose list kernels do not do it on their way)
__global__ void k_commit_I0(int np, const int* __restrict__ I0n, int* __restrict__ I0) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < np) I0[p] = I0n[p];
}

// initialize__LME__ first loop (LME.c:63-115): element search + closest element node
template <int ND>
__global__ __launch_bounds__(BLK) void k_init_I0(PView P, GridD g, NView N, TileCnt tc) {
  const int p = blockIdx.x * BLK + threadIdx.x;
  bool valid = p < P.np;
  int bestnode = 0;
  if (valid) {
    double x[ND];
    int c[3] = {0, 0, 0};
    bool found = true;
#pragma unroll
    for (int a = 0; a < ND; a++) {
      x[a] = PF(P, F_X + a, p);
      int nc = g.n[a] - 1;
      int ci = (int)floor((x[a] - g.o[a]) / g.h);
      ci = ci < 0 ? 0 : (ci > nc - 1 ? nc - 1 : ci);
      while (ci > 0 && x[a] <= g.o[a] + g.h * (double)ci) ci--;
      while (ci < nc - 1 && x[a] > g.o[a] + g.h * (double)(ci + 1)) ci++;
      if (x[a] < g.o[a] + g.h * (double)ci || x[a] > g.o[a] + g.h * (double)(ci + 1)) found = false;
      c[a] = ci;
    }
    if (!found) {
      atomicOr(&P.status[p], ST_CONNECT);
      atomicOr(tc.gstatus, ST_CONNECT);  // the particle is not binned, so no later kernel would report it
      valid = false;
    } else {
      // connectivity chain = reverse GiD file order (Read-GID-Mesh.c:411-413): rank of corner (a,b,t)
      const int fileQ[4][2] = {{0, 0}, {1, 0}, {1, 1}, {0, 1}};
      double best = 0.0;
      int bestrank = 256;
#pragma unroll
      for (int t = 0; t < (ND == 3 ? 2 : 1); t++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          int filepos = 4 * t + q;
          int nnod = (ND == 3) ? 8 : 4;
          int rank = nnod - 1 - filepos;
          int i = c[0] + fileQ[q][0], j = c[1] + fileQ[q][1], k = c[2] + t;
          double D = 0.0, tt;
          tt = x[0] - (g.o[0] + g.h * (double)i);
          D += tt * tt;
          tt = x[1] - (g.o[1] + g.h * (double)j);
          D += tt * tt;
          if (ND == 3) {
            tt = x[ND - 1] - (g.o[2] + g.h * (double)k);
            D += tt * tt;
          }
          D = sqrt(D);
          if (bestrank == 256 || D < best || (D == best && rank < bestrank)) {
            best = D;
            bestrank = rank;
            bestnode = i + g.n[0] * (j + g.n[1] * (ND == 3 ? k : 0));
          }
        }
      P.I0[p] = bestnode;
      P.I0n[p] = bestnode;
      N.seed[bestnode] = 1;
    }
  }
  bin_particle<ND>(P, g, tc, p, bestnode, valid);
}

template <int ND>
__device__ __forceinline__ bool load_lme(const PView& P, const GridD& g, int p, Lme<ND>& c, double* lam, double& beta) {
  double x[ND];
#pragma unroll
  for (int a = 0; a < ND; a++) {
    x[a] = PF(P, F_X + a, p);
    lam[a] = PF(P, F_LAM + a, p);
  }
  beta = PF(P, F_BETA, p);
  c.geom(g, x, P.I0[p]);
  c.mlo = P.mlo[p];
  c.mhi = P.mhi[p];
  c.factors(lam, beta, g.h);
  return (c.mlo | c.mhi) != 0ull;
}

// ------------------------------------------------------------------------------------------------
// S3 (+S4): G2P of grad(dU) -> DF, F_n1, J (U-Newmark-beta.c:1064-1160 / U-Verlet.c:530-632), stress
// (Constitutive.c:18-258), P2G of the internal force (U-Newmark-beta.c:1257-1374)
// ------------------------------------------------------------------------------------------------
template <int ND>
__device__ __forceinline__ void load_block(const PView& P, int f0, int p, double* t, double& zz) {
#pragma unroll
  for (int s = 0; s < ND * ND; s++) t[s] = PF(P, f0 + s, p);
  zz = (ND == 2) ? PF(P, f0 + 4, p) : 0.0;
}
template <int ND>
__device__ __forceinline__ void store_block(const PView& P, int f0, int p, const double* t, double zz, bool with_zz) {
#pragma unroll
  for (int s = 0; s < ND * ND; s++) PF(P, f0 + s, p) = t[s];
  if (ND == 2 && with_zz) PF(P, f0 + 4, p) = zz;
}

// LAW = -1: dispatch on the particle's material at run time (mixed clouds); LAW = 0/1/2: the whole
// cloud uses that one law, so only its code (and register footprint) is compiled into the kernel.
// CEP: also keep the Drucker-Prager tangent moduli (only the implicit driver's Jacobian reads them).
// FRIC: the Matsuoka-Nakai / Lade-Duncan code is compiled in (its 5 x 5 Newton system would otherwise set the register
// budget of every other law).  A kernel without it is never launched on a cloud that holds the law: the level-B
// stress kernel exists in both forms, the fused step runs one launch per law for such a cloud (nlps_gpu_create forces
// k3_per_law, nlps_gpu_set_law_launch_mode refuses the dispatch kernel).
// LAZY (the fused explicit step): the hyperelastic laws do not store tau and W -- they are functions of F_n+1 (and J)
// alone, nothing in the step reads them back, and k_copy_n_to_n1 recomputes them with the same code from the same
// stored inputs when a level-B stage or a download asks (80 B per particle less to store in K3).
// KEEP (with LAZY; the state half of the damage step): tau and W are stored for every law -- the damage hook reads them.
template <int ND, int LAW = -1, bool CEP = false, bool FRIC = (LAW == NLPS_KLAW_FRICTIONAL), bool LAZY = false, bool KEEP = false>
__device__ __forceinline__ int stress_update(const PView& P, int p, const MatD* __restrict__ mats, const ParamsD& prm,
                                             const double* Fn1, const double* DF, double J, double* tau, int mat_idx = -1) {
  MatD m = mats[mat_idx >= 0 ? mat_idx : P.mat[p]];  // (mat_idx: the caller has read the particle's material index already)
  StressIO<ND> o;
  o.fail = 0;
  o.kappa = 0.0;
  o.eps = 0.0;
  o.cep_keep = false;
  const int law = (LAW >= 0) ? LAW : m.type;
  if (law == NLPS_MAT_NEO_HOOKEAN) {
    law_neo_hookean<ND>(m, Fn1, J, o);
  } else if (law == NLPS_MAT_HENCKY) {
    law_hencky<ND>(m, Fn1, o);
  } else {
    double be[ND * ND], bzz;
    load_block<ND>(P, fBEN(P), p, be, bzz);
    if (law == NLPS_MAT_VON_MISES) {
      o.kappa = PF(P, F_KN, p);
#pragma unroll
      for (int a = 0; a < 3; a++) o.back[a] = PF(P, F_BACK + a, p);
      law_von_mises<ND>(m, prm, DF, be, bzz, PF(P, F_EN, p), o);
#pragma unroll
      for (int a = 0; a < 3; a++) PF(P, F_BACK + a, p) = o.back[a];  // in place, like upstream (Constitutive.c:116)
    } else if (FRIC && law == NLPS_KLAW_FRICTIONAL) {
      law_frictional<ND>(m, prm, DF, be, bzz, PF(P, F_KN, p), PF(P, F_EN, p), o);
    } else {
      law_drucker_prager<ND>(m, prm, DF, be, bzz, PF(P, F_KN, p), PF(P, F_EN, p), o);
    }
    store_block<ND>(P, fBEN1(P), p, o.be, o.be_zz, true);
    PF(P, LAZY ? F_KN : F_KN1, p) = o.kappa;  // fused step: straight to the n slots (read above, by this thread)
    PF(P, LAZY ? F_EN : F_EN1, p) = o.eps;
    if (CEP && !(FRIC && o.cep_keep)) {
#pragma unroll
      for (int q = 0; q < ND * ND; q++) PF(P, F_CEP + q, p) = o.cep[q];
    }
  }
#pragma unroll
  for (int s = 0; s < ND * ND; s++) tau[s] = o.tau[s];
  if (!(LAZY && !KEEP && (law == NLPS_MAT_NEO_HOOKEAN || law == NLPS_MAT_HENCKY))) {
    store_block<ND>(P, F_TAU, p, o.tau, o.tau_zz, true);
    PF(P, F_W, p) = o.W;
  }
  return o.fail ? ST_CONSTITUTIVE : 0;
}

// B[i][m] = sign * V0 * sum_jq tau[i][j] DF^-T[j][q] J^-1[q][m];  f_A = p_A * B l_A
template <int ND>
__device__ __forceinline__ bool force_operator(double* B, const double* tau, const double* DF, const double* Jm1,
                                               double V0, double sign) {
  NLPS_FP_CONTRACT
  double DFt[ND * ND], DFmT[ND * ND], M1[ND * ND];
#pragma unroll
  for (int i = 0; i < ND; i++)
#pragma unroll
    for (int j = 0; j < ND; j++) DFt[i * ND + j] = DF[j * ND + i];
  if (!inverse<ND>(DFmT, DFt)) return false;  // compute_adjunt__TensorLib__, TensorLib.c:829-905
#pragma unroll
  for (int i = 0; i < ND; i++)
#pragma unroll
    for (int q = 0; q < ND; q++) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < ND; j++) s += tau[i * ND + j] * DFmT[j * ND + q];
      M1[i * ND + q] = s;
    }
#pragma unroll
  for (int i = 0; i < ND; i++)
#pragma unroll
    for (int m = 0; m < ND; m++) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < ND; q++) s += M1[i * ND + q] * Jm1[q * ND + m];
      B[i * ND + m] = -sign * V0 * s;  // grad p_a = -p_a J^-1 l_a
    }
  return true;
}

// ------------------------------------------------------------------------------------------------
// Eigenerosion: the damage part of __nodal_internal_forces, U-Newmark-beta.c:1313-1331 ->
// compute_damage__Constitutive__ (Constitutive.c:385-435) -> Eigenerosion__Constitutive__ (EigenErosion.c:29-117).
// The epsilon-neighbourhood Beps[p] (Beps.c:16-80: particles q whose closest node lies in the 1-ring of I0_p, within
// Ceps * DeltaX of p) is not stored: the particles are sorted by closest node once per call (first/last = the run of
// every node in `sorted`) and every particle walks the <= 3^d runs around its own closest node.  x_GC does not change
// between the search and the force stage, so this is the list the reference built after its search.  A particle that
// has not moved by more than 1e-6 since the start keeps the list of the initialisation (Beps.c:30-36): it walks the
// same runs of the SNAPSHOT taken before the first search (positions and closest nodes of Initialize_Beps = true,
// fields F_X0 / F_I00, tables first0 / last0 / sorted0) -- the same members, wherever they have moved since.
// ------------------------------------------------------------------------------------------------
__global__ void k_node_ranges(int np, const unsigned long long* __restrict__ keys, int* __restrict__ first,
                              int* __restrict__ last) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
  const unsigned long long k = keys[i];
  if (i == 0 || keys[i - 1] != k) first[k] = i;
  if (i == np - 1 || keys[i + 1] != k) last[k] = i + 1;
}

__global__ void k_beps_snapshot(PView P, int ND) {  // Initialize_Beps = true: the configuration the frozen lists belong to
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P.np) return;
  for (int a = 0; a < ND; a++) PF(P, F_X0 + a, p) = PF(P, F_X + a, p);
  PF(P, F_I00, p) = (double)P.I0[p];
}
__global__ void k_beps_keys0(PView P, unsigned long long* __restrict__ keys, int* __restrict__ vals) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P.np) return;
  keys[p] = (unsigned long long)(long long)PF(P, F_I00, p);
  vals[p] = p;
}

// The same tables without a sort, for the explicit step with the damage hooks (nlps_gpu_set_explicit_damage): three
// passes, no keys.  (1) every particle takes its rank inside its node from the node's counter; (2) every node takes the
// run [first, last) of its count from ONE cursor -- a wave scans its 64 counts and asks for their sum with one atomic, so
// the runs of a wave's nodes are contiguous and the order of the waves' blocks in `sorted` is whatever the atomics made
// it (nothing reads across runs) -- and puts its counter back to zero; (3) every particle goes to first[node] + rank.
// SNAP: the key is the closest node of the snapshot (F_I00) instead of the current one.
// The step's own per-node counters (node_cnt_d / nrank_d of the canonical tile lists) are not used: the search that
// rides on K5 only counts, and k_fill_orders counts the counters down to zero again while it hands out the ranks
// (TileCnt::defer), so neither the counts nor a stored rank outlive the list stage; asking K5 for full ranks instead
// would put the returning atomic back into the kernel it was taken out of.
template <bool SNAP>
__device__ __forceinline__ int run_node(const PView& P, int p, int nn) {
  const int A = SNAP ? (int)PF(P, F_I00, p) : P.I0[p];
  return (A >= 0 && A < nn) ? A : -1;
}
template <bool SNAP>
__global__ __launch_bounds__(BLK) void k_run_count(PView P, int nn, int* __restrict__ cnt, int* __restrict__ rank,
                                                   int* __restrict__ cursor) {
  const int p = blockIdx.x * BLK + threadIdx.x;
  if (p == 0) *cursor = 0;  // (read by k_run_first only, the next launch of the stream)
  if (p >= P.np) return;
  const int A = run_node<SNAP>(P, p, nn);
  rank[p] = A >= 0 ? atomicAdd(&cnt[A], 1) : -1;
}
__global__ __launch_bounds__(BLK) void k_run_first(int nn, int* __restrict__ cnt, int* __restrict__ cursor,
                                                   int* __restrict__ first, int* __restrict__ last) {
  const int A = blockIdx.x * BLK + threadIdx.x;  // (no early return: every lane takes part in the wave's scan)
  const int lane = threadIdx.x & 63;
  const int c = A < nn ? cnt[A] : 0;
  int incl = c;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off);
    if (lane >= off) incl += v;
  }
  const int tot = __shfl(incl, 63);
  int base = 0;
  if (lane == 0 && tot > 0) base = atomicAdd(cursor, tot);
  base = __shfl(base, 0);
  if (A < nn) {
    cnt[A] = 0;  // ready for the next count
    first[A] = base + incl - c;
    last[A] = base + incl;
  }
}
template <bool SNAP>
__global__ __launch_bounds__(BLK) void k_run_fill(PView P, int nn, const int* __restrict__ first, const int* __restrict__ rank,
                                                  int* __restrict__ sorted) {
  const int p = blockIdx.x * BLK + threadIdx.x;
  if (p >= P.np) return;
  const int A = run_node<SNAP>(P, p, nn), r = rank[p];
  if (A < 0 || r < 0) return;
  const int s = first[A] + r;
  if (s < P.np) sorted[s] = p;
}
// Deterministic mode with the damage hooks (nlps_gpu_set_deterministic_damage), behind k_run_fill: the order INSIDE every
// run becomes ascending slot index -- a function of the particle arrays alone, the definition k_tile_order<., true> uses
// for its exact ranks -- whatever ranks the returning atomic of the count handed out.  Where a run lies in `sorted` still
// depends on the cursor's atomic; nothing reads across runs.  One thread per node, insertion sort in place: a run holds
// the particles of one closest node (4 to 8, some tens in a dense cloud) and arrives nearly sorted.  No local array.
__global__ __launch_bounds__(BLK) void k_run_sort(int nn, int np, const int* __restrict__ first, const int* __restrict__ last,
                                                  int* __restrict__ sorted) {
  const int A = blockIdx.x * BLK + threadIdx.x;
  if (A >= nn) return;
  const int lo = max(first[A], 0), hi = min(last[A], np);
  for (int i = lo + 1; i < hi; i++) {
    const int v = sorted[i];
    int j = i;
    while (j > lo) {
      const int u = sorted[j - 1];
      if (u <= v) break;
      sorted[j] = u;
      j--;
    }
    sorted[j] = v;
  }
}
// developer read-out (nlps_gpu_debug_damage_runs): the node every slot is counted under by k_run_count<SNAP>
template <bool SNAP>
__global__ __launch_bounds__(BLK) void k_debug_slot_node(PView P, int nn, int* __restrict__ key) {
  const int p = blockIdx.x * BLK + threadIdx.x;
  if (p < P.np) key[p] = run_node<SNAP>(P, p, nn);
}
// the damage part of the roll behind K5 (U-Newmark-beta.c:1950-1956; k_roll does it for level B)
__global__ __launch_bounds__(BLK) void k_damage_roll(PView P) {
  const int p = blockIdx.x * BLK + threadIdx.x;
  if (p >= P.np) return;
  PF(P, F_DMG, p) = PF(P, F_DMG1, p);
  if (P.softening) PF(P, F_STRF, p) = PF(P, F_STRF1, p);
}

// first0 / last0 / sorted0: the same tables for the closest nodes of the snapshot (nullptr: no frozen lists)
template <int ND>
__global__ __launch_bounds__(BLK) void k_damage(PView P, GridD g, const MatD* __restrict__ mats, const int* __restrict__ first,
                                                const int* __restrict__ last, const int* __restrict__ sorted,
                                                const int* __restrict__ first0, const int* __restrict__ last0,
                                                const int* __restrict__ sorted0, double DeltaX) {
  const int p = blockIdx.x * BLK + threadIdx.x;
  if (p >= P.np) return;
  constexpr int T = (ND == 2) ? 5 : 9;
  const double Dn = PF(P, F_DMG, p);
  double Dn1 = PF(P, F_DMG1, p);
  double tau[ND * ND], z, w[3] = {0.0, 0.0, 0.0}, v[ND * ND];
  load_block<ND>(P, F_TAU, p, tau, z);
  sym_eigen<ND>(w, v, tau);  // ascending like dsyev: w[0] is the smallest principal Kirchhoff stress
  if (Dn < 1.0 && w[0] > 0.0) {
    const MatD m = mats[P.mat[p]];
    const double eps = m.Ceps * DeltaX;
    // a particle whose total displacement is <= 1e-6 keeps the list it had (Beps.c:30-36): the one of the snapshot,
    // i.e. the particles around its closest node THEN that were within eps of it THEN -- wherever they are now
    double xp[ND], d2p = 0.0;
#pragma unroll
    for (int a = 0; a < ND; a++) d2p += dsqr(PF(P, F_DIS + a, p));
    const bool frozen = first0 && !(sqrt(d2p) > 0.000001);
    const int fx = frozen ? F_X0 : F_X;
    if (frozen) {
      first = first0;
      last = last0;
      sorted = sorted0;
    }
#pragma unroll
    for (int a = 0; a < ND; a++) xp[a] = PF(P, fx + a, p);
    const double V_p = PF(P, F_VOL0, p) * PF(P, F_JN1, p);
    double sum_V = V_p, sum_VW = V_p * PF(P, F_W, p);
    const int I0 = frozen ? (int)PF(P, F_I00, p) : P.I0[p];
    const int i0 = I0 % g.n[0], j0 = (I0 / g.n[0]) % g.n[1], k0 = I0 / (g.n[0] * g.n[1]);
    for (int dk = (ND == 3 ? -1 : 0); dk <= (ND == 3 ? 1 : 0); dk++)
      for (int dj = -1; dj <= 1; dj++)
        for (int di = -1; di <= 1; di++) {
          const int i = i0 + di, j = j0 + dj, k = k0 + dk;
          if (i < 0 || i >= g.n[0] || j < 0 || j >= g.n[1] || (ND == 3 && (k < 0 || k >= g.n[2]))) continue;
          const int A = i + g.n[0] * (j + g.n[1] * k);
          for (int s = first[A]; s < last[A]; s++) {
            const int q = sorted[s];
            double d2 = 0.0;
#pragma unroll
            for (int a = 0; a < ND; a++) {
              const double d = xp[a] - PF(P, fx + a, q);
              d2 += d * d;
            }
            if (sqrt(d2) <= eps) {  // q = p included, like the reference's list
              const double V_q = PF(P, F_VOL0, q) * PF(P, F_JN1, q);
              sum_V += V_q;
              if (PF(P, F_DMG, q) < 1.0) sum_VW += V_q * PF(P, F_W, q);
            }
          }
        }
    const double G_p = (m.Ceps * DeltaX / sum_V) * sum_VW;
    if (G_p > m.Gf) {
      Dn1 = 1.0;
      PF(P, F_DMG1, p) = 1.0;
    }
  }
  const double sc = 1.0 - Dn1;  // kirchhoff_p[i] *= (1 - Damage_n1[p]), in place (:1321-1330)
#pragma unroll
  for (int s = 0; s < T; s++) PF(P, F_TAU + s, p) = PF(P, F_TAU + s, p) * sc;
}

// ------------------------------------------------------------------------------------------------
// Eigensoftening: the same hook with Driver_EigenSoftening -> Eigensoftening__Constitutive__
// (EigenSoftening.c:27-163), restated AS WRITTEN: "first principal" value = eigval[0] of the ascending dsyev order (the
// smallest, :60, :106); the neighbour loop ASSIGNS its term (no +=, :118); StrainF_n and StrainF_n1 are one array
// (Constitutive.c:418-419).
// The reference's loop runs one particle after the other and scales every Kirchhoff stress in place while later
// particles still read it; two passes give the same numbers in parallel:
//   pass 1 (per particle, no neighbour): the smallest principal Kirchhoff stress T0 of the UNSCALED stress, and the
//           damage update of the second branch (:146-160), which reads the particle's own strain and history only;
//   pass 2 (first branch, :71-144): mass sum over the epsilon-neighbourhood and the ONE neighbour term that survives the
//           assignment of :118 -- the first particle of compute_Beps's walk (chain of NodalLocality_0[I0_p], inside a
//           node descending particle index, Beps.c:49-70) with Damage_n < 1 -- whose stress counts scaled by
//           (1 - Damage_n1) iff its index in the CALLER's order is below p's (it came earlier in the reference's loop);
//           then every stress is scaled in place (U-Newmark-beta.c:1321-1330).
// Lists: with this driver Beps is never initialised (U-Newmark-beta.c:182 tests Driver_EigenErosion only), a particle
// whose total displacement is <= 1e-6 has an empty list (Beps.c:30-36), any other the list of its current position.
// ------------------------------------------------------------------------------------------------
template <int ND>
__device__ __forceinline__ double almansi_min_principal(const double* F) {  // eulerian_almansi__Particles__ + eigval[0]
  double b[ND * ND], bm1[ND * ND], e[ND * ND], w[3] = {0.0, 0.0, 0.0}, v[ND * ND];
#pragma unroll
  for (int i = 0; i < ND; i++)
#pragma unroll
    for (int j = 0; j < ND; j++) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < ND; k++) a += F[i * ND + k] * F[j * ND + k];
      b[i * ND + j] = a;
    }
  inverse<ND>(bm1, b);
#pragma unroll
  for (int i = 0; i < ND; i++)
#pragma unroll
    for (int j = 0; j < ND; j++) e[i * ND + j] = 0.5 * ((i == j ? 1.0 : 0.0) - bm1[i * ND + j]);
  sym_eigen<ND>(w, v, e);
  return w[0];
}
template <int ND>
__global__ __launch_bounds__(BLK) void k_soften_pass1(PView P, const MatD* __restrict__ mats, double* __restrict__ T0) {
  const int p = blockIdx.x * BLK + threadIdx.x;
  if (p >= P.np) return;
  double tau[ND * ND], z, w[3] = {0.0, 0.0, 0.0}, v[ND * ND];
  load_block<ND>(P, F_TAU, p, tau, z);
  sym_eigen<ND>(w, v, tau);
  T0[p] = w[0];
  const double Dn = PF(P, F_DMG, p), sf = PF(P, F_STRF1, p);
  if (Dn == 0.0 && w[0] > 0.0) return;  // first branch: pass 2
  if (Dn != 1.0 && sf > 0.0) {          // :146-160
    double F[ND * ND], fz;
    load_block<ND>(P, fFN1(P), p, F, fz);
    const MatD m = mats[P.mat[p]];
    const double aux = (almansi_min_principal<ND>(F) - sf) * m.heps / m.wcrit;
    const double mx = aux > Dn ? aux : Dn;
    PF(P, F_DMG1, p) = 1.0 < mx ? 1.0 : mx;
  }
}
template <int ND>
__global__ __launch_bounds__(BLK) void k_soften_pass2(PView P, GridD g, const MatD* __restrict__ mats, const int* __restrict__ first,
                                                      const int* __restrict__ last, const int* __restrict__ sorted,
                                                      const uint8_t* __restrict__ rank1, const int* __restrict__ orig,
                                                      const double* __restrict__ T0, double DeltaX) {
  const int p = blockIdx.x * BLK + threadIdx.x;
  if (p >= P.np) return;
  constexpr int T = (ND == 2) ? 5 : 9;
  const double Dn = PF(P, F_DMG, p), T0p = T0[p];
  if (Dn == 0.0 && T0p > 0.0) {
    const MatD m = mats[P.mat[p]];
    const double m_p = PF(P, F_MASS, p);
    double sum_m = m_p, term = m_p * T0p;
    double xp[ND], d2p = 0.0;
#pragma unroll
    for (int a = 0; a < ND; a++) {
      xp[a] = PF(P, F_X + a, p);
      d2p += dsqr(PF(P, F_DIS + a, p));
    }
    if (sqrt(d2p) > 0.000001) {  // Beps.c:30-36 (lists are never initialised with this driver: empty otherwise)
      const double eps = m.Ceps * DeltaX;
      const int I0 = P.I0[p], op = orig[p];
      int ijk[3] = {I0 % g.n[0], (I0 / g.n[0]) % g.n[1], I0 / (g.n[0] * g.n[1])};
      const uint8_t* rk = rank1 + 27 * class3_of<ND>(g, ijk);
      long long bestkey = 0x7fffffffffffffffll;
      int bestq = -1;
      for (int dk = (ND == 3 ? -1 : 0); dk <= (ND == 3 ? 1 : 0); dk++)
        for (int dj = -1; dj <= 1; dj++)
          for (int di = -1; di <= 1; di++) {
            const int i = ijk[0] + di, j = ijk[1] + dj, k = ijk[2] + dk;
            if (i < 0 || i >= g.n[0] || j < 0 || j >= g.n[1] || (ND == 3 && (k < 0 || k >= g.n[2]))) continue;
            const int A = i + g.n[0] * (j + g.n[1] * k);
            const long long nodekey = (long long)rk[(di + 1) + 3 * (dj + 1) + 9 * (dk + 1)] << 32;
            for (int s = first[A]; s < last[A]; s++) {
              const int q = sorted[s];
              double d2 = 0.0;
#pragma unroll
              for (int a = 0; a < ND; a++) {
                const double d = xp[a] - PF(P, F_X + a, q);
                d2 += d * d;
              }
              if (sqrt(d2) <= eps) {  // q = p included, like the reference's list
                sum_m += PF(P, F_MASS, q);
                if (PF(P, F_DMG, q) < 1.0) {
                  // the walk visits the nodes in chain order and a node's particles in descending caller index; the
                  // reference's assignment keeps the FIRST such particle of the walk
                  const long long key = nodekey + (long long)(0x7fffffff - orig[q]);
                  if (key < bestkey) {
                    bestkey = key;
                    bestq = q;
                  }
                }
              }
            }
          }
      if (bestq >= 0) {
        const double sc = (orig[bestq] < op) ? (1.0 - PF(P, F_DMG1, bestq)) : 1.0;  // scaled in place already, or not yet
        term = PF(P, F_MASS, bestq) * (T0[bestq] * sc);
      }
    }
    const double Teps = term / sum_m;
    if (Teps > m.ft) {
      double F[ND * ND], fz;
      load_block<ND>(P, fFN1(P), p, F, fz);
      PF(P, F_STRF1, p) = almansi_min_principal<ND>(F);
    }
  }
  const double sc = 1.0 - PF(P, F_DMG1, p);  // kirchhoff_p[i] *= (1 - Damage_n1[p]), in place (:1321-1330)
#pragma unroll
  for (int s = 0; s < T; s++) PF(P, F_TAU + s, p) = PF(P, F_TAU + s, p) * sc;
}

// __constitutive_update (U-Newmark-beta.c:1208-1242)
template <int ND, bool FRIC>
__global__ __launch_bounds__(BLK) void k_stress(PView P, const MatD* __restrict__ mats, ParamsD prm,
                                                int* __restrict__ gstatus) {
  int p = blockIdx.x * BLK + threadIdx.x;
  if (p >= P.np) return;
  if (P.erosion && PF(P, F_DMG, p) == 1.0) {  // failed particle: U-Newmark-beta.c:1218-1224
    PF(P, F_W, p) = 0.0;
    return;
  }
  double Fn1[ND * ND], DF[ND * ND], tau[ND * ND], z;
  load_block<ND>(P, fFN1(P), p, Fn1, z);
  if (mats[P.mat[p]].type == NLPS_KLAW_FLUID) {  // Constitutive.c:84-108: F_n1, dt_F_n1, J_n1 -> Stress, nothing else
    double dFn1[ND * ND], tzz;
    load_block<ND>(P, F_DTFN1, p, dFn1, z);
    if (law_newtonian_fluid<ND>(mats[P.mat[p]], Fn1, dFn1, PF(P, F_JN1, p), tau, tzz)) {
      store_block<ND>(P, F_TAU, p, tau, tzz, true);
    } else {
      atomicOr(&P.status[p], ST_CONSTITUTIVE);
      atomicOr(gstatus, ST_CONSTITUTIVE);
    }
    return;
  }
  load_block<ND>(P, F_DF, p, DF, z);
  int st = stress_update<ND, -1, true, FRIC>(P, p, mats, prm, Fn1, DF, PF(P, F_JN1, p), tau);
  if (st) {
    atomicOr(&P.status[p], st);
    atomicOr(gstatus, st);
  }
}

// __update_particles_internal_variables (U-Newmark-beta.c:1917-1978)
// After explicit steps the n+1 slots of F and b_e hold the previous step's values (rolled by renaming);
// the reference's copy semantics (n+1 == n after the roll) are restored on demand, before any level-B stage
// or download looks at them.
// KEEP: the last step was an explicit step with the damage hooks, which stored tau (scaled by the hook) and W itself.
template <int ND, bool KEEP = false>
__global__ __launch_bounds__(BLK) void k_copy_n_to_n1(PView P, const MatD* __restrict__ mats) {
  int p = blockIdx.x * BLK + threadIdx.x;
  if (p >= P.np) return;
  constexpr int T = (ND == 2) ? 5 : 9;
  {
    // DF of the last explicit step, which K3 did not store: the n slot holds F_n+1 of that step, the n+1 slot still
    // the F_n it started from (the roll is a renaming), so DF = F_n+1 F_n^-1 on the d x d block (the 2-D zz slot of DF
    // stays 1, compute-Strains.c:20-44 never touches it)
    double Fnew[ND * ND], Fold[ND * ND], inv[ND * ND], z;
    load_block<ND>(P, fFN(P), p, Fnew, z);
    load_block<ND>(P, fFN1(P), p, Fold, z);
    if (inverse<ND>(inv, Fold)) {
#pragma unroll
      for (int i = 0; i < ND; i++)
#pragma unroll
        for (int j = 0; j < ND; j++) {
          double a2 = 0.0;
#pragma unroll
          for (int k2 = 0; k2 < ND; k2++) a2 += Fnew[i * ND + k2] * inv[k2 * ND + j];
          PF(P, F_DF + i * ND + j, p) = a2;
        }
    }
    // Kirchhoff stress and energy of the hyperelastic laws, which the fused step did not store (stress_update LAZY):
    // the same functions of the same stored F_n+1 and J
    const MatD m = mats[P.mat[p]];
    if (!KEEP && (m.type == NLPS_MAT_NEO_HOOKEAN || m.type == NLPS_MAT_HENCKY)) {
      StressIO<ND> o;
      o.fail = 0;
      if (m.type == NLPS_MAT_NEO_HOOKEAN) law_neo_hookean<ND>(m, Fnew, PF(P, F_JN, p), o);
      else law_hencky<ND>(m, Fnew, o);
      store_block<ND>(P, F_TAU, p, o.tau, o.tau_zz, true);
      PF(P, F_W, p) = o.W;
    }
  }
#pragma unroll
  for (int s = 0; s < T; s++) {
    PF(P, fFN1(P) + s, p) = PF(P, fFN(P) + s, p);
    PF(P, fBEN1(P) + s, p) = PF(P, fBEN(P) + s, p);
  }
  PF(P, F_JN1, p) = PF(P, F_JN, p);
  PF(P, F_KN1, p) = PF(P, F_KN, p);
  PF(P, F_EN1, p) = PF(P, F_EN, p);
  PF(P, F_RHO, p) = PF(P, F_RHOJ, p) / PF(P, F_JN, p);
}

// first explicit step after the upload or after level-B stages: the invariant of the density update (F_RHOJ)
__global__ __launch_bounds__(BLK) void k_init_rhoj(PView P) {
  int p = blockIdx.x * BLK + threadIdx.x;
  if (p < P.np) PF(P, F_RHOJ, p) = PF(P, F_RHO, p) * PF(P, F_JN, p);
}

template <int ND>
__global__ __launch_bounds__(BLK) void k_roll(PView P) {
  int p = blockIdx.x * BLK + threadIdx.x;
  if (p >= P.np) return;
  double J = PF(P, F_JN1, p);
  PF(P, F_JN, p) = J;
  PF(P, F_RHO, p) = PF(P, F_MASS, p) / (PF(P, F_VOL0, p) * J);
  PF(P, F_KN, p) = PF(P, F_KN1, p);
  PF(P, F_EN, p) = PF(P, F_EN1, p);
  if (P.erosion) PF(P, F_DMG, p) = PF(P, F_DMG1, p);  // U-Newmark-beta.c:1950-1953
  if (P.softening) PF(P, F_STRF, p) = PF(P, F_STRF1, p);  // :1954-1956
  constexpr int T = (ND == 2) ? 5 : 9;
#pragma unroll
  for (int s = 0; s < T; s++) {
    PF(P, fBEN(P) + s, p) = PF(P, fBEN1(P) + s, p);
    PF(P, fFN(P) + s, p) = PF(P, fFN1(P) + s, p);
    PF(P, F_DTFN + s, p) = PF(P, F_DTFN1 + s, p);
  }
}

// After explicit steps of a fluid cloud (nlps_gpu_set_explicit_fluid) the step's rate sits in dt_F_n alone, where K3 put
// it: the reference's copy semantics (dt_F_n1 == dt_F_n after the roll) are restored on demand, with k_copy_n_to_n1, for
// the fluid particles; those of other laws keep what they had.
template <int ND>
__global__ __launch_bounds__(BLK) void k_roll_rate(PView P, const MatD* __restrict__ mats) {
  int p = blockIdx.x * BLK + threadIdx.x;
  if (p >= P.np || mats[P.mat[p]].type != NLPS_KLAW_FLUID) return;
#pragma unroll
  for (int s = 0; s < ND * ND; s++) PF(P, F_DTFN1 + s, p) = PF(P, F_DTFN + s, p);
}

// ------------------------------------------------------------------------------------------------
// nodal kernels (grid numbering)
// ------------------------------------------------------------------------------------------------
// Dirichlet sets of one step for the nodal kernel: set i fixes the directions `bits[i]` of its nodes at v[i]; a node
// finds its sets in the bit mask bcmask[A] (built once per set of lists, ensure_bcs), later sets override earlier ones
// like the sequence of k_bc launches they replace (one launch per set and step: 5 us each).
#define NLPS_MAX_BC_INLINE 8
struct BcStep {
  int n;
  int dim[NLPS_MAX_BC_INLINE], bits[NLPS_MAX_BC_INLINE];
  double v[NLPS_MAX_BC_INLINE][3];
};
__global__ void k_bc_mark(const int* __restrict__ nodes, int n, unsigned bit, unsigned* __restrict__ mask) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < n) atomicOr(&mask[nodes[q]], bit);
}

template <int ND>
__global__ void k_nodal_dU(int n0, int nnodes, int n0b, int nnodesb, NView N, const unsigned* __restrict__ bcmask,
                           BcStep bc) {  // U-Verlet.c:357-362 + impose_Dirichlet_Boundary_Conditions :455-527
  int A = blockIdx.x * blockDim.x + threadIdx.x;  // two node ranges: [n0, n0+nnodes) and [n0b, n0b+nnodesb)
  if (A >= nnodes + nnodesb) return;
  A = A < nnodes ? n0 + A : n0b + (A - nnodes);
  double M = N.nm[(size_t)A * (1 + ND)];
  // an active node no particle lists (narrow LME kernels: the 1-ring activation reaches further than the cut-off
  // radius) has M = 0: its value is 0 like VecPointwiseDivide's in the maintained driver, never 0/0 (the gather
  // kernels read every window slot, a NaN there would poison the zero-weighted non-members)
  const bool active = N.active[A];
  bool act = active && M != 0.0;
  double val[ND];
  bool fix[ND];
#pragma unroll
  for (int a = 0; a < ND; a++) {
    val[a] = act ? N.nm[(size_t)A * (1 + ND) + 1 + a] / M : 0.0;
    fix[a] = false;
  }
  const unsigned bm = (bcmask && active) ? bcmask[A] : 0u;
  if (bm) {
    for (int i = 0; i < bc.n; i++) {
      if (!((bm >> i) & 1u)) continue;
#pragma unroll
      for (int k = 0; k < ND; k++)
        if (k < bc.dim[i] && ((bc.bits[i] >> k) & 1)) {
          val[k] = bc.v[i][k];
          fix[k] = true;
        }
    }
  }
#pragma unroll
  for (int a = 0; a < ND; a++) {
    N.dU[(size_t)A * ND + a] = val[a];
    if (fix[a]) N.fixed[(size_t)A * ND + a] = 1;
  }
}

template <int ND>
__global__ void k_bc(const int* __restrict__ nodes, int n, int dim, int dirbits, double v0, double v1, double v2,
                     NView N, int r0, int r1, int inside) {  // impose_Dirichlet_Boundary_Conditions, U-Verlet.c:455-527
  int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  int A = nodes[q];
  if (((A >= r0 && A < r1) ? 1 : 0) != inside) return;  // node-range filter (interior / ghost-band passes)
  if (!N.active[A]) return;
  double v[3] = {v0, v1, v2};
#pragma unroll
  for (int k = 0; k < ND; k++)
    if (k < dim && ((dirbits >> k) & 1)) {
      N.dU[(size_t)A * ND + k] = v[k];
      N.fixed[(size_t)A * ND + k] = 1;
    }
}

// clr_* (search fused into k5_tile): this kernel runs in front of it and resets what that search accumulates into -- the
// seeds and per-node counters of the nodes it visits, and (first launch of the stage only) the tile counters
template <int ND>
__global__ void k_nodal_accel(int n0, int nnodes, int n0b, int nnodesb, NView N, double g0, double g1, double g2,
                              int clr_seed, int* __restrict__ clr_node_cnt, int* __restrict__ clr_tile_count, int ntiles) {  // U-Verlet.c:947-957
  int A = blockIdx.x * blockDim.x + threadIdx.x;
  if (clr_tile_count)
    for (int t = A; t < ntiles; t += gridDim.x * blockDim.x) clr_tile_count[t] = 0;
  if (A >= nnodes + nnodesb) return;
  A = A < nnodes ? n0 + A : n0b + (A - nnodes);
  if (clr_seed) {
    N.seed[A] = 0;
    if (clr_node_cnt) clr_node_cnt[A] = 0;
  }
  double M = N.nm[(size_t)A * (1 + ND)];
  bool act = N.active[A] && M != 0.0;  // massless active node: see k_nodal_dU
  double gv[3] = {g0, g1, g2};
#pragma unroll
  for (int a = 0; a < ND; a++) {
    size_t o = (size_t)A * ND + a;
    double f = N.force[o];
    bool fx = N.fixed[o];
    N.accel[o] = (act && !fx) ? gv[a] + f / M : 0.0;
    N.reaction[o] = (act && fx) ? f : 0.0;
  }
}

// masked <-> grid numbering
__global__ void k_expand(double* __restrict__ grid, const double* __restrict__ masked, const int* __restrict__ n2m,
                         int nnodes, int nf) {
  int A = blockIdx.x * blockDim.x + threadIdx.x;
  if (A >= nnodes) return;
  int m = n2m[A];
  for (int f = 0; f < nf; f++) grid[(size_t)A * nf + f] = (m >= 0) ? masked[(size_t)m * nf + f] : 0.0;
}

// k_expand of the residual call, which also resets the force accumulator of the node window (one launch for the two)
__global__ void k_expand_reset(double* __restrict__ grid, const double* __restrict__ masked, const int* __restrict__ n2m,
                               int nnodes, int nf, double* __restrict__ zero, int n0, int nwn) {
  int A = blockIdx.x * blockDim.x + threadIdx.x;
  if (A >= nnodes) return;
  int m = n2m[A];
  for (int f = 0; f < nf; f++) grid[(size_t)A * nf + f] = (m >= 0) ? masked[(size_t)m * nf + f] : 0.0;
  if (A >= n0 && A < n0 + nwn)
    for (int f = 0; f < nf; f++) zero[(size_t)A * nf + f] = 0.0;
}

// k_expand_reset of a cloud that holds the fluid law: also the nodal velocity increment of
// __compute_nodal_velocity_increments (U-Newmark-beta.c:1834-1870), dU_dt = alpha_4 dU + (alpha_5 - 1) Un_dt + alpha_6 Un_dt2,
// in grid numbering (the second gather window of k3_tile MODE 4)
__global__ void k_expand_reset_rates(double* __restrict__ grid, double* __restrict__ gridv, const double* __restrict__ masked,
                                     const double* __restrict__ v, const double* __restrict__ a, double a4, double a5m1, double a6,
                                     const int* __restrict__ n2m, int nnodes, int nf, double* __restrict__ zero, int n0, int nwn) {
  int A = blockIdx.x * blockDim.x + threadIdx.x;
  if (A >= nnodes) return;
  int m = n2m[A];
  for (int f = 0; f < nf; f++) {
    const size_t i = (size_t)(m >= 0 ? m : 0) * nf + f;
    grid[(size_t)A * nf + f] = (m >= 0) ? masked[i] : 0.0;
    gridv[(size_t)A * nf + f] = (m >= 0) ? a4 * masked[i] + a5m1 * v[i] + a6 * a[i] : 0.0;
  }
  if (A >= n0 && A < n0 + nwn)
    for (int f = 0; f < nf; f++) zero[(size_t)A * nf + f] = 0.0;
}

// mode 0: out = grid[A*gstride + goff + (bcast?0:f)]
// mode 1: out += ... skipping fixed dofs (d2m == -1)
// mode 2: out = (fixed ? 0 : grid) / div[idx]
__global__ void k_compact(double* __restrict__ out, const double* __restrict__ grid, const int* __restrict__ n2m,
                          const int* __restrict__ d2m, const double* __restrict__ div, int nnodes, int nf, int gstride,
                          int goff, int bcast, int mode) {
  int A = blockIdx.x * blockDim.x + threadIdx.x;
  if (A >= nnodes) return;
  int m = n2m[A];
  if (m < 0) return;
  for (int f = 0; f < nf; f++) {
    size_t idx = (size_t)m * nf + f;
    double v = grid[(size_t)A * gstride + goff + (bcast ? 0 : f)];
    if (mode == 0) out[idx] = v;
    else if (mode == 1) {
      if (d2m[idx] != -1) out[idx] += v;
    } else {
      const double dv = div[idx];  // VecPointwiseDivide (U-Newmark-beta.c:695-696): 0 where the lumped mass is 0
      out[idx] = dv != 0.0 ? ((d2m[idx] == -1) ? 0.0 : v) / dv : 0.0;
    }
  }
}

// ---- exclusive scan of byte flags -> (flag ? running index : -1); 1024 items per block
__global__ void k_scan_count(const unsigned char* __restrict__ flags, int n, int invert, int* __restrict__ bsum) {
  __shared__ int sh[256];
  int base = blockIdx.x * 1024 + threadIdx.x * 4, c = 0;
  for (int q = 0; q < 4; q++)
    if (base + q < n) c += ((flags[base + q] != 0) != (invert != 0));
  sh[threadIdx.x] = c;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) bsum[blockIdx.x] = sh[0];
}
__global__ void k_scan_top(int* __restrict__ bsum, int nb, int* __restrict__ total) {
  // one 1024-thread block; each thread owns a contiguous chunk
  __shared__ int sh[1024];
  int chunk = (nb + 1023) / 1024;
  int lo = threadIdx.x * chunk, hi = min(nb, lo + chunk), c = 0;
  for (int q = lo; q < hi; q++) c += bsum[q];
  sh[threadIdx.x] = c;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    int v = ((int)threadIdx.x >= off) ? sh[threadIdx.x - off] : 0;
    __syncthreads();
    sh[threadIdx.x] += v;
    __syncthreads();
  }
  int run = sh[threadIdx.x] - c;
  for (int q = lo; q < hi; q++) {
    int v = bsum[q];
    bsum[q] = run;
    run += v;
  }
  if (threadIdx.x == 1023) *total = sh[1023];
}
__global__ void k_scan_write(const unsigned char* __restrict__ flags, int n, int invert, const int* __restrict__ bsum,
                             int* __restrict__ out) {
  __shared__ int sh[256];
  int base = blockIdx.x * 1024 + threadIdx.x * 4;
  int f[4], c = 0;
  for (int q = 0; q < 4; q++) {
    f[q] = (base + q < n) ? ((flags[base + q] != 0) != (invert != 0)) : 0;
    c += f[q];
  }
  sh[threadIdx.x] = c;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    int v = ((int)threadIdx.x >= off) ? sh[threadIdx.x - off] : 0;
    __syncthreads();
    sh[threadIdx.x] += v;
    __syncthreads();
  }
  int run = bsum[blockIdx.x] + sh[threadIdx.x] - c;
  for (int q = 0; q < 4; q++)
    if (base + q < n) {
      out[base + q] = f[q] ? run : -1;
      run += f[q];
    }
}
// get_active_dofs__MeshTools__ marking loop (Nodes-Tools.c:96-135) in masked numbering
__global__ void k_mark_fixed_masked(const int* __restrict__ nodes, int n, int dim, int dirbits, int ndof,
                                    const int* __restrict__ n2m, unsigned char* __restrict__ fixedm) {
  int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  int m = n2m[nodes[q]];
  if (m < 0) return;
  for (int k = 0; k < dim; k++)
    if ((dirbits >> k) & 1) fixedm[(size_t)m * ndof + k] = 1;
}

#include "nlps_tile_kernels.hpp"

// The two kernels between the search and the tile lists in one launch (they do not depend on each other and both are
// too small to fill the chip: 8 us + 10 us -> 10 us): workgroup 0 = exclusive scan of the tile counts + work lists
// (tile_scan_block), the others = 1-ring activation of NT nodes each.  NT = 256: the launch on the side stream (async
// lists), whose workgroups have to find room on compute units that K5's workgroups keep filled -- a workgroup of 16
// waves does not, and waited for K5 to drain (profiles/r08_async_lists.md).
// Layer tables of the canonical tile lists: layer r of a tile = the r-th particle of every node that has one, nodes in
// lattice order.  The nodes of a tile form NNW words of 64 (3-D: 4^3 nodes = 1 word, 2-D: 16^2 = 4 words);
// mask[tile][r][w] = the nodes of word w that reach layer r, base[tile][r][w] = list offset of the first of them.  A
// particle of node l with rank r inside its node (bin_particle) sits at
// start[tile] + base[r][l / 64] + popcount(mask[r][l / 64] & below(l % 64)).  base[tile][0][0] < 0: some node is
// deeper than LMAX, the tile keeps the order of the binning.  Replaces the per-tile counting sort (k_tile_order,
// 13.6 us) outside deterministic mode.
struct TileTab {
  static constexpr int LMAX = 32;
  int nt[3];
  const int* node_cnt;
  unsigned long long* mask;
  int* base;
};
template <int ND>
struct TileTabCfg {
  static constexpr int NN = (ND == 3) ? TileCfg<3>::TB * TileCfg<3>::TB * TileCfg<3>::TB : TileCfg<2>::TB * TileCfg<2>::TB;
  static constexpr int NNW = NN / 64;
};

template <int ND, int NT = 1024>
__global__ __launch_bounds__(NT) void k_dilate_scan(int n0, int nnodes, GridD g, NView N, TileScanArgs ts,
                                                      int* __restrict__ foreign, int* __restrict__ foreign_host, TileTab tab,
                                                      int clear_nodal) {
  if (blockIdx.x == 0) {
    if (foreign && threadIdx.x < 64) {  // this step's count of displaced particles (bin_particle) -> pinned host word
      int v = foreign[32 * threadIdx.x];
      foreign[32 * threadIdx.x] = 0;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
      if (threadIdx.x == 0) *foreign_host = v;
    }
    tile_scan_block<NT>(ts);
    return;
  }
  const int nbd = (nnodes + NT - 1) / NT;  // workgroups of the activation
  if ((int)blockIdx.x <= nbd) {
    const int A = ((int)blockIdx.x - 1) * NT + (int)threadIdx.x;
    if (A < nnodes) {
      dilate_node<ND>(n0 + A, g, N);
      if (clear_nodal) {  // (k_step_clear's nodal part, when that kernel has nothing else to do: the search ran ahead)
        const size_t B = (size_t)n0 + A;
#pragma unroll
        for (int a = 0; a < 1 + ND; a++) N.nm[B * (1 + ND) + a] = 0.0;
#pragma unroll
        for (int a = 0; a < ND; a++) {
          N.force[B * ND + a] = 0.0;
          N.fixed[B * ND + a] = 0;
        }
      }
    }
    return;
  }
  // layer tables of the canonical tile lists (TileTab), one wave per tile
  constexpr int TB = TileCfg<ND>::TB, NNW = TileTabCfg<ND>::NNW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = ((int)blockIdx.x - 1 - nbd) * (NT / 64) + wave;
  if (q >= ts.n) return;
  const int tile = ts.tile0 + q;
  const int tx = tile % tab.nt[0], ty = (tile / tab.nt[0]) % tab.nt[1], tz = tile / (tab.nt[0] * tab.nt[1]);
  int c[NNW], maxc = 0;
#pragma unroll
  for (int w = 0; w < NNW; w++) {
    const int l = w * 64 + lane;
    const int bx = l % TB, by = (l / TB) % TB, bz = l / (TB * TB);
    const int i = tx * TB + bx, j = ty * TB + by, k = (ND == 3) ? tz * TB + bz : 0;
    const bool in = i < g.n[0] && j < g.n[1] && (ND == 2 || k < g.n[2]);
    c[w] = in ? tab.node_cnt[i + g.n[0] * (j + g.n[1] * k)] : 0;
    maxc = max(maxc, c[w]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) maxc = max(maxc, __shfl_xor(maxc, off));
  unsigned long long* tm = tab.mask + (size_t)tile * TileTab::LMAX * NNW;
  int* tb = tab.base + (size_t)tile * TileTab::LMAX * NNW;
  if (maxc > TileTab::LMAX) {  // deeper than the table: this tile keeps the order of the binning
    if (lane == 0) tb[0] = -1;
    return;
  }
  int run = 0;
  for (int r = 0; r < maxc; r++) {
#pragma unroll
    for (int w = 0; w < NNW; w++) {
      const unsigned long long m = __ballot(c[w] > r);
      if (lane == 0) {
        tm[r * NNW + w] = m;
        tb[r * NNW + w] = run;
      }
      run += (int)__popcll(m);
    }
  }
  if (maxc == 0 && lane == 0) tb[0] = 0;
}
// Both tile lists in one pass over the particles: order = as binned (position = rank of the wave-aggregated tile atomic:
// runs of memory-consecutive particles), order2 = canonical (TileTab).
// cursor != nullptr: the binning only counted (TileCnt::defer) -- the position inside the tile list comes from a cursor
// that starts at the list's first slot (tile_scan_block), one wave-aggregated atomic per (wave, tile), lanes in memory
// order; the rank inside the closest node counts the node's counter DOWN (every value c - 1 .. 0 once; the counter is
// back at zero for the next binning, the layer tables of this step were made from it before this kernel).
template <int ND>
__global__ __launch_bounds__(BLK) void k_fill_orders(int np, const int* __restrict__ tile, const int* __restrict__ rank,
                                                     const int* __restrict__ nrank, int* __restrict__ I0a,
                                                     const int* __restrict__ I0n,
                                                     const int* __restrict__ start, GridD g, TileTab tab,
                                                     int* __restrict__ order, int* __restrict__ order2,
                                                     int* __restrict__ cursor, int* __restrict__ node_cnt) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int t = p < np ? tile[p] : -1;
  int pos = -1, I0 = 0, r = 0;
  if (t >= 0) {  // the search was done ahead by k5_tile: its closest node becomes THE closest node (a particle that is in
    I0 = I0a[p];  // no list was not visited: its I0n equals I0)
    if (I0n) {
      const int In = I0n[p];
      if (In != I0) I0a[p] = I0 = In;
    }
    // (asked for first: its round trip runs under the one of the list cursor below)
    if (cursor) r = atomicSub(&node_cnt[I0], 1) - 1;
  }
  if (cursor) {  // (every lane of the wave takes part)
    const int lane = threadIdx.x & 63;
    int my_leader = lane, my_off = 0, my_cnt = 0;
    bool todo_l = t >= 0;
    while (true) {  // (groups by ballots, then one atomic per group in ONE instruction: see bin_particle)
      const u64 todo = __ballot(todo_l);
      if (!todo) break;
      const int leader = __ffsll((unsigned long long)todo) - 1;
      const int t0 = __shfl(t, leader);
      const bool mine = todo_l && (t == t0);
      const u64 same = __ballot(mine);
      if (mine) {
        my_leader = leader;
        my_off = (int)__popcll(same & ((1ull << lane) - 1ull));
        my_cnt = (int)__popcll(same);
        todo_l = false;
      }
    }
    int base = 0;
    if (t >= 0 && lane == my_leader) base = atomicAdd(&cursor[t], my_cnt);
    base = __shfl(base, my_leader);
    if (t >= 0) pos = base + my_off;
  }
  if (t < 0) return;
  constexpr int TB = TileCfg<ND>::TB;
  const int s0 = start[t];
  if (!cursor) pos = s0 + rank[p];
  order[pos] = p;
  constexpr int NNW = TileTabCfg<ND>::NNW;
  const int* tb = tab.base + (size_t)t * TileTab::LMAX * NNW;
  if (tb[0] < 0) {
    order2[pos] = p;
    return;
  }
  if (!cursor) r = nrank[p];
  const int bx = (I0 % g.n[0]) % TB, by = ((I0 / g.n[0]) % g.n[1]) % TB, bz = (ND == 3) ? (I0 / (g.n[0] * g.n[1])) % TB : 0;
  const int l = bx + TB * (by + TB * bz), w = l >> 6;
  const unsigned long long m = tab.mask[((size_t)t * TileTab::LMAX + r) * NNW + w];
  order2[s0 + tb[r * NNW + w] + (int)__popcll(m & ((1ull << (l & 63)) - 1ull))] = p;
}
#include "nlps_tangent_kernels.hpp"
#include "nlps_tangent_operator.hpp"
#include "nlps_tangent_csr.hpp"
#include "nlps_tangent_bsr.hpp"
#include "nlps_krylov.hpp"
#include "nlps_minres.hpp"
#include "nlps_eigen.hpp"
#include "nlps_newton.hpp"
#include "nlps_record.hpp"
#include "nlps_snapshot.hpp"

// ------------------------------------------------------------------------------------------------
// physical re-sort of the particle SoA (maintenance, every few dozen steps): restores the
// (tile of I0, corner type, I0 in tile) memory order that makes waves hit distinct window slots
// ------------------------------------------------------------------------------------------------
template <int ND>
__global__ void k_sort_keys(PView P, GridD g, TileCnt tc, unsigned long long* __restrict__ keys, int* __restrict__ vals,
                            const unsigned char* __restrict__ leaving, const MatD* __restrict__ mats) {
  int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P.np) return;
  if (leaving && leaving[p]) {  // migration: the emigrants sort behind everything that stays
    keys[p] = ~0ull;
    vals[p] = p;
    return;
  }
  constexpr int TB = TileCfg<ND>::TB;
  const int I0 = P.I0[p];
  int ijk[3] = {I0 % g.n[0], (I0 / g.n[0]) % g.n[1], I0 / (g.n[0] * g.n[1])};
  unsigned long long kt = 0, kn = 0, kc = 0, mt = 1, mn = 1, mc = 1;
#pragma unroll
  for (int a = 0; a < ND; a++) {
    const double xi = (PF(P, F_X + a, p) - g.o[a]) / g.h;
    int c = (int)floor(xi);
    c = c < 0 ? 0 : (c > g.n[a] - 2 ? g.n[a] - 2 : c);
    kt += mt * (unsigned long long)(ijk[a] / TB);
    mt *= (unsigned long long)tc.nt[a];
    kn += mn * (unsigned long long)(ijk[a] % TB);
    mn *= TB;
    kc += mc * (unsigned long long)(ijk[a] > c ? 1 : 0);
    mc *= 2;
  }
  (void)mats;  // (tile, law, corner type, node) was tried for clouds with several laws: K3's per-law launches load
               // coalesced, but K2's waves lose their distinct closest nodes (0.25 -> 0.35 ms) -- net loss
  keys[p] = (kt * mc + kc) * mn + kn;
  vals[p] = p;
}
// ---- particle migration between slab ranks: packed rows of MIG_WORDS 8-byte words:
// the NFD fields in canonical order (F_n / b_e,n in their n slots whatever the current renaming), then
// I0, material, NumberNodes, status, caller index, global id (as integers in words), then the two mask words.
static constexpr int MIG_WORDS = NFD + 8;
__device__ __forceinline__ int mig_field(const PView& P, int f) {  // canonical field -> current physical field
  if (!P.flip) return f;
  if (f >= F_FN && f < F_FN + 9) return f + (F_FN1 - F_FN);
  if (f >= F_FN1 && f < F_FN1 + 9) return f - (F_FN1 - F_FN);
  if (f >= F_BEN && f < F_BEN + 9) return f + (F_BEN1 - F_BEN);
  if (f >= F_BEN1 && f < F_BEN1 + 9) return f - (F_BEN1 - F_BEN);
  return f;
}
template <int ND>
__global__ void k_mig_flag(PView P, GridD g, int keep_lo, int keep_hi, unsigned char* __restrict__ leaving,
                           int* __restrict__ slot, int* __restrict__ counts) {
  int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P.np) return;
  const int layer = P.I0[p] / (g.nnodes / g.n[ND - 1]);
  const int dir = layer < keep_lo ? 1 : (layer > keep_hi ? 2 : 0);
  leaving[p] = (unsigned char)dir;
  if (dir) slot[p] = atomicAdd(&counts[dir - 1], 1);
}
__global__ void k_mig_pack(PView P, const unsigned char* __restrict__ leaving, const int* __restrict__ slot,
                           const int* __restrict__ perm, const int* __restrict__ gid, double* __restrict__ down,
                           double* __restrict__ up) {
  int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P.np || !leaving[p]) return;
  double* row = (leaving[p] == 1 ? down : up) + (size_t)slot[p] * MIG_WORDS;
  for (int f = 0; f < NFD; f++) row[f] = PF(P, mig_field(P, f), p);
  long long* w = reinterpret_cast<long long*>(row + NFD);
  w[0] = P.I0[p];
  w[1] = P.mat[p];
  w[2] = P.nn[p];
  w[3] = P.status[p];
  w[4] = perm[p];
  w[5] = gid[p];
  w[6] = (long long)P.mlo[p];
  w[7] = (long long)P.mhi[p];
}
__global__ void k_mig_unpack(PView P, int first, int n, const double* __restrict__ rows, int* __restrict__ perm,
                             int* __restrict__ gid, unsigned char* __restrict__ leaving) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int p = first + j;
  const double* row = rows + (size_t)j * MIG_WORDS;
  for (int f = 0; f < NFD; f++) PF(P, mig_field(P, f), p) = row[f];
  const long long* w = reinterpret_cast<const long long*>(row + NFD);
  P.I0[p] = (int)w[0];
  P.I0n[p] = (int)w[0];
  P.mat[p] = (int)w[1];
  P.nn[p] = (int)w[2];
  P.status[p] = (int)w[3];
  perm[p] = (int)w[4];
  gid[p] = (int)w[5];
  P.mlo[p] = (u64)w[6];
  P.mhi[p] = (u64)w[7];
  leaving[p] = 0;
}

template <class T>
__global__ void k_copy(T* __restrict__ out, const T* __restrict__ in, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[i];
}

// all particle fields of the re-sort in one launch: thread = new slot, blockIdx.y = group of GATHER_FIELDS fields
static constexpr int GATHER_FIELDS = 8;
__global__ void k_gather_fields(double* __restrict__ out, const double* __restrict__ in, const int* __restrict__ idx,
                                int n, size_t npad, int nf) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t j = (size_t)idx[i];
  const int f0 = blockIdx.y * GATHER_FIELDS, f1 = min(nf, f0 + GATHER_FIELDS);
  for (int f = f0; f < f1; f++) out[(size_t)f * npad + i] = in[(size_t)f * npad + j];
}

// the live components of the re-sort as ONE launch: blockIdx.y = group of GATHER_FIELDS entries of a list of components
struct FieldList {
  int n;
  unsigned char f[128];
};
__global__ void k_gather_field_list(double* __restrict__ out, const double* __restrict__ in, const int* __restrict__ idx,
                                    int n, size_t npad, FieldList fl) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t j = (size_t)idx[i];
  const int q0 = blockIdx.y * GATHER_FIELDS, q1 = min(fl.n, q0 + GATHER_FIELDS);
  for (int q = q0; q < q1; q++) {
    const size_t f = fl.f[q];
    out[f * npad + i] = in[f * npad + j];
  }
}

// the integer arrays of the particles (closest nodes, material, list length, status, permutation, ids; the two mask
// words) through one scratch block: one gather launch and one copy-back launch instead of two per array
struct SmallArrays {
  int* ia[7];
  unsigned long long* ua[2];
};
__global__ void k_gather_small(SmallArrays A, const int* __restrict__ idx, int n, size_t npad, int* __restrict__ si,
                               unsigned long long* __restrict__ su) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int j = idx[i];
#pragma unroll
  for (int a = 0; a < 7; a++) si[(size_t)a * npad + i] = A.ia[a][j];
#pragma unroll
  for (int a = 0; a < 2; a++) su[(size_t)a * npad + i] = A.ua[a][j];
}
__global__ void k_copy_small(SmallArrays A, int n, size_t npad, const int* __restrict__ si,
                             const unsigned long long* __restrict__ su) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
#pragma unroll
  for (int a = 0; a < 7; a++) A.ia[a][i] = si[(size_t)a * npad + i];
#pragma unroll
  for (int a = 0; a < 2; a++) A.ua[a][i] = su[(size_t)a * npad + i];
}

template <class T>
__global__ void k_gather(T* __restrict__ out, const T* __restrict__ in, const int* __restrict__ idx, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[idx[i]];
}

template <class T>
__global__ void k_scatter(T* __restrict__ out, const T* __restrict__ in, const int* __restrict__ idx, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[idx[i]] = in[i];
}

// Periodic re-sort with the tile lists as the permutation: the particles that are in NO list of the step that built the
// lists (flagged by its search instead of binned: failed element search, stencil outside the node window) go behind them.
// Membership is read off the lists themselves -- P.tile[] may already belong to the NEXT step (the search k5_tile runs
// ahead), so "tile < 0" would miss a particle that was listed and is flagged now, and count one twice.
__global__ void k_mark_listed(int np, const int* __restrict__ last_start, const int* __restrict__ last_count,
                              const int* __restrict__ order, unsigned char* __restrict__ listed) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = min(np, *last_start + *last_count);
  if (q < total) listed[order[q]] = 1;
}
__global__ void k_append_unlisted(int np, const unsigned char* __restrict__ listed, const int* __restrict__ last_start,
                                  const int* __restrict__ last_count, int* __restrict__ counter, int* __restrict__ order) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= np || listed[p]) return;
  const int pos = *last_start + *last_count + atomicAdd(counter, 1);
  if (pos < np) order[pos] = p;
}

__global__ void k_node_tables(int nn, const double* __restrict__ h_avg, double gamma_lme, double neg_log_tol_zero,
                              double4* __restrict__ out) {
  const int A = blockIdx.x * blockDim.x + threadIdx.x;
  if (A >= nn) return;
  const double hv = h_avg[A];
  const double beta = gamma_lme / (hv * hv);
  const double Ra = sqrt(neg_log_tol_zero / beta);
  out[A] = make_double4(beta, sqrt_threshold(Ra), Ra, 0.0);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct BcDev {
  const int* host_nodes;
  int n;
  DevBuf<int> dnodes;
};

struct nlps_gpu {
  int nd, T;
  GridD g;
  ParamsD prm;
  nlps_params hprm;
  int nsteps;
  hipStream_t stream;
  bool own_stream;
  std::string err;

  // The device arrays below are owned here (DevBuf frees them when the handle is deleted); P, N and the other views that
  // kernels take by value hold pointers borrowed from them, filled where the arrays are made.
  PView P;
  DevBuf<double> Pd;  // P.d
  DevBuf<int> P_I0, P_I0n, P_mat, P_nn, P_status, P_tile, P_rank;
  DevBuf<u64> P_mlo, P_mhi;
  std::vector<int> perm;  // sorted slot -> caller's particle index
  NView N;
  DevBuf<unsigned char> N_seed;  // (active, fixed, nm and force belong to the tile-list set: ListSet)
  DevBuf<double> N_dU, N_accel, N_reaction;
  DevBuf<double> h_avg_d;
  DevBuf<double4> beta_t2_d;  // NView::beta_t2
  DevBuf<MatD> mats_d;
  int nmats;
  std::vector<int> mat_klaw;  // kernel law of every material (what nlps_gpu_set_explicit_fbar checks its flags against)
  int uniform_law;  // material law shared by every particle, or -1
  int law_present;  // bit l set: some material follows law l
  bool k3_per_law = true;  // several laws: one K3 launch per law (few mixed tiles) or one run-time-dispatch kernel
  DevBuf<uint8_t> rank1_d;
  nlps_host::StencilTables tab;

  // masks
  DevBuf<int> n2m_d, d2m_d;
  // nlps_gpu_set_node_numbering: lattice node of file node A (canon_d), and the scratch of the file-order mask scan
  DevBuf<int> canon_d;
  DevBuf<unsigned char> mask_flags_d;
  DevBuf<int> mask_idx_d;
  DevBuf<unsigned char> fixedm_d;
  DevBuf<int> bsum_d, total_d, gstatus_d;
  int nactive, nfree;
  bool masks_valid;
  bool binned;  // order[] / tile tables describe the current I0s
  // The last kernel of the fused explicit step (k5_tile<., ., true>) does the search of the NEXT step for the particles
  // it moves.  searched: the closest nodes already belong to the current positions (a search that follows must not
  // update them a second time, LME.c:927-929); ahead: seeds, tile counters, per-particle tile / rank and per-node
  // counters of that search are in place, the next explicit step starts at the activation kernel.
  bool searched = false, ahead = false;
  int lazy_nodal = 1;  // the folded explicit step (k3_tile_lazy / k5_tile_lazy): 1 below 2 M particles, 2 always, 0 never (NLPS_LAZY_NODAL)
  int ncu = 256;
  bool nodal_stale = false;
  BcStep last_bc;
  const unsigned* last_bm = nullptr;
  double last_gv[3] = {0, 0, 0};
  // migration
  DevBuf<int> gid_d;               // global particle id (default: the caller's index)
  DevBuf<unsigned char> leaving_d;  // 0 stay, 1 leaves downwards, 2 upwards (between select and commit)
  DevBuf<int> mig_slot_d, mig_cnt_d;
  DevBuf<double> mig_down_d, mig_up_d;
  int mig_n[2] = {0, 0};
  bool mig_selected = false;
  bool migrated = false;             // downloads are ordered by ascending global id from now on
  bool rolled = false;  // explicit steps renamed the n/n+1 tensor slots since the last materialise_roll()
  bool level_b_fields = false;  // C_ep / rate tensors hold data (a level-B constitutive or rate call was made)

  // scratch nodal arrays
  DevBuf<double> gridA;  // [nnodes][2*ND] general purpose
  DevBuf<double> gridB;  // [nnodes][ND] x4 for kinetics
  DevBuf<double> maskedA;

  std::vector<BcDev> bcs;
  DevBuf<unsigned> bcmask_d;  // per node: bit i = member of Dirichlet set i (<= NLPS_MAX_BC_INLINE sets; k_nodal_dU)

  // periodic physical re-sort
  DevBuf<int> perm_d;     // sorted slot -> caller's particle index (device copy of perm)
  bool perm_dirty;        // device perm newer than the host copy
  int resort_every, steps_since_sort;
  DevBuf<unsigned long long> skey_d, skey2_d;
  DevBuf<int> sval_d, sval2_d;
  DevBuf<char> cub_tmp;
  size_t cub_tmp_bytes = 0;
  DevBuf<double> gather_tmp;  // [npad] scratch for the gather of the integer arrays
  DevBuf<double> Pd_alt;      // twin of Pd, target of the re-sort (allocated at the first one)

  // per-step tile binning
  int nt[3], ntiles;
  DevBuf<int> tile_count_d;
  DevBuf<int> tile_count2_d;  // the counters the search ahead (k5_tile) fills while tile_count_d still sizes the lists in use
  // canonical lists from per-node counters (TileTab): node_cnt[nnodes], nrank[npad], layer tables [ntiles][LMAX]
  DevBuf<int> node_cnt_d, nrank_d, tabo_d;
  DevBuf<int> tile_cursor_d;  // [ntiles + 1] list cursors of the deferred ranks (TileCnt::defer, k_fill_orders)
  bool ranks_deferred = false;   // the search riding on K5 only counted in the step before: the lists of this step take their ranks from cursors
  DevBuf<unsigned long long> tabm_d;
  // adaptive re-sort (nlps_gpu_set_adaptive_resort): see TileCnt::home.  The count of displaced particles of a step
  // reaches the pinned host word at the end of its search stage; explicit_step adds count / NumGP to `debt` every
  // step and re-sorts ahead of the interval when the debt since the last re-sort exceeds `adaptive_resort`
  DevBuf<int> home_d, foreign_d;
  Pinned<int> foreign_h;
  // pinned landing word of check_status (one asynchronous copy + one synchronise per check); through its device alias a
  // kernel at the end of a call can leave the status there itself
  Pinned<int> status_h;
  bool rehome = true;
  double adaptive_resort = 0.8, debt = 0.0;  // default budget: about one re-sort's cost
  int adaptive_min_steps = 4;
  bool beps_snapshot = false;  // F_X0 / F_I00 hold the configuration of Initialize_Beps = true
  bool explicit_fluid = false;  // nlps_gpu_set_explicit_fluid: the explicit step of a cloud that holds the fluid law

  // Feature state.  Each type below is "off" as default-constructed; a setter builds a value and assigns it behind the
  // synchronise it performs anyway, a drop assigns {}.
  //
  // Caller's index -> memory slot, the inverse of perm_d, for whoever addresses particles by the caller's numbering: the
  // explicit loads, the probes of the step record, the snapshot pack.  Their setters reserve it (reserve_inv_perm: no
  // step allocates), inv_perm() rebuilds it when a renumbering has made it stale (slots_renumbered) and it lives as long
  // as the handle: 4 bytes per particle beside a field block of NFD doubles.
  struct InvPerm {
    DevBuf<int> d;  // [npad]
    bool stale = true;
  } inv;
  // The Neumann contours of the explicit step (nlps_gpu_set_explicit_loads): one entry per contour particle
  // in the caller's contour order -- caller's index, contour number, A0 (3-D) -- and the traction vector of every
  // (step, contour) with the carry-over resolved.
  struct Loads {
    int n = 0, nloads = 0;
    double thickness = 1.0;
    DevBuf<int> ids, load;
    DevBuf<double> a0, T;
  } loads;
  // (not part of a set of loads: the developer switch between the two work mappings of the kernel, and the bracket of
  // the kernel -- timing only, slot 7 of nlps_gpu_get_timing -- which is made once and outlives every set)
  bool loads_lane_map = false;
  hipEvent_t loads_ev[2] = {};
  // The step record (nlps_gpu_set_step_record; kernels in nlps_record.hpp).  `on` is all a step looks at
  // with no record set.  The ring `rows` holds `capacity` rows of `row` doubles; row number g (0-based since the set)
  // lives in slot g % capacity.  The probes find their particles through inv_perm().
  struct StepRecord {
    int on = 0;
    int every = 1, capacity = 0, nsets = 0, nprobes = 0, row = 0, probe_doubles = 0;
    unsigned fields = 0;
    long long total = 0;
    double time = 0.0;
    DevBuf<double> rows, part;  // [capacity][row], [REC_NQ][blocks of k_rec_particles <= REC_MAX_BLOCKS]
    DevBuf<int> probes;         // [nprobes] caller's indices
  } rec;
  // The particle snapshot (nlps_gpu_set_snapshots; kernel in nlps_snapshot.hpp).  Per slot one staging block
  // on the device and its pinned twin, `bytes` each, made by the setter for `cap` particles; the pack kernel runs on the
  // handle's stream, the one copy of a slot on `stream` -- a stream of the snapshots' own: `side` is joined back into the
  // handle's stream by every async step, which would then wait for the copy.
  struct SnapSlot {
    DevBuf<double> dev;
    Pinned<double> pin;
    hipEvent_t packed = nullptr, copied = nullptr;  // behind the pack on the handle's stream; behind the copy on the snapshots'
    int state = 0;                                  // 0 free, 1 begun (in flight or waiting for its release)
    int tag = 0, np = 0;
    SnapSlot() = default;
    SnapSlot(SnapSlot&& o) noexcept { *this = std::move(o); }
    SnapSlot& operator=(SnapSlot&& o) noexcept {  // (a swap: what this one held goes with o)
      dev.swap(o.dev), pin.swap(o.pin), std::swap(packed, o.packed), std::swap(copied, o.copied);
      std::swap(state, o.state), std::swap(tag, o.tag), std::swap(np, o.np);
      return *this;
    }
    ~SnapSlot() {
      if (packed) (void)hipEventDestroy(packed);
      if (copied) (void)hipEventDestroy(copied);
    }
    hipError_t create(size_t words) {
      hipError_t e = dev.reserve(words);
      if (e == hipSuccess) e = pin.alloc(words);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&packed, hipEventDisableTiming);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&copied, hipEventDisableTiming);
      return e;
    }
  };
  struct Snapshots {
    SideStream stream;  // (first: assigning or destroying a Snapshots waits for the copies in flight before a slot is freed)
    int slots = 0, cap = 0;
    unsigned fields = 0;
    size_t bytes = 0;
    SnapSlot slot[NLPS_SNAP_MAX_SLOTS];
  } snap;
  // The pack kernel runs one thread per caller's index through inv_perm(): gathered reads, coalesced writes, 0.33 against
  // 0.40 ms at 1 M particles for one thread per memory slot, which nlps_gpu_debug_option "snapshot_by_caller" 0 keeps for
  // comparison (a developer switch like loads_lane_map: it outlives every set).
  bool snap_by_caller = true;
  // The node runs of the damage hooks.  The explicit step with the hooks (nlps_gpu_set_explicit_damage) builds them without
  // a sort (k_run_count / k_run_first / k_run_fill) into tables of its own -- the level-B force stage rebuilds its b_* tables
  // with its sorts every call.  *0: the tables of the snapshot's closest nodes, made once and again after a re-sort has
  // renumbered the slots.  The fused damage residual (nlps_gpu_set_implicit_damage) uses the same tables; the runs of the
  // current closest nodes are built at the first evaluation and reused while nothing has moved, reordered or re-listed
  // particles (gen == tan_gen).
  struct DamageRuns {
    DevBuf<int> b_first, b_last;              // level B, eigenerosion: run of every node in the I0-sorted particle list
    DevBuf<int> b_first0, b_last0, b_sorted0;  // the same for the snapshot's closest nodes
    unsigned long long gen = 0;
    int builds = 0, fused_evals = 0;  // developer read-out (nlps_gpu_debug_damage_counters)
    DevBuf<int> cnt, cursor, rank;    // [nnodes], [1], [npad]
    DevBuf<int> first, last, sorted;  // [nnodes], [nnodes], [npad]
    DevBuf<int> first0, last0, sorted0;
    bool tables0 = false;
    bool tables = false;  // the runs of the current closest nodes have been built since the last drop (read-out only)
    // Run tables built in arrival order are never summed over in the deterministic mode, and sorted ones are not kept for
    // the atomic path either: both switches drop every cached table.  The buffers stay.
    void drop() { gen = 0, tables0 = tables = false; }
  } dmg;
  // F-bar on lattice-cell patches inside the explicit step (nlps_gpu_set_explicit_fbar).  F / J: Fbar_n
  // [T][npad] and Jbar_n [npad] of every particle, by memory slot: they travel with every re-sort (resort gathers them
  // into the twins and swaps).  sums / pid: the patch sums and the patch of every particle of the step in flight.
  struct Fbar {
    bool on = false;
    int block[3] = {1, 1, 1}, np[3] = {1, 1, 1};
    size_t npatch = 0;
    DevBuf<double> F, J, F_alt, J_alt, sums, alpha;
    DevBuf<int> pid;
  } fbar;
  bool explicit_damage = false, implicit_damage = false;
  // nlps_gpu_set_deterministic_damage: in deterministic mode the runs are sorted behind k_run_fill (k_run_sort), the force
  // half runs one wave per tile into slabs (k3f_wave) and det_implicit admits the damage cloud
  bool det_damage = false;
  bool rolled_keep = false;  // `rolled`, and the last step stored tau and W itself (k_copy_n_to_n1 KEEP)
  bool rolled_rate = false;  // `rolled`, and the last step left the fluid particles' rate in dt_F_n alone (k_roll_rate)
  DevBuf<double> slab_d;    // P2G window slabs [ntiles][slab_n][fields][NWA] (TileD::slab), deterministic mode only: sized by the
                            // explicit step and, for the largest user of the implicit path, by det_prepare
  bool deterministic = false;
  bool lists_exact = false;  // the canonical tile lists are the exact ones (k_tile_order<., true>): a function of the particle
                             // arrays alone.  Lists built outside the deterministic mode take their ranks from binning atomics.
  int band_lo = -(1 << 30), band_hi = 1 << 30;  // ghost bands: layers <= band_lo and >= band_hi are shared with neighbours
  int overlap = 0;          // halo exchanges: 0 blocking in place; 1 behind the interior tiles of the NEXT stage (split
                            // launches, two-phase callback); 2 behind the interior tiles of the SAME launch (library RCCL only)
  DevBuf<unsigned long long> phase_d;
  DevBuf<double> vec_d;  // scratch pool for host vectors of the a21 per-dof updates
  // nlps_gpu_lagrangian_evaluation with host vectors: device copies of Un_dt, Un_dt2, M, which do not change between the
  // evaluations of one SNES solve (NLPS_LAGR_SAME_STEP reuses them: two transfers per evaluation instead of five)
  DevBuf<double> lagr_d;
  bool lagr_valid = false;
  // tangent assembly, allocated on first use
  DevBuf<double> kst_d;               // [nnodes][S][d*d]
  DevBuf<unsigned char> ktouched_d;   // [nnodes][S]
  DevBuf<int> kcnt_d, koffs_d;  // visited blocks per row node, exclusive scan
  DevBuf<int> khead_d, kng_d;   // group heads of the I0-sorted particle list, group count
  DevBuf<char> kscan_tmp;
  size_t kscan_bytes = 0;
  long long knnz_blocks = -1;
  double tan_alpha4 = 0.0;  // alpha_4 of the fluid law's tangent (nlps_gpu_set_tangent_alpha4; 0 = quasi-static)
  bool tangent_grouped = true;  // one workgroup per closest node (false: one wave per particle, kept for comparison)
  bool tangent_symmetric = true;  // Neo-Hookean clouds: only the upper half of every row is assembled (nlps_gpu_debug_option "tangent_symmetric")
  bool ktan_sym = false;          // how the last nlps_gpu_tangent_assemble filled the stencil array (nlps_gpu_tangent_coo mirrors the rest)
  // matrix-free tangent (nlps_gpu_tangent_operator), allocated on first use.  tan_gen counts the calls that move, reorder
  // or re-list particles (tan_stale); the operator is valid while top_gen == tan_gen.
  DevBuf<double> top_d;  // Dh [d^4][top_np]
  DevBuf<double> top_m;  // alpha_1 M snapshot, masked [N_A d] (valid when top_mass)
  DevBuf<double> top_g;  // grid scratch [nnodes][d^2]: x and K x (2 d fields) or the diagonal blocks (d^2)
  DevBuf<double> top_b;  // staging of nlps_gpu_tangent_block_diagonal for host destinations [N_A d^2]
  int top_np = 0;
  bool top_mass = false, top_dir = false;
  unsigned long long tan_gen = 1, top_gen = 0;  // top_gen 0: no operator yet
  const char* tan_why = "";
  // the tangent in CSR (nlps_gpu_tangent_csr_pattern / nlps_gpu_tangent_csr, nlps_tangent_csr.hpp), allocated on first
  // use.  The pattern belongs to one linearisation: csr_serial is the top_serial it was built from (0: none).
  DevBuf<double> csr_e;      // E [np][d^4], particles in the order by closest node (like csr_f and csr_mk)
  DevBuf<double> csr_f;      // separable factors and position [np][6 d]
  DevBuf<unsigned long long> csr_mk;  // membership masks [np][2]
  DevBuf<int> csr_run;       // run starts [nnodes + 1]
  DevBuf<unsigned long long> csr_mask;  // visited column offsets of every row node [nnodes][2 | 12]
  DevBuf<int> csr_cnt, csr_off;         // blocks per masked node and their exclusive scan [N_A + 1]
  unsigned long long csr_serial = 0;
  long long csr_blocks = 0;
  // the same tangent in block CSR (nlps_gpu_tangent_bsr_pattern / nlps_gpu_tangent_bsr, nlps_tangent_bsr.hpp): the records,
  // runs and masks above are shared (csr_rec_serial: the top_serial they were built from, whichever pattern call built
  // them); of its own only the counts of the kind asked for
  unsigned long long csr_rec_serial = 0, bsr_serial = 0;
  DevBuf<int> bsr_cnt, bsr_off;  // the upper form: blocks per masked node's block row (and, behind them, one flag: some
                                 // row's upper blocks are not its offsets >= 0, a caller's numbering) [N_A + 2]; their
                                 // exclusive scan [N_A + 1].  The full form reads csr_cnt and csr_off
  long long bsr_blocks = 0;
  int bsr_kind = 0;
  bool bsr_half = false;         // the upper form walks the kept half only (k_tanbsr_rows<ND, true>)
  // device GMRES (nlps_gpu_tangent_solve, nlps_krylov.hpp), allocated on first use and kept (they only grow).  The
  // preconditioner belongs to one linearisation: top_serial counts the successful nlps_gpu_tangent_operator calls
  // (top_gen does not move when the caller re-linearises without moving particles), ksp_pc_serial says which one
  // ksp_pc was built from.
  unsigned long long top_serial = 0, ksp_pc_serial = 0;
  int ksp_pc_kind = -1;
  int ksp_type = NLPS_KSP_TYPE_GMRES;  // nlps_gpu_set_linear_solver: which Krylov method nlps_gpu_tangent_solve runs
  DevBuf<double> ksp_pc;    // [N_A d^2]: the inverted blocks (PBJACOBI) or reciprocals on the block diagonals (JACOBI)
  DevBuf<double> ksp_v;     // [(m + 3) n]: the basis V[0..m], z = M^-1 v, t = K x
  DevBuf<double> ksp_part;  // [(m + 2) nb]: per-block partial sums
  DevBuf<double> ksp_s;     // the cycle's small state (KspSmall)
  DevBuf<int> ksp_bad_d;    // first masked node whose PC block does not invert
  Mirrored<KspHost> ksp_h;  // what the host reads per step
  Mirrored<EigHost> eig_h;  // the same for nlps_gpu_tangent_lambda_max (nlps_eigen.hpp), which shares ksp_v / ksp_part / ksp_s
  // Newton solve (nlps_gpu_newton_solve, nlps_newton.hpp), allocated on first use and kept (they only grow)
  DevBuf<double> snes_v;     // [8 n]: X, Y, W, F, K Y and the device copies of Un_dt, Un_dt2, M
  DevBuf<double> snes_part;  // [5 nb]: per-block partials of the trial update (3 columns) and the dots (2)
  Mirrored<double> snes_h;   // [SNES_H_N]: the scalars the host reads after a residual evaluation
  bool snes_tail = false;       // the next fused residual evaluation queues F . F ahead of its own synchronisation
  int snes_nb = 0;
  // implicit time step (nlps_gpu_newmark_step): M, Un_dt, Un_dt2, dU, dU_dt, dU_dt2, masked [N_A d] each
  DevBuf<double> nm_v;
  // The tile-list set: what the list stage of a step writes and its tile kernels read.  It exists twice (below).
  // order2: canonical (layer, closest node) order of every tile list each step for the LDS-atomic-bound K2 and K3; the
  // memory-bound K5 keeps the lists as binned.  13 us per step at 1 M particles.  A freshly sorted cloud has its lists in
  // that order already (0.685 vs 0.677 ms/step), but once particles have changed closest node -- 45 steps into the bench
  // cloud's fall -- K2 runs 0.231 instead of 0.300 ms and K3 0.260 instead of 0.304, and the stirred cloud of DESIGN.md
  // 0.84 instead of 0.95 ms/step
  struct ListSet {
    DevBuf<int2> work;   // compacted work list of the non-empty tiles, see TileD
    DevBuf<int> nwork;   // ranges[3 classes][begin,end] of the work list (tile_scan_block)
    DevBuf<int> start;   // [ntiles + 1] first list position of every tile
    DevBuf<int> order;   // tile lists as binned
    DevBuf<int> order2;  // canonical tile lists (k_fill_orders; k_tile_order in deterministic mode), allocated on first use
    DevBuf<unsigned char> active, fixed;  // NView::active, fixed
    DevBuf<double> nm, force;             // NView::nm, force: the nodal accumulators the list stage resets
  };
  // Async lists (the folded one-rank explicit step, nlps_gpu_explicit_step): the search of the next step runs as a
  // kernel of its own between K3 and K5 (k_search_ahead), and the activation and list kernels of the next step run on
  // `side` while K5 runs on the handle's stream.  What they write and K5 still reads exists twice, as two ListSets; the
  // step that finds lists_ready exchanges the sets (and the two closest-node arrays) instead of launching those kernels
  // (adopt_ready_lists).  `lists` is always the set in use, for every reader, and h->N views it (bind_lists); `twin` is
  // made at the first step that builds lists on the side stream (ensure_list_twins).
  ListSet lists, twin;
  SideStream side;
  bool async_lists = true;   // nlps_gpu_debug_option "async_lists"
  bool lists_ready = false;  // `ahead`, and the twin set holds the lists, flags and reset accumulators made from it
  // The deferred move (k_search_ahead): an async step with the step record off whose successor does not start with a
  // re-sort runs K5 without the move x += d_dis, dis += d_dis and has the search mark the particles K5 would have moved.
  // K2 of the next step applies the marks of the particles it lists; while move_pending, everything else that reads or
  // writes x / dis, reorders the particles or rebuilds lists from them calls materialise_move() first, so x is current
  // at every boundary of the API.
  DevBuf<unsigned char> moved_d;  // [npad] marks, all zero while !move_pending
  bool move_pending = false;
  // Below this many particles a step keeps the in-place K5: every kernel of the step is then a few microseconds of
  // launch and latency, and the operands K2 and the search take on cost more than K5 saves (13 824 particles: 0.1272
  // -> 0.1285 ms per step; equal at 110 000, ahead from 373 000 on).  nlps_gpu_debug_option "defer_move_min".
  int defer_move_min = 100000;

  nlps_halo_fn halo;
  void* halo_ctx;
  struct RcclHalo* rccl = nullptr;  // ghost-layer exchange over RCCL owned by the library (nlps_gpu_rccl_attach)
  bool rccl_wait_value = false;     // the attached exchange can be released through signal memory (overlap mode 2)

  bool timing;
  hipEvent_t ev[8];
  hipEvent_t evw[12] = {};  // brackets of the exchanges a step waits for (timing only)
  int nwait = 0;
  float ms[8];
  int slab_lo, slab_hi;
  int win_lo, win_hi;  // node window (layers of the slowest axis) the per-step nodal work is limited to
  int n0, nwn;         // first node / node count of the window
  int tile0, ntw;      // first tile / tile count of the window
};

#define HIPCHK(call)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      h->err = std::string(#call) + ": " + hipGetErrorString(e_);                            \
      fprintf(stderr, "\033[1;31mError in nlps_gpu: %s\033[0m\n", h->err.c_str());           \
      return 1;                                                                              \
    }                                                                                        \
  } while (0)

static inline int nblk(int n, int b = BLK) { return n > 0 ? (n + b - 1) / b : 1; }
// a call that moves, reorders or re-lists particles: the matrix-free tangent of nlps_gpu_tangent_operator goes stale
static inline void tan_stale(nlps_gpu* h, const char* why) {
  h->tan_gen++;
  h->tan_why = why;
}
static int materialise_nodal(nlps_gpu* h);  // the nodal arrays the folded explicit step left unmade (defined with the step)

// The move the last explicit step left to the next K2 (nlps_gpu::move_pending), for every marked particle, on the
// handle's stream -- behind the join of the side stream, whose search made the marks.
static int materialise_move(nlps_gpu* h) {
  if (!h->move_pending) return 0;
  LAUNCH_ND((k_materialise_move<2>), (k_materialise_move<3>), nblk(h->P.np), h->P, h->moved_d.get());
  HIPCHK(hipGetLastError());
  h->move_pending = false;
  return 0;
}

static bool is_device_ptr(const void* p) {
  hipPointerAttribute_t a;
  hipError_t e = hipPointerGetAttributes(&a, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

static MatD make_mat(const nlps_material& m, int nd) {
  MatD d;
  memset(&d, 0, sizeof(d));
  d.type = m.type;
  d.E = m.E;
  d.nu = m.nu;
  d.G = m.E / (2.0 * (1.0 + m.nu));
  d.lame = m.nu * m.E / ((1 - m.nu * 2) * (1 + m.nu));
  d.K = m.E / (3.0 * (1.0 - 2.0 * m.nu));
  const double PI = 3.14159265358979323846;
  double rf = (PI / 180.0) * m.phi_deg, rd = (PI / 180.0) * m.psi_deg;
  auto sq = [](double a) { return a == 0.0 ? 0.0 : a * a; };
  if (nd == 2) {  // Drucker-Prager.c:362-368
    d.alpha_F = sqrt(2. / 3.) * tan(rf) / sqrt(3. + 4. * sq(tan(rf)));
    d.alpha_Q = sqrt(2. / 3.) * tan(rd) / sqrt(3. + 4. * sq(tan(rd)));
    d.beta_dp = sqrt(2. / 3.) * 3. / sqrt(3. + 4. * sq(tan(rf)));
  } else {  // :370-375
    d.alpha_F = sqrt(2 / 3.) * 2 * sin(rf) / (3 - sin(rf));
    d.alpha_Q = sqrt(2 / 3.) * 2 * sin(rd) / (3 - sin(rd));
    d.beta_dp = sqrt(2 / 3.) * 6 * cos(rf) / (3 - sin(rf));
  }
  d.kappa_0 = m.kappa_0;
  d.exp_param = m.exponent_ortiz;
  d.eps_0 = m.eps_0;
  d.p_ref = m.p_ref;
  d.H = m.hardening_modulus;
  d.theta = m.theta_voce;
  d.K_0 = m.K0_voce;
  d.K_inf = m.Kinf_voce;
  d.delta = m.delta_voce;
  d.Ceps = m.Ceps;
  d.ft = m.ft;
  d.heps = m.heps;
  d.wcrit = m.wcrit;
  d.Gf = m.Gf;
  if (m.type == NLPS_MAT_MATSUOKA_NAKAI || m.type == NLPS_MAT_LADE_DUNCAN) {  // one kernel law, two surfaces
    d.type = NLPS_KLAW_FRICTIONAL;
    d.surface = m.type == NLPS_MAT_LADE_DUNCAN;
    d.c_cotphi = rf > 0.0 ? m.cohesion / tan(rf) : 0.0;  // Matsuoka-Nakai.c:334-336
    d.alpha_b = m.alpha_borja;
    for (int i = 0; i < 3; i++) d.a_b[i] = m.a_borja[i];
  }
  if (m.type == NLPS_MAT_NEWTONIAN_FLUID) {
    d.type = NLPS_KLAW_FLUID;
    d.viscosity = m.viscosity;
    d.K_fluid = m.compressibility;
    d.n_macdonald = m.n_macdonald;
  }
  return d;
}
static inline int klaw_of(int type) {
  if (type == NLPS_MAT_NEWTONIAN_FLUID) return NLPS_KLAW_FLUID;
  return type >= NLPS_KLAW_FRICTIONAL ? NLPS_KLAW_FRICTIONAL : type;
}

// h_avg exactly as compute_nodal_distance_local does it (Read_GramsBox.c:460-507): chain order sum
static void host_h_avg(const nlps_grid& G, const nlps_host::StencilTables& tab, std::vector<double>& out) {
  int nd = G.ndim;
  int n[3] = {G.n[0], G.n[1], nd == 3 ? G.n[2] : 1};
  size_t nn = (size_t)n[0] * n[1] * n[2];
  out.resize(nn);
  // per class: offsets sorted by chain position
  std::vector<std::vector<std::array<int, 3>>> chains(27);
  for (int cls = 0; cls < 27; cls++) {
    std::vector<std::pair<int, int>> v;
    for (int o = 0; o < 27; o++)
      if (tab.rank1[cls][o] != 255) v.push_back({tab.rank1[cls][o], o});
    std::sort(v.begin(), v.end());
    for (auto& pr : v) chains[cls].push_back({pr.second % 3 - 1, (pr.second / 3) % 3 - 1, pr.second / 9 - 1});
  }
  for (size_t I = 0; I < nn; I++) {
    int ijk[3] = {(int)(I % n[0]), (int)((I / n[0]) % n[1]), (int)(I / ((size_t)n[0] * n[1]))};
    int cls = 0, mul = 1;
    for (int a = 0; a < 3; a++) {
      int ca = a < nd ? nlps_host::class3(ijk[a], n[a]) : 1;
      cls += ca * mul;
      mul *= 3;
    }
    double avg = 0.0;
    int cnt = 0;
    for (auto& o : chains[cls]) {
      if (o[0] == 0 && o[1] == 0 && o[2] == 0) continue;
      double aux = 0.0;
      for (int a = 0; a < nd; a++) {
        double xb = G.origin[a] + G.h * (double)(ijk[a] + o[a]);
        double xa = G.origin[a] + G.h * (double)ijk[a];
        double d = xb - xa;
        aux += (d == 0.0 ? 0.0 : d * d);
      }
      avg += pow(aux, 0.5);
      cnt++;
    }
    out[I] = avg / (double)cnt;
  }
}

// n zeroed elements; view: the pointer of a kernel view (PView, NView) that borrows the block
template <class T, class V = T>
static int dev_alloc(nlps_gpu* h, DevBuf<T>& b, size_t n, V** view = nullptr) {
  HIPCHK(b.alloc_zeroed(n));
  if (view) *view = b.get();
  return 0;
}

// grow-only scratch of the handle (contents discarded when it grows)
template <class T>
static int reserve(nlps_gpu* h, const char* who, DevBuf<T>& b, size_t n, const char* what) {
  if (b.reserve(n) == hipSuccess) return 0;
  (void)hipGetLastError();
  char buf[200];
  snprintf(buf, sizeof buf, "%s: cannot allocate %zu bytes for %s", who, n * sizeof(T), what);
  h->err = buf;
  return 1;
}

extern "C" int nlps_host_stencil_tables(int ndim, unsigned char* rank1, unsigned char* order2, unsigned char* count2,
                                        double* h_avg1) {
  if (ndim != 2 && ndim != 3) return 1;
  nlps_host::StencilTables t = nlps_host::build_tables(ndim);
  if (rank1) memcpy(rank1, t.rank1, sizeof(t.rank1));
  if (order2) memcpy(order2, t.order2, sizeof(t.order2));
  if (count2) memcpy(count2, t.count2, sizeof(t.count2));
  if (h_avg1) memcpy(h_avg1, t.h_avg1, sizeof(t.h_avg1));
  return 0;
}

extern "C" const char* nlps_gpu_last_error(const nlps_gpu* h) { return h ? h->err.c_str() : "null handle"; }

extern "C" int nlps_gpu_synchronize(nlps_gpu* h) {
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int nlps_gpu_set_halo_exchange(nlps_gpu* h, nlps_halo_fn fn, void* ctx) {
  h->halo = fn;
  h->halo_ctx = ctx;
  return 0;
}

static void apply_window(nlps_gpu* h, int lo, int hi) {
  const int nd = h->nd, nl = h->g.n[nd - 1], plane = h->g.nnodes / nl;
  const int TB = nd == 3 ? TileCfg<3>::TB : TileCfg<2>::TB;
  const int tiles_per_layer = h->ntiles / h->nt[nd - 1];
  h->win_lo = lo;
  h->win_hi = hi;
  h->n0 = lo * plane;
  h->nwn = (hi - lo + 1) * plane;
  h->tile0 = (lo / TB) * tiles_per_layer;
  h->ntw = (hi / TB - lo / TB + 1) * tiles_per_layer;
}

extern "C" int nlps_gpu_set_node_window(nlps_gpu* h, int layer_lo, int layer_hi) {
  const int nl = h->g.n[h->nd - 1];
  if (layer_lo < 0 || layer_hi >= nl || layer_lo > layer_hi) {
    h->err = "nlps_gpu_set_node_window: layers outside the grid";
    return 1;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  apply_window(h, layer_lo, layer_hi);
  // clean slate outside the new window (nothing resets those nodes any more); the nodal results of an explicit step
  // before this call are gone with it, made or not
  h->nodal_stale = false;
  const size_t nn = (size_t)h->g.nnodes, ND = (size_t)h->nd;
  HIPCHK(hipMemsetAsync(h->N.active, 0, nn, h->stream));
  HIPCHK(hipMemsetAsync(h->N.seed, 0, nn, h->stream));
  HIPCHK(hipMemsetAsync(h->N.nm, 0, nn * (1 + ND) * sizeof(double), h->stream));
  HIPCHK(hipMemsetAsync(h->N.dU, 0, nn * ND * sizeof(double), h->stream));
  HIPCHK(hipMemsetAsync(h->N.force, 0, nn * ND * sizeof(double), h->stream));
  HIPCHK(hipMemsetAsync(h->N.accel, 0, nn * ND * sizeof(double), h->stream));
  HIPCHK(hipMemsetAsync(h->N.reaction, 0, nn * ND * sizeof(double), h->stream));
  HIPCHK(hipMemsetAsync(h->N.fixed, 0, nn * ND, h->stream));
  HIPCHK(hipMemsetAsync(h->tile_count_d, 0, ((size_t)h->ntiles + 1) * sizeof(int), h->stream));
  h->masks_valid = false;
  h->binned = false;
  h->ahead = h->lists_ready = false;
  return 0;
}

#if NLPS_PHASE_TIMING
extern "C" __attribute__((visibility("default"))) int nlps_gpu_debug_phases(nlps_gpu* h, unsigned long long* out, int reset) {
  HIPCHK(hipStreamSynchronize(h->stream));
  std::vector<unsigned long long> tmp(16 * 1024);
  HIPCHK(hipMemcpy(tmp.data(), h->phase_d, tmp.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  for (int k = 0; k < 16; k++) {
    out[k] = 0;
    for (int b = 0; b < 1024; b++) out[k] += tmp[k + 16 * b];
  }
  if (reset) HIPCHK(hipMemset(h->phase_d, 0, tmp.size() * sizeof(unsigned long long)));
  return 0;
}
#endif

extern "C" int nlps_gpu_set_ghost_bands(nlps_gpu* h, int band_lo, int band_hi, int overlap) {
  if (materialise_nodal(h)) return 1;  // (the node ranges of the last step's nodal kernels are about to change)
  h->band_lo = band_lo;
  h->band_hi = band_hi;
  if (overlap == 2 && !h->rccl_wait_value) {
    h->err = "nlps_gpu_set_ghost_bands: overlap 2 needs the library's RCCL path (nlps_gpu_rccl_attach)";
    return 1;
  }
  h->overlap = overlap;
  return 0;
}

extern "C" int nlps_gpu_touched_layers(nlps_gpu* h, int* lo, int* hi) {
  *lo = h->slab_lo;
  *hi = h->slab_hi;
  return 0;
}

extern "C" int nlps_gpu_set_timing(nlps_gpu* h, int on) {
  h->timing = on != 0;
  return 0;
}
extern "C" int nlps_gpu_get_timing(nlps_gpu* h, float ms[8]) {
  for (int i = 0; i < 8; i++) ms[i] = h->ms[i];
  return 0;
}

static int upload_field(nlps_gpu* h, int f, int ncomp, const double* src, int stride, std::vector<double>& tmp,
                        const double* dflt_diag /*identity rows*/, double dflt) {
  // gathers component c of the caller's AoS rows into the sorted SoA slot
  int np = h->P.np;
  for (int c = 0; c < ncomp; c++) {
    for (int s = 0; s < np; s++) {
      int p = h->perm[s];
      tmp[s] = src ? src[(size_t)p * stride + c] : (dflt_diag ? dflt_diag[c] : dflt);
    }
    for (size_t s = np; s < h->P.npad; s++) tmp[s] = 0.0;
    HIPCHK(hipMemcpy(h->P.d + (size_t)(f + c) * h->P.npad, tmp.data(), h->P.npad * sizeof(double),
                     hipMemcpyHostToDevice));
  }
  return 0;
}

extern "C" int nlps_gpu_create(nlps_gpu** out, const nlps_grid* grid, const nlps_params* prm,
                               const nlps_material* mats, int nmats, const nlps_particles* host, int nsteps,
                               void* hip_stream) {
  nlps_gpu* h = new nlps_gpu();
  *out = h;
  h->nd = grid->ndim;
  h->T = grid->ndim == 2 ? 5 : 9;
  h->nsteps = nsteps;
  h->halo = nullptr;
  h->halo_ctx = nullptr;
  h->timing = false;
  h->masks_valid = false;
  h->binned = false;
  h->perm_dirty = false;
  h->resort_every = 50;
  h->steps_since_sort = 0;
  memset(h->ms, 0, sizeof(h->ms));
  if (grid->ndim != 2 && grid->ndim != 3) {
    h->err = "ndim must be 2 or 3";
    return 1;
  }
  for (int a = 0; a < grid->ndim; a++)
    if (grid->n[a] < 5) {
      h->err = "structured grid needs >= 5 nodes per axis";
      return 1;
    }
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (ndev < 1) {
    h->err = "no HIP device: the MI355X path has no CPU fallback";
    return 1;
  }
  if (hip_stream) {
    h->stream = (hipStream_t)hip_stream;
    h->own_stream = false;
  } else {
    HIPCHK(hipStreamCreate(&h->stream));
    h->own_stream = true;
  }
  for (int i = 0; i < 8; i++) HIPCHK(hipEventCreate(&h->ev[i]));
  HIPCHK(h->side.create());

  GridD& g = h->g;
  g.nd = grid->ndim;
  for (int a = 0; a < 3; a++) {
    g.n[a] = a < g.nd ? grid->n[a] : 1;
    g.o[a] = a < g.nd ? grid->origin[a] : 0.0;
  }
  g.h = grid->h;
  g.nnodes = g.n[0] * g.n[1] * g.n[2];
  {
    int TB = g.nd == 3 ? TileCfg<3>::TB : TileCfg<2>::TB;
    for (int a = 0; a < 3; a++) h->nt[a] = a < g.nd ? (g.n[a] + TB - 1) / TB : 1;
    h->ntiles = h->nt[0] * h->nt[1] * h->nt[2];
  }
  apply_window(h, 0, g.n[g.nd - 1] - 1);
  h->hprm = *prm;
  h->prm.gamma_lme = prm->gamma_lme;
  h->prm.neg_log_tol_zero = -log(prm->tol_zero_lme);
  h->prm.tol_wrapper = prm->tol_wrapper_lme;
  h->prm.max_iter_lme = prm->max_iter_lme;
  h->prm.tol_radial = prm->tol_radial_returning;
  h->prm.max_iter_radial = prm->max_iter_radial_returning;
  h->P.erosion = prm->driver_eigenerosion != 0 || prm->driver_eigensoftening != 0;
  h->P.softening = prm->driver_eigensoftening != 0 && prm->driver_eigenerosion == 0;
#if NLPS_DEV  // developer builds only (tools/build_variant.sh): the shipped library reads no environment variable
  if (const char* e = getenv("NLPS_LAZY_NODAL")) h->lazy_nodal = atoi(e);
#endif
  {
    int dev = 0, ncu = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ncu > 0)
      h->ncu = ncu;
  }

  h->tab = nlps_host::build_tables(g.nd);
  HIPCHK(h->rank1_d.reserve(27 * 27));
  HIPCHK(hipMemcpy(h->rank1_d, h->tab.rank1, 27 * 27, hipMemcpyHostToDevice));

  // nodal arrays
  size_t nn = (size_t)g.nnodes;
  int ND = g.nd;
  if (dev_alloc(h, h->lists.active, nn, &h->N.active)) return 1;
  if (dev_alloc(h, h->N_seed, nn, &h->N.seed)) return 1;
  if (dev_alloc(h, h->lists.nm, nn * (1 + ND), &h->N.nm)) return 1;
  if (dev_alloc(h, h->N_dU, nn * ND, &h->N.dU)) return 1;
  if (dev_alloc(h, h->lists.force, nn * ND, &h->N.force)) return 1;
  if (dev_alloc(h, h->N_accel, nn * ND, &h->N.accel)) return 1;
  if (dev_alloc(h, h->N_reaction, nn * ND, &h->N.reaction)) return 1;
  if (dev_alloc(h, h->lists.fixed, nn * ND, &h->N.fixed)) return 1;
  if (dev_alloc(h, h->h_avg_d, nn)) return 1;
  if (dev_alloc(h, h->n2m_d, nn)) return 1;
  if (dev_alloc(h, h->d2m_d, nn * ND)) return 1;
  if (dev_alloc(h, h->fixedm_d, nn * ND)) return 1;
  if (dev_alloc(h, h->bsum_d, nn * ND / 1024 + 2)) return 1;
  if (dev_alloc(h, h->total_d, 4)) return 1;
  if (dev_alloc(h, h->gstatus_d, 4)) return 1;
  if (dev_alloc(h, h->gridA, nn * 2 * ND)) return 1;
  if (dev_alloc(h, h->gridB, nn * 4 * ND)) return 1;
  {
    std::vector<double> hv;
    if (grid->h_avg) hv.assign(grid->h_avg, grid->h_avg + nn);
    else host_h_avg(*grid, h->tab, hv);
    HIPCHK(hipMemcpy(h->h_avg_d, hv.data(), nn * sizeof(double), hipMemcpyHostToDevice));
    h->N.h_avg = h->h_avg_d;
    HIPCHK(h->beta_t2_d.reserve(nn));
    hipLaunchKernelGGL(k_node_tables, dim3(nblk((int)nn)), dim3(BLK), 0, 0, (int)nn, (const double*)h->h_avg_d,
                       h->prm.gamma_lme, h->prm.neg_log_tol_zero, h->beta_t2_d.get());
    HIPCHK(hipGetLastError());
    h->N.beta_t2 = h->beta_t2_d;
  }
  // materials
  h->nmats = nmats;
  h->uniform_law = nmats > 0 ? klaw_of(mats[0].type) : -1;
  h->law_present = 0;
  for (int i = 0; i < nmats; i++) {
    if (mats[i].type < 0 || mats[i].type > NLPS_MAT_NEWTONIAN_FLUID) {
      h->err = "material type outside 0..6 (Neo-Hookean, Hencky, Drucker-Prager, Von-Mises, Matsuoka-Nakai, Lade-Duncan, "
               "Newtonian-Fluid-Compressible)";
      return 1;
    }
    if (klaw_of(mats[i].type) != klaw_of(mats[0].type)) h->uniform_law = -1;
    h->mat_klaw.push_back(klaw_of(mats[i].type));
    h->law_present |= 1 << klaw_of(mats[i].type);
  }
  {
    std::vector<MatD> md(nmats);
    for (int i = 0; i < nmats; i++) md[i] = make_mat(mats[i], g.nd);
    HIPCHK(h->mats_d.reserve(nmats));
    HIPCHK(hipMemcpy(h->mats_d, md.data(), sizeof(MatD) * nmats, hipMemcpyHostToDevice));
  }

  // particles: sort by background-grid cell
  int np = host->np;
  h->P.np = np;
  // capacity: room for immigrants (nlps_gpu_migration_commit), fixed at create
  h->P.npad = ((size_t)np + std::max<size_t>((size_t)np / 4, 1024) + 255) / 256 * 256;
  h->perm.resize(np);
  std::iota(h->perm.begin(), h->perm.end(), 0);
  {
    std::vector<long long> key(np);
    std::vector<unsigned char> tile_laws(h->uniform_law < 0 ? (size_t)h->ntiles : 0, 0);
    int slab_axis = ND - 1;
    int lo = 1 << 30, hi = -1;
    const int TB = ND == 3 ? TileCfg<3>::TB : TileCfg<2>::TB;
    for (int p = 0; p < np; p++) {
      // Physical order = (tile of the closest node, corner type, closest node inside the tile).
      // "Corner type" = which corner of its cell the closest node is.  Particles that share a closest
      // node come from different cells, i.e. have different corner types, so any 64 consecutive
      // particles (one wave) have 64 DISTINCT closest nodes: their window accesses (LDS atomics of
      // the scatter, LDS reads of the gather) never collide on an address and spread over all banks.
      long long kt = 0, kn = 0, kc = 0, mt = 1, mn = 1, mc = 1;
      for (int a = 0; a < ND; a++) {
        int nc = g.n[a] - 1;
        double xi = (host->x_GC[(size_t)p * ND + a] - g.o[a]) / g.h;
        int c = (int)floor(xi);
        c = c < 0 ? 0 : (c > nc - 1 ? nc - 1 : c);
        int nd = (int)floor(xi + 0.5);
        nd = nd < 0 ? 0 : (nd > g.n[a] - 1 ? g.n[a] - 1 : nd);
        kt += mt * (nd / TB);
        mt *= h->nt[a];
        kn += mn * (nd % TB);
        mn *= TB;
        kc += mc * (nd > c ? 1 : 0);
        mc *= 2;
        if (a == slab_axis) {
          lo = std::min(lo, c);
          hi = std::max(hi, c + 1);
        }
      }
      const int mi = host->MatIdx ? host->MatIdx[p] : 0;
      if (mi < 0 || mi >= nmats) {
        h->err = "MatIdx outside the material table";
        return 1;
      }
      key[p] = (kt * mc + kc) * mn + kn;
      if (h->uniform_law < 0) {  // which laws meet in which tile (decides how K3 treats a cloud with several laws)
        unsigned char& m = tile_laws[(size_t)kt];
        m |= (unsigned char)(1 << klaw_of(mats[mi].type));
      }
    }
    if (h->uniform_law < 0) {
      size_t used = 0, mixed = 0;
      for (unsigned char m : tile_laws) {
        used += m != 0;
        mixed += (m & (m - 1)) != 0;
      }
      // blocks of different materials (a footing on soil): nearly every tile holds one law and K3 runs as one launch of
      // the single-law kernel per law, each taking its tiles (0 scratch, the speed of the uniform cloud).  Laws
      // interleaved particle by particle: every launch would touch every tile and every cache line (measured 0.68 ms
      // against 0.51 ms for the one kernel that dispatches on the law at run time), so that kernel stays for them.
      h->k3_per_law = used > 0 && 4 * mixed <= used;
      if (h->law_present & ((1 << NLPS_KLAW_FRICTIONAL) | (1 << NLPS_KLAW_FLUID))) h->k3_per_law = 1;  // not in the dispatch kernel (stress_update)
    }
    std::stable_sort(h->perm.begin(), h->perm.end(), [&](int a, int b) { return key[a] < key[b]; });
    h->slab_lo = std::max(0, lo - 3);
    h->slab_hi = std::min(g.n[slab_axis] - 1, hi + 3);
  }
  if (dev_alloc(h, h->Pd, (size_t)NFD * h->P.npad, &h->P.d)) return 1;
  if (dev_alloc(h, h->P_I0, h->P.npad, &h->P.I0)) return 1;
  if (dev_alloc(h, h->P_I0n, h->P.npad, &h->P.I0n)) return 1;
  if (dev_alloc(h, h->P_mat, h->P.npad, &h->P.mat)) return 1;
  if (dev_alloc(h, h->P_nn, h->P.npad, &h->P.nn)) return 1;
  if (dev_alloc(h, h->P_status, h->P.npad, &h->P.status)) return 1;
  if (dev_alloc(h, h->P_mlo, h->P.npad, &h->P.mlo)) return 1;
  if (dev_alloc(h, h->P_mhi, h->P.npad, &h->P.mhi)) return 1;
  if (dev_alloc(h, h->P_tile, h->P.npad, &h->P.tile)) return 1;
  if (dev_alloc(h, h->P_rank, h->P.npad, &h->P.rank)) return 1;
  if (dev_alloc(h, h->lists.order, h->P.npad)) return 1;
  if (dev_alloc(h, h->tile_count_d, (size_t)h->ntiles + 1)) return 1;
  if (dev_alloc(h, h->tile_count2_d, (size_t)h->ntiles + 1)) return 1;
  if (dev_alloc(h, h->lists.start, (size_t)h->ntiles + 1)) return 1;
  if (dev_alloc(h, h->lists.work, (size_t)h->ntiles)) return 1;
  if (dev_alloc(h, h->lists.nwork, 6)) return 1;
#if NLPS_DEV
  if (const char* e = getenv("NLPS_ADAPTIVE_RESORT")) h->adaptive_resort = atof(e);  // (0 = off)
#endif
  if (dev_alloc(h, h->node_cnt_d, (size_t)h->g.nnodes)) return 1;
  if (dev_alloc(h, h->nrank_d, h->P.npad)) return 1;
  if (dev_alloc(h, h->tile_cursor_d, (size_t)h->ntiles + 1)) return 1;
  {
    const size_t nnw = h->g.nd == 3 ? TileTabCfg<3>::NNW : TileTabCfg<2>::NNW;
    if (dev_alloc(h, h->tabo_d, (size_t)h->ntiles * TileTab::LMAX * nnw)) return 1;
    if (dev_alloc(h, h->tabm_d, (size_t)h->ntiles * TileTab::LMAX * nnw)) return 1;
  }
  if (dev_alloc(h, h->home_d, h->P.npad)) return 1;
  if (dev_alloc(h, h->foreign_d, 64 * 32)) return 1;
  HIPCHK(h->foreign_h.alloc());
  *h->foreign_h.host() = 0;
  HIPCHK(h->status_h.alloc());  // (without a device alias check_status copies)
  *h->status_h.host() = 0;
#if NLPS_PHASE_TIMING
  if (dev_alloc(h, h->phase_d, 16 * 1024)) return 1;
#endif
  {
    std::vector<double> tmp(h->P.npad);
    int T = h->T;
    double idrow[9] = {0};
    idrow[0] = 1.0;
    idrow[ND + 1] = 1.0;
    idrow[T - 1] = 1.0;
    if (upload_field(h, F_X, ND, host->x_GC, ND, tmp, nullptr, 0.0)) return 1;
    if (upload_field(h, F_DIS, ND, host->dis, ND, tmp, nullptr, 0.0)) return 1;
    if (upload_field(h, F_VEL, ND, host->vel, ND, tmp, nullptr, 0.0)) return 1;
    if (upload_field(h, F_ACC, ND, host->acc, ND, tmp, nullptr, 0.0)) return 1;
    if (upload_field(h, F_FN, T, host->F_n, T, tmp, idrow, 0.0)) return 1;
    if (upload_field(h, F_FN1, T, host->F_n1 ? host->F_n1 : host->F_n, T, tmp, idrow, 0.0)) return 1;
    if (upload_field(h, F_DF, T, host->DF, T, tmp, idrow, 0.0)) return 1;
    if (upload_field(h, F_TAU, T, host->Stress, T, tmp, nullptr, 0.0)) return 1;
    if (upload_field(h, F_BEN, T, host->b_e_n, T, tmp, idrow, 0.0)) return 1;
    if (upload_field(h, F_BEN1, T, host->b_e_n1 ? host->b_e_n1 : host->b_e_n, T, tmp, idrow, 0.0)) return 1;
    if (upload_field(h, F_JN, 1, host->J_n, 1, tmp, nullptr, 1.0)) return 1;
    if (upload_field(h, F_JN1, 1, host->J_n1 ? host->J_n1 : host->J_n, 1, tmp, nullptr, 1.0)) return 1;
    if (upload_field(h, F_RHO, 1, host->rho, 1, tmp, nullptr, 0.0)) return 1;
    if (upload_field(h, F_MASS, 1, host->mass, 1, tmp, nullptr, 0.0)) return 1;
    if (upload_field(h, F_VOL0, 1, host->Vol_0, 1, tmp, nullptr, 0.0)) return 1;
    if (upload_field(h, F_W, 1, host->W, 1, tmp, nullptr, 0.0)) return 1;
    if (upload_field(h, F_KN, 1, host->Kappa_n, 1, tmp, nullptr, 0.0)) return 1;
    if (upload_field(h, F_KN1, 1, host->Kappa_n1 ? host->Kappa_n1 : host->Kappa_n, 1, tmp, nullptr, 0.0)) return 1;
    if (upload_field(h, F_EN, 1, host->EPS_n, 1, tmp, nullptr, 0.0)) return 1;
    if (upload_field(h, F_EN1, 1, host->EPS_n1 ? host->EPS_n1 : host->EPS_n, 1, tmp, nullptr, 0.0)) return 1;
    if (upload_field(h, F_LAM, ND, host->lambda, ND, tmp, nullptr, 0.0)) return 1;
    if (upload_field(h, F_BETA, 1, host->Beta, 1, tmp, nullptr, 0.0)) return 1;
    if (upload_field(h, F_LAMP, ND, host->lambda, ND, tmp, nullptr, 0.0)) return 1;
    if (upload_field(h, F_BACK, 3, host->Back_stress, 3, tmp, nullptr, 0.0)) return 1;
    if (upload_field(h, F_DMG, 1, host->Damage_n, 1, tmp, nullptr, 0.0)) return 1;
    if (upload_field(h, F_DMG1, 1, host->Damage_n1 ? host->Damage_n1 : host->Damage_n, 1, tmp, nullptr, 0.0)) return 1;
    if (upload_field(h, F_STRF, 1, host->Strain_f_n, 1, tmp, nullptr, 0.0)) return 1;
    if (upload_field(h, F_STRF1, 1, host->Strain_f_n1 ? host->Strain_f_n1 : host->Strain_f_n, 1, tmp, nullptr, 0.0)) return 1;
    if (h->P.erosion) h->level_b_fields = true;  // the damage fields travel with the re-sort
    if (host->dt_F_n || host->dt_F_n1 || host->dt_DF) h->level_b_fields = true;
    if (h->law_present & (1 << NLPS_KLAW_FLUID)) h->level_b_fields = true;  // the fluid's rate tensors are state: they travel with the re-sort
    if (host->dt_F_n && upload_field(h, F_DTFN, T, host->dt_F_n, T, tmp, nullptr, 0.0)) return 1;
    if (host->dt_F_n1 && upload_field(h, F_DTFN1, T, host->dt_F_n1, T, tmp, nullptr, 0.0)) return 1;
    if (host->dt_DF && upload_field(h, F_DTDF, T, host->dt_DF, T, tmp, nullptr, 0.0)) return 1;
    std::vector<int> it(h->P.npad, 0);
    for (int s = 0; s < np; s++) it[s] = host->MatIdx ? host->MatIdx[h->perm[s]] : 0;
    HIPCHK(hipMemcpy(h->P.mat, it.data(), h->P.npad * sizeof(int), hipMemcpyHostToDevice));
    if (host->I0) {
      for (int s = 0; s < np; s++) it[s] = host->I0[h->perm[s]];
      HIPCHK(hipMemcpy(h->P.I0, it.data(), h->P.npad * sizeof(int), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(h->P.I0n, it.data(), h->P.npad * sizeof(int), hipMemcpyHostToDevice));
    }
  }
  // re-sort buffers
  if (dev_alloc(h, h->perm_d, h->P.npad)) return 1;
  HIPCHK(hipMemcpy(h->perm_d, h->perm.data(), (size_t)np * sizeof(int), hipMemcpyHostToDevice));
  if (dev_alloc(h, h->gid_d, h->P.npad)) return 1;
  HIPCHK(hipMemcpy(h->gid_d, h->perm.data(), (size_t)np * sizeof(int), hipMemcpyHostToDevice));
  if (dev_alloc(h, h->leaving_d, h->P.npad)) return 1;
  if (dev_alloc(h, h->mig_slot_d, h->P.npad)) return 1;
  if (dev_alloc(h, h->mig_cnt_d, 2)) return 1;
  if (dev_alloc(h, h->skey_d, h->P.npad)) return 1;
  if (dev_alloc(h, h->skey2_d, h->P.npad)) return 1;
  if (dev_alloc(h, h->sval_d, h->P.npad)) return 1;
  if (dev_alloc(h, h->sval2_d, h->P.npad)) return 1;
  if (dev_alloc(h, h->gather_tmp, h->P.npad)) return 1;
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, h->cub_tmp_bytes, h->skey_d.get(), h->skey2_d.get(), h->sval_d.get(), h->sval2_d.get(),
                                            (int)h->P.npad, 0, 64, h->stream));
  HIPCHK(h->cub_tmp.reserve(h->cub_tmp_bytes + 16));
  HIPCHK(hipStreamSynchronize(h->stream));
  // the uploads above are ordered on the default stream only: a caller-provided non-blocking stream (torch
  // streams are) would not wait for their DMA
  HIPCHK(hipDeviceSynchronize());
  return 0;
}

// The particles have changed memory slots (the re-sort, and a migration through it).  Whoever caches something per slot
// registers here; at present:
//   the host copy of perm_d (refresh_perm) and the inverse permutation (inv_perm: loads, record probes, snapshot pack);
//   the tile lists, and the per-particle tile / rank of a search done ahead, which belong to the old slots;
//   the adaptive re-sort: the slots have new owners, the next search records their tiles (TileCnt::home);
//   the node runs of the damage hooks, which hold slot numbers (tables: read-out only, until the next build).
static void slots_renumbered(nlps_gpu* h) {
  h->perm_dirty = true;
  h->inv.stale = true;
  h->binned = false;
  h->ahead = h->lists_ready = false;
  h->rehome = true;
  h->debt = 0.0;
  h->steps_since_sort = 0;
  h->dmg.tables0 = h->dmg.tables = false;
}

// Physical re-sort of every particle array by (tile of I0, corner type, I0 in tile).
// live_only: called at the head of an explicit step -- the fields that step rewrites in full before anything reads them
// (d_dis, the n+1 slots of F and b_e, DF, tau, J_n+1, W, kappa_n+1, eps_n+1: 43 of the 89 components) are not moved.
static int resort(nlps_gpu* h, const unsigned char* leaving = nullptr, bool live_only = false) {
  tan_stale(h, "a re-sort of the particle arrays");
  const int np = h->P.np;
  if (np == 0) return 0;
  if (materialise_move(h)) return 1;  // (d_dis does not travel with live_only, and the marks are per slot)
  // The tile lists of the last step in canonical order (lists.order2: layer r = the r-th particle of every closest node,
  // nodes in lattice order) ARE the memory order the kernels want -- each wave then reads 64 consecutive slots that hit
  // 64 distinct window rows -- so the periodic re-sort of the fused step takes them as its permutation: no keys, no
  // radix sort.  Otherwise (first sort, migration, level-B callers): sort by (tile, corner type, node).
  const bool from_lists = !leaving && live_only && h->binned && h->lists.order2 && h->ntw > 0;
  if (!from_lists) {
    TileCnt tc;
    for (int a = 0; a < 3; a++) tc.nt[a] = h->nt[a];
    tc.count = nullptr;
    tc.home = nullptr;
    tc.node_cnt = nullptr;
    LAUNCH_ND(k_sort_keys<2>, k_sort_keys<3>, nblk(np), h->P, h->g, tc, h->skey_d, h->sval_d, leaving, h->mats_d);
    HIPCHK(hipGetLastError());
    size_t bytes = h->cub_tmp_bytes;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(h->cub_tmp.get(), bytes, h->skey_d.get(), h->skey2_d.get(), h->sval_d.get(), h->sval2_d.get(), np, 0, 64,
                                              h->stream));
  }
  if (from_lists) {  // particles that are in no list go behind the lists (k_mark_listed / k_append_unlisted)
    unsigned char* listed = reinterpret_cast<unsigned char*>(h->gather_tmp.get());  // [npad] bytes of the gather scratch, idle here
    HIPCHK(hipMemsetAsync(h->mig_cnt_d, 0, sizeof(int), h->stream));
    HIPCHK(hipMemsetAsync(listed, 0, (size_t)np, h->stream));
    const int last = h->tile0 + h->ntw - 1;
    hipLaunchKernelGGL(k_mark_listed, dim3(nblk(np)), dim3(BLK), 0, h->stream, np, (const int*)h->lists.start + last,
                       (const int*)h->tile_count_d + last, (const int*)h->lists.order2, listed);
    hipLaunchKernelGGL(k_append_unlisted, dim3(nblk(np)), dim3(BLK), 0, h->stream, np, (const unsigned char*)listed,
                       (const int*)h->lists.start + last, (const int*)h->tile_count_d + last, h->mig_cnt_d, h->lists.order2);
  }
  const int* idx = from_lists ? h->lists.order2 : h->sval2_d;  // new slot -> old slot
  const size_t npad = h->P.npad;
  const int nf = h->level_b_fields ? (int)NFD : (int)F_CEP;  // C_ep and the rate tensors only exist for level B
  // the field block moves into its twin in one launch and the two swap roles (no copy back; the twin costs a second
  // NFD x npad block of HBM, allocated at the first re-sort)
  if (!h->Pd_alt) {
    HIPCHK(h->Pd_alt.reserve((size_t)NFD * npad));
    HIPCHK(hipMemsetAsync(h->Pd_alt, 0, (size_t)NFD * npad * sizeof(double), h->stream));
  }
  if (live_only && !h->level_b_fields) {
    // contiguous runs of live components (enum at the top of this file; F and b_e by their current n slots)
    const int fn = fFN(h->P), ben = fBEN(h->P);
    const int runs[][2] = {{F_X, 12}, {fn, 9}, {ben, 9}, {F_JN, 1}, {F_RHO, 3}, {F_KN, 1}, {F_EN, 1}, {F_LAM, 11}};
    FieldList fl;
    fl.n = 0;
    for (auto& r : runs)
      for (int q = 0; q < r[1]; q++) fl.f[fl.n++] = (unsigned char)(r[0] + q);
    if (h->nd == 2) {  // the zz slots of F_n+1 and DF are never written by the 2-D kernels (they stay 1 from the upload)
      fl.f[fl.n++] = (unsigned char)(fFN1(h->P) + 4);
      fl.f[fl.n++] = (unsigned char)(F_DF + 4);
    }
    static_assert((int)NFD <= 255, "component indices travel as bytes");
    hipLaunchKernelGGL(k_gather_field_list, dim3(nblk(np), (fl.n + GATHER_FIELDS - 1) / GATHER_FIELDS), dim3(BLK), 0, h->stream,
                       h->Pd_alt, (const double*)h->P.d, idx, np, npad, fl);
  } else {
    hipLaunchKernelGGL(k_gather_fields, dim3(nblk(np), (nf + GATHER_FIELDS - 1) / GATHER_FIELDS), dim3(BLK), 0, h->stream,
                       h->Pd_alt, (const double*)h->P.d, idx, np, npad, nf);
  }
  h->Pd.swap(h->Pd_alt);
  h->P.d = h->Pd;  // (the view is passed by value: it must follow the owner)
  if (h->fbar.on) {  // Fbar_n / Jbar_n travel with the particles, into their twins (nlps_gpu_set_explicit_fbar made them)
    hipLaunchKernelGGL(k_gather_fields, dim3(nblk(np), (h->T + GATHER_FIELDS - 1) / GATHER_FIELDS), dim3(BLK), 0, h->stream,
                       h->fbar.F_alt.get(), (const double*)h->fbar.F.get(), idx, np, npad, h->T);
    hipLaunchKernelGGL(k_gather<double>, dim3(nblk(np)), dim3(BLK), 0, h->stream, h->fbar.J_alt.get(), (const double*)h->fbar.J.get(),
                       idx, np);
    h->fbar.F.swap(h->fbar.F_alt);
    h->fbar.J.swap(h->fbar.J_alt);
  }
  {
    // (the twin block now holds the OLD field values, which nothing reads any more: its head is the scratch of the
    // integer arrays -- 2 x npad doubles for the mask words, then 7 x npad ints)
    SmallArrays A;
    int* iarr[7] = {h->P.I0, h->P.I0n, h->P.mat, h->P.nn, h->P.status, h->perm_d, h->gid_d};
    for (int a = 0; a < 7; a++) A.ia[a] = iarr[a];
    A.ua[0] = h->P.mlo;
    A.ua[1] = h->P.mhi;
    static_assert((int)NFD >= 6, "the scratch of the integer arrays needs 2 + 3.5 components of the twin block");
    unsigned long long* su = reinterpret_cast<unsigned long long*>(h->Pd_alt.get());
    int* si = reinterpret_cast<int*>(h->Pd_alt + 2 * npad);
    hipLaunchKernelGGL(k_gather_small, dim3(nblk(np)), dim3(BLK), 0, h->stream, A, idx, np, npad, si, su);
    hipLaunchKernelGGL(k_copy_small, dim3(nblk(np)), dim3(BLK), 0, h->stream, A, np, npad, (const int*)si,
                       (const unsigned long long*)su);
  }
  HIPCHK(hipGetLastError());
  slots_renumbered(h);
  return 0;
}

static int refresh_perm(nlps_gpu* h) {
  if (!h->perm_dirty) return 0;
  HIPCHK(hipStreamSynchronize(h->stream));
  const int np = h->P.np;
  h->perm.resize(np);
  if (!h->migrated) {
    HIPCHK(hipMemcpy(h->perm.data(), h->perm_d, (size_t)np * sizeof(int), hipMemcpyDeviceToHost));
  } else if (np > 0) {
    // after a migration the caller's original order is gone: rows come back in ascending global id
    std::vector<int> gid(np), idx(np);
    HIPCHK(hipMemcpy(gid.data(), h->gid_d, (size_t)np * sizeof(int), hipMemcpyDeviceToHost));
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return gid[a] < gid[b]; });
    for (int r = 0; r < np; r++) h->perm[idx[r]] = r;
  }
  h->perm_dirty = false;
  return 0;
}

extern "C" int nlps_gpu_num_particles(nlps_gpu* h, int* np) {
  *np = h->P.np;
  return 0;
}

extern "C" int nlps_gpu_set_particle_ids(nlps_gpu* h, const int* ids) {
  if (refresh_perm(h)) return 1;
  const int np = h->P.np;
  std::vector<int> g(np);
  for (int s = 0; s < np; s++) g[s] = ids[h->perm[s]];
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(h->gid_d, g.data(), (size_t)np * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipDeviceSynchronize());
  return 0;
}

extern "C" int nlps_gpu_download_ids(nlps_gpu* h, int* ids) {
  if (refresh_perm(h)) return 1;
  const int np = h->P.np;
  std::vector<int> g(np);
  HIPCHK(hipStreamSynchronize(h->stream));
  if (np) HIPCHK(hipMemcpy(g.data(), h->gid_d, (size_t)np * sizeof(int), hipMemcpyDeviceToHost));
  for (int s = 0; s < np; s++) ids[h->perm[s]] = g[s];
  return 0;
}

// Migration, step 1: particles whose closest node lies below layer keep_lo leave "down", above keep_hi "up";
// their packed rows are written to two device buffers owned by the handle.
extern "C" int nlps_gpu_migration_select(nlps_gpu* h, int keep_lo, int keep_hi, int* n_down, int* n_up, int* row_words,
                                         void** down_rows, void** up_rows) {
  const int np = h->P.np;
  if (materialise_move(h)) return 1;
  HIPCHK(hipMemsetAsync(h->mig_cnt_d, 0, 2 * sizeof(int), h->stream));
  HIPCHK(hipMemsetAsync(h->leaving_d, 0, h->P.npad, h->stream));
  if (np > 0) LAUNCH_ND((k_mig_flag<2>), (k_mig_flag<3>), nblk(np), h->P, h->g, keep_lo, keep_hi, h->leaving_d, h->mig_slot_d, h->mig_cnt_d);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h->mig_n, h->mig_cnt_d, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->mig_down_d.reset();  // (a new block at the size of this selection every call)
  h->mig_up_d.reset();
  HIPCHK(h->mig_down_d.reserve(((size_t)h->mig_n[0] + 1) * MIG_WORDS));
  HIPCHK(h->mig_up_d.reserve(((size_t)h->mig_n[1] + 1) * MIG_WORDS));
  if (h->mig_n[0] + h->mig_n[1] > 0) {
    hipLaunchKernelGGL(k_mig_pack, dim3(nblk(np)), dim3(BLK), 0, h->stream, h->P, h->leaving_d, h->mig_slot_d, h->perm_d,
                       h->gid_d, h->mig_down_d, h->mig_up_d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  *n_down = h->mig_n[0];
  *n_up = h->mig_n[1];
  *row_words = MIG_WORDS;
  if (down_rows) *down_rows = h->mig_down_d.get();
  if (up_rows) *up_rows = h->mig_up_d.get();
  h->mig_selected = true;
  return 0;
}

// Migration, step 2: the selected particles leave, the immigrants (packed rows from the neighbours, host or device
// pointers) join, the arrays are re-sorted and the next search re-bins everything.
extern "C" int nlps_gpu_migration_commit(nlps_gpu* h, const void* rows_a, int n_a, const void* rows_b, int n_b) {
  tan_stale(h, "a particle migration");
  if (!h->mig_selected) {
    h->err = "nlps_gpu_migration_commit: call nlps_gpu_migration_select() first";
    return 1;
  }
  const int np = h->P.np, n_in = n_a + n_b, n_out = h->mig_n[0] + h->mig_n[1];
  if ((size_t)np + n_in > h->P.npad) {
    h->err = "nlps_gpu_migration_commit: more immigrants than the capacity reserved at create (np + max(np/4, 1024))";
    return 1;
  }
  h->mig_selected = false;
  if (n_in == 0 && n_out == 0) return 0;
  if (materialise_move(h)) return 1;
  const void* src[2] = {rows_a, rows_b};
  const int cnt[2] = {n_a, n_b};
  int first = np;
  for (int k = 0; k < 2; k++) {
    if (cnt[k] <= 0) continue;
    DevBuf<double> tmp;
    HIPCHK(tmp.reserve((size_t)cnt[k] * MIG_WORDS));
    HIPCHK(hipMemcpyAsync(tmp, src[k], (size_t)cnt[k] * MIG_WORDS * sizeof(double), hipMemcpyDefault, h->stream));
    hipLaunchKernelGGL(k_mig_unpack, dim3(nblk(cnt[k])), dim3(BLK), 0, h->stream, h->P, first, cnt[k], tmp, h->perm_d,
                       h->gid_d, h->leaving_d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    first += cnt[k];
  }
  h->P.np = np + n_in;
  h->searched = false;  // the immigrants' closest nodes are those of their last search: everyone searches again
  if (resort(h, h->leaving_d)) return 1;  // emigrants sort to the end ...
  h->P.np = np + n_in - n_out;           // ... and fall off
  h->migrated = true;
  h->perm_dirty = true;
  h->masks_valid = false;
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int nlps_gpu_resort(nlps_gpu* h) { return resort(h); }
// Developer / test switches as an explicit call (never read from the environment in the shipped build): which of the
// equivalent launch forms a handle uses.  Not part of include/nlps_gpu.h.  Results do not depend on any of them.
extern "C" __attribute__((visibility("default"))) int nlps_gpu_debug_option(nlps_gpu* h, const char* name, double value) {
  const std::string k(name ? name : "");
  if (k == "lazy_nodal") h->lazy_nodal = (int)value;             // folded explicit step: 0 never, 1 below 2 M particles, 2 always
  else if (k == "defer_move_min") h->defer_move_min = (int)value;  // deferred move: the smallest cloud that defers (tests: 0)
  else if (k == "async_lists") h->async_lists = value != 0;      // one-rank folded step: next step's lists on the side stream (1) or in front of K2 (0)
  else if (k == "tangent_symmetric") h->tangent_symmetric = value != 0;  // Neo-Hookean clouds: half rows + mirror (1) or every pair (0)
  else if (k == "loads_lane_map") h->loads_lane_map = value != 0;  // explicit loads: one lane per contour particle (1) or one wave (0)
  else if (k == "snapshot_by_caller") h->snap_by_caller = value != 0;  // snapshot pack: one thread per caller's index (1) or per slot (0)
  else {
    h->err = "nlps_gpu_debug_option: unknown option " + k;
    return 1;
  }
  h->ahead = h->lists_ready = false;  // (lists made under another form are not reused)
  return 0;
}
extern "C" int nlps_gpu_set_law_launch_mode(nlps_gpu* h, int mode) {
  if (mode != 1 && mode != 2) {
    h->err = "nlps_gpu_set_law_launch_mode: 1 = one launch per law, 2 = one kernel dispatching on the law";
    return 1;
  }
  if (mode == 2 && (h->law_present & (1 << NLPS_KLAW_FRICTIONAL))) {
    h->err = "nlps_gpu_set_law_launch_mode: the dispatch kernel does not hold Matsuoka-Nakai / Lade-Duncan";
    return 1;
  }
  if (mode == 2 && (h->law_present & (1 << NLPS_KLAW_FLUID))) {
    h->err = "nlps_gpu_set_law_launch_mode: the dispatch kernel does not hold Newtonian-Fluid-Compressible";
    return 1;
  }
  h->k3_per_law = mode == 1;
  return 0;
}
// every table of the node runs (both damage setters), so that neither a step nor a residual evaluation allocates
static int xrun_alloc(nlps_gpu* h) {
  if (!h->dmg.cnt) {
    const size_t nn = (size_t)h->g.nnodes, npad = h->P.npad;
    if (dev_alloc(h, h->dmg.cnt, nn) || dev_alloc(h, h->dmg.cursor, 1) || dev_alloc(h, h->dmg.rank, npad)) return 1;
    if (dev_alloc(h, h->dmg.first, nn) || dev_alloc(h, h->dmg.last, nn) || dev_alloc(h, h->dmg.sorted, npad)) return 1;
    if (!h->P.softening &&
        (dev_alloc(h, h->dmg.first0, nn) || dev_alloc(h, h->dmg.last0, nn) || dev_alloc(h, h->dmg.sorted0, npad)))
      return 1;
    HIPCHK(hipMemsetAsync(h->dmg.cnt, 0, nn * sizeof(int), h->stream));  // (k_run_first leaves the counters at zero)
  }
  return 0;
}
extern "C" int nlps_gpu_set_explicit_fluid(nlps_gpu* h, int on) {
  if (!(h->law_present & (1 << NLPS_KLAW_FLUID))) {
    h->err = "nlps_gpu_set_explicit_fluid: the cloud holds no Newtonian-Fluid-Compressible material";
    return 1;
  }
  h->explicit_fluid = on != 0;
  return 0;
}
extern "C" int nlps_gpu_set_explicit_damage(nlps_gpu* h, int on) {
  if (!h->P.erosion) {
    h->err = "nlps_gpu_set_explicit_damage: the cloud was created without driver_eigenerosion / driver_eigensoftening "
             "(nlps_params): it has no damage hooks to run";
    return 1;
  }
  if (on && xrun_alloc(h)) return 1;
  h->explicit_damage = on != 0;
  return 0;
}
static int refresh_perm(nlps_gpu* h);
// F-bar on lattice-cell patches (include/nlps_gpu.h).  The setter checks, builds a fresh nlps_gpu::Fbar
// -- the patch array, the patch of every particle, the flags, Fbar_n / Jbar_n with their re-sort twins -- and assigns
// it behind a synchronise; nothing is stored when it refuses.
extern "C" int nlps_gpu_set_explicit_fbar(nlps_gpu* h, const nlps_fbar_cfg* cfg) {
  const std::string who = "nlps_gpu_set_explicit_fbar: ";
  if (!cfg) {
    HIPCHK(hipStreamSynchronize(h->stream));
    h->fbar = {};
    return 0;
  }
  const int ND = h->nd, T = h->T, np = h->P.np;
  for (int a = 0; a < ND; a++)
    if (cfg->block[a] < 1) {
      h->err = who + "a block entry is < 1 (cells per patch along each axis)";
      return 1;
    }
  if (!cfg->alpha) {
    h->err = who + "alpha is NULL (one entry per material)";
    return 1;
  }
  bool any = false;
  for (int m = 0; m < h->nmats; m++) {
    const double al = cfg->alpha[m];
    if (al > 1.0) {
      h->err = who + "an alpha is > 1 (alpha_Fbar lies in [0, 1]; < 0: the material does not read F-bar)";
      return 1;
    }
    if (!(al < 0.0)) {
      const int law = h->mat_klaw[m];
      if (!(al >= 0.0) || (law != NLPS_MAT_NEO_HOOKEAN && law != NLPS_KLAW_FLUID)) {
        h->err = who + "alpha >= 0 on a material that is neither Neo-Hookean nor Newtonian-Fluid-Compressible (the laws that "
                       "carry Fbar upstream)";
        return 1;
      }
      any = true;
    }
  }
  if (!any) {
    h->err = who + "every alpha is < 0: no material reads F-bar (pass NULL to switch it off)";
    return 1;
  }
  if (h->P.erosion) {
    h->err = who + "the cloud was created with driver_eigenerosion / driver_eigensoftening; the step with the damage hooks has "
                   "its own split of K3";
    return 1;
  }
  if (h->halo || h->rccl) {
    h->err = who + "built for one rank: not with a halo callback or an RCCL exchange attached (a patch across a slab face "
                   "would need its sums exchanged)";
    return 1;
  }
  if (h->migrated) {
    h->err = who + "not available after a migration (particle order is by global id)";
    return 1;
  }
  nlps_gpu::Fbar fresh;
  fresh.on = true;
  fresh.npatch = 1;
  for (int a = 0; a < 3; a++) {
    fresh.block[a] = a < ND ? cfg->block[a] : 1;
    fresh.np[a] = a < ND ? (std::max(1, h->g.n[a] - 1) + fresh.block[a] - 1) / fresh.block[a] : 1;
    fresh.npatch *= (size_t)fresh.np[a];
  }
  if (fresh.npatch >= ((size_t)1 << 30)) {
    h->err = who + "more than 2^30 patches";
    return 1;
  }
  const size_t npad = h->P.npad;
  HIPCHK(fresh.sums.alloc_zeroed(2 * fresh.npatch));
  HIPCHK(fresh.pid.alloc_zeroed(npad));
  HIPCHK(fresh.alpha.alloc_zeroed((size_t)std::max(1, h->nmats)));
  HIPCHK(fresh.F.alloc_zeroed((size_t)T * npad));
  HIPCHK(fresh.J.alloc_zeroed(npad));
  HIPCHK(fresh.F_alt.alloc_zeroed((size_t)T * npad));
  HIPCHK(fresh.J_alt.alloc_zeroed(npad));
  HIPCHK(hipMemcpy(fresh.alpha, cfg->alpha, (size_t)h->nmats * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipStreamSynchronize(h->stream));
  if ((cfg->Fbar_n || cfg->Jbar_n) && refresh_perm(h)) return 1;
  std::vector<double> tmp(npad, 0.0);
  if (cfg->Fbar_n) {
    for (int c = 0; c < T; c++) {
      for (int s = 0; s < np; s++) tmp[s] = cfg->Fbar_n[(size_t)h->perm[s] * T + c];
      HIPCHK(hipMemcpy(fresh.F + (size_t)c * npad, tmp.data(), npad * sizeof(double), hipMemcpyHostToDevice));
    }
  } else {  // F_n as it stands on the device
    HIPCHK(hipMemcpy(fresh.F, h->P.d + (size_t)fFN(h->P) * npad, (size_t)T * npad * sizeof(double), hipMemcpyDeviceToDevice));
  }
  if (cfg->Jbar_n) {
    for (int s = 0; s < np; s++) tmp[s] = cfg->Jbar_n[h->perm[s]];
    HIPCHK(hipMemcpy(fresh.J, tmp.data(), npad * sizeof(double), hipMemcpyHostToDevice));
  } else {
    HIPCHK(hipMemcpy(fresh.J, h->P.d + (size_t)F_JN * npad, npad * sizeof(double), hipMemcpyDeviceToDevice));
  }
  HIPCHK(hipDeviceSynchronize());  // (the copies above are ordered on the default stream only, see ensure_bcs)
  h->fbar = std::move(fresh);
  return 0;
}
extern "C" int nlps_gpu_download_fbar(nlps_gpu* h, double* Fbar_n, double* Jbar_n) {
  if (!h->fbar.on) {
    h->err = "nlps_gpu_download_fbar: F-bar is not set on this handle (nlps_gpu_set_explicit_fbar)";
    return 1;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  if (refresh_perm(h)) return 1;
  const int T = h->T, np = h->P.np;
  const size_t npad = h->P.npad;
  std::vector<double> tmp(npad);
  for (int c = 0; Fbar_n && c < T; c++) {
    HIPCHK(hipMemcpy(tmp.data(), h->fbar.F + (size_t)c * npad, (size_t)np * sizeof(double), hipMemcpyDeviceToHost));
    for (int s = 0; s < np; s++) Fbar_n[(size_t)h->perm[s] * T + c] = tmp[s];
  }
  if (Jbar_n) {
    HIPCHK(hipMemcpy(tmp.data(), h->fbar.J.get(), (size_t)np * sizeof(double), hipMemcpyDeviceToHost));
    for (int s = 0; s < np; s++) Jbar_n[h->perm[s]] = tmp[s];
  }
  return 0;
}
// the level-B stages and the implicit path while F-bar is set: their law would have to read it, and its consistent
// tangent couples all particles of a patch
static int fbar_refuse(nlps_gpu* h, const char* who) {
  if (!h->fbar.on) return 0;
  h->err = std::string(who) + ": F-bar is set on this handle (nlps_gpu_set_explicit_fbar), which only the explicit step reads; "
                              "pass NULL to it first";
  return 1;
}

static const char* implicit_damage_halo_msg =
    "the fused damage residual is built for one rank: with a halo callback or an RCCL exchange attached, an "
    "epsilon-neighbourhood across a slab face would need ghost particles";
extern "C" int nlps_gpu_set_implicit_damage(nlps_gpu* h, int on) {
  if (!h->P.erosion) {
    h->err = "nlps_gpu_set_implicit_damage: the cloud was created without driver_eigenerosion / driver_eigensoftening "
             "(nlps_params): it has no damage hooks to run";
    return 1;
  }
  if (h->law_present & (1 << NLPS_KLAW_FLUID)) {
    h->err = "nlps_gpu_set_implicit_damage: the cloud holds the Newtonian-Fluid-Compressible law; the state half of the fused "
             "damage residual is cut for the solid laws";
    return 1;
  }
  if (h->halo || h->rccl) {
    h->err = std::string("nlps_gpu_set_implicit_damage: ") + implicit_damage_halo_msg;
    return 1;
  }
  if (on && xrun_alloc(h)) return 1;
  h->implicit_damage = on != 0;
  h->dmg.gen = 0;
  return 0;
}

static int det_slab_reserve(nlps_gpu* h, const char* who);  // (defined with det_prepare)
extern "C" int nlps_gpu_set_deterministic_damage(nlps_gpu* h, int on) {
  if (!h->P.erosion) {
    h->err = "nlps_gpu_set_deterministic_damage: the cloud was created without driver_eigenerosion / driver_eigensoftening "
             "(nlps_params): it has no damage hooks to run";
    return 1;
  }
  // (the run tables, shared with the two damage setters, and the window slabs of the largest user: no step or evaluation
  // allocates, whichever switch comes first)
  if (on && (xrun_alloc(h) || det_slab_reserve(h, "nlps_gpu_set_deterministic_damage"))) return 1;
  h->det_damage = on != 0;
  h->dmg.drop();
  return 0;
}

extern "C" int nlps_gpu_set_deterministic(nlps_gpu* h, int on) {
  h->deterministic = on != 0;
  h->dmg.drop();
  h->ahead = h->lists_ready = false;
  h->rehome = true;
  h->debt = 0.0;
  return 0;
}
extern "C" int nlps_gpu_set_resort_interval(nlps_gpu* h, int every_n_steps) {
  h->resort_every = every_n_steps;
  h->steps_since_sort = 0;  // the interval counts from this call
  return 0;
}
extern "C" int nlps_gpu_set_adaptive_resort(nlps_gpu* h, double budget, int min_steps) {
  if (budget < 0.0 || min_steps < 1) {
    h->err = "nlps_gpu_set_adaptive_resort: budget >= 0 (0 = off), min_steps >= 1";
    return 1;
  }
  h->adaptive_resort = budget;
  h->adaptive_min_steps = min_steps;
  h->ahead = h->lists_ready = false;
  h->rehome = true;
  h->debt = 0.0;
  return 0;
}
extern "C" __attribute__((visibility("default"))) int nlps_gpu_debug_displaced(nlps_gpu* h, int* count, double* debt) {
  HIPCHK(hipStreamSynchronize(h->stream));  // developer read-out: the count of the last completed search stage
  *count = h->foreign_h.host() ? *(volatile int*)h->foreign_h.host() : 0;
  *debt = h->debt;
  return 0;
}

// developer read-out: the node runs as the last step or residual evaluation left them -- the tables of the current closest
// nodes (snapshot = 0) or of the eigenerosion snapshot's (1).  key[np]: the node every slot is counted under (-1: none),
// first / last [nnodes], sorted[np].  Returns 1 when that table has not been built (or was dropped by a mode switch).
extern "C" __attribute__((visibility("default"))) int nlps_gpu_debug_damage_runs(nlps_gpu* h, int snapshot, int* key, int* first,
                                                                                 int* last, int* sorted) {
  const bool have = snapshot ? (h->dmg.tables0 && h->dmg.sorted0) : (h->dmg.tables && h->dmg.sorted);
  if (!have || h->P.np <= 0) {
    h->err = "nlps_gpu_debug_damage_runs: no such run table has been built";
    return 1;
  }
  const size_t np = (size_t)h->P.np, nn = (size_t)h->g.nnodes;
  DevBuf<int> kd;
  HIPCHK(kd.reserve(np));
  if (snapshot) hipLaunchKernelGGL(k_debug_slot_node<true>, dim3(nblk((int)np)), dim3(BLK), 0, h->stream, h->P, (int)nn, kd.get());
  else hipLaunchKernelGGL(k_debug_slot_node<false>, dim3(nblk((int)np)), dim3(BLK), 0, h->stream, h->P, (int)nn, kd.get());
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(key, kd.get(), np * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(first, snapshot ? h->dmg.first0.get() : h->dmg.first.get(), nn * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(last, snapshot ? h->dmg.last0.get() : h->dmg.last.get(), nn * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(sorted, snapshot ? h->dmg.sorted0.get() : h->dmg.sorted.get(), np * sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

// developer read-out: how often the node runs of the current closest nodes were built, and how many residual evaluations
// took the fused damage form (tests: the runs are reused inside a solve; NLPS_LAGR_SEPARATE stays on the separate stages)
extern "C" __attribute__((visibility("default"))) int nlps_gpu_debug_damage_counters(nlps_gpu* h, int* run_builds, int* fused_evaluations) {
  *run_builds = h->dmg.builds;
  *fused_evaluations = h->dmg.fused_evals;
  return 0;
}

extern "C" int nlps_gpu_destroy(nlps_gpu* h) {
  if (!h) return 0;
  (void)nlps_gpu_rccl_detach(h);
  h->snap = {};  // (waits for the copies in flight)
  (void)materialise_move(h);  // (nothing reads it any more; the handle just never dies with a state half written)
  (void)hipStreamSynchronize(h->stream);
  for (int i = 0; i < 8; i++) (void)hipEventDestroy(h->ev[i]);
  for (hipEvent_t e : h->evw)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : h->loads_ev)
    if (e) (void)hipEventDestroy(e);
  // the members free their memory here: after the synchronise above, before the stream they were used on goes
  const hipStream_t owned = h->own_stream ? h->stream : nullptr;
  delete h;
  if (owned) (void)hipStreamDestroy(owned);
  return 0;
}

static int download_field(nlps_gpu* h, int f, int ncomp, double* dst, int stride, std::vector<double>& tmp) {
  if (!dst) return 0;
  int np = h->P.np;
  for (int c = 0; c < ncomp; c++) {
    HIPCHK(hipMemcpy(tmp.data(), h->P.d + (size_t)(f + c) * h->P.npad, (size_t)np * sizeof(double),
                     hipMemcpyDeviceToHost));
    for (int s = 0; s < np; s++) dst[(size_t)h->perm[s] * stride + c] = tmp[s];
  }
  return 0;
}

static int materialise_roll(nlps_gpu* h);

extern "C" int nlps_gpu_download_state(nlps_gpu* h, nlps_particles* o) {
  if (materialise_roll(h)) return 1;
  HIPCHK(hipStreamSynchronize(h->stream));
  if (refresh_perm(h)) return 1;
  int ND = h->nd, T = h->T, np = h->P.np;
  std::vector<double> tmp(h->P.npad);
  if (download_field(h, F_X, ND, o->x_GC, ND, tmp)) return 1;
  if (download_field(h, F_DIS, ND, o->dis, ND, tmp)) return 1;
  if (download_field(h, F_VEL, ND, o->vel, ND, tmp)) return 1;
  if (download_field(h, F_ACC, ND, o->acc, ND, tmp)) return 1;
  if (download_field(h, fFN(h->P), T, o->F_n, T, tmp)) return 1;
  if (download_field(h, fFN1(h->P), T, o->F_n1, T, tmp)) return 1;
  if (download_field(h, F_DF, T, o->DF, T, tmp)) return 1;
  if (download_field(h, F_TAU, T, o->Stress, T, tmp)) return 1;
  if (download_field(h, fBEN(h->P), T, o->b_e_n, T, tmp)) return 1;
  if (download_field(h, fBEN1(h->P), T, o->b_e_n1, T, tmp)) return 1;
  if (download_field(h, F_JN, 1, o->J_n, 1, tmp)) return 1;
  if (download_field(h, F_JN1, 1, o->J_n1, 1, tmp)) return 1;
  if (download_field(h, F_RHO, 1, o->rho, 1, tmp)) return 1;
  if (download_field(h, F_MASS, 1, o->mass, 1, tmp)) return 1;
  if (download_field(h, F_VOL0, 1, o->Vol_0, 1, tmp)) return 1;
  if (download_field(h, F_W, 1, o->W, 1, tmp)) return 1;
  if (download_field(h, F_KN, 1, o->Kappa_n, 1, tmp)) return 1;
  if (download_field(h, F_KN1, 1, o->Kappa_n1, 1, tmp)) return 1;
  if (download_field(h, F_EN, 1, o->EPS_n, 1, tmp)) return 1;
  if (download_field(h, F_EN1, 1, o->EPS_n1, 1, tmp)) return 1;
  if (download_field(h, F_LAM, ND, o->lambda, ND, tmp)) return 1;
  if (download_field(h, F_BETA, 1, o->Beta, 1, tmp)) return 1;
  if (download_field(h, F_DTFN, T, o->dt_F_n, T, tmp)) return 1;
  if (download_field(h, F_DTFN1, T, o->dt_F_n1, T, tmp)) return 1;
  if (download_field(h, F_DTDF, T, o->dt_DF, T, tmp)) return 1;
  if (download_field(h, F_CEP, ND * ND, o->C_ep, ND * ND, tmp)) return 1;
  if (download_field(h, F_BACK, 3, o->Back_stress, 3, tmp)) return 1;
  if (download_field(h, F_DMG, 1, o->Damage_n, 1, tmp)) return 1;
  if (download_field(h, F_DMG1, 1, o->Damage_n1, 1, tmp)) return 1;
  if (download_field(h, F_STRF, 1, o->Strain_f_n, 1, tmp)) return 1;
  if (download_field(h, F_STRF1, 1, o->Strain_f_n1, 1, tmp)) return 1;
  if (o->I0) {
    std::vector<int> it(np);
    HIPCHK(hipMemcpy(it.data(), h->P.I0, (size_t)np * sizeof(int), hipMemcpyDeviceToHost));
    for (int s = 0; s < np; s++) o->I0[h->perm[s]] = it[s];
  }
  return 0;
}

extern "C" int nlps_gpu_download_lists(nlps_gpu* h, int* nn_out, int* list) {
  HIPCHK(hipStreamSynchronize(h->stream));
  if (refresh_perm(h)) return 1;
  int np = h->P.np, ND = h->nd;
  std::vector<int> I0(np);
  std::vector<u64> lo(np), hi(np);
  HIPCHK(hipMemcpy(I0.data(), h->P.I0, (size_t)np * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(lo.data(), h->P.mlo, (size_t)np * sizeof(u64), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hi.data(), h->P.mhi, (size_t)np * sizeof(u64), hipMemcpyDeviceToHost));
  const GridD& g = h->g;
  for (int s = 0; s < np; s++) {
    int p = h->perm[s];
    int ijk[3] = {I0[s] % g.n[0], (I0[s] / g.n[0]) % g.n[1], I0[s] / (g.n[0] * g.n[1])};
    int cls = 0, mul = 1;
    for (int a = 0; a < 3; a++) {
      cls += (a < ND ? nlps_host::class5(ijk[a], g.n[a]) : 2) * mul;
      mul *= 5;
    }
    // walk NodalLocality[I0] in chain order, keep members, then reverse (prepend-push, LME.c:1077)
    int tmp[NLPS_MAXNB], nt = 0;
    for (int q = 0; q < h->tab.count2[cls]; q++) {
      int b = h->tab.order2[cls][q];
      bool on = b < 64 ? ((lo[s] >> b) & 1ull) : ((hi[s] >> (b - 64)) & 1ull);
      if (!on) continue;
      int i = b % 5, j = (b / 5) % 5, k = b / 25;
      tmp[nt++] = I0[s] + (i - 2) + g.n[0] * ((j - 2) + (ND == 3 ? g.n[1] * (k - 2) : 0));
    }
    nn_out[p] = nt;
    for (int a = 0; a < nt; a++) list[(size_t)p * NLPS_MAXNB + a] = tmp[nt - 1 - a];
    for (int a = nt; a < NLPS_MAXNB; a++) list[(size_t)p * NLPS_MAXNB + a] = -1;
  }
  return 0;
}

static int check_status(nlps_gpu* h, int fatal_mask, const char* where, bool mirrored = false);
// Level A: the shape functions themselves.  One thread per requested particle (device slot): p_a = e_a / Z for the 5^d
// stencil slots (0 for non-members) and dp_a = -p_a J^-1 l_a (LME.c:836-891: r and J from the same p), written per SLOT;
// the host puts them into the particle's list order (the walk of nlps_gpu_download_lists).
template <int ND>
__global__ void k_shape_slots(PView P, GridD g, const int* __restrict__ slots, int n, double* __restrict__ Ns,
                              double* __restrict__ dNs, int* __restrict__ gstatus) {
  constexpr int NS = (ND == 3) ? 125 : 25, KN = Lme<ND>::KN;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const int p = slots[q];
  double* Nq = Ns + (size_t)q * NS;
  double* dq = dNs + (size_t)q * NS * ND;
  for (int b = 0; b < NS; b++) {
    Nq[b] = 0.0;
    for (int a = 0; a < ND; a++) dq[b * ND + a] = 0.0;
  }
  Lme<ND> c;
  double lam[ND], beta;
  if (!load_lme<ND>(P, g, p, c, lam, beta)) return;
  // plain sums in slot order (not the wave-cooperative row form of the step kernels: lanes hold unrelated particles here)
  double Z = 0.0;
  for (int b = 0; b < NS; b++)
    if (c.on(b)) Z += c.ex[b % 5] * c.ey[(b / 5) % 5] * ((ND == 3) ? c.ez[(b / 25) % KN] : 1.0);
  const double Zinv = 1.0 / Z;
  double r[ND], J[ND * ND], Jm1[ND * ND];
  for (int a = 0; a < ND; a++) r[a] = 0.0;
  for (int a = 0; a < ND * ND; a++) J[a] = 0.0;
  for (int b = 0; b < NS; b++) {
    if (!c.on(b)) continue;
    const int i = b % 5, j = (b / 5) % 5, k = b / 25;
    const double pa = c.ex[i] * c.ey[j] * ((ND == 3) ? c.ez[k % KN] : 1.0) * Zinv;
    const double l[3] = {c.lx[i], c.ly[j], (ND == 3) ? c.lz[k % KN] : 0.0};
    for (int a = 0; a < ND; a++) {
      r[a] += pa * l[a];
      for (int m = 0; m < ND; m++) J[a * ND + m] += pa * l[a] * l[m];
    }
  }
  for (int a = 0; a < ND; a++)
    for (int m = 0; m < ND; m++) J[a * ND + m] -= r[a] * r[m];
  if (!inverse<ND>(Jm1, J)) {
    atomicOr(&P.status[p], ST_NEWTON);
    atomicOr(gstatus, ST_NEWTON);
    return;
  }
  for (int b = 0; b < NS; b++) {
    if (!c.on(b)) continue;
    const int i = b % 5, j = (b / 5) % 5, k = b / 25;
    const double pa = c.ex[i] * c.ey[j] * ((ND == 3) ? c.ez[k % KN] : 1.0) * Zinv;
    const double l[3] = {c.lx[i], c.ly[j], (ND == 3) ? c.lz[k % KN] : 0.0};
    Nq[b] = pa;
    for (int a = 0; a < ND; a++) {
      double v = 0.0;
      for (int m = 0; m < ND; m++) v += Jm1[a * ND + m] * l[m];
      dq[b * ND + a] = -pa * v;
    }
  }
}

extern "C" int nlps_gpu_shape_functions(nlps_gpu* h, int first, int count, double* N_out, double* dN_out) {
  const int np = h->P.np, ND = h->nd, NS = ND == 3 ? 125 : 25;
  if (first < 0 || count < 0 || first + count > np) {
    h->err = "nlps_gpu_shape_functions(): particle range outside the cloud";
    return 1;
  }
  if (count == 0) return 0;
  if (materialise_move(h)) return 1;
  if (refresh_perm(h)) return 1;
  // device slots of the caller's particles first .. first + count - 1
  std::vector<int> slot_of(np), slots(count), I0(np);
  for (int s = 0; s < np; s++) slot_of[h->perm[s]] = s;
  for (int q = 0; q < count; q++) slots[q] = slot_of[first + q];
  DevBuf<int> slots_d;
  DevBuf<double> Ns_d, dNs_d;
  HIPCHK(slots_d.reserve((size_t)count));
  HIPCHK(Ns_d.reserve((size_t)count * NS));
  HIPCHK(dNs_d.reserve((size_t)count * NS * ND));
  HIPCHK(hipMemcpyAsync(slots_d, slots.data(), (size_t)count * sizeof(int), hipMemcpyHostToDevice, h->stream));
  LAUNCH_ND(k_shape_slots<2>, k_shape_slots<3>, nblk(count), h->P, h->g, slots_d, count, Ns_d, dNs_d, h->gstatus_d);
  HIPCHK(hipGetLastError());
  std::vector<double> Ns((size_t)count * NS), dNs((size_t)count * NS * ND);
  std::vector<u64> lo(np), hi(np);
  HIPCHK(hipMemcpyAsync(Ns.data(), Ns_d, Ns.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(dNs.data(), dNs_d, dNs.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(I0.data(), h->P.I0, (size_t)np * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(lo.data(), h->P.mlo, (size_t)np * sizeof(u64), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hi.data(), h->P.mhi, (size_t)np * sizeof(u64), hipMemcpyDeviceToHost));
  const GridD& g = h->g;
  for (int q = 0; q < count; q++) {
    const int s = slots[q];
    int ijk[3] = {I0[s] % g.n[0], (I0[s] / g.n[0]) % g.n[1], I0[s] / (g.n[0] * g.n[1])};
    int cls = 0, mul = 1;
    for (int a = 0; a < 3; a++) {
      cls += (a < ND ? nlps_host::class5(ijk[a], g.n[a]) : 2) * mul;
      mul *= 5;
    }
    int tmp[NLPS_MAXNB], nt = 0;  // the members in chain order, then reversed: the order of ListNodes (nlps_gpu_download_lists)
    for (int w = 0; w < h->tab.count2[cls]; w++) {
      const int b = h->tab.order2[cls][w];
      const bool on = b < 64 ? ((lo[s] >> b) & 1ull) : ((hi[s] >> (b - 64)) & 1ull);
      if (on) tmp[nt++] = b;
    }
    for (int a = 0; a < NLPS_MAXNB; a++) {
      const int b = a < nt ? tmp[nt - 1 - a] : -1;
      if (N_out) N_out[(size_t)q * NLPS_MAXNB + a] = b >= 0 ? Ns[(size_t)q * NS + b] : 0.0;
      if (dN_out)
        for (int d = 0; d < ND; d++)
          dN_out[((size_t)q * NLPS_MAXNB + a) * ND + d] = b >= 0 ? dNs[((size_t)q * NS + b) * ND + d] : 0.0;
    }
  }
  return check_status(h, ST_NEWTON, "nlps_gpu_shape_functions()");
}

extern "C" int nlps_gpu_download_active(nlps_gpu* h, unsigned char* active) {
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(active, h->N.active, (size_t)h->g.nnodes, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int nlps_gpu_status_flags(nlps_gpu* h, int* flags) {
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(flags, h->gstatus_d, sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}


// ------------------------------------------------------------------------------------------------
// Ghost-layer exchange over RCCL, owned by the library (no Python, no callback).
// Slab partition along the slowest grid axis: rank r may touch node layers [lo[r], hi[r]]; the layers it shares with
// rank r-1 / r+1 are one contiguous slice of every grid-numbered nodal array.  An exchange = ncclSend of the slice
// + ncclRecv of the neighbour's into a receive buffer (one group, two xGMI links busy at once), then slice += buffer
// (sums) or slice = max(slice, buffer) (flags).  Mode 1 keeps the simple all-reduce of the whole array.
// Phases (nlps_halo_fn): 0 = in the order of the handle's stream; 1 = on the library's side stream, behind everything
// queued on the handle's stream so far; 2 = the handle's stream waits for it.
// ------------------------------------------------------------------------------------------------
struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;
};
static RcclApi g_rccl;
static const char* rccl_load() {  // nullptr = loaded
  if (g_rccl.lib) return nullptr;
  // the soname every ROCm build of RCCL carries: a copy the host process has loaded already (torch's, the MPI
  // driver's) is reused, otherwise the system one is loaded
  void* L = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!L) L = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!L) return "librccl.so.1 not found (dlopen)";
#define NLPS_SYM(field, name)                                  \
  *(void**)(&g_rccl.field) = dlsym(L, name);                   \
  if (!g_rccl.field) return "RCCL symbol missing: " name;
  NLPS_SYM(GetUniqueId, "ncclGetUniqueId")
  NLPS_SYM(CommInitRank, "ncclCommInitRank")
  NLPS_SYM(CommDestroy, "ncclCommDestroy")
  NLPS_SYM(GroupStart, "ncclGroupStart")
  NLPS_SYM(GroupEnd, "ncclGroupEnd")
  NLPS_SYM(Send, "ncclSend")
  NLPS_SYM(Recv, "ncclRecv")
  NLPS_SYM(AllReduce, "ncclAllReduce")
  NLPS_SYM(Reduce, "ncclReduce")
  NLPS_SYM(GetErrorString, "ncclGetErrorString")
  NLPS_SYM(CommCount, "ncclCommCount")
  NLPS_SYM(CommUserRank, "ncclCommUserRank")
  NLPS_SYM(CommAbort, "ncclCommAbort")
#undef NLPS_SYM
  g_rccl.lib = L;
  return nullptr;
}

struct RcclHalo {
  ncclComm_t comm = nullptr;
  bool own_comm = false;
  int rank = 0, world = 1, mode = 0;  // mode 0: neighbour send/recv, 1: all-reduce of the whole array
  std::vector<int> lo, hi;            // node layers rank r may touch (inclusive)
  hipStream_t side = nullptr;
  DevBuf<char> rbuf[2];  // receive buffers: from rank-1, from rank+1
  struct Ev {
    hipEvent_t start = nullptr, done = nullptr;
    bool pending = false;
  };
  std::map<const void*, Ev> ev;  // one pair of events per nodal array, re-recorded every step
  bool self_loop = false;        // world 1 self-test: the rank is its own two neighbours
  DevBuf<int> mig_cnt_d;         // nlps_gpu_rccl_migrate: {rows to below, rows to above, rows from below, rows from above}
  // single-launch overlap (TileD::sig_flag): counters in device memory, flags in signal memory, one pair per stage
  DevBuf<unsigned> sig_cnt;      // [2]
  DevBuf<unsigned> sig_flag[2];
  unsigned sig_seq = 0;
  bool can_wait_value = false;
};

// Holds the exchange stream until the boundary tiles of the launch in flight on the handle's stream have published
// `seq` (tile_signal).  One lane polls an agent-scope load with s_sleep in between; it occupies one wave slot of one CU
// and depends on nothing but the flag, and it gives up after about one second of the constant 100 MHz clock
// (wall_clock64), so that a launch that never happens cannot hang it (hipStreamWaitValue32 does the same through the
// host: measured 55 us from the store to the next command, against a few us for this kernel).
__global__ void k_wait_flag(const unsigned* __restrict__ flag, unsigned seq, int* __restrict__ gstatus) {
  if (threadIdx.x != 0) return;
  const unsigned long long t0 = wall_clock64();
  while (wall_clock64() - t0 < 100000000ull) {
    const unsigned v = __hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
    if ((int)(v - seq) >= 0) return;
    __builtin_amdgcn_s_sleep(32);
  }
  atomicOr(gstatus, ST_HALO);  // timed out: reported like a particle outside the node window
}

template <class T>
__global__ void k_halo_add(T* __restrict__ a, const T* __restrict__ b, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] += b[i];
}
__global__ void k_halo_max(unsigned char* __restrict__ a, const unsigned char* __restrict__ b, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] = a[i] > b[i] ? a[i] : b[i];
}

#define RCCLCHK(call)                                                                                   \
  do {                                                                                                  \
    ncclResult_t r_ = (call);                                                                           \
    if (r_ != ncclSuccess) {                                                                            \
      h->err = std::string(#call) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r_) : "?");   \
      fprintf(stderr, "\033[1;31mError in nlps_gpu (RCCL): %s\033[0m\n", h->err.c_str());               \
      return 1;                                                                                         \
    }                                                                                                   \
  } while (0)

// the exchange itself, in the order of stream s
static int rccl_exchange_on(nlps_gpu* h, void* dptr, int nfield, int elem, int kind, hipStream_t s) {
  RcclHalo* R = h->rccl;
  const int nl = h->g.n[h->nd - 1];
  const size_t plane = (size_t)h->g.nnodes / nl;
  const ncclDataType_t dt = elem == 8 ? ncclDouble : ncclUint8;
  if (R->mode == 1) {
    if (R->world > 1)
      RCCLCHK(g_rccl.AllReduce(dptr, dptr, (size_t)h->g.nnodes * nfield, dt, kind == 0 ? ncclSum : ncclMax, R->comm, s));
    return 0;
  }
  struct Part {
    char* sl;
    size_t count;
    int peer, k;
  } parts[2];
  int np = 0;
  for (int k = 0; k < 2; k++) {
    const int nb = R->rank + (k == 0 ? -1 : 1);
    int a, b;
    if (R->self_loop) {  // self-test: the lowest / highest three layers stand for the two shared slices
      a = k == 0 ? R->lo[0] : std::max(R->lo[0], R->hi[0] - 2);
      b = k == 0 ? std::min(R->hi[0], R->lo[0] + 2) : R->hi[0];
    } else {
      if (nb < 0 || nb >= R->world) continue;
      a = std::max(R->lo[R->rank], R->lo[nb]);
      b = std::min(R->hi[R->rank], R->hi[nb]);
      if (a > b) continue;
    }
    const size_t count = (size_t)(b - a + 1) * plane * nfield, bytes = count * elem;
    if (bytes > R->rbuf[k].size()) {
      HIPCHK(hipDeviceSynchronize());
      HIPCHK(R->rbuf[k].reserve(bytes));
    }
    parts[np++] = {(char*)dptr + (size_t)a * plane * nfield * elem, count, R->self_loop ? R->rank : nb, k};
  }
  if (np == 0) return 0;
  RCCLCHK(g_rccl.GroupStart());
  for (int q = 0; q < np; q++) {
    // self-test: what goes "down" comes back as what arrives "from above" and vice versa
    RCCLCHK(g_rccl.Send(parts[q].sl, parts[q].count, dt, parts[q].peer, R->comm, s));
    RCCLCHK(g_rccl.Recv(R->rbuf[R->self_loop ? 1 - parts[q].k : parts[q].k].get(), parts[q].count, dt, parts[q].peer, R->comm, s));
  }
  RCCLCHK(g_rccl.GroupEnd());
  // after the sends in stream order, so the neighbour got the un-summed slice
  for (int q = 0; q < np; q++) {
    const size_t n = parts[q].count;
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (elem == 8 && kind == 0)
      hipLaunchKernelGGL(k_halo_add<double>, dim3(grid), dim3(256), 0, s, (double*)parts[q].sl, (const double*)R->rbuf[parts[q].k].get(), n);
    else
      hipLaunchKernelGGL(k_halo_max, dim3(grid), dim3(256), 0, s, (unsigned char*)parts[q].sl, (const unsigned char*)R->rbuf[parts[q].k].get(), n);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

static int rccl_halo(nlps_gpu* h, void* dptr, int nfield, int elem, int kind, int phase) {
  RcclHalo* R = h->rccl;
  // (a rank without neighbours still goes through the stream choreography: that is how a one-GPU box rehearses it)
  if (phase == 0) {
    // the receive buffers are shared with the side stream: an exchange still pending there finishes first
    for (auto& kv : R->ev)
      if (kv.second.pending) {
        HIPCHK(hipStreamWaitEvent(h->stream, kv.second.done, 0));
        kv.second.pending = false;
      }
    return rccl_exchange_on(h, dptr, nfield, elem, kind, h->stream);
  }
  RcclHalo::Ev& e = R->ev[dptr];
  if (!e.start) {
    HIPCHK(hipEventCreateWithFlags(&e.start, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&e.done, hipEventDisableTiming));
  }
  if (phase == 1) {
    HIPCHK(hipEventRecord(e.start, h->stream));
    HIPCHK(hipStreamWaitEvent(R->side, e.start, 0));
    if (rccl_exchange_on(h, dptr, nfield, elem, kind, R->side)) return 1;
    HIPCHK(hipEventRecord(e.done, R->side));
    e.pending = true;
    return 0;
  }
  if (phase == 3 || phase == 4) {  // start behind the boundary tiles of the launch that is in flight (stage 0 = K2, 1 = K3)
    const int stage = phase - 3;
    hipLaunchKernelGGL(k_wait_flag, dim3(1), dim3(64), 0, R->side, R->sig_flag[stage], R->sig_seq, h->gstatus_d);
    if (rccl_exchange_on(h, dptr, nfield, elem, kind, R->side)) return 1;
    HIPCHK(hipEventRecord(e.done, R->side));
    e.pending = true;
    return 0;
  }
  if (e.pending) {
    HIPCHK(hipStreamWaitEvent(h->stream, e.done, 0));
    e.pending = false;
  }
  return 0;
}

extern "C" int nlps_gpu_rccl_unique_id(void* id128) {
  if (rccl_load()) return 1;
  ncclUniqueId id;
  if (g_rccl.GetUniqueId(&id) != ncclSuccess) return 1;
  memcpy(id128, &id, NCCL_UNIQUE_ID_BYTES);
  return 0;
}

extern "C" int nlps_gpu_rccl_detach(nlps_gpu* h);
static int rccl_attach_common(nlps_gpu* h, ncclComm_t comm, bool own, int rank, int world, const int* layer_lo,
                              const int* layer_hi, int mode) {
  if (h->rccl) {
    h->err = "nlps_gpu_rccl_attach: a communicator is attached already (nlps_gpu_rccl_detach first)";
    return 1;
  }
  if (materialise_nodal(h)) return 1;  // (window and bands change below)
  const int nl = h->g.n[h->nd - 1];
  if (world < 1 || rank < 0 || rank >= world || (mode != 0 && mode != 1)) {
    h->err = "nlps_gpu_rccl_attach: bad rank / world / mode";
    return 1;
  }
  RcclHalo* R = new RcclHalo();
  R->comm = comm;
  R->own_comm = own;
  R->rank = rank;
  R->world = world;
  R->mode = mode;
  for (int r = 0; r < world; r++) {
    const int a = layer_lo ? layer_lo[r] : 0, b = layer_hi ? layer_hi[r] : nl - 1;
    if (a < 0 || b >= nl || a > b) {
      delete R;
      h->err = "nlps_gpu_rccl_attach: layer range outside the grid";
      return 1;
    }
    R->lo.push_back(a);
    R->hi.push_back(b);
  }
  for (int r = 0; r + 2 < world; r++)
    if (R->hi[r] >= R->lo[r + 2]) {
      delete R;
      h->err = "nlps_gpu_rccl_attach: slabs too thin (a rank overlaps its second neighbour)";
      return 1;
    }
  if (hipStreamCreateWithFlags(&R->side, hipStreamNonBlocking) != hipSuccess) {
    delete R;
    h->err = "nlps_gpu_rccl_attach: hipStreamCreateWithFlags failed";
    return 1;
  }
  {
    bool ok = R->sig_cnt.alloc_zeroed(2) == hipSuccess;
    for (int k = 0; k < 2 && ok; k++) ok = R->sig_flag[k].alloc_zeroed(2) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    R->can_wait_value = ok;
  }
  h->rccl = R;
  h->rccl_wait_value = R->can_wait_value;
  // ghost bands (layers shared with a neighbour) and the node window follow from the layer ranges
  const int band_lo = rank > 0 ? std::min(R->hi[rank], R->hi[rank - 1]) : -1;
  const int band_hi = rank + 1 < world ? std::max(R->lo[rank], R->lo[rank + 1]) : nl;
  h->band_lo = rank > 0 && R->hi[rank - 1] >= R->lo[rank] ? band_lo : -(1 << 30);
  h->band_hi = rank + 1 < world && R->lo[rank + 1] <= R->hi[rank] ? band_hi : (1 << 30);
  // 2: one launch per stage, the exchange released by the boundary tiles through signal memory; 1: split launches
  h->overlap = world > 1 ? (R->can_wait_value ? 2 : 1) : 0;
  if (world > 1 && nlps_gpu_set_node_window(h, R->lo[rank], R->hi[rank])) {
    // the handle must not keep a half-attached exchange: the caller still owns `comm` (it destroys its own, or the
    // wrapper below destroys the one it made), so the detach here must leave it alone
    const std::string err = h->err;
    R->own_comm = false;
    (void)nlps_gpu_rccl_detach(h);
    h->err = err;
    return 1;
  }
  return 0;
}

extern "C" int nlps_gpu_rccl_attach(nlps_gpu* h, const void* id128, int rank, int world, const int* layer_lo,
                                    const int* layer_hi, int mode) {
  if (const char* e = rccl_load()) {
    h->err = e;
    return 1;
  }
  if (h->rccl) {  // before the collective below: a second attach must not block on (or create) a communicator
    h->err = "nlps_gpu_rccl_attach: a communicator is attached already (nlps_gpu_rccl_detach first)";
    return 1;
  }
  ncclUniqueId id;
  memcpy(&id, id128, NCCL_UNIQUE_ID_BYTES);
  ncclComm_t comm = nullptr;
  RCCLCHK(g_rccl.CommInitRank(&comm, world, id, rank));
  if (rccl_attach_common(h, comm, true, rank, world, layer_lo, layer_hi, mode)) {
    (void)g_rccl.CommDestroy(comm);
    return 1;
  }
  return 0;
}

extern "C" int nlps_gpu_rccl_attach_comm(nlps_gpu* h, void* nccl_comm, int rank, int world, const int* layer_lo,
                                         const int* layer_hi, int mode) {
  if (const char* e = rccl_load()) {
    h->err = e;
    return 1;
  }
  return rccl_attach_common(h, (ncclComm_t)nccl_comm, false, rank, world, layer_lo, layer_hi, mode);
}

extern "C" int nlps_gpu_rccl_detach(nlps_gpu* h) {
  RcclHalo* R = h->rccl;
  if (!R) return 0;
  if (materialise_nodal(h)) return 1;
  (void)hipDeviceSynchronize();
  for (auto& kv : R->ev) {
    if (kv.second.start) (void)hipEventDestroy(kv.second.start);
    if (kv.second.done) (void)hipEventDestroy(kv.second.done);
  }
  for (int k = 0; k < 2; k++) {  // (the buffers go before the stream and the communicator that used them)
    R->rbuf[k].reset();
    R->sig_flag[k].reset();
  }
  R->sig_cnt.reset();
  R->mig_cnt_d.reset();
  if (R->side) (void)hipStreamDestroy(R->side);
  if (R->own_comm && R->comm) (void)g_rccl.CommDestroy(R->comm);
  delete R;
  h->rccl = nullptr;
  h->rccl_wait_value = false;
  h->overlap = 0;
  h->band_lo = -(1 << 30);
  h->band_hi = 1 << 30;
  return 0;
}

// Implicit driver on several ranks: the masked residual / lumped-mass vector of every rank summed onto
// the rank that runs the PETSc solve (root >= 0) or onto all ranks (root < 0).  vec: device pointer, n doubles.
extern "C" int nlps_gpu_rccl_reduce(nlps_gpu* h, double* vec, size_t n, int root) {
  RcclHalo* R = h->rccl;
  if (!R) {
    h->err = "nlps_gpu_rccl_reduce: no communicator attached";
    return 1;
  }
  if (R->world == 1 || n == 0) return 0;
  if (root < 0) RCCLCHK(g_rccl.AllReduce(vec, vec, n, ncclDouble, ncclSum, R->comm, h->stream));
  else RCCLCHK(g_rccl.Reduce(vec, vec, n, ncclDouble, ncclSum, root, R->comm, h->stream));
  return 0;
}

// World-size-1 self-test of the exchange machinery (a one-GPU box cannot hold two ranks): the rank acts as its own
// two neighbours, i.e. the lowest three layers of its range are exchanged with the highest three through
// ncclSend / ncclRecv to itself.  After the call array[low slice] += old array[high slice] and vice versa.
extern "C" int nlps_gpu_rccl_selftest_exchange(nlps_gpu* h, void* dptr, int nfield, int elem_bytes, int kind, int overlap) {
  RcclHalo* R = h->rccl;
  if (!R || R->world != 1) {
    h->err = "nlps_gpu_rccl_selftest_exchange: needs an attached communicator of world size 1";
    return 1;
  }
  R->self_loop = true;
  int st = 0;
  if (overlap) st = rccl_halo(h, dptr, nfield, elem_bytes, kind, 1) || rccl_halo(h, dptr, nfield, elem_bytes, kind, 2);
  else st = rccl_halo(h, dptr, nfield, elem_bytes, kind, 0);
  R->self_loop = false;
  return st;
}

static int halo_dispatch(nlps_gpu* h, void* dptr, int nfield, int elem, int kind, int phase);
// What the attached communicator says about itself (ncclCommCount / ncclCommUserRank: the rank count RCCL really
// runs with, not the one the caller asked for) and the overlap choreography in force (0 blocking, 1 split launches,
// 2 one launch per stage).
extern "C" int nlps_gpu_rccl_info(nlps_gpu* h, int* nranks, int* rank, int* overlap_mode) {
  RcclHalo* R = h->rccl;
  if (!R) {
    h->err = "nlps_gpu_rccl_info: no communicator attached";
    return 1;
  }
  int n = 0, r = 0;
  RCCLCHK(g_rccl.CommCount(R->comm, &n));
  RCCLCHK(g_rccl.CommUserRank(R->comm, &r));
  if (nranks) *nranks = n;
  if (rank) *rank = r;
  if (overlap_mode) *overlap_mode = h->overlap;
  return 0;
}

// Particle migration between slab ranks with the transport inside the library (a C driver needs no Python):
// select + pack (nlps_gpu_migration_select), the row counts and then the rows themselves exchanged with the two
// neighbours by ncclSend / ncclRecv on the handle's stream, commit.  self_loop (world 1 only): the rank is its own two
// neighbours, so what leaves comes straight back -- every call on the wire runs on a one-GPU box.
// Collective: every rank makes the same sequence of RCCL calls whatever happens locally.  A rank whose select fails or
// whose capacity would overflow says so in a status word that all ranks agree on (one 4-byte all-reduce) BEFORE any row
// moves: then every rank returns 1 with its cloud unchanged (a select without commit has no effect).  A HIP / RCCL error
// after that point cannot be negotiated: the communicator is aborted so that the peers get an error, never a hang.
static int rccl_migrate(nlps_gpu* h, int keep_lo, int keep_hi, int* sent_down, int* sent_up, int* received, bool self_loop) {
  RcclHalo* R = h->rccl;
  if (!R) {
    h->err = "nlps_gpu_rccl_migrate: no communicator attached (nlps_gpu_rccl_attach)";
    return 1;
  }
  if (self_loop && R->world != 1) {
    h->err = "nlps_gpu_rccl_selftest_migrate: needs an attached communicator of world size 1";
    return 1;
  }
  if (materialise_move(h)) return 1;  // (steps run before the communicator was attached)
  const int nl = h->g.n[h->nd - 1];
  if (!self_loop) {  // an edge rank has no neighbour on its outer side: nothing may be selected towards it
    if (R->rank == 0) keep_lo = 0;
    if (R->rank == R->world - 1) keep_hi = nl - 1;
  }
  DevBuf<double> rows_in[2];
  auto fatal = [&](const std::string& what) {  // unrecoverable local error in the middle of the collective
    h->err = "nlps_gpu_rccl_migrate: " + what + " (communicator aborted)";
    fprintf(stderr, "\033[1;31mError in nlps_gpu: %s\033[0m\n", h->err.c_str());
    for (int k = 0; k < 2; k++) rows_in[k].reset();
    if (R->comm) (void)g_rccl.CommAbort(R->comm);
    R->comm = nullptr;
    return 1;
  };
#define MIG_HIP(call)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess) return fatal(std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define MIG_RCCL(call)                                                                  \
  do {                                                                                  \
    ncclResult_t r_ = (call);                                                           \
    if (r_ != ncclSuccess) return fatal(std::string(#call) + ": " + g_rccl.GetErrorString(r_)); \
  } while (0)
  if (!R->comm) {
    h->err = "nlps_gpu_rccl_migrate: the communicator was aborted by an earlier failure";
    return 1;
  }
  int n_out[2] = {0, 0}, rw = 0;
  void* rows_out[2] = {nullptr, nullptr};
  int bad = nlps_gpu_migration_select(h, keep_lo, keep_hi, &n_out[0], &n_out[1], &rw, &rows_out[0], &rows_out[1]) ? 1 : 0;
  const std::string select_err = bad ? h->err : std::string();
  if (bad) n_out[0] = n_out[1] = 0;
  if (sent_down) *sent_down = n_out[0];
  if (sent_up) *sent_up = n_out[1];
  if (received) *received = 0;
  int peer[2] = {R->rank - 1, R->rank + 1};
  bool has[2] = {peer[0] >= 0, peer[1] < R->world};
  if (self_loop) {
    peer[0] = peer[1] = R->rank;
    has[0] = has[1] = true;
  }
  if (!has[0] && !has[1]) {  // world 1: nobody to agree with
    if (bad) return 1;
    return nlps_gpu_migration_commit(h, nullptr, 0, nullptr, 0);
  }
  MIG_HIP(R->mig_cnt_d.reserve(8));
  // 1. how many rows come from each neighbour
  int cnt[8] = {n_out[0], n_out[1], 0, 0, 0, 0, 0, 0};
  MIG_HIP(hipMemcpyAsync(R->mig_cnt_d, cnt, 8 * sizeof(int), hipMemcpyHostToDevice, h->stream));
  MIG_RCCL(g_rccl.GroupStart());
  for (int k = 0; k < 2; k++) {
    if (!has[k]) continue;
    // (self-loop: sends and receives between one pair match in the order posted, so what went "down" arrives as
    // "from below" -- which neighbour it stands for does not matter to the commit)
    MIG_RCCL(g_rccl.Send(R->mig_cnt_d + k, 1, ncclInt32, peer[k], R->comm, h->stream));
    MIG_RCCL(g_rccl.Recv(R->mig_cnt_d + 2 + k, 1, ncclInt32, peer[k], R->comm, h->stream));
  }
  MIG_RCCL(g_rccl.GroupEnd());
  MIG_HIP(hipMemcpyAsync(cnt, R->mig_cnt_d, 4 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  MIG_HIP(hipStreamSynchronize(h->stream));
  const int n_in[2] = {cnt[2], cnt[3]};
  const bool overflow = n_in[0] < 0 || n_in[1] < 0 || (size_t)h->P.np + n_in[0] + n_in[1] > h->P.npad;
  // 2. one status word for the whole communicator: 0 go, 1 some rank cannot
  int status[2] = {(bad || overflow) ? 1 : 0, 0};
  MIG_HIP(hipMemcpyAsync(R->mig_cnt_d + 4, status, sizeof(int), hipMemcpyHostToDevice, h->stream));
  MIG_RCCL(g_rccl.AllReduce(R->mig_cnt_d + 4, R->mig_cnt_d + 5, 1, ncclInt32, ncclMax, R->comm, h->stream));
  MIG_HIP(hipMemcpyAsync(status + 1, R->mig_cnt_d + 5, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  MIG_HIP(hipStreamSynchronize(h->stream));
  if (status[1] != 0) {  // every rank takes this branch together; nothing has moved, nothing is committed
    if (bad) h->err = select_err;
    else if (overflow) h->err = "nlps_gpu_rccl_migrate: more immigrants than the capacity reserved at create (np + max(np/4, 1024))";
    else h->err = "nlps_gpu_rccl_migrate: another rank of the communicator could not migrate (its select failed or its capacity is exhausted); no particle moved";
    return 1;
  }
  // 3. the rows
  for (int k = 0; k < 2; k++)
    if (n_in[k] > 0) MIG_HIP(rows_in[k].reserve((size_t)n_in[k] * rw));
  MIG_RCCL(g_rccl.GroupStart());
  for (int k = 0; k < 2; k++) {
    if (!has[k]) continue;
    if (n_out[k] > 0) MIG_RCCL(g_rccl.Send(rows_out[k], (size_t)n_out[k] * rw, ncclDouble, peer[k], R->comm, h->stream));
    if (n_in[k] > 0) MIG_RCCL(g_rccl.Recv(rows_in[k].get(), (size_t)n_in[k] * rw, ncclDouble, peer[k], R->comm, h->stream));
  }
  MIG_RCCL(g_rccl.GroupEnd());
  MIG_HIP(hipStreamSynchronize(h->stream));
#undef MIG_HIP
#undef MIG_RCCL
  const int st = nlps_gpu_migration_commit(h, rows_in[0].get(), n_in[0], rows_in[1].get(), n_in[1]);
  if (received) *received = n_in[0] + n_in[1];
  return st;
}
extern "C" int nlps_gpu_rccl_migrate(nlps_gpu* h, int keep_lo, int keep_hi, int* sent_down, int* sent_up, int* received) {
  return rccl_migrate(h, keep_lo, keep_hi, sent_down, sent_up, received, false);
}
extern "C" int nlps_gpu_rccl_selftest_migrate(nlps_gpu* h, int keep_lo, int keep_hi, int* sent_down, int* sent_up,
                                              int* received) {
  return rccl_migrate(h, keep_lo, keep_hi, sent_down, sent_up, received, true);
}

static int halo(nlps_gpu* h, void* dptr, int nfield, int elem, int kind, int phase = 0) {
  // (with timing on, the exchanges the handle's stream has to wait for -- blocking ones, and the pick-up of overlapped
  // ones -- are bracketed: their sum is what a step loses to communication, nlps_gpu_get_timing slot 6)
  const bool bracket = h->timing && (phase == 0 || phase == 2) && (h->rccl || h->halo) && h->nwait < 6;
  if (bracket) {
    if (!h->evw[2 * h->nwait]) {
      HIPCHK(hipEventCreate(&h->evw[2 * h->nwait]));
      HIPCHK(hipEventCreate(&h->evw[2 * h->nwait + 1]));
    }
    HIPCHK(hipEventRecord(h->evw[2 * h->nwait], h->stream));
  }
  const int st_ = halo_dispatch(h, dptr, nfield, elem, kind, phase);
  if (bracket) {
    HIPCHK(hipEventRecord(h->evw[2 * h->nwait + 1], h->stream));
    h->nwait++;
  }
  return st_;
}
static int halo_dispatch(nlps_gpu* h, void* dptr, int nfield, int elem, int kind, int phase) {
  if (h->rccl) return rccl_halo(h, dptr, nfield, elem, kind, phase);
  if (!h->halo) return 0;
  int st = h->halo(h->halo_ctx, dptr, nfield, elem, kind, phase);
  if (st) {
    h->err = "halo exchange callback failed";
    return 1;
  }
  return 0;
}



static int compute_node_mask(nlps_gpu* h) {
  int nn = h->g.nnodes, nb = (nn + 1023) / 1024;
  if (h->canon_d) {
    // the running index of get_active_nodes__MeshTools__ (Nodes-Tools.c:46-66) follows the mesh FILE's node order: scan
    // the flags in that order, then hand every lattice node its index
    hipLaunchKernelGGL(k_gather<unsigned char>, dim3(nblk(nn)), dim3(BLK), 0, h->stream, h->mask_flags_d,
                       (const unsigned char*)h->N.active, (const int*)h->canon_d, nn);
    hipLaunchKernelGGL(k_scan_count, dim3(nb), dim3(256), 0, h->stream, h->mask_flags_d, nn, 0, h->bsum_d);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, h->stream, h->bsum_d, nb, h->total_d);
    hipLaunchKernelGGL(k_scan_write, dim3(nb), dim3(256), 0, h->stream, h->mask_flags_d, nn, 0, h->bsum_d, h->mask_idx_d);
    hipLaunchKernelGGL(k_scatter<int>, dim3(nblk(nn)), dim3(BLK), 0, h->stream, h->n2m_d, (const int*)h->mask_idx_d,
                       (const int*)h->canon_d, nn);
    HIPCHK(hipGetLastError());
    return 0;
  }
  hipLaunchKernelGGL(k_scan_count, dim3(nb), dim3(256), 0, h->stream, h->N.active, nn, 0, h->bsum_d);
  hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, h->stream, h->bsum_d, nb, h->total_d);
  hipLaunchKernelGGL(k_scan_write, dim3(nb), dim3(256), 0, h->stream, h->N.active, nn, 0, h->bsum_d, h->n2m_d);
  HIPCHK(hipGetLastError());
  return 0;
}

// Masked numbering in the node order of the mesh file (see include/nlps_gpu.h)
extern "C" int nlps_gpu_set_node_numbering(nlps_gpu* h, const int* lattice_of_file) {
  const int nn = h->g.nnodes;
  h->masks_valid = false;
  if (!lattice_of_file) {
    if (h->canon_d) {
      HIPCHK(hipStreamSynchronize(h->stream));
      h->canon_d.reset();
    }
    return 0;
  }
  std::vector<unsigned char> seen(nn, 0);
  for (int A = 0; A < nn; A++) {
    const int l = lattice_of_file[A];
    if (l < 0 || l >= nn || seen[l]) {
      h->err = "nlps_gpu_set_node_numbering: lattice_of_file is not a permutation of the grid's nodes";
      return 1;
    }
    seen[l] = 1;
  }
  if (!h->canon_d) {
    HIPCHK(h->canon_d.reserve((size_t)nn));
    HIPCHK(h->mask_flags_d.reserve((size_t)nn));  // (these two stay when the numbering is taken back)
    HIPCHK(h->mask_idx_d.reserve((size_t)nn));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(h->canon_d, lattice_of_file, (size_t)nn * sizeof(int), hipMemcpyHostToDevice));
  return 0;
}

// canonical tile lists from per-node counters (TileTab) instead of the per-tile counting sort: every mode but the
// deterministic one (which needs ranks that do not depend on the arrival order of an atomic)
static bool node_lists(const nlps_gpu* h) { return !h->deterministic; }
static TileTab tile_tab(const nlps_gpu* h) {
  TileTab tab;
  for (int a = 0; a < 3; a++) tab.nt[a] = h->nt[a];
  tab.node_cnt = h->node_cnt_d;
  tab.mask = h->tabm_d;
  tab.base = h->tabo_d;
  return tab;
}
static TileCnt tile_cnt(nlps_gpu* h, bool on) {
  TileCnt tc;
  for (int a = 0; a < 3; a++) tc.nt[a] = h->nt[a];
  tc.count = on ? h->tile_count_d : nullptr;
  tc.tile0 = h->tile0;
  tc.ntw = h->ntw;
  tc.win_lo = h->win_lo;
  tc.win_hi = h->win_hi;
  tc.plane = h->g.nnodes / h->g.n[h->nd - 1];
  tc.gstatus = h->gstatus_d;
  tc.home = nullptr;
  tc.rehome = 0;
  tc.foreign = nullptr;
  tc.node_cnt = (on && node_lists(h)) ? h->node_cnt_d : nullptr;
  tc.nrank = h->nrank_d;
  tc.defer = 0;
  if (on && h->adaptive_resort > 0.0 && !h->deterministic) {
    tc.home = h->home_d;
    tc.foreign = h->foreign_d;
    tc.rehome = h->rehome ? 1 : 0;
    h->rehome = false;
  }
  return tc;
}
static TileD tile_view(nlps_gpu* h, int cls = 0) {  // cls: 0 all tiles, 1 boundary, 2 interior
  TileD td;
  for (int a = 0; a < 3; a++) td.nt[a] = h->nt[a];
  td.ntiles = h->ntiles;
  td.tile0 = h->tile0;
  td.ntw = h->ntw;
  td.slab = h->deterministic ? h->slab_d : nullptr;
  td.slab_n = 1;
  td.slab_slot = 0;
  td.sig_cnt = nullptr;
  td.sig_flag = nullptr;
  td.sig_seq = 0;
  td.work = h->lists.work;
  td.range = h->lists.nwork + 2 * cls;
  td.phase = h->phase_d;
  td.start = h->lists.start;
  td.count = h->tile_count_d;
  td.order_m = h->lists.order;
  td.order = h->lists.order2;
  return td;
}
// What the kernels that BUILD a list set take (k_dilate_scan, k_fill_orders): the nodal view with the flags and
// accumulators of that set (the seeds are the search's, whichever set) and the scan arguments.  count: the tile counters
// that size the set; cursor: TileScanArgs::cursor.
struct ListBuild {
  NView N;
  TileScanArgs ts;
};
static NView list_nview(const nlps_gpu* h, const nlps_gpu::ListSet& s) {
  NView N = h->N;
  N.active = s.active;
  N.fixed = s.fixed;
  N.nm = s.nm;
  N.force = s.force;
  return N;
}
static ListBuild list_build(nlps_gpu* h, const nlps_gpu::ListSet& s, const int* count, int* cursor) {
  const int TB = h->nd == 3 ? TileCfg<3>::TB : TileCfg<2>::TB;
  return {list_nview(h, s), {count + h->tile0, s.start + h->tile0, h->ntw, h->tile0, h->ntiles / h->nt[h->nd - 1], TB,
                             h->band_lo, h->band_hi, s.work, s.nwork, cursor}};
}
// h->N views the set in use
static void bind_lists(nlps_gpu* h) { h->N = list_nview(h, h->lists); }

// S1: closest node + activation (+ binning of the particles to I0-tiles when `tiled`), then lists,
// beta and the Newton iteration (+ predictor and P2G of mass / m*dD when `p2g`, tiled form only)
// node ranges of the per-step nodal kernels: part 0 = the whole node window, 1 = the nodes outside the ghost
// bands, 2 = the ghost bands (two ranges)
struct NodeRanges {
  int a0, an, b0, bn;
};
static NodeRanges node_ranges(nlps_gpu* h, int part) {
  const int plane = h->g.nnodes / h->g.n[h->nd - 1];
  const int lo = h->win_lo, hi = h->win_hi;
  const int il = std::max(lo, std::min(hi + 1, h->band_lo + 1));  // first layer outside the low band
  const int ih = std::min(hi + 1, std::max(il, h->band_hi));      // first layer of the high band
  if (part == 0) return {lo * plane, (hi - lo + 1) * plane, 0, 0};
  if (part == 1) return {il * plane, (ih - il) * plane, 0, 0};
  return {lo * plane, (il - lo) * plane, ih * plane, (hi + 1 - ih) * plane};
}

// The folded explicit step never stored dU, the accelerations and the reactions of its step: made here,
// from the nodal sums of that step, before somebody reads them or overwrites the sums they come from.
static int materialise_nodal(nlps_gpu* h) {
  if (!h->nodal_stale) return 0;
  const NodeRanges r = node_ranges(h, 0);
  LAUNCH_ND((k_nodal_dU<2>), (k_nodal_dU<3>), nblk(r.an + r.bn), r.a0, r.an, r.b0, r.bn, h->N, h->last_bm, h->last_bc);
  LAUNCH_ND((k_nodal_accel<2>), (k_nodal_accel<3>), nblk(r.an + r.bn), r.a0, r.an, r.b0, r.bn, h->N, h->last_gv[0],
            h->last_gv[1], h->last_gv[2], 0, (int*)nullptr, (int*)nullptr, 0);
  HIPCHK(hipGetLastError());
  h->nodal_stale = false;
  return 0;
}

// Deterministic mode on the implicit path (nlps_gpu_set_deterministic): the level-B scatters, the fused residual and the
// matrix-free tangent run one wave per tile over the exact canonical lists and leave their windows as slabs, which
// k_slab_gather sums per node in a fixed order.  One rank without a halo callback; a cloud with the damage hooks keeps
// the atomic path unless nlps_gpu_set_deterministic_damage is on.
static bool det_implicit(const nlps_gpu* h) {
  return h->deterministic && !h->halo && !h->rccl && (!h->P.erosion || h->det_damage) && h->P.np > 0;
}
// What a deterministic implicit-path call needs before its tile kernel: the exact lists and room for its slabs.  Lists
// that a search built with the mode off hold the same particles per tile, in an order that depends on binning
// atomics: the exact per-tile sort is run over them here (it reads the binned lists, whose CONTENT per tile is
// exact), so no sum ever runs over a non-exact list.  An exact list is a valid canonical list for every other kernel.
static int det_prepare(nlps_gpu* h, const char* who) {
  if (!h->lists_exact) {
    if (!h->binned || !h->lists.order2) {
      h->err = std::string(who) + ": deterministic mode needs tile lists: call nlps_gpu_local_search() first";
      return 1;
    }
    LAUNCH_ND_BLK((k_tile_order<2, true>), (k_tile_order<3, true>), h->ntw, 256, h->P, h->g, tile_view(h, 0), (const int*)h->lists.order,
                  h->lists.order2);
    HIPCHK(hipGetLastError());
    h->lists_exact = true;
  }
  return det_slab_reserve(h, who);
}
static int det_slab_reserve(nlps_gpu* h, const char* who) {
  const int ND = h->nd;
  // fields per window of the largest user: the explicit step (K2: 1 + d, K3: d per law, sized for four; the force half
  // of a damage step: d), the block diagonal (d^2), the nodal field (2 d) and the residual (d per law present)
  const size_t NWs = ND == 3 ? TileCfg<3>::NWA : TileCfg<2>::NWA;
  const size_t fields = std::max<size_t>(std::max<size_t>(4 * ND, ND * ND), (size_t)ND * __builtin_popcount(h->law_present));
  return reserve(h, who, h->slab_d, (size_t)h->ntiles * fields * NWs, "the window slabs of the deterministic mode");
}
// arms the boundary-done signal of a single-launch stage (overlap mode 2): stage 0 = K2, 1 = K3
static void arm_signal(nlps_gpu* h, TileD& td, int stage) {
  RcclHalo* R = h->rccl;
  td.sig_cnt = R->sig_cnt + stage;
  td.sig_flag = R->sig_flag[stage];
  td.sig_seq = ++R->sig_seq;
}

// K3: the one place that names k3_tile<ND, LAW, MODE, FILT, NT, UMAT> (nlps_gpu_compatibility's MODE 0 / 2 apart).
// Every MODE below exists plain per dimension and law, per law with the tile's particles of that law compacted first
// (FILT; a cloud of several laws, one launch per law present) and in the one-material form of the 3-D laws 1-3 (UMAT).
// What only some have is stated here, and launch_k3 instantiates a form only where its flag is set, so the set of
// kernels in the library is this table:
//   MODE 1  the fused K3 of the explicit step        + LAW = -1 + one wave per tile (FILT, NT = 64)
//   MODE 5  its state half (damage hooks)            + LAW = -1   (a deterministic damage step launches these forms too)
//   MODE 3  the fused residual                       + one wave per tile; the fluid law's particles go to MODE 4
//   MODE 4  MODE 3 with the rate tensors (dV)          the fluid law only: plain, FILT, one wave per tile
//   MODE 6  the state half of MODE 3 (damage hooks)    nothing else (tests/test_isa_implicit_damage.py)
//   MODE 7  MODE 1 with the step's mean rate (dt)      the fluid law only: plain, FILT, one wave per tile
//                                                      (nlps_gpu_set_explicit_fluid; MODE 1 hands the law's particles to it)
//   MODE 8  the kinematic half of the F-bar step       no law at all: LAW = -1, plain, one form per dimension.  Its kernel
//           (MODE 5 up to the law, the patch sums)     is k3_kin_tile<ND> -- dt and the patch arrays as arguments -- and its
//                                                      one launch site is launch_k3_fbar_kin below, not launch_k3
template <int MODE>
struct K3Forms {
  static constexpr bool dispatch = MODE == 1 || MODE == 5;  // LAW = -1: the law of every particle looked up at run time
  static constexpr bool wave = MODE == 1 || MODE == 3;      // the deterministic form
  static constexpr int fluid = MODE == 3 ? 4 : MODE == 1 ? 7 : 0;  // NLPS_KLAW_FLUID exists, as MODE 4 / MODE 7
};
struct K3Launch {
  bool signal = false;         // arm the boundary-done signal of overlap mode 2 in front of the (last) launch
  bool wave = false;           // one wave per tile and per law present over the exact lists, one slab per (tile, law)
  const double* dV = nullptr;  // the nodal rate vector, read by MODE 4 alone
  double dt = 0.0;             // the step, read by MODE 7 alone
};
// 3-D, one material, laws 1-3: its constants by scalar loads (k3_body, UMAT)
static bool one_material_3d(const nlps_gpu* h) {
  return h->nd == 3 && h->nmats == 1 && h->uniform_law >= 1 && h->uniform_law <= 3;
}
// one workgroup of nt threads per tile; every K3 kernel takes this argument block in front of its own last argument
template <class K, class X>
static void k3_go(nlps_gpu* h, K kernel, int nt, const TileD& td, const X& last) {
  hipLaunchKernelGGL(kernel, dim3(h->ntw), dim3(nt), 0, h->stream, h->P, h->g, h->N, td, h->mats_d, h->prm, h->gstatus_d, last);
}
static const double* const no_rates = nullptr;
// one launch of the kernel of law l (out of range: the last law, with_law_in); MODE 3 hands the fluid law to MODE 4,
// MODE 1 to MODE 7, whose kernel is the k3_tile overload that takes dt
using K3StepKernel = void (*)(PView, GridD, NView, TileD, const MatD*, ParamsD, int*, double);
template <int MODE, bool FILT, int NT>
static void launch_k3_law(nlps_gpu* h, const TileD& td, int l, const K3Launch& a) {
  with_nd(h->nd, [&](auto D) {
    if constexpr (K3Forms<MODE>::fluid == 4) {
      if (l == NLPS_KLAW_FLUID) return k3_go(h, k3_tile<CT(D), NLPS_KLAW_FLUID, 4, FILT, NT>, NT, td, a.dV);
    }
    if constexpr (K3Forms<MODE>::fluid == 7) {
      if (l == NLPS_KLAW_FLUID) return k3_go(h, K3StepKernel(k3_tile<CT(D), NLPS_KLAW_FLUID, 7, FILT, NT>), NT, td, a.dt);
    }
    with_law(l, [&](auto L) { k3_go(h, k3_tile<CT(D), CT(L), MODE, FILT, NT>, NT, td, no_rates); });
  });
}
// The launch form of this cloud.  td is the caller's: with or without a slab pointer, for the tile class it wants.
template <int MODE>
static void launch_k3(nlps_gpu* h, TileD td, const K3Launch& a) {
  const int law = h->uniform_law;  // -1: several laws in the cloud (law_present)
  // one launch of the single-law kernel per law present (FILT); MODE 1 / 5 on request only (nlps_gpu_set_law_launch_mode)
  const bool per_law = law < 0 && (!K3Forms<MODE>::dispatch || h->k3_per_law);
  if (a.signal && !per_law) arm_signal(h, td, 1);
  if constexpr (K3Forms<MODE>::wave) {
    if (a.wave) {  // (a cloud of one law too: slab_n = 1, slot 0)
      td.slab_n = __builtin_popcount(h->law_present);
      td.slab_slot = -1;
      for_each_law_present(h->law_present, [&](int l, bool) {
        td.slab_slot++;
        launch_k3_law<MODE, true, 64>(h, td, l, a);
      });
      return;
    }
  }
  if (per_law) {  // only the last launch releases the exchange (launches of one stream run in order)
    for_each_law_present(h->law_present, [&](int l, bool last) {
      if (a.signal && last) arm_signal(h, td, 1);
      launch_k3_law<MODE, true, K3_BLK>(h, td, l, a);
    });
  } else if (law < 0) {  // several laws, many mixed tiles: the kernel that dispatches on the law at run time
    if constexpr (K3Forms<MODE>::dispatch) {
      with_nd(h->nd, [&](auto D) { k3_go(h, k3_tile<CT(D), -1, MODE>, K3_BLK, td, no_rates); });
    }
  } else if (one_material_3d(h)) {
    with_law_in<1, 3>(law, [&](auto L) { k3_go(h, k3_tile<3, CT(L), MODE, false, K3_BLK, true>, K3_BLK, td, no_rates); });
  } else {
    launch_k3_law<MODE, false, K3_BLK>(h, td, law, a);
  }
}
// The step with F-bar (nlps_gpu_set_explicit_fbar): the clear of the patch array and of the patch per particle, then the
// kinematic half (k3_tile's MODE 8); fluid_dt > 0: the cloud holds the fluid law, whose particles get their rate.
static void launch_k3_fbar_kin(nlps_gpu* h, const TileD& td, double fluid_dt) {
  nlps_gpu::Fbar& fb = h->fbar;
  const int n = std::max((int)(2 * fb.npatch), h->P.np);
  hipLaunchKernelGGL(k_fbar_clear, dim3(nblk(n)), dim3(BLK), 0, h->stream, fb.sums.get(), (int)(2 * fb.npatch), fb.pid.get(), h->P.np);
  FbarKin k{fb.sums.get(), fb.pid.get(), {fb.block[0], fb.block[1], fb.block[2]}, {fb.np[0], fb.np[1], fb.np[2]}};
  with_nd(h->nd, [&](auto D) {
    hipLaunchKernelGGL(k3_kin_tile<CT(D)>, dim3(h->ntw), dim3(K3_BLK), 0, h->stream, h->P, h->g, h->N, td, h->mats_d.get(), h->prm,
                       h->gstatus_d.get(), fluid_dt, k);
  });
}
// ... and behind it the stress kernel, in the launch form of the cloud (one law; one launch per law present; the
// run-time dispatch where nlps_gpu_set_law_launch_mode allows it), and the force half of the damage step, k3f_tile
static void launch_fbar_stress(nlps_gpu* h) {
  const nlps_gpu::Fbar& fb = h->fbar;
  const FbarD d{fb.sums.get(), fb.pid.get(), fb.F.get(), fb.J.get(), fb.alpha.get()};
  const dim3 grid(nblk(h->P.np)), blk(BLK);
  with_nd(h->nd, [&](auto D) {
    auto one = [&](int l, auto FILT) {
      if (l == NLPS_KLAW_FLUID)
        hipLaunchKernelGGL((k_fbar_stress<CT(D), NLPS_KLAW_FLUID, CT(FILT)>), grid, blk, 0, h->stream, h->P, h->mats_d.get(), h->prm,
                           h->gstatus_d.get(), d);
      else
        with_law(l, [&](auto L) {
          hipLaunchKernelGGL((k_fbar_stress<CT(D), CT(L), CT(FILT)>), grid, blk, 0, h->stream, h->P, h->mats_d.get(), h->prm,
                             h->gstatus_d.get(), d);
        });
    };
    if (h->uniform_law >= 0) one(h->uniform_law, std::false_type{});
    else if (!h->k3_per_law)
      hipLaunchKernelGGL((k_fbar_stress<CT(D), -1, false>), grid, blk, 0, h->stream, h->P, h->mats_d.get(), h->prm, h->gstatus_d.get(), d);
    else for_each_law_present(h->law_present, [&](int l, bool) { one(l, std::true_type{}); });
  });
  LAUNCH_ND(k3f_tile<2>, k3f_tile<3>, h->ntw, h->P, h->g, h->N, tile_view(h, 0), h->gstatus_d);
}
// The folded form of the explicit step (one law, 0 .. NLPS_KLAW_FRICTIONAL): k3_tile_lazy, plain or one-material
static void launch_k3_lazy(nlps_gpu* h, TileD td, bool signal, const LazyNodal& ln) {
  if (signal) arm_signal(h, td, 1);
  if (one_material_3d(h)) {
    with_law_in<1, 3>(h->uniform_law, [&](auto L) { k3_go(h, k3_tile_lazy<3, CT(L), true>, K3_BLK, td, ln); });
  } else {
    with_nd(h->nd, [&](auto D) {
      with_law(h->uniform_law, [&](auto L) { k3_go(h, k3_tile_lazy<CT(D), CT(L)>, K3_BLK, td, ln); });
    });
  }
}

// One scatter per tile into `out`, which the caller has zeroed and exchanges afterwards.  On the deterministic implicit
// path (det_implicit) the one-wave form leaves its windows as slab_count slabs per tile and k_slab_gather<ND, NF>
// sums them per node in a fixed order; otherwise the 256-thread form flushes by atomics.  launch(NT, td) launches either:
// NT = ic<64> or ic<BLK>, td the tile view to launch on.
template <int NF2, int NF3>  // out[node][NF] of a part of the node window (node_ranges) from the slabs; other nodes keep theirs
static void det_gather(nlps_gpu* h, int part, int slab_count, double* out) {
  const NodeRanges r = node_ranges(h, part);
  TileD tg = tile_view(h, 0);
  tg.slab_n = slab_count;
  if (r.an + r.bn > 0)
    LAUNCH_ND((k_slab_gather<2, NF2>), (k_slab_gather<3, NF3>), nblk(r.an + r.bn), r.a0, r.an, r.b0, r.bn, h->g, tg, out);
}
template <int NF2, int NF3, class F>
static int scatter_tiles(nlps_gpu* h, const char* who, int slab_count, double* out, F&& launch) {
  if (!det_implicit(h)) {
    launch(ic<BLK>{}, tile_view(h));
    return 0;
  }
  if (det_prepare(h, who)) return 1;
  launch(ic<64>{}, tile_view(h));
  det_gather<NF2, NF3>(h, 0, slab_count, out);
  return 0;
}

static void launch_k2(nlps_gpu* h, bool p2g, int cls, double dt, double gamma_nm, bool signal = false) {
  TileD td = tile_view(h, cls);
  if (signal) arm_signal(h, td, 0);
  if (h->deterministic && p2g) {  // one wave per tile, sorted list, slab flush (nlps_gpu_set_deterministic)
    LAUNCH_ND_BLK((k2_tile<2, true, 64>), (k2_tile<3, true, 64>), h->ntw, 64, h->P, h->g, h->N, td, h->prm, dt, gamma_nm,
                  h->gstatus_d, (unsigned char*)nullptr);
    return;
  }
  // A move still pending here is this K2's to apply: nlps_gpu_explicit_step has left it pending for its async form only
  // (one launch over all tiles, p2g), and every other caller of search_and_lists has materialised it.  The marks of
  // particles outside the lists stay set, and move_pending with them, until the search of this step (k_search_ahead).
  unsigned char* moved = (p2g && h->move_pending) ? h->moved_d.get() : nullptr;
  with_nd(h->nd, [&](auto D) {
    with_bool(p2g, [&](auto P2G) {
      hipLaunchKernelGGL((k2_tile<CT(D), CT(P2G)>), dim3(h->ntw), dim3(BLK), 0, h->stream, h->P, h->g, h->N, td,
                         h->prm, dt, gamma_nm, h->gstatus_d, moved);
    });
  });
}

// Async lists: the twin set (see nlps_gpu::side), made at the first step that builds lists on the side stream
static int ensure_list_twins(nlps_gpu* h) {
  nlps_gpu::ListSet& t = h->twin;
  if (t.order) return 0;
  const size_t nn = (size_t)h->g.nnodes, ND = (size_t)h->nd;
  if (dev_alloc(h, t.work, (size_t)h->ntiles) || dev_alloc(h, t.nwork, 6) || dev_alloc(h, t.start, (size_t)h->ntiles + 1)) return 1;
  if (dev_alloc(h, t.order2, h->P.npad)) return 1;
  if (dev_alloc(h, t.active, nn) || dev_alloc(h, t.fixed, nn * ND)) return 1;
  if (dev_alloc(h, t.nm, nn * (1 + ND)) || dev_alloc(h, t.force, nn * ND)) return 1;
  return dev_alloc(h, t.order, h->P.npad);  // (last: its presence says the twin is complete)
}
// The step that finds the lists of its search built (lists_ready): the twin set becomes the set in use.  The closest
// nodes of that search, I0n, hold a value for every particle (k_search_ahead), so they are adopted by exchanging the
// two arrays; the tile counters change places as after any search done ahead (search_and_lists).
static void adopt_ready_lists(nlps_gpu* h) {
  std::swap(h->lists, h->twin);
  bind_lists(h);
  h->P_I0.swap(h->P_I0n);
  h->P.I0 = h->P_I0;
  h->P.I0n = h->P_I0n;
}

// S1: closest-node update + 1-ring activation + binning of the particles to I0-tiles, then lists, beta and the
// Newton iteration (+ predictor and P2G of mass / m*dD when `p2g`).  With `overlap` the exchange of the active
// flags runs behind the tiles that do not touch a ghost band.
static int search_and_lists(nlps_gpu* h, bool init, bool p2g, double dt, double gamma_nm, int overlap = 0,
                            bool launch_lists_kernel = true) {
  int np = h->P.np;
  if (!p2g && materialise_nodal(h)) return 1;  // (a level-B search rewrites the active flags the lazy nodal arrays depend on)
  if (!p2g && materialise_move(h)) return 1;   // (the explicit step decides for itself: K2 below may be the one that moves)
  // ahead: the search of this step was done by the last kernel of the previous one (k5_tile<., ., true>); only the
  // nodal accumulators are reset here
  const bool ahead = h->ahead && !init, searched = h->searched;
  const bool deferred = ahead && h->ranks_deferred && node_lists(h);  // that search only counted: ranks from cursors (k_fill_orders)
  h->ranks_deferred = false;
  if (ahead) h->tile_count_d.swap(h->tile_count2_d);  // the counters that search filled size the lists from here on
  // async lists: the side stream of the last step has run the activation and list kernels below into the twin set
  // (a level-B search, p2g = false, has the nodal arrays of the last step made first and builds its lists here)
  const bool ready = ahead && p2g && h->lists_ready;
  h->lists_ready = false;
  if (ready) adopt_ready_lists(h);
  if (ready) h->lists_exact = false;
  h->searched = h->ahead = false;  // consumed
  if (!ready) {
  const bool clear_in_dilate = ahead && p2g;  // nothing but the nodal accumulators to reset: k_dilate_scan does it
  if (!clear_in_dilate)
    LAUNCH_ND((k_step_clear<2>), (k_step_clear<3>), nblk(std::max(h->nwn, h->ntw)), h->n0, h->nwn, h->N,
              h->tile_count_d + h->tile0, h->ntw, p2g ? 1 : 0, node_lists(h) ? h->node_cnt_d : nullptr, ahead ? 0 : 1);
  if (!ahead) {
    TileCnt tc = tile_cnt(h, true);
    if (init) LAUNCH_ND((k_init_I0<2>), (k_init_I0<3>), nblk(np), h->P, h->g, h->N, tc);
    else LAUNCH_ND((k_search<2>), (k_search<3>), nblk(np), h->P, h->g, h->N, h->rank1_d, tc, searched ? 0 : 1);
  }
  {
    const TileScanArgs ts = list_build(h, h->lists, h->tile_count_d, deferred ? h->tile_cursor_d + h->tile0 : nullptr).ts;
    const int nb = 1 + (h->nwn + 1023) / 1024 + (node_lists(h) ? (h->ntw + 15) / 16 : 0);
    int* fo = (h->adaptive_resort > 0.0 && !h->deterministic) ? h->foreign_d : nullptr;
    LAUNCH_ND_BLK(k_dilate_scan<2>, k_dilate_scan<3>, nb, 1024, h->n0, h->nwn, h->g, h->N, ts, fo, h->foreign_h.host(), tile_tab(h),
                  clear_in_dilate ? 1 : 0);
  }
  HIPCHK(hipGetLastError());
  if (halo(h, h->N.active, 1, 1, 1, overlap ? 1 : 0)) return 1;
  if (!h->lists.order2) {
    HIPCHK(h->lists.order2.reserve(h->P.npad));
    HIPCHK(hipMemsetAsync(h->lists.order2, 0, h->P.npad * sizeof(int), h->stream));
  }
  if (node_lists(h)) {  // both lists in one pass, the canonical one through the layer tables of this step (TileTab)
    const int* adopt = ahead ? h->P.I0n : nullptr;
    LAUNCH_ND(k_fill_orders<2>, k_fill_orders<3>, nblk(np), np, h->P.tile, h->P.rank, h->nrank_d, h->P.I0, adopt, h->lists.start,
              h->g, tile_tab(h), h->lists.order, h->lists.order2, deferred ? h->tile_cursor_d : (int*)nullptr, h->node_cnt_d);
  } else {  // deterministic mode: the exact per-tile sort
    if (ahead) hipLaunchKernelGGL(k_commit_I0, dim3(nblk(np)), dim3(BLK), 0, h->stream, np, (const int*)h->P.I0n, h->P.I0);
    hipLaunchKernelGGL(k_fill_order, dim3(nblk(np)), dim3(BLK), 0, h->stream, np, h->P.tile, h->P.rank, h->lists.start,
                       h->lists.order);
    LAUNCH_ND_BLK((k_tile_order<2, true>), (k_tile_order<3, true>), h->ntw, 256, h->P, h->g, tile_view(h, 0), (const int*)h->lists.order,
                  h->lists.order2);
  }
  h->lists_exact = !node_lists(h);
  HIPCHK(hipGetLastError());
  }  // !ready
  if (h->timing) HIPCHK(hipEventRecord(h->ev[1], h->stream));
  if (overlap == 1) {
    launch_k2(h, p2g, 2, dt, gamma_nm);
    if (halo(h, h->N.active, 1, 1, 1, 2)) return 1;
    launch_k2(h, p2g, 1, dt, gamma_nm);
  } else if (overlap == 2) {  // the flags travelled behind the binning kernels; one launch, boundary tiles first
    if (halo(h, h->N.active, 1, 1, 1, 2)) return 1;
    launch_k2(h, p2g, 0, dt, gamma_nm, true);
  } else if (launch_lists_kernel) {
    launch_k2(h, p2g, 0, dt, gamma_nm);
  }
  HIPCHK(hipGetLastError());
  h->masks_valid = false;
  h->binned = true;
  return 0;
}

static int materialise_roll(nlps_gpu* h) {
  if (materialise_move(h)) return 1;  // (whoever wants the n+1 slots in place wants x and dis in place too)
  if (!h->rolled) return 0;
  if (h->rolled_keep) LAUNCH_ND((k_copy_n_to_n1<2, true>), (k_copy_n_to_n1<3, true>), nblk(h->P.np), h->P, h->mats_d);
  else LAUNCH_ND((k_copy_n_to_n1<2>), (k_copy_n_to_n1<3>), nblk(h->P.np), h->P, h->mats_d);
  if (h->rolled_rate) LAUNCH_ND(k_roll_rate<2>, k_roll_rate<3>, nblk(h->P.np), h->P, h->mats_d);
  HIPCHK(hipGetLastError());
  h->rolled = h->rolled_keep = h->rolled_rate = false;
  return 0;
}

// mirrored: the last kernel of the call has already stored the status word into the pinned host word (the alias of status_h)
static int check_status(nlps_gpu* h, int fatal_mask, const char* where, bool mirrored) {
  // the status word travels to a pinned host word in stream order: one wait instead of a synchronise and a blocking copy
  if (!mirrored) HIPCHK(hipMemcpyAsync(h->status_h.host(), h->gstatus_d, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  const int st = *(volatile int*)h->status_h.host();
  if (st & fatal_mask) {
    char buf[160];
    snprintf(buf, sizeof buf, "Error in %s: particle failure flags 0x%x (1 Newton, 2 connectivity, 4 J<=0, 8 law, 16 outside node window)",
             where, st);
    h->err = buf;
    fprintf(stderr, "\033[1;31m%s\033[0m\n", buf);
    return 1;
  }
  return 0;
}

extern "C" int nlps_gpu_initialize_lme(nlps_gpu* h) {
  // beta and lambda start at zero (Generate-One-Phase-Analysis.c:190-192) => first list is the
  // whole active 2-ring (LME.c:150-154)
  HIPCHK(hipMemsetAsync(h->P.d + (size_t)F_LAM * h->P.npad, 0, 7 * h->P.npad * sizeof(double), h->stream));
  if (search_and_lists(h, true, false, 0.0, 0.0)) return 1;
  if (compute_node_mask(h)) return 1;
  return check_status(h, ST_NEWTON | ST_CONNECT | ST_HALO, "initialize__LME__()");
}

// Driver_EigenErosion: compute_Beps__Constitutive__(.., true) runs once before the first step (U-Newmark-beta.c:182-183);
// what it sees -- positions and closest nodes -- is kept for the lists that stay frozen afterwards
static int beps_snapshot(nlps_gpu* h) {
  if (h->beps_snapshot || !h->P.erosion || h->P.softening || h->P.np == 0) return 0;
  if (materialise_move(h)) return 1;
  hipLaunchKernelGGL(k_beps_snapshot, dim3(nblk(h->P.np)), dim3(BLK), 0, h->stream, h->P, h->nd);
  HIPCHK(hipGetLastError());
  h->beps_snapshot = true;
  return 0;
}

extern "C" int nlps_gpu_local_search(nlps_gpu* h) {
  tan_stale(h, "nlps_gpu_local_search");
  if (beps_snapshot(h)) return 1;  // (before this search moves any closest node)
  if (search_and_lists(h, false, false, 0.0, 0.0)) return 1;
  if (compute_node_mask(h)) return 1;
  return check_status(h, ST_NEWTON | ST_CONNECT | ST_HALO, "local_search__LME__()");
}

static int ensure_bcs(nlps_gpu* h, const nlps_bcc* bcc, int nbcc) {
  bool same = (int)h->bcs.size() == nbcc;
  for (int i = 0; same && i < nbcc; i++) same = h->bcs[i].host_nodes == bcc[i].nodes && h->bcs[i].n == bcc[i].nnodes;
  if (same) return 0;
  if (materialise_nodal(h)) return 1;  // (the nodal arrays of the last folded step still want the old sets' mask)
  h->bcs.clear();
  for (int i = 0; i < nbcc; i++) {
    BcDev b{bcc[i].nodes, bcc[i].nnodes, {}};
    if (b.n > 0) {
      HIPCHK(b.dnodes.reserve((size_t)b.n));
      HIPCHK(hipMemcpy(b.dnodes, bcc[i].nodes, (size_t)b.n * sizeof(int), hipMemcpyHostToDevice));
    }
    h->bcs.push_back(std::move(b));
  }
  HIPCHK(h->bcmask_d.reserve((size_t)h->g.nnodes));
  HIPCHK(hipMemset(h->bcmask_d, 0, (size_t)h->g.nnodes * sizeof(unsigned)));
  if (nbcc <= NLPS_MAX_BC_INLINE)
    for (int i = 0; i < nbcc; i++)
      if (h->bcs[i].n > 0)
        hipLaunchKernelGGL(k_bc_mark, dim3(nblk(h->bcs[i].n)), dim3(BLK), 0, 0, h->bcs[i].dnodes, h->bcs[i].n, 1u << i,
                           h->bcmask_d);
  HIPCHK(hipGetLastError());
  // the copies above are ordered on the default stream only: a caller-provided non-blocking stream (torch
  // streams are) would not wait for their DMA
  HIPCHK(hipDeviceSynchronize());
  return 0;
}

// bcc[i].dir / value are indexed [k * nsteps + step] (Types.h:296-351): a step outside the range given at create
// would read past the caller's arrays
static int check_step(nlps_gpu* h, int step, const char* who) {
  if (step >= 0 && step < h->nsteps) return 0;
  h->err = std::string(who) + ": step outside [0, nsteps) (nsteps is fixed at nlps_gpu_create)";
  return 1;
}

static int dirbits_of(const nlps_bcc& b, int step, int nsteps) {
  int bits = 0;
  for (int k = 0; k < b.dim && k < 3; k++)
    if (b.dir[(size_t)k * nsteps + step] == 1) bits |= 1 << k;
  return bits;
}
// the values of a Dirichlet set at a step, one per direction it has (0 beyond)
static void bc_values(const nlps_bcc& b, int step, int nsteps, double v[3]) {
  for (int k = 0; k < 3; k++) v[k] = k < b.dim ? b.value[(size_t)k * nsteps + step] : 0.0;
}
// the caller's gravity[ndim], or NULL, as three components
static void gravity3(const double* gravity, int nd, double g[3]) {
  for (int k = 0; k < 3; k++) g[k] = (gravity && k < nd) ? gravity[k] : 0.0;
}

extern "C" int nlps_gpu_active_masks(nlps_gpu* h, const nlps_bcc* bcc, int nbcc, int step, int* nactive,
                                     int* nfree_dofs, int* nodes2mask, int* dofs2mask) {
  tan_stale(h, "nlps_gpu_active_masks");
  int ND = h->nd, nn = h->g.nnodes;
  if (nbcc > 0 && check_step(h, step, "nlps_gpu_active_masks")) return 1;
  if (compute_node_mask(h)) return 1;
  HIPCHK(hipMemcpyAsync(&h->nactive, h->total_d, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  int order = h->nactive * ND;
  if (ensure_bcs(h, bcc, nbcc)) return 1;
  HIPCHK(hipMemsetAsync(h->fixedm_d, 0, (size_t)nn * ND, h->stream));
  for (int i = 0; i < nbcc; i++) {
    if (h->bcs[i].n == 0) continue;
    hipLaunchKernelGGL(k_mark_fixed_masked, dim3(nblk(h->bcs[i].n)), dim3(BLK), 0, h->stream, h->bcs[i].dnodes,
                       h->bcs[i].n, bcc[i].dim, dirbits_of(bcc[i], step, h->nsteps), ND, h->n2m_d, h->fixedm_d);
  }
  int nb = (order + 1023) / 1024;
  if (order > 0) {
    hipLaunchKernelGGL(k_scan_count, dim3(nb), dim3(256), 0, h->stream, h->fixedm_d, order, 1, h->bsum_d);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, h->stream, h->bsum_d, nb, h->total_d + 1);
    hipLaunchKernelGGL(k_scan_write, dim3(nb), dim3(256), 0, h->stream, h->fixedm_d, order, 1, h->bsum_d, h->d2m_d);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&h->nfree, h->total_d + 1, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (order == 0) h->nfree = 0;
  if (nactive) *nactive = h->nactive;
  if (nfree_dofs) *nfree_dofs = h->nfree;
  // (with a file numbering set, Nodes2Mask is indexed by the file's node, like the reference's array)
  if (nodes2mask)
    HIPCHK(hipMemcpy(nodes2mask, h->canon_d ? h->mask_idx_d : h->n2m_d, (size_t)nn * sizeof(int), hipMemcpyDeviceToHost));
  if (dofs2mask && order) HIPCHK(hipMemcpy(dofs2mask, h->d2m_d, (size_t)order * sizeof(int), hipMemcpyDeviceToHost));
  h->masks_valid = true;
  h->lagr_valid = false;  // (the masked numbering may have changed: cached residual vectors are void)
  return 0;
}

// masked nodal vector of the caller (host or device) -> grid-numbered device array
static int to_grid(nlps_gpu* h, double* grid, const double* masked, int nf) {
  size_t n = (size_t)h->nactive * nf;
  const double* src = masked;
  if (!is_device_ptr(masked)) {
    if (reserve(h, "to_grid", h->maskedA, n, "the masked vector")) return 1;
    HIPCHK(hipMemcpyAsync(h->maskedA, masked, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    src = h->maskedA;
  }
  hipLaunchKernelGGL(k_expand, dim3(nblk(h->g.nnodes)), dim3(BLK), 0, h->stream, grid, src, h->n2m_d, h->g.nnodes, nf);
  HIPCHK(hipGetLastError());
  return 0;
}

// grid-numbered device array -> caller's masked vector (mode: see k_compact)
static int from_grid(nlps_gpu* h, double* masked, const double* grid, int nf, int gstride, int goff, int bcast, int mode,
                     const double* div_masked) {
  size_t n = (size_t)h->nactive * nf;
  if (n == 0) return 0;
  bool dev_out = is_device_ptr(masked);
  if (reserve(h, "from_grid", h->maskedA, 2 * n, "the masked vectors")) return 1;
  double* dst = dev_out ? masked : h->maskedA;
  if (!dev_out && mode == 1) HIPCHK(hipMemcpyAsync(dst, masked, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  const double* div = div_masked;
  if (div_masked && !is_device_ptr(div_masked)) {
    HIPCHK(hipMemcpyAsync(h->maskedA + n, div_masked, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    div = h->maskedA + n;
  }
  hipLaunchKernelGGL(k_compact, dim3(nblk(h->g.nnodes)), dim3(BLK), 0, h->stream, dst, grid, h->n2m_d, h->d2m_d, div,
                     h->g.nnodes, nf, gstride, goff, bcast, mode);
  HIPCHK(hipGetLastError());
  if (!dev_out) {
    HIPCHK(hipMemcpyAsync(masked, dst, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

static int need_binning(nlps_gpu* h, const char* who) {
  if (h->binned) return 0;
  h->err = std::string(who) + ": call nlps_gpu_local_search() first (particles are not binned to tiles)";
  return 1;
}

static int need_masks(nlps_gpu* h, const char* who) {
  if (need_binning(h, who)) return 1;
  if (h->masks_valid) return 0;
  h->err = std::string(who) + ": call nlps_gpu_active_masks() after the local search first";
  return 1;
}

extern "C" int nlps_gpu_lumped_mass(nlps_gpu* h, double* M) {
  if (need_masks(h, "nlps_gpu_lumped_mass")) return 1;
  if (materialise_move(h)) return 1;
  int ND = h->nd;
  HIPCHK(hipMemsetAsync(h->gridA, 0, (size_t)h->g.nnodes * sizeof(double), h->stream));
  if (scatter_tiles<1, 1>(h, "nlps_gpu_lumped_mass", 1, h->gridA, [&](auto NT, TileD td) {
        LAUNCH_ND_BLK((kb_p2g_tile<2, 0, CT(NT)>), (kb_p2g_tile<3, 0, CT(NT)>), h->ntw, CT(NT), h->P, h->g, td, h->gridA);
      }))
    return 1;
  HIPCHK(hipGetLastError());
  if (halo(h, h->gridA, 1, 8, 0)) return 1;
  return from_grid(h, M, h->gridA, ND, 1, 0, 1, 0, nullptr);
}

extern "C" int nlps_gpu_nodal_field_n(nlps_gpu* h, double* V, double* A, const double* M) {
  if (need_masks(h, "nlps_gpu_nodal_field_n")) return 1;
  if (materialise_move(h)) return 1;
  int ND = h->nd;
  HIPCHK(hipMemsetAsync(h->gridA, 0, (size_t)h->g.nnodes * 2 * ND * sizeof(double), h->stream));
  if (scatter_tiles<4, 6>(h, "nlps_gpu_nodal_field_n", 1, h->gridA, [&](auto NT, TileD td) {
        LAUNCH_ND_BLK((kb_p2g_tile<2, 1, CT(NT)>), (kb_p2g_tile<3, 1, CT(NT)>), h->ntw, CT(NT), h->P, h->g, td, h->gridA);
      }))
    return 1;
  HIPCHK(hipGetLastError());
  if (halo(h, h->gridA, 2 * ND, 8, 0)) return 1;
  if (from_grid(h, V, h->gridA, ND, 2 * ND, 0, 0, 2, M)) return 1;
  return from_grid(h, A, h->gridA, ND, 2 * ND, ND, 0, 2, M);
}

extern "C" int nlps_gpu_compatibility(nlps_gpu* h, const double* dU, const double* dU_dt) {
  if (fbar_refuse(h, "nlps_gpu_compatibility")) return 1;
  if (need_masks(h, "nlps_gpu_compatibility")) return 1;
  if (!dU_dt && (h->law_present & (1 << NLPS_KLAW_FLUID))) {
    h->err = "nlps_gpu_compatibility: the cloud holds the Newtonian-Fluid-Compressible law, whose stress reads dt_F_n1: "
             "dU_dt is required (nlps_gpu_nodal_kinetic_increments)";
    return 1;
  }
  if (materialise_roll(h)) return 1;
  if (to_grid(h, h->N.dU, dU, h->nd)) return 1;
  if (dU_dt && to_grid(h, h->gridB, dU_dt, h->nd)) return 1;
  if (dU_dt) h->level_b_fields = true;
  TileD td = tile_view(h);
  const dim3 grid(h->ntw), blk(K3_BLK);
  const double* dV = dU_dt ? h->gridB : nullptr;
  with_nd(h->nd, [&](auto D) {
    with_bool(dV != nullptr, [&](auto RATES) {  // MODE 2: the rate tensors too
      hipLaunchKernelGGL((k3_tile<CT(D), 0, CT(RATES) ? 2 : 0>), grid, blk, 0, h->stream, h->P, h->g, h->N, td, h->mats_d, h->prm,
                         h->gstatus_d, dV);
    });
  });
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int nlps_gpu_constitutive(nlps_gpu* h) {
  if (fbar_refuse(h, "nlps_gpu_constitutive")) return 1;
  if (materialise_roll(h)) return 1;
  h->level_b_fields = true;
  if (h->law_present & (1 << NLPS_KLAW_FRICTIONAL))
    LAUNCH_ND((k_stress<2, true>), (k_stress<3, true>), nblk(h->P.np), h->P, h->mats_d, h->prm, h->gstatus_d);
  else
    LAUNCH_ND((k_stress<2, false>), (k_stress<3, false>), nblk(h->P.np), h->P, h->mats_d, h->prm, h->gstatus_d);
  HIPCHK(hipGetLastError());
  return check_status(h, ST_CONSTITUTIVE, "Stress_integration__Constitutive__()");
}

extern "C" int nlps_gpu_internal_forces(nlps_gpu* h, double* R) {
  if (need_masks(h, "nlps_gpu_internal_forces")) return 1;
  if (materialise_roll(h)) return 1;
  int ND = h->nd;
  if (h->P.erosion && h->P.np > 0) {  // damage of every particle, then its Kirchhoff stress scaled in place (:1313-1331)
    const int np = h->P.np;
    const size_t nn = (size_t)h->g.nnodes;
    if (!h->dmg.b_first) {
      HIPCHK(h->dmg.b_first.reserve(nn));
      HIPCHK(h->dmg.b_last.reserve(nn));
    }
    HIPCHK(hipMemsetAsync(h->dmg.b_first, 0, nn * sizeof(int), h->stream));
    HIPCHK(hipMemsetAsync(h->dmg.b_last, 0, nn * sizeof(int), h->stream));
    hipLaunchKernelGGL(k_tangent_keys, dim3(nblk(np)), dim3(BLK), 0, h->stream, h->P, h->skey_d, h->sval_d);
    size_t bytes = h->cub_tmp_bytes;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(h->cub_tmp.get(), bytes, h->skey_d.get(), h->skey2_d.get(), h->sval_d.get(), h->sval2_d.get(), np, 0, 32,
                                              h->stream));
    hipLaunchKernelGGL(k_node_ranges, dim3(nblk(np)), dim3(BLK), 0, h->stream, np, h->skey2_d, h->dmg.b_first, h->dmg.b_last);
    if (h->P.softening) {
      double* T0 = h->gather_tmp.get();  // [npad] scratch of the re-sort, idle here
      LAUNCH_ND((k_soften_pass1<2>), (k_soften_pass1<3>), nblk(np), h->P, h->mats_d, T0);
      LAUNCH_ND((k_soften_pass2<2>), (k_soften_pass2<3>), nblk(np), h->P, h->g, h->mats_d, h->dmg.b_first, h->dmg.b_last, h->sval2_d,
                (const uint8_t*)h->rank1_d, (const int*)h->perm_d, (const double*)T0, h->g.h);
    } else {
      // frozen lists (Beps.c:30-36): the node tables of the snapshot's closest nodes, rebuilt per call like the others
      if (beps_snapshot(h)) return 1;
      if (!h->dmg.b_first0) {
        HIPCHK(h->dmg.b_first0.reserve(nn));
        HIPCHK(h->dmg.b_last0.reserve(nn));
        HIPCHK(h->dmg.b_sorted0.reserve(h->P.npad));
      }
      // dmg.b_sorted0: the CURRENT order just sorted; sval2_d: free for the next sort.  (Both blocks hold npad ints, so
      // an error return between the two swaps leaves either owner with a block of the right size.)
      h->dmg.b_sorted0.swap(h->sval2_d);
      HIPCHK(hipMemsetAsync(h->dmg.b_first0, 0, nn * sizeof(int), h->stream));
      HIPCHK(hipMemsetAsync(h->dmg.b_last0, 0, nn * sizeof(int), h->stream));
      hipLaunchKernelGGL(k_beps_keys0, dim3(nblk(np)), dim3(BLK), 0, h->stream, h->P, h->skey_d, h->sval_d);
      bytes = h->cub_tmp_bytes;
      HIPCHK(hipcub::DeviceRadixSort::SortPairs(h->cub_tmp.get(), bytes, h->skey_d.get(), h->skey2_d.get(), h->sval_d.get(), h->sval2_d.get(), np, 0, 32,
                                                h->stream));
      hipLaunchKernelGGL(k_node_ranges, dim3(nblk(np)), dim3(BLK), 0, h->stream, np, h->skey2_d, h->dmg.b_first0, h->dmg.b_last0);
      // (current order in dmg.b_sorted0, snapshot order in sval2_d)
      LAUNCH_ND((k_damage<2>), (k_damage<3>), nblk(np), h->P, h->g, h->mats_d, h->dmg.b_first, h->dmg.b_last, h->dmg.b_sorted0,
                h->dmg.b_first0, h->dmg.b_last0, h->sval2_d, h->g.h);
      h->dmg.b_sorted0.swap(h->sval2_d);  // the sort buffers go back to where the re-sort expects them
    }
    HIPCHK(hipGetLastError());
  }
  if (materialise_nodal(h)) return 1;  // (the forces of the last explicit step are about to go)
  HIPCHK(hipMemsetAsync(h->N.force, 0, (size_t)h->g.nnodes * ND * sizeof(double), h->stream));
  if (scatter_tiles<2, 3>(h, "nlps_gpu_internal_forces", 1, h->N.force, [&](auto NT, TileD td) {
        LAUNCH_ND_BLK((kb_fint_tile<2, CT(NT)>), (kb_fint_tile<3, CT(NT)>), h->ntw, CT(NT), h->P, h->g, td, h->N.force, h->gstatus_d);
      }))
    return 1;
  HIPCHK(hipGetLastError());
  if (halo(h, h->N.force, ND, 8, 0)) return 1;
  return from_grid(h, R, h->N.force, ND, ND, 0, 0, 1, nullptr);
}

// __nodal_traction_forces (U-Newmark-beta.c:1376-1500): R_A -= N_pA T A0_p over the particles of the Neumann contours.
// One thread per listed particle (a contour holds few), global atomics into a grid array.
__global__ void k_inverse_perm(const int* __restrict__ perm, int np, int* __restrict__ inv) {
  int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < np) inv[perm[s]] = s;
}
// nlps_gpu::inv.  The setters of its users reserve it; the users (none of which accepts a migrated handle, where perm_d
// is no permutation of [0, np) any more) take the pointer from inv_perm(), which rebuilds the map behind a renumbering.
static hipError_t reserve_inv_perm(nlps_gpu* h) { return h->inv.d.reserve(std::max<size_t>(h->P.npad, 1)); }
static const int* inv_perm(nlps_gpu* h) {
  if (h->inv.stale) hipLaunchKernelGGL(k_inverse_perm, dim3(nblk(h->P.np)), dim3(BLK), 0, h->stream, h->perm_d, h->P.np, h->inv.d.get());
  h->inv.stale = false;
  return h->inv.d;
}
template <int ND>
__global__ void k_traction(PView P, GridD g, int n, const int* __restrict__ ids, const int* __restrict__ inv,
                           const double* __restrict__ T, const double* __restrict__ A0, double thickness,
                           double* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int p = inv[ids[e]];
  Lme<ND> c;
  double lam[ND], beta;
  if (!load_lme<ND>(P, g, p, c, lam, beta)) return;
  const double a0 = A0 ? A0[e] : PF(P, F_VOL0, p) / thickness;  // :1440-1444
  const double zinv = lme_zinv<ND>(c);
  for (int k = 0; k < Lme<ND>::KN; k++)
    for (int j = 0; j < 5; j++)
      for (int i = 0; i < 5; i++) {
        if (!c.on(i + 5 * j + 25 * k)) continue;
        const double Npa = c.ex[i] * c.ey[j] * (ND == 3 ? c.ez[k % Lme<ND>::KN] : 1.0) * zinv;
        const int node = c.I0 + c.node_offset(g, i, j, k + (ND == 3 ? 0 : 2));
        for (int a = 0; a < ND; a++) atomic_add_f64(out + (size_t)node * ND + a, -Npa * T[(size_t)e * ND + a] * a0);
      }
}

// Deterministic form (nlps_gpu_set_deterministic): ONE wave walks the contour particles in the caller's order, its lanes
// over the 5^d stencil slots of the particle -- distinct nodes, so a plain read-add-write per member -- and meets
// between two particles: every nodal sum is added in list order.  Contours are surface sets; no sort is needed.
template <int ND>
__global__ __launch_bounds__(64) void k_traction_serial(PView P, GridD g, int n, const int* __restrict__ ids,
                                                        const int* __restrict__ inv, const double* __restrict__ T,
                                                        const double* __restrict__ A0, double thickness, double* out) {
  constexpr int KN = Lme<ND>::KN, NS = 25 * KN;
  for (int e = 0; e < n; e++) {  // uniform
    const int p = inv[ids[e]];
    Lme<ND> c;
    double lam[ND], beta;
    if (load_lme<ND>(P, g, p, c, lam, beta)) {  // (every lane holds the particle's factors)
      const double a0 = A0 ? A0[e] : PF(P, F_VOL0, p) / thickness;
      const double zinv = lme_zinv<ND>(c);
      for (int m = threadIdx.x; m < NS; m += 64) {
        if (!c.on(m)) continue;
        const int i = m % 5, j = (m / 5) % 5, k = m / 25;
        const double Npa = c.ex[i] * c.ey[j] * (ND == 3 ? c.ez[k % KN] : 1.0) * zinv;
        const int node = c.I0 + c.node_offset(g, i, j, k + (ND == 3 ? 0 : 2));
        for (int a = 0; a < ND; a++) {
          double* o = out + (size_t)node * ND + a;
          *o = *o + (-Npa * T[(size_t)e * ND + a] * a0);
        }
      }
    }
    __syncthreads();  // the stores of this particle are done before the next one reads the same nodes
  }
}

// the traction sums of the Neumann contours in grid numbering: out[nnodes][ND] = - sum N_pA T A0_p (zeroed first);
// *any = 0 when the contours hold no particle (out is then left alone)
static int traction_to_grid(nlps_gpu* h, const char* who, double* out, const nlps_bcc* loads, int nloads, int step,
                            double thickness, const double* area0, int* any) {
  const int ND = h->nd, np = h->P.np;
  *any = 0;
  if (step < 0 || step >= h->nsteps) {
    h->err = std::string(who) + ": step outside [0, nsteps)";
    return 1;
  }
  if (ND == 3 && !area0) {
    h->err = std::string(who) + ": the 3-D build needs Phi.Area_0 (area0)";
    return 1;
  }
  if (h->migrated) {
    h->err = std::string(who) + ": not available after a migration (particle order is by global id)";
    return 1;
  }
  // the traction vector carries over from contour to contour where a direction is switched off (:1457-1461)
  std::vector<int> ids;
  std::vector<double> T, A;
  double Tc[3] = {0.0, 0.0, 0.0};
  for (int l = 0; l < nloads; l++) {
    for (int i = 0; i < ND; i++)
      if (loads[l].dir[(size_t)i * h->nsteps + step] == 1) Tc[i] = loads[l].value[(size_t)i * h->nsteps + step];
    for (int q = 0; q < loads[l].nnodes; q++) {
      const int p = loads[l].nodes[q];
      if (p < 0 || p >= np) {
        h->err = std::string(who) + ": particle index outside the cloud";
        return 1;
      }
      ids.push_back(p);
      for (int i = 0; i < ND; i++) T.push_back(Tc[i]);
      if (ND == 3) A.push_back(area0[p]);
    }
  }
  const int n = (int)ids.size();
  if (n == 0) return 0;
  *any = 1;
  DevBuf<int> ids_d;
  DevBuf<double> T_d, A_d;
  HIPCHK(ids_d.reserve((size_t)n));
  HIPCHK(T_d.reserve((size_t)n * ND));
  if (ND == 3) HIPCHK(A_d.reserve((size_t)n));
  HIPCHK(hipMemcpyAsync(ids_d, ids.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(T_d, T.data(), (size_t)n * ND * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (ND == 3) HIPCHK(hipMemcpyAsync(A_d, A.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  // (not inv_perm(): this call is open to a migrated handle, whose perm_d holds other ranks' indices too)
  hipLaunchKernelGGL(k_inverse_perm, dim3(nblk(np)), dim3(BLK), 0, h->stream, h->perm_d, np, h->sval_d);
  HIPCHK(hipMemsetAsync(out, 0, (size_t)h->g.nnodes * ND * sizeof(double), h->stream));
  if (det_implicit(h))
    LAUNCH_ND_BLK(k_traction_serial<2>, k_traction_serial<3>, 1, 64, h->P, h->g, n, ids_d, h->sval_d, T_d, A_d, thickness, out);
  else
    LAUNCH_ND(k_traction<2>, k_traction<3>, nblk(n), h->P, h->g, n, ids_d, h->sval_d, T_d, A_d, thickness, out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));  // (the host vectors above are about to go)
  return 0;
}

extern "C" int nlps_gpu_nodal_traction_forces(nlps_gpu* h, double* R, const nlps_bcc* loads, int nloads, int step,
                                              double thickness, const double* area0) {
  if (need_masks(h, "nlps_gpu_nodal_traction_forces")) return 1;
  if (materialise_move(h)) return 1;
  int any = 0;
  if (traction_to_grid(h, "nlps_gpu_nodal_traction_forces", h->gridA, loads, nloads, step, thickness, area0, &any)) return 1;
  if (!any) return 0;
  return from_grid(h, R, h->gridA, h->nd, h->nd, 0, 0, 1, nullptr);
}

// The Neumann contours inside the explicit step (nlps_gpu_set_explicit_loads; compute_Nodal_Nominal_traction_Forces,
// U-Verlet.c:805-902, called at :695 behind the internal forces): force_A += N_pA T A0_p on every dof, into the nodal
// force accumulator of the step.  The entries are the contour particles in the caller's contour order; a.T is the row of
// this step in the table of carried traction vectors ([contour][3]).  Contour particles lie on surfaces: their rows are
// scattered in memory whatever the mapping, so the mapping is chosen for the atomics:
//   MAP 0  one wave per entry, its lanes over the (stencil slot, direction) pairs of the particle, direction fastest: every
//          lane re-forms the factors of the one particle (wave-uniform loads) and a wave-instruction of atomics covers
//          runs of 5 x d consecutive doubles (one lattice row of the stencil each), 6 instructions in 3-D, 1 in 2-D --
//          float atomics run at the memory side and are priced per 64-B request, so the shape decides;
//   MAP 1  one lane per entry (k_traction's mapping, kept behind the developer switch "loads_lane_map" to measure against):
//          up to 125 x d dependent global atomics per lane, 64 particles' rows per wave-instruction;
//   MAP 2  deterministic mode: ONE wave walks the entries in order like k_traction_serial, a plain read-add-write per
//          member (distinct addresses inside one entry) and a barrier between two entries.
struct XlArgs {
  const int *ids, *load, *inv;  // [n] caller's index, [n] contour number, [np] caller's index -> slot
  const double *a0, *T;         // [n] A0 (3-D; 2-D: Vol_0 / thickness), [nloads][3] traction vectors of this step
  double thickness;
  int n;
};
template <int N>
__device__ __forceinline__ double pick_factor(const double (&e)[N], int i) {  // e[i] without an indexed (scratch) array
  double v = e[0];
#pragma unroll
  for (int q = 1; q < N; q++) v = i == q ? e[q] : v;
  return v;
}
template <int ND, int MAP>
__device__ __forceinline__ void explicit_traction_entry(const PView& P, const GridD& g, const XlArgs& a, int e, int lane,
                                                        double* __restrict__ force) {
  constexpr int KN = Lme<ND>::KN, NS = 25 * KN;
  const int p = a.inv[a.ids[e]];
  Lme<ND> c;
  double lam[ND], beta;
  if (!load_lme<ND>(P, g, p, c, lam, beta)) return;
  const double a0 = ND == 3 ? a.a0[e] : PF(P, F_VOL0, p) / a.thickness;  // U-Verlet.c:851-857
  const double zinv = lme_zinv<ND>(c);
  const double* T = a.T + (size_t)a.load[e] * 3;
  if (MAP == 1) {
    double Ta[ND];
#pragma unroll
    for (int d = 0; d < ND; d++) Ta[d] = T[d];
    for (int k = 0; k < KN; k++)
      for (int j = 0; j < 5; j++)
        for (int i = 0; i < 5; i++) {
          if (!c.on(i + 5 * j + 25 * k)) continue;
          const double Npa = c.ex[i] * c.ey[j] * (ND == 3 ? c.ez[k % KN] : 1.0) * zinv;
          const int node = c.I0 + c.node_offset(g, i, j, k + (ND == 3 ? 0 : 2));
#pragma unroll
          for (int d = 0; d < ND; d++) atomic_add_f64(force + (size_t)node * ND + d, Npa * Ta[d] * a0);
        }
    return;
  }
  for (int q = lane; q < NS * ND; q += 64) {
    const int m = q / ND, d = q - m * ND;
    if (!c.on(m)) continue;
    const int i = m % 5, j = (m / 5) % 5, k = m / 25;
    const double Npa = pick_factor(c.ex, i) * pick_factor(c.ey, j) * (ND == 3 ? pick_factor(c.ez, k) : 1.0) * zinv;
    const int node = c.I0 + c.node_offset(g, i, j, k + (ND == 3 ? 0 : 2));
    double* o = force + (size_t)node * ND + d;
    const double v = Npa * T[d] * a0;
    if (MAP == 2) *o = *o + v;
    else atomic_add_f64(o, v);
  }
}
template <int ND, int MAP>
__global__ __launch_bounds__(MAP == 2 ? 64 : BLK) void k_explicit_traction(PView P, GridD g, XlArgs a, double* force) {
  if (MAP == 2) {
    for (int e = 0; e < a.n; e++) {  // uniform
      explicit_traction_entry<ND, 2>(P, g, a, e, threadIdx.x, force);
      __syncthreads();  // the stores of this particle are done before the next one reads the same nodes
    }
  } else {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int e = MAP == 1 ? t : t >> 6;
    if (e < a.n) explicit_traction_entry<ND, MAP>(P, g, a, e, threadIdx.x & 63, force);
  }
}

static const char* explicit_loads_halo_msg =
    "the contour tractions inside the explicit step are built for one rank: with a halo callback or an RCCL exchange "
    "attached, a contour particle near a slab face would add to band nodes behind the exchange of the nodal forces";
extern "C" int nlps_gpu_set_explicit_loads(nlps_gpu* h, const nlps_bcc* loads, int nloads, double thickness,
                                           const double* area0) {
  const char* who = "nlps_gpu_set_explicit_loads: ";
  const int ND = h->nd, np = h->P.np, nsteps = h->nsteps;
  if (nloads < 0 || (nloads > 0 && !loads)) {
    h->err = std::string(who) + "nloads < 0, or loads is NULL";
    return 1;
  }
  if (nloads > 0) {
    if (h->halo || h->rccl) {
      h->err = std::string(who) + explicit_loads_halo_msg;
      return 1;
    }
    if (h->migrated) {
      h->err = std::string(who) + "not available after a migration (particle order is by global id)";
      return 1;
    }
    if (ND == 3 && !area0) {
      h->err = std::string(who) + "the 3-D build needs Phi.Area_0 (area0)";
      return 1;
    }
    if (ND == 2 && !(thickness > 0.0)) {
      h->err = std::string(who) + "the 2-D build needs Thickness_Plain_Stress (thickness) > 0";
      return 1;
    }
  }
  std::vector<int> ids, lidx;
  std::vector<double> A;
  for (int l = 0; l < nloads; l++)
    for (int q = 0; q < loads[l].nnodes; q++) {
      const int p = loads[l].nodes[q];
      if (p < 0 || p >= np) {
        h->err = std::string(who) + "particle index outside the cloud";
        return 1;
      }
      ids.push_back(p);
      lidx.push_back(l);
      if (ND == 3) A.push_back(area0[p]);
    }
  const size_t n = ids.size();
  // the traction vector of every step: zero at the start of the step, each contour in turn overwrites the directions it
  // switches on and hands the others on to the next contour (U-Verlet.c:865-869)
  std::vector<double> T(n ? (size_t)nsteps * nloads * 3 : 0, 0.0);
  if (n)
    for (int t = 0; t < nsteps; t++) {
      double Tc[3] = {0.0, 0.0, 0.0};
      for (int l = 0; l < nloads; l++) {
        for (int i = 0; i < ND && i < loads[l].dim; i++)
          if (loads[l].dir[(size_t)i * nsteps + t] == 1) Tc[i] = loads[l].value[(size_t)i * nsteps + t];
        for (int i = 0; i < 3; i++) T[((size_t)t * nloads + l) * 3 + i] = Tc[i];
      }
    }
  nlps_gpu::Loads fresh;
  fresh.n = (int)n;
  fresh.nloads = n ? nloads : 0;
  fresh.thickness = thickness;
  if (n) {
    HIPCHK(fresh.ids.reserve(n));
    HIPCHK(fresh.load.reserve(n));
    HIPCHK(fresh.T.reserve(T.size()));
    if (ND == 3) HIPCHK(fresh.a0.reserve(n));
    HIPCHK(hipMemcpy(fresh.ids, ids.data(), n * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(fresh.load, lidx.data(), n * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(fresh.T, T.data(), T.size() * sizeof(double), hipMemcpyHostToDevice));
    if (ND == 3) HIPCHK(hipMemcpy(fresh.a0, A.data(), n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(reserve_inv_perm(h));
  }
  // the copies above are ordered on the default stream only (see ensure_bcs), and a step in flight may still read the
  // tables this call replaces
  HIPCHK(hipDeviceSynchronize());
  h->loads = std::move(fresh);
  return 0;
}

// the contour tractions of `step` into the nodal force of the explicit step (loads.n > 0; the checks are the step's)
static int explicit_loads_launch(nlps_gpu* h, int step) {
  const XlArgs a{h->loads.ids, h->loads.load, inv_perm(h), h->loads.a0, h->loads.T + (size_t)step * h->loads.nloads * 3, h->loads.thickness,
                 h->loads.n};
  if (h->timing) {
    for (hipEvent_t& e : h->loads_ev)
      if (!e) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventRecord(h->loads_ev[0], h->stream));
  }
  if (h->deterministic) LAUNCH_ND_BLK((k_explicit_traction<2, 2>), (k_explicit_traction<3, 2>), 1, 64, h->P, h->g, a, h->N.force);
  else if (h->loads_lane_map) LAUNCH_ND((k_explicit_traction<2, 1>), (k_explicit_traction<3, 1>), nblk(h->loads.n), h->P, h->g, a, h->N.force);
  else LAUNCH_ND((k_explicit_traction<2, 0>), (k_explicit_traction<3, 0>), nblk(h->loads.n, BLK / 64), h->P, h->g, a, h->N.force);
  HIPCHK(hipGetLastError());
  if (h->timing) HIPCHK(hipEventRecord(h->loads_ev[1], h->stream));
  return 0;
}


// ------------------------------------------------------------------------------------------------
// The step record (nlps_gpu_set_step_record; kernels: nlps_record.hpp)
// ------------------------------------------------------------------------------------------------
static const char* step_record_halo_msg =
    "reaction totals and probes are built for one rank: not with a halo callback or an RCCL exchange attached, nor after a "
    "migration (the particle sums alone are allowed there)";
static int rec_probe_doubles_of(int nd, unsigned fields) {
  const int T = nd == 2 ? 5 : 9;
  int n = 0;
  for (int b = 0; b < 10; b++)
    if ((fields >> b) & 1u) n += b < 4 ? nd : (b < 6 ? T : 1);
  return n;
}
extern "C" int nlps_gpu_set_step_record(nlps_gpu* h, const nlps_record_cfg* cfg) {
  const char* who = "nlps_gpu_set_step_record: ";
  if (!cfg) {
    HIPCHK(hipDeviceSynchronize());  // (a step in flight may still write the ring)
    h->rec = {};
    return 0;
  }
  const int np = h->P.np;
  if (cfg->every < 1 || cfg->capacity < 1) {
    h->err = std::string(who) + "every >= 1 and capacity >= 1";
    return 1;
  }
  if (cfg->nsets < 0 || cfg->nprobes < 0 || (cfg->nprobes > 0 && !cfg->probes)) {
    h->err = std::string(who) + "a negative count, or probes is NULL";
    return 1;
  }
  if (cfg->nprobes > 0 && (cfg->probe_fields == 0 || (cfg->probe_fields >> 10) != 0)) {
    h->err = std::string(who) + "probes need probe_fields (NLPS_PROBE_*)";
    return 1;
  }
  for (int q = 0; q < cfg->nprobes; q++)
    if (cfg->probes[q] < 0 || cfg->probes[q] >= np) {
      h->err = std::string(who) + "probe index outside the cloud";
      return 1;
    }
  if ((cfg->nprobes > 0 || cfg->nsets > 0) && (h->halo || h->rccl || h->migrated)) {
    h->err = std::string(who) + step_record_halo_msg;
    return 1;
  }
  nlps_gpu::StepRecord fresh;
  fresh.on = 1;
  fresh.every = cfg->every;
  fresh.capacity = cfg->capacity;
  fresh.nsets = cfg->nsets;
  fresh.nprobes = cfg->nprobes;
  fresh.fields = cfg->nprobes > 0 ? cfg->probe_fields : 0u;
  fresh.probe_doubles = cfg->nprobes > 0 ? rec_probe_doubles_of(h->nd, cfg->probe_fields) : 0;
  const size_t row = (size_t)NLPS_REC_NGLOBAL + (size_t)cfg->nsets * 3 + (size_t)cfg->nprobes * fresh.probe_doubles;
  fresh.row = (int)row;
  HIPCHK(fresh.rows.reserve(row * (size_t)cfg->capacity));
  HIPCHK(fresh.part.reserve((size_t)REC_NQ * REC_MAX_BLOCKS));  // (for any particle count: a migration changes it)
  if (cfg->nprobes > 0) {
    HIPCHK(fresh.probes.reserve((size_t)cfg->nprobes));
    HIPCHK(hipMemcpy(fresh.probes, cfg->probes, (size_t)cfg->nprobes * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(reserve_inv_perm(h));
  }
  HIPCHK(hipMemset(fresh.rows, 0, row * (size_t)cfg->capacity * sizeof(double)));
  // the copies above are ordered on the default stream only, and a step in flight may still write the ring this call replaces
  HIPCHK(hipDeviceSynchronize());
  h->rec = std::move(fresh);
  return 0;
}

extern "C" int nlps_gpu_step_record_layout(nlps_gpu* h, int* row_doubles, int* reaction_offset, int* probe_offset,
                                           int* probe_doubles) {
  if (!h->rec.on) {
    h->err = "nlps_gpu_step_record_layout: no step record is set";
    return 1;
  }
  if (row_doubles) *row_doubles = h->rec.row;
  if (reaction_offset) *reaction_offset = NLPS_REC_NGLOBAL;
  if (probe_offset) *probe_offset = NLPS_REC_NGLOBAL + 3 * h->rec.nsets;
  if (probe_doubles) *probe_doubles = h->rec.probe_doubles;
  return 0;
}

// a record with reaction totals or probes on a handle that has become a slab rank (or migrated) since the set
static int rec_check(nlps_gpu* h, const char* who) {
  if ((h->rec.nprobes > 0 || h->rec.nsets > 0) && (h->halo || h->rccl || h->migrated)) {
    h->err = std::string(who) + ": the step record is set with reaction totals or probes: " + step_record_halo_msg;
    return 1;
  }
  return 0;
}

// One row of the state as it stands, on the handle's stream: no allocation, no synchronisation, no copy.  bcc / nbcc /
// step: the Dirichlet sets of the explicit step that has just run (kind NLPS_REC_KIND_EXPLICIT), else nbcc = 0.
static int rec_write(nlps_gpu* h, int kind, int step, double dt, const nlps_bcc* bcc, int nbcc) {
  if (materialise_move(h)) return 1;  // (nlps_gpu_record_now between two steps; a step with the record on defers nothing)
  const int np = h->P.np, nb = np > 0 ? std::min(nblk(np, REC_NT), REC_MAX_BLOCKS) : 0;
  double* row = h->rec.rows + (size_t)(h->rec.total % h->rec.capacity) * h->rec.row;
  const int lazy = (h->rolled && !h->rolled_keep) ? 1 : 0;  // tau and W of the hyperelastic laws are not stored
  if (np > 0) LAUNCH_ND_BLK(k_rec_particles<2>, k_rec_particles<3>, nb, REC_NT, h->P, h->mats_d, lazy, h->rec.part.get(), nb);
  const RecHead hd{(double)step, (double)kind, dt, h->rec.time, (double)np};
  hipLaunchKernelGGL(k_rec_finish, dim3(REC_NQ), dim3(REC_NT), 0, h->stream, (const double*)h->rec.part.get(), nb, hd,
                     (const int*)h->gstatus_d.get(), row);
  for (int s0 = 0; s0 < h->rec.nsets; s0 += REC_SETS_PER_LAUNCH) {
    const int cnt = std::min(REC_SETS_PER_LAUNCH, h->rec.nsets - s0);
    RecSets rs;
    memset(&rs, 0, sizeof rs);
    rs.nlive = std::max(0, std::min(cnt, nbcc - s0));
    for (int i = 0; i < rs.nlive; i++) {
      const BcDev& b = h->bcs[s0 + i];
      rs.nodes[i] = b.dnodes;
      rs.n[i] = b.n;
      rs.dim[i] = bcc[s0 + i].dim;
      rs.bits[i] = b.n > 0 ? dirbits_of(bcc[s0 + i], step, h->nsteps) : 0;
    }
    LAUNCH_ND_BLK(k_rec_reactions<2>, k_rec_reactions<3>, cnt, REC_NT, h->N, rs, h->n0, h->nwn, row + NLPS_REC_NGLOBAL + (size_t)3 * s0);
  }
  if (h->rec.nprobes > 0) {
    const int* inv = inv_perm(h);
    LAUNCH_ND_BLK(k_rec_probes<2>, k_rec_probes<3>, nblk(h->rec.nprobes * 10, REC_NT), REC_NT, h->P, h->mats_d, lazy,
                  (const int*)h->rec.probes.get(), inv, h->rec.nprobes, h->rec.fields, h->rec.probe_doubles,
                  row + NLPS_REC_NGLOBAL + (size_t)3 * h->rec.nsets);
  }
  HIPCHK(hipGetLastError());
  h->rec.total++;
  return 0;
}
// the tail of a step (rec_on): the clock runs for every step, a row is written for the steps of the interval
static int rec_step(nlps_gpu* h, int kind, int step, double dt, const nlps_bcc* bcc, int nbcc) {
  h->rec.time += dt;
  if (step % h->rec.every != 0) return 0;
  return rec_write(h, kind, step, dt, bcc, nbcc);
}

extern "C" int nlps_gpu_record_now(nlps_gpu* h, int tag) {
  if (!h->rec.on) {
    h->err = "nlps_gpu_record_now: no step record is set";
    return 1;
  }
  if (rec_check(h, "nlps_gpu_record_now")) return 1;
  return rec_write(h, NLPS_REC_KIND_NOW, tag, 0.0, nullptr, 0);
}

extern "C" int nlps_gpu_read_step_records(nlps_gpu* h, long long* total, int* count, double* rows, int max_rows) {
  if (!h->rec.on) {
    h->err = "nlps_gpu_read_step_records: no step record is set";
    return 1;
  }
  if (max_rows < 0) {
    h->err = "nlps_gpu_read_step_records: max_rows < 0";
    return 1;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  const long long have = std::min<long long>(h->rec.total, h->rec.capacity);
  const int n = (int)std::min<long long>(have, max_rows);
  if (total) *total = h->rec.total;
  if (count) *count = n;
  if (!rows) return 0;
  for (int r = 0; r < n; r++) {  // (row number g lives in slot g % capacity: at most two runs of slots, copied row by row)
    const long long g = h->rec.total - n + r;
    HIPCHK(hipMemcpy(rows + (size_t)r * h->rec.row, h->rec.rows + (size_t)(g % h->rec.capacity) * h->rec.row,
                     (size_t)h->rec.row * sizeof(double), hipMemcpyDeviceToHost));
  }
  return 0;
}

extern "C" double nlps_host_courant_dt(double CFL, double hh, double Cel, const double* row) {
  return CFL * hh / (row ? Cel + row[NLPS_REC_VMAX_COMP] : Cel);  // U_DeltaT__SolversLib__, Courant.c:26-50
}

// ------------------------------------------------------------------------------------------------
// the particle snapshot (include/nlps_gpu.h)
// ------------------------------------------------------------------------------------------------
extern "C" int nlps_gpu_set_snapshots(nlps_gpu* h, const nlps_snapshot_cfg* cfg) {
  const char* who = "nlps_gpu_set_snapshots: ";
  if (!cfg) {
    h->snap = {};  // (waits for the copies in flight, then frees)
    return 0;
  }
  if (cfg->slots < 1 || cfg->slots > NLPS_SNAP_MAX_SLOTS) {
    h->err = std::string(who) + "slots outside [1, NLPS_SNAP_MAX_SLOTS]";
    return 1;
  }
  if (cfg->fields == 0 || (cfg->fields >> SNAP_NFIELDS) != 0) {
    h->err = std::string(who) + "fields is 0 or has a bit outside NLPS_SNAP_*";
    return 1;
  }
  if (h->migrated) {
    h->err = std::string(who) + "the handle has migrated particles: its rows are by global id, which a snapshot does not follow";
    return 1;
  }
  const int np = h->P.np;
  const size_t per = (size_t)8 * snap_doubles_before(cfg->fields, SNAP_NFIELDS - 1, h->nd) + ((cfg->fields & NLPS_SNAP_I0) ? 4 : 0);
  const size_t bytes = std::max<size_t>(8, (size_t)np * per), words = (bytes + 7) / 8;
  // everything is made first: a failure leaves the snapshots that were set as they are
  nlps_gpu::Snapshots fresh;
  fresh.slots = cfg->slots;
  fresh.cap = np;
  fresh.fields = cfg->fields;
  fresh.bytes = bytes;
  hipError_t e = fresh.stream.create();
  for (int i = 0; i < cfg->slots && e == hipSuccess; i++) e = fresh.slot[i].create(words);
  if (e == hipSuccess) e = reserve_inv_perm(h);  // (last: a refused call leaves nothing on the handle)
  if (e != hipSuccess) {
    (void)hipGetLastError();
    char buf[200];
    snprintf(buf, sizeof buf, "%scannot allocate %d slots of %zu bytes on the device and in pinned memory (%s)", who, cfg->slots,
             bytes, hipGetErrorString(e));
    h->err = buf;
    return 1;
  }
  h->snap = std::move(fresh);  // (waits for the copies in flight of the snapshots that were set, then frees them)
  return 0;
}

static int snap_check(nlps_gpu* h, const char* who, int slot, bool begun) {
  if (h->snap.slots == 0) {
    h->err = std::string(who) + ": no snapshots are set (nlps_gpu_set_snapshots)";
    return 1;
  }
  if (begun && (slot < 0 || slot >= h->snap.slots || h->snap.slot[slot].state == 0)) {
    h->err = std::string(who) + ": that slot was not begun";
    return 1;
  }
  return 0;
}

extern "C" int nlps_gpu_snapshot_begin(nlps_gpu* h, int tag, int* slot) {
  const char* who = "nlps_gpu_snapshot_begin";
  if (snap_check(h, who, 0, false)) return 1;
  const int np = h->P.np;
  if (h->migrated || np > h->snap.cap) {
    h->err = std::string(who) + ": the handle has migrated particles since the snapshots were set: its rows are by global id";
    return 1;
  }
  int i = 0;
  while (i < h->snap.slots && h->snap.slot[i].state != 0) i++;
  if (i == h->snap.slots) {
    h->err = std::string(who) + ": every slot is in flight or unreleased (nlps_gpu_snapshot_release)";
    return 1;
  }
  nlps_gpu::SnapSlot& s = h->snap.slot[i];
  const int D = snap_doubles_before(h->snap.fields, SNAP_NFIELDS - 1, h->nd);
  const size_t bytes = (size_t)np * ((size_t)8 * D + ((h->snap.fields & NLPS_SNAP_I0) ? 4 : 0));
  if (np > 0) {
    const SnapArgs a{h->snap.fields, h->rolled ? 1 : 0, (h->rolled && !h->rolled_keep) ? 1 : 0,
                     h->move_pending ? h->moved_d.get() : nullptr, h->snap_by_caller ? inv_perm(h) : h->perm_d.get(),
                     s.dev.get()};
    if (h->snap_by_caller) LAUNCH_ND_BLK((k_snap_pack<2, true>), (k_snap_pack<3, true>), nblk(np, SNAP_NT), SNAP_NT, h->P, h->mats_d, a);
    else LAUNCH_ND_BLK(k_snap_pack<2>, k_snap_pack<3>, nblk(np, SNAP_NT), SNAP_NT, h->P, h->mats_d, a);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(s.packed, h->stream));
  const hipStream_t ss = h->snap.stream.stream();
  HIPCHK(hipStreamWaitEvent(ss, s.packed, 0));
  if (bytes > 0) HIPCHK(hipMemcpyAsync(s.pin.host(), s.dev.get(), bytes, hipMemcpyDeviceToHost, ss));
  HIPCHK(hipEventRecord(s.copied, ss));
  s.state = 1;
  s.tag = tag;
  s.np = np;
  if (slot) *slot = i;
  return 0;
}

extern "C" int nlps_gpu_snapshot_wait(nlps_gpu* h, int slot, nlps_particles* view, int* tag) {
  if (snap_check(h, "nlps_gpu_snapshot_wait", slot, true)) return 1;
  nlps_gpu::SnapSlot& s = h->snap.slot[slot];
  HIPCHK(hipEventSynchronize(s.copied));
  if (tag) *tag = s.tag;
  if (!view) return 0;
  memset(view, 0, sizeof *view);
  view->np = s.np;
  double** member[SNAP_NFIELDS - 1] = {&view->x_GC, &view->dis, &view->vel, &view->acc, &view->F_n, &view->Stress, &view->b_e_n,
                                       &view->J_n, &view->rho, &view->mass, &view->Vol_0, &view->W, &view->Kappa_n, &view->EPS_n,
                                       &view->Back_stress, &view->Damage_n, &view->Strain_f_n, &view->lambda, &view->Beta};
  double* o = s.pin.host();
  for (int b = 0; b < SNAP_NFIELDS - 1; b++) {
    if (!((h->snap.fields >> b) & 1u)) continue;
    *member[b] = o;
    o += (size_t)s.np * snap_ncomp(b, h->nd);
  }
  if (h->snap.fields & NLPS_SNAP_I0) view->I0 = reinterpret_cast<int*>(o);
  return 0;
}

extern "C" int nlps_gpu_snapshot_release(nlps_gpu* h, int slot) {
  if (snap_check(h, "nlps_gpu_snapshot_release", slot, true)) return 1;
  HIPCHK(hipEventSynchronize(h->snap.slot[slot].copied));  // (a copy in flight still writes the pinned block the next begin reuses)
  h->snap.slot[slot].state = 0;
  return 0;
}

extern "C" int nlps_gpu_snapshot_bytes(nlps_gpu* h, size_t* device, size_t* pinned) {
  if (snap_check(h, "nlps_gpu_snapshot_bytes", 0, false)) return 1;
  if (device) *device = (size_t)h->snap.slots * h->snap.bytes + (size_t)std::max(h->snap.cap, 1) * sizeof(int);  // (+ the inverse permutation)
  if (pinned) *pinned = (size_t)h->snap.slots * h->snap.bytes;
  return 0;
}

extern "C" int nlps_gpu_roll_state(nlps_gpu* h) {
  tan_stale(h, "nlps_gpu_roll_state");
  if (materialise_roll(h)) return 1;
  LAUNCH_ND((k_roll<2>), (k_roll<3>), nblk(h->P.np), h->P);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int nlps_gpu_update_kinetics(nlps_gpu* h, double alpha_blend, const double* dU, const double* Un_dt,
                                        const double* dU_dt, const double* dU_dt2) {
  tan_stale(h, "nlps_gpu_update_kinetics");
  if (need_masks(h, "nlps_gpu_update_kinetics")) return 1;
  if (materialise_move(h)) return 1;
  h->searched = h->ahead = h->lists_ready = false;  // the particles move: the next search is a search
  int ND = h->nd;
  size_t st = (size_t)h->g.nnodes * ND;
  // Un_dt = dU_dt = dU_dt2 = NULL: the quasi-static driver's __update_Particles (U-Static.c:1380-1470) moves the
  // particles by sum N dU and leaves velocity and acceleration alone
  const bool quasi_static = !Un_dt && !dU_dt && !dU_dt2;
  if (!quasi_static && (!Un_dt || !dU_dt || !dU_dt2)) {
    h->err = "nlps_gpu_update_kinetics: pass all of Un_dt, dU_dt, dU_dt2 or none of them (quasi-static update)";
    return 1;
  }
  if (!dU) {
    h->err = "nlps_gpu_update_kinetics: dU is NULL";
    return 1;
  }
  if (to_grid(h, h->gridB, dU, ND)) return 1;
  if (quasi_static) {
    HIPCHK(hipMemsetAsync(h->gridB + st, 0, 3 * st * sizeof(double), h->stream));
  } else {
    if (to_grid(h, h->gridB + st, Un_dt, ND)) return 1;
    if (to_grid(h, h->gridB + 2 * st, dU_dt, ND)) return 1;
    if (to_grid(h, h->gridB + 3 * st, dU_dt2, ND)) return 1;
  }
  {
    TileD td = tile_view(h);
    const int qs = quasi_static ? 1 : 0;
    LAUNCH_ND(kb_kinetics_tile<2>, kb_kinetics_tile<3>, h->ntw, h->P, h->g, td, alpha_blend, h->gridB, h->gridB + st,
              h->gridB + 2 * st, h->gridB + 3 * st, qs);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

__global__ void k_null_bracket(PView, GridD, NView, TileD, const MatD*, ParamsD, int*, const double*) {}

// The node runs and the damage hook, shared by the explicit step with the damage hooks (nlps_gpu_set_explicit_damage) and
// the fused damage residual (nlps_gpu_set_implicit_damage): with `rebuild` the runs of the current closest nodes (k_run_*:
// no sort), once per numbering of the slots those of the snapshot's closest nodes (eigenerosion's frozen lists,
// Beps.c:30-36), then the hook, which sets Damage_n1 (Strain_f_n1) and scales every Kirchhoff stress in place.  All on the
// handle's stream, no sort call, no synchronisation, no allocation (the setters made the tables).
template <bool SNAP>  // the runs of the current (false) or the snapshot's (true) closest nodes
static void build_runs(nlps_gpu* h, int* first, int* last, int* sorted, bool sort_runs) {
  const int np = h->P.np, nn = h->g.nnodes;
  const dim3 gp(nblk(np)), gn(nblk(nn)), blk(BLK);
  hipLaunchKernelGGL(k_run_count<SNAP>, gp, blk, 0, h->stream, h->P, nn, h->dmg.cnt.get(), h->dmg.rank.get(), h->dmg.cursor.get());
  hipLaunchKernelGGL(k_run_first, gn, blk, 0, h->stream, nn, h->dmg.cnt.get(), h->dmg.cursor.get(), first, last);
  hipLaunchKernelGGL(k_run_fill<SNAP>, gp, blk, 0, h->stream, h->P, nn, (const int*)first, (const int*)h->dmg.rank.get(), sorted);
  if (sort_runs) hipLaunchKernelGGL(k_run_sort, gn, blk, 0, h->stream, nn, np, (const int*)first, (const int*)last, sorted);
}
static int damage_runs_and_hook(nlps_gpu* h, bool rebuild) {
  const int np = h->P.np;
  // deterministic mode (nlps_gpu_set_deterministic_damage): ascending slot index inside every run, so that the hook's sums
  // over a neighbourhood run in an order the particle arrays alone decide.  (Both switches drop the cached tables.)
  const bool sort_runs = h->deterministic && h->det_damage;
  if (rebuild) {
    build_runs<false>(h, h->dmg.first.get(), h->dmg.last.get(), h->dmg.sorted.get(), sort_runs);
    h->dmg.builds++;
    h->dmg.tables = true;
  }
  if (h->P.softening) {
    double* T0 = h->gather_tmp.get();  // [npad] scratch of the re-sort, idle here
    LAUNCH_ND((k_soften_pass1<2>), (k_soften_pass1<3>), nblk(np), h->P, h->mats_d, T0);
    // (orig[] = the caller's index of every slot: perm_d travels with the re-sorts)
    LAUNCH_ND((k_soften_pass2<2>), (k_soften_pass2<3>), nblk(np), h->P, h->g, h->mats_d, h->dmg.first, h->dmg.last, h->dmg.sorted,
              (const uint8_t*)h->rank1_d, (const int*)h->perm_d, (const double*)T0, h->g.h);
  } else {
    if (!h->dmg.tables0) {  // frozen lists (Beps.c:30-36): the runs of the snapshot's closest nodes
      build_runs<true>(h, h->dmg.first0.get(), h->dmg.last0.get(), h->dmg.sorted0.get(), sort_runs);
      h->dmg.tables0 = true;
    }
    LAUNCH_ND((k_damage<2>), (k_damage<3>), nblk(np), h->P, h->g, h->mats_d, h->dmg.first, h->dmg.last, h->dmg.sorted,
              h->dmg.first0, h->dmg.last0, h->dmg.sorted0, h->g.h);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// The fused explicit step: refuse, re-sort, decide the form (StepForm), search + lists + K2, one of three schedules.
static int explicit_step_refuse(nlps_gpu* h, int nbcc, int step) {
  const bool fluid = (h->law_present & (1 << NLPS_KLAW_FLUID)) != 0;
  if (fluid && !h->explicit_fluid) {
    h->err = "nlps_gpu_explicit_step: the cloud holds the Newtonian-Fluid-Compressible law, which reads the rate tensor dt_F_n1; "
             "the reference has no working explicit driver that defines it (implicit path only)";
    return 1;
  }
  if (fluid && (h->halo || h->rccl)) {  // (nlps_gpu_set_explicit_fluid)
    h->err = "nlps_gpu_explicit_step: the explicit step of the Newtonian-Fluid-Compressible law is built for one rank: not with "
             "a halo callback or an RCCL exchange attached";
    return 1;
  }
  if (fluid && h->P.erosion) {
    h->err = "nlps_gpu_explicit_step: the cloud holds the Newtonian-Fluid-Compressible law and was created with "
             "driver_eigenerosion / driver_eigensoftening; the state half of the damage step is cut for the solid laws";
    return 1;
  }
  const bool dmg = h->P.erosion != 0;
  if (dmg && !h->explicit_damage) {
    h->err = "nlps_gpu_explicit_step: the eigenerosion hooks exist in the level-B stages only (the reference defines them in "
             "U-Newmark-beta.c / U-Static.c; its explicit drivers are stubs)";
    return 1;
  }
  if (dmg && (h->halo || h->rccl)) {
    h->err = "nlps_gpu_explicit_step: the damage hooks inside the explicit step are built for one rank: with a halo callback or "
             "an RCCL exchange attached, an epsilon-neighbourhood across a slab face would need ghost particles";
    return 1;
  }
  if (dmg && h->deterministic && !h->det_damage) {  // (nlps_gpu_set_deterministic_damage)
    h->err = "nlps_gpu_explicit_step: the damage hooks inside the explicit step are not built for the deterministic mode (their "
             "node runs take ranks and run starts from atomics)";
    return 1;
  }
  if (h->fbar.on) {  // (nlps_gpu_set_explicit_fbar; the setter has refused what it could see)
    if (h->halo || h->rccl) {
      h->err = "nlps_gpu_explicit_step: F-bar is built for one rank: not with a halo callback or an RCCL exchange attached (a "
               "patch across a slab face would need its sums exchanged)";
      return 1;
    }
    if (h->deterministic) {
      h->err = "nlps_gpu_explicit_step: F-bar is not built for the deterministic mode (its patch sums are taken by atomics)";
      return 1;
    }
    if (h->migrated) {
      h->err = "nlps_gpu_explicit_step: F-bar is not available after a migration (particle order is by global id)";
      return 1;
    }
  }
  const bool loads = h->loads.n > 0 && h->P.np > 0;
  if (loads && (h->halo || h->rccl)) {
    h->err = std::string("nlps_gpu_explicit_step: ") + explicit_loads_halo_msg;
    return 1;
  }
  if (loads && h->migrated) {
    h->err = "nlps_gpu_explicit_step: the explicit loads are not available after a migration (particle order is by global id)";
    return 1;
  }
  if ((nbcc > 0 || loads) && check_step(h, step, "nlps_gpu_explicit_step")) return 1;
  if (h->rec.on && rec_check(h, "nlps_gpu_explicit_step")) return 1;  // (nlps_gpu_set_step_record)
  return 0;
}

// Is a re-sort due: the fixed interval, or earlier when enough particles have left the tiles their memory slots were
// sorted into (the estimates since the last one, `debt`, add up to the budget).  A re-sort moment read from an
// asynchronous word is not reproducible: the deterministic mode keeps the fixed interval.  Asked at the head of a step
// (behind this step's `debt +=`) and by the async fork about the NEXT step; the fork's own spelling left out
// `!deterministic` and `np > 0`, which hold wherever it runs (the async form is never deterministic and rides, np > 0)
// and without which `debt` has never grown.
static bool resort_due(const nlps_gpu* h) {
  if (h->resort_every <= 0) return false;
  const bool drifted = h->adaptive_resort > 0.0 && !h->deterministic && h->P.np > 0 && h->debt > h->adaptive_resort &&
                       h->steps_since_sort >= h->adaptive_min_steps;
  return h->steps_since_sort >= h->resort_every || drifted;
}

// What one step runs, decided once in front of its first launch.  (Which K3 kernel: launch_k3 / launch_k3_lazy.)
struct StepForm {
  bool dmg;    // the step with the damage hooks (nlps_gpu_set_explicit_damage)
  bool fbar;   // the step with F-bar (nlps_gpu_set_explicit_fbar): K3 split like the damage step's
  bool loads;  // the Neumann contours (nlps_gpu_set_explicit_loads)
  bool det;    // nlps_gpu_set_deterministic: one wave per tile, slabs, k_slab_gather
  // With a halo callback and ghost bands set, every exchange is started right after the tiles that touch a
  // ghost band have produced their part and is waited for only before those tiles need the result; the tiles
  // (and nodes) away from the bands run in between, on the handle's stream, while the exchange proceeds on the
  // callee's stream.  Without overlap each stage is one pass over all tiles and the exchange blocks in place.
  bool ov2;  // one launch per stage, exchange behind its interior tiles
  bool ov;   // boundary tiles, exchange, interior tiles
  // the search of the next step rides on K5 (k5_tile<., ., true>, seeds and bins included).  A slab rank that holds no
  // particles has nothing to search: it launches k5_tile<., ., false> and leaves `searched` / `ahead` false.
  bool ride;
  // Folded form (k3_tile_lazy / k5_tile_lazy): one law, the Dirichlet sets small enough to travel as kernel arguments:
  // no nodal kernels between the stages (dU, accelerations, reactions are made later if somebody asks).  With a ghost
  // exchange too, in every overlap form: a K3 / K5 launch comes behind the pick-up of the exchange its nodes need (interior
  // tiles never touch a band node), exactly where the nodal kernel of its node range stood.
  // (measured: 3 % faster per step at 1 M particles -- three launches less -- and equal within the noise at 4 M and 8 M,
  // where the window loads of 17 k tiles redo the two divisions per node 16 times over: on below 2 M particles,
  // NLPS_LAZY_NODAL=2 always)
  // (a step with the damage hooks always runs the non-folded form on the handle's stream: neither lazy nor async_form)
  bool lazy;
  // Async lists: the folded form of ONE rank (no ghost exchange, the whole grid as node window).  Nothing the list stage
  // of the next step needs comes from K5 -- the position K5 writes is x + d_dis, and d_dis is K3's -- so the search
  // leaves K5 for a kernel of its own in front of it (k_search_ahead, full ranks), and the activation and the list
  // kernels run on the side stream beside K5, into the twin set (nlps_gpu::side); the handle's stream waits for them at
  // the end of this call.  The multi-rank forms, the deterministic mode, the non-folded form and clouds of several laws
  // keep the riding search and the deferred ranks.
  bool async_form;
  bool inline_bc;      // the Dirichlet sets of this step travel as one kernel argument (bs, bm)
  int law;             // -1: several laws in the cloud (law_present)
  BcStep bs;
  const unsigned* bm;  // the bit mask of the sets per node, nullptr without inline sets
};
static StepForm step_form(const nlps_gpu* h, const nlps_bcc* bcc, int nbcc, int step) {
  StepForm f{};
  f.dmg = h->P.erosion != 0;
  f.fbar = h->fbar.on && h->P.np > 0;
  f.loads = h->loads.n > 0 && h->P.np > 0;
  f.det = h->deterministic;
  f.ov2 = h->rccl && h->overlap == 2 && !h->deterministic;
  f.ov = !f.ov2 && (h->halo || h->rccl) && h->overlap;
  f.ride = h->P.np > 0;
  f.lazy = (h->lazy_nodal == 2 || (h->lazy_nodal == 1 && h->P.np <= 2000000)) && f.ride && !f.det && h->uniform_law >= 0 &&
           h->uniform_law <= NLPS_KLAW_FRICTIONAL && nbcc <= NLPS_MAX_BC_INLINE && !f.dmg && !f.fbar;
  f.async_form = f.lazy && h->async_lists && !h->halo && !h->rccl && node_lists(h) && h->nwn == h->g.nnodes;
  f.inline_bc = nbcc <= NLPS_MAX_BC_INLINE;
  f.law = h->uniform_law;
  if (f.inline_bc) {
    f.bs.n = nbcc;
    for (int i = 0; i < nbcc; i++) {
      f.bs.dim[i] = bcc[i].dim;
      f.bs.bits[i] = h->bcs[i].n > 0 ? dirbits_of(bcc[i], step, h->nsteps) : 0;
      bc_values(bcc[i], step, h->nsteps, f.bs.v[i]);
    }
  }
  f.bm = (f.inline_bc && nbcc > 0) ? h->bcmask_d.get() : nullptr;
  return f;
}

// One step in flight: the stages of the schedules below as methods, what they share as members.
struct ExplicitStep {
  nlps_gpu* h;
  const nlps_bcc* bcc;
  int nbcc, step;
  double dt, gamma_nm;
  StepForm f;
  double gv[3];
  LazyNodal ln;  // (lazy)
  K5Search ks;
  bool tiles_cleared = false;  // the tile counters of the riding search are reset by the first nodal_accel that runs
  bool ks_made = false;        // ks.tc is made by the first K5 launch
  bool forked = false;         // the side stream holds the list kernels of the next step
  bool deferred = false;       // K5 of this step leaves the move to the next K2 (nlps_gpu::move_pending)

  // second half of the deterministic flushes: per node, the window slabs of the tiles that hold it (part: node_ranges)
  void gather_nm(int part) { if (f.det) det_gather<3, 4>(h, part, 1, h->N.nm); }
  // (one slab per law present; the force half of a damage step: one slab per tile)
  void gather_force(int part) { if (f.det) det_gather<2, 3>(h, part, f.dmg ? 1 : __builtin_popcount(h->law_present), h->N.force); }
  // nodal dU = (sum m N dD) / M + Dirichlet values
  void nodal_dU(int part) {
    if (f.lazy) return;  // (K3 makes dU of its window nodes itself)
    const NodeRanges r = node_ranges(h, part);
    if (r.an + r.bn == 0) return;
    LAUNCH_ND(k_nodal_dU<2>, k_nodal_dU<3>, nblk(r.an + r.bn), r.a0, r.an, r.b0, r.bn, h->N, f.bm, f.bs);
    if (f.inline_bc) return;
    // Dirichlet values (nodes of the same range only)
    const NodeRanges in = node_ranges(h, 1);
    for (int i = 0; i < nbcc; i++) {
      if (h->bcs[i].n == 0) continue;
      double v[3];
      bc_values(bcc[i], step, h->nsteps, v);
      const int bits = dirbits_of(bcc[i], step, h->nsteps);
      const int r0 = part == 0 ? 0 : in.a0, r1 = part == 0 ? h->g.nnodes : in.a0 + in.an, inside = part == 2 ? 0 : 1;
      LAUNCH_ND(k_bc<2>, k_bc<3>, nblk(h->bcs[i].n), h->bcs[i].dnodes, h->bcs[i].n, bcc[i].dim, bits, v[0], v[1], v[2], h->N, r0,
                r1, inside);
    }
  }
  void nodal_accel(int part) {
    if (f.lazy) return;  // (K5 makes the accelerations itself; K3's workgroups have reset the search accumulators)
    const NodeRanges r = node_ranges(h, part);
    int* ctile = (f.ride && !tiles_cleared) ? h->tile_count2_d + h->tile0 : nullptr;
    if (r.an + r.bn == 0 && !ctile) return;
    tiles_cleared = true;
    int* cnode = (f.ride && node_lists(h)) ? h->node_cnt_d.get() : nullptr;
    LAUNCH_ND(k_nodal_accel<2>, k_nodal_accel<3>, nblk(std::max(1, r.an + r.bn)), r.a0, r.an, r.b0, r.bn, h->N, gv[0], gv[1], gv[2],
              f.ride ? 1 : 0, cnode, ctile, h->ntw);
  }
  // MODE 1: the fused K3; MODE 5: its state half (the step with the damage hooks; a gather and per-particle stores, no
  // nodal sum: the same launch forms in deterministic mode)
  void k3(int cls, bool signal = false) {
    const TileD td = tile_view(h, cls);
    if (f.lazy) return launch_k3_lazy(h, td, signal, ln);
    if (f.fbar) return launch_k3_fbar_kin(h, td, (h->law_present & (1 << NLPS_KLAW_FLUID)) ? dt : 0.0);
    const K3Launch a{signal, f.det && !f.dmg, nullptr, dt};
    if (f.dmg) launch_k3<5>(h, td, a);
    else launch_k3<1>(h, td, a);
  }
  void k5(int cls) {
    const TileD td = tile_view(h, cls);
    if (f.ride && !ks_made && !f.async_form) {  // (one TileCnt per step: it consumes the re-home flag of the adaptive re-sort)
      ks.tc = tile_cnt(h, true);
      ks.tc.count = h->tile_count2_d;  // (tile_count_d sizes the lists this very launch walks)
      ks.tc.defer = node_lists(h) ? 1 : 0;
      h->ranks_deferred = ks.tc.defer != 0;
      ks_made = true;
    }
    const dim3 grid(h->ntw), blk(K5_BLK);
    with_nd(h->nd, [&](auto D) {
      // K5 exists in two forms: LAW = 0 serves laws 0 and 1, LAW = 2 every other law and the cloud of several
      with_bool(f.law == 0 || f.law == 1, [&](auto L01) {
        constexpr int LAW = CT(L01) ? 0 : 2;
        if (deferred) {  // (its search is in flight beside it, or has run: search_next_and_fork)
          hipLaunchKernelGGL((k5_tile_lazy<CT(D), LAW, false, true>), grid, blk, 0, h->stream, h->P, h->g, h->N, td, dt, gamma_nm,
                             ks, ln, h->gstatus_d);
        } else if (f.async_form) {  // (its search has run: search_next_and_fork)
          hipLaunchKernelGGL((k5_tile_lazy<CT(D), LAW, false>), grid, blk, 0, h->stream, h->P, h->g, h->N, td, dt, gamma_nm, ks, ln,
                             h->gstatus_d);
        } else if (f.lazy) {
          hipLaunchKernelGGL((k5_tile_lazy<CT(D), LAW>), grid, blk, 0, h->stream, h->P, h->g, h->N, td, dt, gamma_nm, ks, ln,
                             h->gstatus_d);
        } else {
          with_bool(f.ride, [&](auto SEARCH) {
            hipLaunchKernelGGL((k5_tile<CT(D), LAW, CT(SEARCH)>), grid, blk, 0, h->stream, h->P, h->g, h->N, td, dt, gamma_nm, ks);
          });
        }
      });
    });
  }
  // async lists, between K3 and K5: the search of the next step on the handle's stream, then -- unless the brackets of
  // nlps_gpu_set_timing are on, which keep every kernel on the handle's stream and leave the lists to the next step, or
  // the next step starts with a re-sort and has to search again anyway -- its activation and list kernels on the side
  // stream, which K5 then runs beside.  They read what the search wrote (seeds, counters, tile / rank per particle, I0n)
  // and write the twin set only; K5 reads neither.
  // The deferred form (step record off, no re-sort at the head of the next step: nlps_gpu::move_pending) runs K5 without
  // the move, so nothing K5 writes is read by the search, and the fork comes in front of the search: the whole chain
  // k_search_ahead, k_dilate_scan, k_fill_orders runs beside K5.  Who touches what between the fork and the join:
  //   k5_tile_lazy<., ., false, true>  reads   x, lambda, beta, I0, mlo, mhi, vel of the particles of this step's lists
  //                                            (td.order_m, lists.start / tile_count_d of the set in use), nm, force, active
  //                                            and fixed of the set in use, the Dirichlet sets;   writes acc, vel, gstatus (or)
  //   k_search_ahead                   reads   I0, tile, mlo, mhi, x, dis, d_dis, moved, rank1;   writes I0n, tile, rank, nrank,
  //                                            seed, tile_count2, node_cnt, home / foreign, moved, status / gstatus (or), and
  //                                            x, dis of a particle whose mark K2 did not take -- one in no list, which K5
  //                                            never visits
  //   k_dilate_scan<., 256>            reads   seed, tile_count2, node_cnt;   writes active, fixed, nm, force of the TWIN set,
  //                                            twin.start, twin.work, twin.nwork, the layer tables (tile_tab), foreign_h
  //   k_fill_orders                    reads   tile, rank, nrank, I0n, twin.start, the layer tables;   writes twin.order, twin.order2
  // tile_count2, node_cnt and the seeds are reset by K3's workgroups (LazyNodal), so the fork stands behind K3.  With the
  // timing brackets on, the same K5 runs behind the search on the handle's stream and the lists are left to the next step.
  int search_next_and_fork() {
    const int np = h->P.np, ND = h->nd;
    TileCnt tc = tile_cnt(h, true);  // (one per step: it consumes the re-home flag of the adaptive re-sort)
    tc.count = h->tile_count2_d;     // (tile_count_d sizes the lists K5 walks)
    h->ranks_deferred = false;
    const bool next_sorts = resort_due(h);
    deferred = !h->rec.on && !next_sorts && np >= h->defer_move_min;
    const bool lists = !h->timing && !next_sorts;
    if (deferred && !h->moved_d) {
      HIPCHK(h->moved_d.reserve(h->P.npad));
      HIPCHK(hipMemsetAsync(h->moved_d, 0, h->P.npad, h->stream));
    }
    if (lists && ensure_list_twins(h)) return 1;
    const bool side_search = deferred && lists;  // (nothing K5 writes is read by the search any more: the whole chain beside K5)
    if (side_search) HIPCHK(h->side.fork(h->stream));
    const hipStream_t ss = h->side.stream();
    with_nd(ND, [&](auto D) {
      hipLaunchKernelGGL(k_search_ahead<CT(D)>, dim3(nblk(np)), dim3(BLK), 0, side_search ? ss : h->stream, h->P, h->g, h->N,
                         h->rank1_d.get(), tc, h->moved_d.get(), deferred ? 1 : 0);
    });
    HIPCHK(hipGetLastError());
    if (h->moved_d) h->move_pending = deferred;  // (stale marks are gone either way; new ones exist in the deferred form)
    if (!lists) return 0;
    if (!side_search) HIPCHK(h->side.fork(h->stream));
    const ListBuild b2 = list_build(h, h->twin, h->tile_count2_d, nullptr);
    // (workgroups of 256: they are placed beside K5's, which leave one wave per SIMD free -- see k_dilate_scan)
    constexpr int SNT = 256;
    const int nb = 1 + (h->nwn + SNT - 1) / SNT + (h->ntw + SNT / 64 - 1) / (SNT / 64);
    int* fo = h->adaptive_resort > 0.0 ? h->foreign_d : nullptr;
    with_nd(ND, [&](auto D) {
      hipLaunchKernelGGL((k_dilate_scan<CT(D), SNT>), dim3(nb), dim3(SNT), 0, ss, h->n0, h->nwn, h->g, b2.N, b2.ts, fo, h->foreign_h.host(),
                         tile_tab(h), 1);
      // (non-deferred: position = start + rank, canonical position from the rank inside the node; the closest node is read
      // from I0n and nothing is committed -- K5 reads I0)
      hipLaunchKernelGGL(k_fill_orders<CT(D)>, dim3(nblk(np)), dim3(BLK), 0, ss, np, h->P.tile, h->P.rank, h->nrank_d, h->P.I0n,
                         (const int*)nullptr, h->twin.start, h->g, tile_tab(h), h->twin.order, h->twin.order2, (int*)nullptr,
                         h->node_cnt_d);
    });
    HIPCHK(hipGetLastError());
    forked = true;
    return 0;
  }
  // The step with the damage hooks, between the state half of K3 (MODE 5, launched by k3 above) and the nodal
  // accelerations: the node runs of this step's closest nodes (and, once per numbering of the slots, of the snapshot's),
  // the hook, which sets Damage_n1 (Strain_f_n1) and scales every Kirchhoff stress in place, and the force half.  All
  // on the handle's stream, no sort, no synchronisation, no allocation (nlps_gpu_set_explicit_damage made the tables).
  int damage_hook_and_forces() {
    if (damage_runs_and_hook(h, true)) return 1;  // (every step has searched: the runs are this step's)
    if (f.det)  // one wave per tile over the exact list, one slab per tile (slab_n = 1, slot 0); gather_force sums them
      LAUNCH_ND_BLK((k3f_wave<2, false>), (k3f_wave<3, false>), h->ntw, 64, h->P, h->g, h->N, tile_view(h, 0), h->gstatus_d);
    else
      LAUNCH_ND(k3f_tile<2>, k3f_tile<3>, h->ntw, h->P, h->g, h->N, tile_view(h, 0), h->gstatus_d);
    HIPCHK(hipGetLastError());
    return 0;
  }

  // The three schedules, each from behind search_and_lists (K2 is in flight) to the last particle kernel.  ev[3] .. ev[5]
  // are the timing brackets of nlps_gpu_set_timing.
  // Overlap mode 2: K2 is in flight as ONE launch; its boundary tiles release the exchange of the shared layers of nm,
  // which runs beside its interior tiles; the handle's stream picks the result up before the nodal kernel.  (RCCL ranks,
  // never deterministic: no slab gathers; no damage hooks, no contour loads, no async lists.)
  int run_overlap2() {
    const int ND = h->nd;
    if (halo(h, h->N.nm, 1 + ND, 8, 0, 3)) return 1;
    if (halo(h, h->N.nm, 1 + ND, 8, 0, 2)) return 1;
    nodal_dU(0);
    if (h->timing) HIPCHK(hipEventRecord(h->ev[3], h->stream));
    k3(0, true);
    HIPCHK(hipGetLastError());
    if (h->timing) HIPCHK(hipEventRecord(h->ev[4], h->stream));
    if (halo(h, h->N.force, ND, 8, 0, 4)) return 1;
    if (halo(h, h->N.force, ND, 8, 0, 2)) return 1;
    nodal_accel(0);
    if (h->timing) HIPCHK(hipEventRecord(h->ev[5], h->stream));
    k5(0);
    HIPCHK(hipGetLastError());
    return 0;
  }
  // Overlap mode 1: with ghost bands the shared layers are gathered first (only boundary tiles reach them) and go on
  // their way while the rest is summed.  (Ranks with an exchange: no damage hooks, no contour loads, no async lists.)
  int run_overlap1() {
    const int ND = h->nd;
    gather_nm(2);
    if (halo(h, h->N.nm, 1 + ND, 8, 0, 1)) return 1;
    gather_nm(1);
    nodal_dU(1);
    // timing brackets: the K3 bucket starts before the interior tiles (the band nodes' dU then counts as K3 time)
    if (h->timing) HIPCHK(hipEventRecord(h->ev[3], h->stream));
    k3(2);
    if (halo(h, h->N.nm, 1 + ND, 8, 0, 2)) return 1;
    nodal_dU(2);
    k3(1);
    HIPCHK(hipGetLastError());
    if (h->timing) HIPCHK(hipEventRecord(h->ev[4], h->stream));
    gather_force(2);
    if (halo(h, h->N.force, ND, 8, 0, 1)) return 1;
    gather_force(1);
    nodal_accel(1);
    if (h->timing) HIPCHK(hipEventRecord(h->ev[5], h->stream));
    k5(2);
    if (halo(h, h->N.force, ND, 8, 0, 2)) return 1;
    nodal_accel(2);
    k5(1);
    HIPCHK(hipGetLastError());
    return 0;
  }
  // One pass over all tiles per stage; an exchange, where there is one, blocks in place.
  int run_one_pass() {
    const int ND = h->nd, np = h->P.np;
    gather_nm(0);
    if (halo(h, h->N.nm, 1 + ND, 8, 0, 0)) return 1;
    nodal_dU(0);
    if (h->timing) HIPCHK(hipEventRecord(h->ev[3], h->stream));
    k3(0);
    if (f.dmg && np > 0 && damage_hook_and_forces()) return 1;
    if (f.fbar) launch_fbar_stress(h);  // (between the kinematic half of K3, launched by k3 above, and the nodal accelerations)
    HIPCHK(hipGetLastError());
    if (h->timing) HIPCHK(hipEventRecord(h->ev[4], h->stream));
    gather_force(0);
    // the contour tractions: behind K3's atomics -- or the fixed-order sum of its slabs -- in stream order, in front of
    // the readers of N.force (k_nodal_accel, K5's windows; the folded form keeps N.force for materialise_nodal).  Nothing
    // resets N.force between k_step_clear / k_dilate_scan at the head of the step and here; the side stream of the async
    // lists forks behind this launch and resets the twin set only.
    if (f.loads && explicit_loads_launch(h, step)) return 1;
    if (halo(h, h->N.force, ND, 8, 0, 0)) return 1;
    nodal_accel(0);
    if (f.async_form && search_next_and_fork()) return 1;
    if (h->timing) HIPCHK(hipEventRecord(h->ev[5], h->stream));
    k5(0);
    if (f.dmg && np > 0) hipLaunchKernelGGL(k_damage_roll, dim3(nblk(np)), dim3(BLK), 0, h->stream, h->P);
    HIPCHK(hipGetLastError());
    // (anything later on the handle's stream, from any entry of the API, is ordered behind the side work too)
    if (forked) HIPCHK(h->side.join(h->stream));
    return 0;
  }
};

// The timing brackets of nlps_gpu_set_timing behind a step: ms[0 .. 7] of nlps_gpu_get_timing.  (Synchronises.)
static int step_timing_read(nlps_gpu* h, bool loads) {
  HIPCHK(hipEventRecord(h->ev[6], h->stream));
  // calibration bracket: a kernel of K3's grid and argument block that does nothing; what it reads is the part of
  // a one-kernel bracket that is not kernel time (records, dispatch, launch of the empty grid)
  k3_go(h, k_null_bracket, BLK, tile_view(h, 0), no_rates);
  HIPCHK(hipEventRecord(h->ev[7], h->stream));
  HIPCHK(hipEventSynchronize(h->ev[7]));
  float t[7];  // t[q]: from ev[q] to ev[q + 1]
  for (int q = 0; q < 7; q++) HIPCHK(hipEventElapsedTime(&t[q], h->ev[q], h->ev[q + 1]));
  h->ms[0] = t[0];  // search
  h->ms[1] = t[1];  // lists + K2
  h->ms[2] = t[3];  // K3
  h->ms[3] = t[5];  // K5
  h->ms[4] = t[2] + t[4];  // the nodal kernels
  h->ms[5] = t[6];  // the calibration bracket
  h->ms[7] = 0.f;  // the contour-traction kernel (nlps_gpu_set_explicit_loads)
  if (loads) HIPCHK(hipEventElapsedTime(&h->ms[7], h->loads_ev[0], h->loads_ev[1]));
  h->ms[6] = 0.f;  // time the handle's stream spent in / waiting for the ghost-layer exchanges of this step
  for (int q = 0; q < h->nwait; q++) {
    float tw = 0.f;
    HIPCHK(hipEventElapsedTime(&tw, h->evw[2 * q], h->evw[2 * q + 1]));
    h->ms[6] += tw;
  }
  return 0;
}

extern "C" int nlps_gpu_explicit_step(nlps_gpu* h, const nlps_bcc* bcc, int nbcc, int step, double dt, double gamma_nm,
                                      const double* gravity) {
  tan_stale(h, "nlps_gpu_explicit_step");
  const int ND = h->nd;
  if (explicit_step_refuse(h, nbcc, step)) return 1;
  if ((h->law_present & (1 << NLPS_KLAW_FLUID)) && !(dt > 0.0)) {  // (the rate of such a step is dU / dt: nlps_gpu_set_explicit_fluid)
    h->err = "nlps_gpu_explicit_step: the cloud holds the Newtonian-Fluid-Compressible law, whose rate is the increment over dt: dt must be positive";
    return 1;
  }
  if (ensure_bcs(h, bcc, nbcc)) return 1;
  if (!h->Pd_alt && h->resort_every > 0 && h->P.np > 0) {
    // the twin block of the periodic re-sort, at the first step of the fused scheme rather than inside the first
    // re-sort: a hipMalloc of this size (1.3 GB per million particles) takes milliseconds, the re-sort itself 0.3
    HIPCHK(h->Pd_alt.reserve((size_t)NFD * h->P.npad));
    HIPCHK(hipMemsetAsync(h->Pd_alt, 0, (size_t)NFD * h->P.npad * sizeof(double), h->stream));
  }
  if (!h->rolled && h->P.np > 0) {  // entering the fused scheme: rho J of every particle (see F_RHOJ)
    hipLaunchKernelGGL(k_init_rhoj, dim3(nblk(h->P.np)), dim3(BLK), 0, h->stream, h->P);
    HIPCHK(hipGetLastError());
  }
  // the periodic re-sort (resort_due).  This step's cost estimate first: the count of particles outside their tiles at a
  // recent step sits in the pinned word (no synchronisation: it may be a step old), its share of the cloud is the estimate
  if (h->adaptive_resort > 0.0 && !h->deterministic && h->resort_every > 0 && h->P.np > 0)
    h->debt += (double)*(volatile int*)h->foreign_h.host() / (double)h->P.np;
  if (resort_due(h) && resort(h, nullptr, true)) return 1;
  h->steps_since_sort++;
  h->nwait = 0;
  if (h->timing) HIPCHK(hipEventRecord(h->ev[0], h->stream));

  ExplicitStep s{h, bcc, nbcc, step, dt, gamma_nm, step_form(h, bcc, nbcc, step)};
  const StepForm& f = s.f;
  // A move the last step left pending is applied by K2 of this step where the step goes from here straight to its one K2
  // launch: the async form, on lists from the search done ahead -- nothing in front of that K2 reads x or dis (a re-sort
  // above has materialised it).  Every other form has it applied now; so has a step with contour loads, whose traction
  // kernel reads x of every contour particle between K2 and the search, one left out of the lists included.
  if (!(f.async_form && h->ahead && !f.loads) && materialise_move(h)) return 1;
  gravity3(gravity, ND, s.gv);
  if (f.det && !h->slab_d) {
    const size_t NWs = ND == 3 ? TileCfg<3>::NWA : TileCfg<2>::NWA;
    const size_t per_tile = std::max<size_t>((size_t)(1 + ND), (size_t)4 * ND) * NWs;  // K2: one slab; K3: one per law
    HIPCHK(h->slab_d.reserve((size_t)h->ntiles * per_tile));
  }
  if (f.lazy) {
    s.ln.fs.bc = f.bs;
    s.ln.fs.bcmask = f.bm;
    for (int a = 0; a < 3; a++) s.ln.fs.gv[a] = s.gv[a];
    s.ln.n0 = h->n0;
    s.ln.nwn = h->nwn;
    s.ln.node_cnt = node_lists(h) ? h->node_cnt_d.get() : nullptr;
    s.ln.ntw = h->ntw;  // (ln.tile_count: behind search_and_lists, which swaps the two counter arrays)
  }
  s.ks.rank1 = h->rank1_d;
  s.ks.bin = 1;
  if (f.dmg && beps_snapshot(h)) return 1;  // (eigenerosion, first step: before the search moves any closest node)
  h->nodal_stale = false;
  // S1 + S2 (ev[1] is recorded between the search and the lists/Newton/P2G kernel; the nodal accumulators of
  // the node window are reset by k_step_clear inside search_and_lists)
  if (search_and_lists(h, false, true, dt, gamma_nm, f.ov2 ? 2 : (f.ov ? 1 : 0))) return 1;
  if (h->timing) HIPCHK(hipEventRecord(h->ev[2], h->stream));
  if (f.lazy) {  // (what nlps_gpu_explicit_nodal needs to make the nodal arrays of this step later)
    s.ln.tile_count = h->tile_count2_d + h->tile0;
    h->nodal_stale = true;
    h->last_bc = s.ln.fs.bc;
    h->last_bm = s.ln.fs.bcmask;
    for (int a = 0; a < 3; a++) h->last_gv[a] = s.gv[a];
  }
  // S3 + S4 (K3 between the nodal dU and the forces), S5 (nodal acceleration, K5)
  if (f.ov2 ? s.run_overlap2() : f.ov ? s.run_overlap1() : s.run_one_pass()) return 1;

  h->P.flip ^= 1;  // F_n <- F_n+1, b_e,n <- b_e,n+1 by renaming
  h->rolled = true;
  h->rolled_keep = f.dmg || f.fbar;  // (tau and W of this step are stored: k_copy_n_to_n1 must not re-make them)
  h->rolled_rate = (h->law_present & (1 << NLPS_KLAW_FLUID)) != 0;  // (K3 wrote the step's rate into dt_F_n: k_roll_rate)
  h->searched = f.ride;    // K5 has updated the closest nodes for the positions it wrote ...
  h->ahead = f.ride;       // ... and binned the particles for the next step
  h->lists_ready = s.forked;
  if (h->timing && step_timing_read(h, f.loads)) return 1;
  // the step record: behind the last particle kernel of the step (and the join of the side stream), outside the timing brackets; N.active, N.nm and
  // N.force of this step are intact in every form (placement table), nothing here writes them
  if (h->rec.on && rec_step(h, NLPS_REC_KIND_EXPLICIT, step, dt, bcc, nbcc)) return 1;
  return 0;
}

extern "C" int nlps_gpu_num_active(nlps_gpu* h, int* nactive) {
  if (compute_node_mask(h)) return 1;
  HIPCHK(hipMemcpyAsync(&h->nactive, h->total_d, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  *nactive = h->nactive;
  return 0;
}

extern "C" int nlps_gpu_explicit_nodal(nlps_gpu* h, double* mass, double* dU, double* force, double* accel,
                                       double* reaction) {
  int ND = h->nd;
  if (materialise_nodal(h)) return 1;
  if (compute_node_mask(h)) return 1;
  HIPCHK(hipMemcpyAsync(&h->nactive, h->total_d, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (mass && from_grid(h, mass, h->N.nm, ND, 1 + ND, 0, 1, 0, nullptr)) return 1;
  if (dU && from_grid(h, dU, h->N.dU, ND, ND, 0, 0, 0, nullptr)) return 1;
  if (force && from_grid(h, force, h->N.force, ND, ND, 0, 0, 0, nullptr)) return 1;
  if (accel && from_grid(h, accel, h->N.accel, ND, ND, 0, 0, 0, nullptr)) return 1;
  if (reaction && from_grid(h, reaction, h->N.reaction, ND, ND, 0, 0, 0, nullptr)) return 1;
  return check_status(h, ST_NEWTON | ST_CONNECT | ST_JACOBIAN | ST_CONSTITUTIVE | ST_HALO, "nlps_gpu_explicit_step()");
}

// ------------------------------------------------------------------------------------------------
// a21: the per-dof vector updates of the implicit driver (masked numbering, N_A*d doubles)
// ------------------------------------------------------------------------------------------------
__global__ void k_vec_initial_guess(int n, double* __restrict__ dU, const double* __restrict__ v, const double* __restrict__ a,
                                    double dt, int trial) {  // __form_initial_guess, U-Newmark-beta.c:893-901
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && trial) dU[i] = dt * v[i] + 0.5 * dsqr(dt) * a[i];
}
__global__ void k_vec_guess_bc(const int* __restrict__ nodes, int n, int nd, int dim, int dirbits, double v0, double v1,
                               double v2, const int* __restrict__ n2m, double* __restrict__ dU) {  // :909-950
  int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const int m = n2m[nodes[q]];
  if (m == -1) return;
  const double v[3] = {v0, v1, v2};
  for (int k = 0; k < nd; k++)
    if (k < dim && ((dirbits >> k) & 1)) dU[m * nd + k] = v[k];
}
__global__ void k_vec_increments(int n, double* __restrict__ dV, double* __restrict__ dA, const double* __restrict__ dU,
                                 const double* __restrict__ v, const double* __restrict__ a, double a1, double a2,
                                 double a3, double a4, double a5, double a6) {  // :1834-1906
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (dV) dV[i] = a4 * dU[i] + (a5 - 1) * v[i] + a6 * a[i];
  if (dA) dA[i] = a1 * dU[i] - a2 * v[i] - (a3 + 1) * a[i];
}
__global__ void k_vec_inertial(int n, int nd, double* __restrict__ R, const double* __restrict__ M,
                               const double* __restrict__ dU, const double* __restrict__ v, const double* __restrict__ a,
                               const int* __restrict__ d2m, double a1, double a2, double a3, double b0, double b1,
                               double b2) {  // __nodal_inertial_forces, :1519-1557
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || d2m[i] == -1) return;
  const double b[3] = {b0, b1, b2};
  R[i] += M[i] * (a1 * dU[i] - a2 * v[i] - a3 * a[i] - b[i % nd]);
}

// host or device vectors of the caller: inputs are staged into a scratch pool when they live on the host,
// outputs are written in place (device) or copied back (host)
struct VecIO {
  nlps_gpu* h;
  size_t n;
  int slot = 0;
  std::vector<std::pair<double*, double*>> back;  // (host destination, device source)
  const double* in(const double* p) {
    if (!p || is_device_ptr(p)) return p;
    double* d = h->vec_d + (size_t)(slot++) * n;
    (void)hipMemcpyAsync(d, p, n * sizeof(double), hipMemcpyHostToDevice, h->stream);
    return d;
  }
  double* out(double* p, bool load) {
    if (!p || is_device_ptr(p)) return p;
    double* d = h->vec_d + (size_t)(slot++) * n;
    if (load) (void)hipMemcpyAsync(d, p, n * sizeof(double), hipMemcpyHostToDevice, h->stream);
    back.push_back({p, d});
    return d;
  }
  int finish() {
    for (auto& b : back)
      if (hipMemcpyAsync(b.first, b.second, n * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess) return 1;
    if (hipGetLastError() != hipSuccess) return 1;
    if (!back.empty() && hipStreamSynchronize(h->stream) != hipSuccess) return 1;
    return 0;
  }
};
static int vec_begin(nlps_gpu* h, const char* who, VecIO& io) {
  if (need_masks(h, who)) return 1;
  io.h = h;
  io.n = (size_t)h->nactive * h->nd;
  return reserve(h, who, h->vec_d, io.n * 6, "the staging of host vectors");
}

extern "C" int nlps_gpu_form_initial_guess(nlps_gpu* h, double* dU, const double* Un_dt, const double* Un_dt2, double dt,
                                           int use_explicit_trial, const nlps_bcc* bcc, int nbcc, int step) {
  VecIO io;
  if (vec_begin(h, "nlps_gpu_form_initial_guess", io)) return 1;
  if (nbcc > 0 && check_step(h, step, "nlps_gpu_form_initial_guess")) return 1;
  if (ensure_bcs(h, bcc, nbcc)) return 1;
  const int n = (int)io.n, ND = h->nd;
  double* d = io.out(dU, true);
  const double *v = io.in(Un_dt), *a = io.in(Un_dt2);
  if (n > 0) hipLaunchKernelGGL(k_vec_initial_guess, dim3(nblk(n)), dim3(BLK), 0, h->stream, n, d, v, a, dt, use_explicit_trial);
  for (int i = 0; i < nbcc; i++) {
    if (h->bcs[i].n == 0) continue;
    double val[3];
    bc_values(bcc[i], step, h->nsteps, val);
    hipLaunchKernelGGL(k_vec_guess_bc, dim3(nblk(h->bcs[i].n)), dim3(BLK), 0, h->stream, h->bcs[i].dnodes, h->bcs[i].n, ND,
                       bcc[i].dim, dirbits_of(bcc[i], step, h->nsteps), val[0], val[1], val[2], h->n2m_d, d);
  }
  if (io.finish()) {
    h->err = "nlps_gpu_form_initial_guess: HIP error";
    return 1;
  }
  return 0;
}

extern "C" int nlps_gpu_nodal_kinetic_increments(nlps_gpu* h, double* dU_dt, double* dU_dt2, const double* dU,
                                                 const double* Un_dt, const double* Un_dt2, const double* alpha) {
  VecIO io;
  if (vec_begin(h, "nlps_gpu_nodal_kinetic_increments", io)) return 1;
  const int n = (int)io.n;
  double *dV = io.out(dU_dt, false), *dA = io.out(dU_dt2, false);
  const double *u = io.in(dU), *v = io.in(Un_dt), *a = io.in(Un_dt2);
  if (n > 0)
    hipLaunchKernelGGL(k_vec_increments, dim3(nblk(n)), dim3(BLK), 0, h->stream, n, dV, dA, u, v, a, alpha[0], alpha[1], alpha[2],
                       alpha[3], alpha[4], alpha[5]);
  if (io.finish()) {
    h->err = "nlps_gpu_nodal_kinetic_increments: HIP error";
    return 1;
  }
  return 0;
}

extern "C" int nlps_gpu_nodal_inertial_forces(nlps_gpu* h, double* R, const double* M, const double* dU,
                                              const double* Un_dt, const double* Un_dt2, const double* alpha,
                                              const double* gravity) {
  VecIO io;
  if (vec_begin(h, "nlps_gpu_nodal_inertial_forces", io)) return 1;
  const int n = (int)io.n, ND = h->nd;
  double* r = io.out(R, true);
  const double *m = io.in(M), *u = io.in(dU), *v = io.in(Un_dt), *a = io.in(Un_dt2);
  double b[3];
  gravity3(gravity, ND, b);
  if (n > 0)
    hipLaunchKernelGGL(k_vec_inertial, dim3(nblk(n)), dim3(BLK), 0, h->stream, n, ND, r, m, u, v, a, h->d2m_d, alpha[0], alpha[1],
                       alpha[2], b[0], b[1], b[2]);
  if (io.finish()) {
    h->err = "nlps_gpu_nodal_inertial_forces: HIP error";
    return 1;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------
// __lagrangian_evaluation (U-Newmark-beta.c:970-1058): the residual of the maintained driver's SNES solve, evaluated at
// every Newton iterate and line-search trial, as one device call
// ------------------------------------------------------------------------------------------------
// Closing nodal kernel: L = f_int (+ traction) + M (alpha_1 dU - alpha_2 v - alpha_3 a - b) on the free dofs, 0 on the
// Dirichlet ones (VecZeroEntries :1003, then the three += of :1028-1036 in that order: __nodal_internal_forces skips the
// Dirichlet dofs at :1359, __nodal_inertial_forces at :1550, k_traction's sums are taken for the free dofs only like
// :1489).  force / trac: grid numbering [nnodes][ND]; everything else masked.
template <int ND>
__global__ void k_lagrangian_nodal(int nnodes, const int* __restrict__ n2m, const int* __restrict__ d2m,
                                   const double* __restrict__ force, const double* __restrict__ trac, double* __restrict__ R,
                                   const double* __restrict__ M, const double* __restrict__ dU, const double* __restrict__ v,
                                   const double* __restrict__ a, double a1, double a2, double a3, double b0, double b1,
                                   double b2, const int* __restrict__ gstatus, int* __restrict__ status_out) {
  const int A = blockIdx.x * blockDim.x + threadIdx.x;
  // the failure flags of the stress update, left where the host reads them after its one synchronise (check_status,
  // mirrored): every kernel that can set them has finished before this one starts
  if (A == 0 && status_out) *status_out = *gstatus;
  if (A >= nnodes) return;
  const int m = n2m[A];
  if (m < 0) return;
  const double b[3] = {b0, b1, b2};
#pragma unroll
  for (int f = 0; f < ND; f++) {
    const size_t i = (size_t)m * ND + f;
    double r = 0.0;
    if (d2m[i] != -1) {
      r += force[(size_t)A * ND + f];
      if (trac) r += trac[(size_t)A * ND + f];
      r += M[i] * (a1 * dU[i] - a2 * v[i] - a3 * a[i] - b[f]);
    }
    R[i] = r;
  }
}

static int snes_fnorm_launch(nlps_gpu* h, const double* F);  // (defined with nlps_gpu_newton_solve)

// The fused damage residual (nlps_gpu_set_implicit_damage) between k_expand_reset and the closing nodal
// kernel: the state half of MODE 3 (k3_tile<., ., 6>: DF, F_n1, J_n1, tau, W, the n+1 internal variables, C_ep; failed
// particles skipped), the node runs of the current closest nodes -- built once per numbering: nothing between two calls
// that make the matrix-free operator stale (tan_stale) changes a closest node --, the hook, which sets Damage_n1
// (Strain_f_n1) and scales every Kirchhoff stress in place, and the force half with the Lagrangian's sign.  All on the
// handle's stream, no sort, no synchronisation, no allocation (the setter made the tables).  The level-B stages keep
// tables of their own (dmg.b_*, the sort buffers): nothing here touches them.
static int lagrangian_damage_launches(nlps_gpu* h) {
  if (beps_snapshot(h)) return 1;  // (taken by the first search: nothing to do here for a handle that has searched)
  // deterministic mode with nlps_gpu_set_deterministic_damage: the exact lists, sorted runs, the one-wave force half and
  // the fixed-order sum of its slabs; the atomic flush otherwise.  (The lists are made exact in front of the state half
  // already; scatter_tiles below then finds nothing left to prepare.)
  const bool det = det_implicit(h);
  if (det && det_prepare(h, "nlps_gpu_lagrangian_evaluation")) return 1;
  TileD td = tile_view(h);
  if (!det) td.slab = nullptr;
  launch_k3<6>(h, td, K3Launch{});  // (a cloud of several laws: per law present, FILT)
  // (built once per numbering: nothing between two calls that make the matrix-free operator stale changes a closest node)
  if (damage_runs_and_hook(h, h->dmg.gen != h->tan_gen)) return 1;
  h->dmg.gen = h->tan_gen;
  h->dmg.fused_evals++;
  if (scatter_tiles<2, 3>(h, "nlps_gpu_lagrangian_evaluation", 1, h->N.force, [&](auto NT, TileD) {  // (on this site's td)
        if (CT(NT) == 64) LAUNCH_ND_BLK((k3f_wave<2, true>), (k3f_wave<3, true>), h->ntw, 64, h->P, h->g, h->N, td, h->gstatus_d);
        else LAUNCH_ND_BLK((k3f_tile<2, true>), (k3f_tile<3, true>), h->ntw, K3_BLK, h->P, h->g, h->N, td, h->gstatus_d);
      }))
    return 1;
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int nlps_gpu_lagrangian_evaluation(nlps_gpu* h, double* R, const double* dU, const double* Un_dt,
                                              const double* Un_dt2, const double* M, const double* alpha,
                                              const double* gravity, const nlps_bcc* loads, int nloads, int step,
                                              double thickness, const double* area0, int flags) {
  if (fbar_refuse(h, "nlps_gpu_lagrangian_evaluation")) return 1;
  if (need_masks(h, "nlps_gpu_lagrangian_evaluation")) return 1;
  if (materialise_move(h)) return 1;
  if (!R || !dU || !Un_dt || !Un_dt2 || !M || !alpha) {
    h->err = "nlps_gpu_lagrangian_evaluation: R, dU, Un_dt, Un_dt2, M and alpha are required";
    return 1;
  }
  const int ND = h->nd;
  const size_t n = (size_t)h->nactive * ND;
  // The composition of the separate stage calls, in the order of :1018-1036 -- on request (NLPS_LAGR_SEPARATE: the form
  // the fused one is measured and tested against), for what the fused kernel does not carry (rate tensors, which only the
  // Newtonian-fluid law reads; the damage hooks, which sit between the stress update and the force scatter and need
  // every particle's stress before any force)
  // (a cloud that holds the fluid law always carries the rates: fused in MODE 4, or through the separate stages)
  const bool fluid = (h->law_present & (1 << NLPS_KLAW_FLUID)) != 0;
  // (a damage cloud takes the fused damage form with nlps_gpu_set_implicit_damage on, the separate stages otherwise)
  const bool dmg = h->P.erosion && h->implicit_damage && !(flags & (NLPS_LAGR_SEPARATE | NLPS_LAGR_RATES)) && h->P.np > 0;
  if (dmg && (h->halo || h->rccl)) {
    h->err = std::string("nlps_gpu_lagrangian_evaluation: ") + implicit_damage_halo_msg;
    return 1;
  }
  const bool fused = !(flags & NLPS_LAGR_SEPARATE) && (fluid || !(flags & NLPS_LAGR_RATES)) && (!h->P.erosion || dmg) &&
                     h->uniform_law <= NLPS_KLAW_FLUID && h->P.np > 0;
  if (!fused) {
    DevBuf<double> dV;
    if ((flags & NLPS_LAGR_RATES) || fluid) {  // __compute_nodal_velocity_increments, :1018
      HIPCHK(dV.reserve(std::max<size_t>(n, 1)));
      if (nlps_gpu_nodal_kinetic_increments(h, dV, nullptr, dU, Un_dt, Un_dt2, alpha)) return 1;
    }
    int st = nlps_gpu_compatibility(h, dU, dV);
    if (dV) {
      (void)hipStreamSynchronize(h->stream);
      dV.reset();
    }
    if (st) return 1;
    if (nlps_gpu_constitutive(h)) return 1;
    if (is_device_ptr(R)) HIPCHK(hipMemsetAsync(R, 0, n * sizeof(double), h->stream));
    else memset(R, 0, n * sizeof(double));
    if (nlps_gpu_internal_forces(h, R)) return 1;
    if (nloads > 0 && nlps_gpu_nodal_traction_forces(h, R, loads, nloads, step, thickness, area0)) return 1;
    return nlps_gpu_nodal_inertial_forces(h, R, M, dU, Un_dt, Un_dt2, alpha, gravity);
  }
  if (materialise_roll(h)) return 1;
  if (materialise_nodal(h)) return 1;  // (the forces of the last explicit step are about to go)
  h->level_b_fields = true;            // C_ep holds data from here on
  VecIO io;
  if (vec_begin(h, "nlps_gpu_lagrangian_evaluation", io)) return 1;
  if (h->timing) HIPCHK(hipEventRecord(h->ev[0], h->stream));  // slots of nlps_gpu_get_timing: [0] staging, [2] the kernel, [4] nodal + copy back
  double* r = io.out(R, false);
  const double* u = io.in(dU);
  const double* cst[3] = {Un_dt, Un_dt2, M};  // constant over the evaluations of one SNES solve
  if (!is_device_ptr(Un_dt) || !is_device_ptr(Un_dt2) || !is_device_ptr(M)) {
    if (h->lagr_d.size() < 3 * n) {
      h->lagr_valid = false;
      if (reserve(h, "nlps_gpu_lagrangian_evaluation", h->lagr_d, 3 * n, "the constant vectors of the step")) return 1;
    }
    if ((flags & NLPS_LAGR_SAME_STEP) && !h->lagr_valid) {
      h->err = "nlps_gpu_lagrangian_evaluation: NLPS_LAGR_SAME_STEP without an earlier evaluation since nlps_gpu_active_masks";
      return 1;
    }
    for (int q = 0; q < 3; q++) {
      if (is_device_ptr(cst[q])) continue;
      double* d = h->lagr_d + (size_t)q * n;
      if (!(flags & NLPS_LAGR_SAME_STEP)) HIPCHK(hipMemcpyAsync(d, cst[q], n * sizeof(double), hipMemcpyHostToDevice, h->stream));
      cst[q] = d;
    }
    h->lagr_valid = true;
  }
  const double *v = cst[0], *a = cst[1], *m = cst[2];
  // the caller's dU in grid numbering (the gather windows read N.dU), the force accumulator of the node window reset
  if (fluid)
    hipLaunchKernelGGL(k_expand_reset_rates, dim3(nblk(h->g.nnodes)), dim3(BLK), 0, h->stream, h->N.dU, h->gridB.get(), u, v, a,
                       alpha[3], alpha[4] - 1.0, alpha[5], h->n2m_d, h->g.nnodes, ND, h->N.force, h->n0, h->nwn);
  else
    hipLaunchKernelGGL(k_expand_reset, dim3(nblk(h->g.nnodes)), dim3(BLK), 0, h->stream, h->N.dU, u, h->n2m_d, h->g.nnodes, ND,
                       h->N.force, h->n0, h->nwn);
  if (h->timing) HIPCHK(hipEventRecord(h->ev[2], h->stream));
  if (dmg) {  // (before the deterministic form below, which does not hold the hook: it has a deterministic form of its own)
    if (lagrangian_damage_launches(h)) return 1;
  } else {
    // MODE 3, the fluid's particles in the rate-carrying MODE 4 (dV = gridB, k_expand_reset_rates).  Deterministic mode:
    // one wave per tile and per law present over the exact lists (ordered compaction), one slab per (tile, law) -- a
    // tile without a particle of the law writes zeros --, then the fixed-order sum into N.force.  Otherwise the atomic
    // flush, without a slab pointer: one launch, or one per law present (FILT) for a cloud of several laws.
    const int nlaws = __builtin_popcount(h->law_present);
    if (scatter_tiles<2, 3>(h, "nlps_gpu_lagrangian_evaluation", nlaws, h->N.force, [&](auto NT, TileD td) {
          const bool wave = CT(NT) == 64;
          if (!wave) td.slab = nullptr;
          launch_k3<3>(h, td, K3Launch{false, wave, h->gridB.get()});
        }))
      return 1;
  }
  HIPCHK(hipGetLastError());
  if (h->timing) HIPCHK(hipEventRecord(h->ev[3], h->stream));
  if (halo(h, h->N.force, ND, 8, 0)) return 1;
  int any = 0;
  if (nloads > 0 && traction_to_grid(h, "nlps_gpu_lagrangian_evaluation", h->gridA, loads, nloads, step, thickness, area0, &any))
    return 1;
  double b[3];
  gravity3(gravity, ND, b);
  LAUNCH_ND((k_lagrangian_nodal<2>), (k_lagrangian_nodal<3>), nblk(h->g.nnodes), h->g.nnodes, (const int*)h->n2m_d,
            (const int*)h->d2m_d, (const double*)h->N.force, any ? (const double*)h->gridA : (const double*)nullptr, r, m, u, v,
            a, alpha[0], alpha[1], alpha[2], b[0], b[1], b[2], (const int*)h->gstatus_d, h->status_h.alias());
  HIPCHK(hipGetLastError());
  if (h->snes_tail && snes_fnorm_launch(h, r)) return 1;  // (nlps_gpu_newton_solve: ||R||^2 arrives with the wait below)
  if (io.finish()) {
    h->err = "nlps_gpu_lagrangian_evaluation: HIP error";
    return 1;
  }
  if (h->timing) HIPCHK(hipEventRecord(h->ev[6], h->stream));
  if (check_status(h, ST_CONSTITUTIVE, "Stress_integration__Constitutive__()", h->status_h.alias() != nullptr)) return 1;  // (synchronises)
  if (h->timing) {
    for (int q = 0; q < 8; q++) h->ms[q] = 0.f;
    HIPCHK(hipEventElapsedTime(&h->ms[0], h->ev[0], h->ev[2]));
    HIPCHK(hipEventElapsedTime(&h->ms[2], h->ev[2], h->ev[3]));
    HIPCHK(hipEventElapsedTime(&h->ms[4], h->ev[3], h->ev[6]));
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------
// tangent assembly
// ------------------------------------------------------------------------------------------------
extern "C" int nlps_gpu_tangent_assemble(nlps_gpu* h, long long* nnz) {
  if (fbar_refuse(h, "nlps_gpu_tangent_assemble")) return 1;
  if (need_masks(h, "nlps_gpu_tangent_assemble")) return 1;
  if (materialise_roll(h)) return 1;
  const int ND = h->nd, S = ND == 3 ? TanCfg<3>::S : TanCfg<2>::S;
  const size_t nn = (size_t)h->g.nnodes, nblk_st = nn * S;
  if (!h->kst_d) {
    HIPCHK(h->kst_d.reserve(nblk_st * ND * ND));
    HIPCHK(h->ktouched_d.reserve(nblk_st));
    HIPCHK(h->kcnt_d.reserve(nn + 1));
    HIPCHK(h->koffs_d.reserve(nn + 1));
    HIPCHK(h->khead_d.reserve(h->P.npad));
    HIPCHK(h->kng_d.reserve(1));
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, h->kscan_bytes, h->kcnt_d.get(), h->koffs_d.get(), (int)nn + 1, h->stream));
    HIPCHK(h->kscan_tmp.reserve(h->kscan_bytes + 16));
  }
  HIPCHK(hipMemsetAsync(h->kst_d, 0, nblk_st * ND * ND * sizeof(double), h->stream));
  HIPCHK(hipMemsetAsync(h->ktouched_d, 0, nblk_st, h->stream));
  HIPCHK(hipMemsetAsync(h->kcnt_d, 0, (nn + 1) * sizeof(int), h->stream));
  const int np = h->P.np;
  h->ktan_sym = false;
  if (np > 0 && h->tangent_grouped) {
    // particles grouped by closest node (radix sort of (I0, p) in the re-sort buffers), one workgroup per node
    hipLaunchKernelGGL(k_tangent_keys, dim3(nblk(np)), dim3(BLK), 0, h->stream, h->P, h->skey_d, h->sval_d);
    size_t bytes = h->cub_tmp_bytes;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(h->cub_tmp.get(), bytes, h->skey_d.get(), h->skey2_d.get(), h->sval_d.get(), h->sval2_d.get(), np, 0, 32,
                                              h->stream));
    HIPCHK(hipMemsetAsync(h->kng_d, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(k_tangent_groups, dim3(nblk(np)), dim3(BLK), 0, h->stream, np, h->skey2_d, h->khead_d, h->kng_d);
    const int ngrid = std::min(np, h->g.nnodes);  // upper bound of the number of groups; surplus workgroups exit
    // a cloud of Neo-Hookean particles only: the upper half of every row, the rest by symmetry in nlps_gpu_tangent_coo
    h->ktan_sym = h->tangent_symmetric && h->uniform_law == NLPS_MAT_NEO_HOOKEAN;
    LAUNCH_ND_BLK(k_tangent_nh_grouped<2>, k_tangent_nh_grouped<3>, ngrid, TAN_NT, h->P, h->g, h->mats_d, np, h->skey2_d, h->sval2_d,
                  h->khead_d, h->kng_d, h->kst_d, h->ktouched_d, h->gstatus_d, h->ktan_sym ? 1 : 0, h->tan_alpha4);
  } else if (np > 0) {
    h->ktan_sym = false;
    LAUNCH_ND_BLK(k_tangent_nh<2>, k_tangent_nh<3>, np, 64, h->P, h->g, h->mats_d, h->kst_d, h->ktouched_d, h->gstatus_d);
  }
  LAUNCH_ND((k_tangent_count<2>), (k_tangent_count<3>), ((int)nn + 3) / 4, (int)nn, h->ktouched_d, h->kcnt_d);  // (one wave per row node)
  HIPCHK(hipGetLastError());
  size_t bytes = h->kscan_bytes;
  HIPCHK(hipcub::DeviceScan::ExclusiveSum(h->kscan_tmp.get(), bytes, h->kcnt_d.get(), h->koffs_d.get(), (int)nn + 1, h->stream));
  int total = 0;
  HIPCHK(hipMemcpyAsync(&total, h->koffs_d + nn, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (check_status(h, ST_NEWTON | ST_CONSTITUTIVE, "nlps_gpu_tangent_assemble() (Neo-Hookean particles only)")) return 1;
  h->knnz_blocks = total;
  if (nnz) *nnz = (long long)total * ND * ND;
  return 0;
}

extern "C" int nlps_gpu_set_tangent_alpha4(nlps_gpu* h, double alpha_4) {
  h->tan_alpha4 = alpha_4;
  return 0;
}

extern "C" int nlps_gpu_tangent_set_grouped(nlps_gpu* h, int grouped) {
  h->tangent_grouped = grouped != 0;
  return 0;
}

extern "C" int nlps_gpu_tangent_coo(nlps_gpu* h, double alpha_1, const double* lumped_mass, int apply_dirichlet,
                                    int* rows, int* cols, double* vals) {
  if (h->knnz_blocks < 0) {
    h->err = "nlps_gpu_tangent_coo: call nlps_gpu_tangent_assemble() first";
    return 1;
  }
  if (need_masks(h, "nlps_gpu_tangent_coo")) return 1;
  if (materialise_move(h)) return 1;
  const int ND = h->nd, nn = h->g.nnodes;
  const size_t ne = (size_t)h->knnz_blocks * ND * ND;
  if (ne == 0) return 0;
  const double* mass_d = nullptr;
  if (lumped_mass) {
    if (reserve(h, "nlps_gpu_tangent_coo", h->maskedA, (size_t)h->nactive * ND, "the mass term")) return 1;
    HIPCHK(hipMemcpyAsync(h->maskedA, lumped_mass, (size_t)h->nactive * ND * sizeof(double), hipMemcpyDefault, h->stream));
    mass_d = h->maskedA;
  }
  if (is_device_ptr(rows) && is_device_ptr(cols) && is_device_ptr(vals)) {  // (MatSetValuesCOO of a GPU matrix type: no staging)
    LAUNCH_ND((k_tangent_emit<2>), (k_tangent_emit<3>), (nn + 3) / 4, nn, h->g, h->ktouched_d, h->kst_d, h->koffs_d, h->n2m_d,
              apply_dirichlet ? h->d2m_d : (const int*)nullptr, alpha_1, mass_d, rows, cols, vals, h->ktan_sym ? 1 : 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
  }
  DevBuf<int> rows_d, cols_d;
  DevBuf<double> vals_d;
  HIPCHK(rows_d.reserve(ne));
  HIPCHK(cols_d.reserve(ne));
  HIPCHK(vals_d.reserve(ne));
  LAUNCH_ND((k_tangent_emit<2>), (k_tangent_emit<3>), (nn + 3) / 4, nn, h->g, h->ktouched_d, h->kst_d, h->koffs_d, h->n2m_d,
            apply_dirichlet ? h->d2m_d : (const int*)nullptr, alpha_1, mass_d, rows_d.get(), cols_d.get(), vals_d.get(), h->ktan_sym ? 1 : 0);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(rows, rows_d, ne * sizeof(int), hipMemcpyDefault, h->stream));
  HIPCHK(hipMemcpyAsync(cols, cols_d, ne * sizeof(int), hipMemcpyDefault, h->stream));
  HIPCHK(hipMemcpyAsync(vals, vals_d, ne * sizeof(double), hipMemcpyDefault, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));  // (the copies land in the caller's memory before the blocks go)
  return 0;
}

extern "C" int nlps_gpu_sparsity_pattern(nlps_gpu* h, int* nnz_per_row) {
  if (h->knnz_blocks < 0) {
    h->err = "nlps_gpu_sparsity_pattern: call nlps_gpu_tangent_assemble() first";
    return 1;
  }
  if (need_masks(h, "nlps_gpu_sparsity_pattern")) return 1;
  if (materialise_move(h)) return 1;
  const int ND = h->nd, nn = h->g.nnodes;
  DevBuf<int> pat_d;
  HIPCHK(pat_d.reserve((size_t)h->nactive * ND + 4));
  LAUNCH_ND((k_tangent_pattern<2>), (k_tangent_pattern<3>), nblk(nn), nn, h->kcnt_d, h->n2m_d, pat_d.get());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(nnz_per_row, pat_d, (size_t)h->nactive * ND * sizeof(int), hipMemcpyDefault, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}


// ------------------------------------------------------------------------------------------------
// matrix-free tangent (nlps_tangent_operator.hpp): MatShell MATOP_MULT / MATOP_GET_DIAGONAL
// ------------------------------------------------------------------------------------------------
static int tanop_valid(nlps_gpu* h, const char* who) {
  if (h->top_gen == 0) {
    h->err = std::string(who) + ": call nlps_gpu_tangent_operator() first";
    return 1;
  }
  if (h->top_gen != h->tan_gen) {
    h->err = std::string(who) + ": the operator is stale: " + h->tan_why +
             " moved, reordered or re-listed the particles after nlps_gpu_tangent_operator(); linearise again";
    return 1;
  }
  return need_masks(h, who);
}

extern "C" int nlps_gpu_tangent_operator(nlps_gpu* h, double alpha_1, const double* lumped_mass, int apply_dirichlet,
                                         size_t* bytes) {
  if (fbar_refuse(h, "nlps_gpu_tangent_operator")) return 1;
  if (need_masks(h, "nlps_gpu_tangent_operator")) return 1;
  if (materialise_roll(h)) return 1;
  h->top_gen = 0;  // (no operator until this call succeeds)
  const int ND = h->nd, E = ND * ND, np = h->P.np;
  const size_t nD = (size_t)E * E * std::max(np, 1), nm = (size_t)h->nactive * ND, ngr = (size_t)h->g.nnodes * E;
  const char* who = "nlps_gpu_tangent_operator";
  if (reserve(h, who, h->top_d, nD, ND == 3 ? "81 doubles per particle" : "16 doubles per particle")) return 1;
  if (reserve(h, who, h->top_m, std::max<size_t>(nm, 1), "the mass term")) return 1;
  if (reserve(h, who, h->top_g, ngr, "the grid scratch")) return 1;  // (the grid does not change size)
  h->top_np = np;
  h->top_dir = apply_dirichlet != 0;
  h->top_mass = lumped_mass != nullptr;
  if (lumped_mass && nm > 0) {
    HIPCHK(hipMemcpyAsync(h->top_m, lumped_mass, nm * sizeof(double), hipMemcpyDefault, h->stream));
    hipLaunchKernelGGL(k_tanop_scale, dim3(nblk((int)nm)), dim3(BLK), 0, h->stream, nm, alpha_1, h->top_m);
  }
  if (np > 0) {
    const int nb = (np + TANOP_SETUP_NT - 1) / TANOP_SETUP_NT;
    LAUNCH_ND_BLK(k_tanop_setup<2>, k_tanop_setup<3>, nb, TANOP_SETUP_NT, h->P, h->g, h->mats_d, h->top_d, np, h->gstatus_d,
                  h->tan_alpha4);
  }
  HIPCHK(hipGetLastError());
  if (check_status(h, ST_NEWTON | ST_CONSTITUTIVE, "nlps_gpu_tangent_operator()")) return 1;  // (synchronises)
  if (bytes) *bytes = (nD + nm + ngr) * sizeof(double);  // (the header's formula: what this linearisation needs)
  h->top_gen = h->tan_gen;
  h->top_serial++;  // (a new linearisation: the preconditioner of nlps_gpu_tangent_solve is rebuilt)
  return 0;
}

// y = K M^-1 v on device masked vectors.  pc == nullptr: y = K v, the product of nlps_gpu_tangent_apply.  Otherwise the
// solve's form: k_ksp_pc_expand folds z = M^-1 v (kind 0: z = v, not written) into the expansion and zeroes the
// accumulator, and the nodal epilogue reads z.
struct KspPc {
  int kind;
  const double* Minv;
  double* z;
};
static int tanop_product(nlps_gpu* h, const double* v, double* y, const KspPc* pc) {
  const int ND = h->nd, nn = h->g.nnodes;
  double *xg = h->top_g, *yg = h->top_g + (size_t)nn * ND;
  const int* d2m = h->top_dir ? (const int*)h->d2m_d : nullptr;
  const double* xin = v;
  if (pc) {
    LAUNCH_ND((k_ksp_pc_expand<2>), (k_ksp_pc_expand<3>), nblk(nn), nn, (const int*)h->n2m_d, d2m, pc->kind, pc->Minv, v,
              pc->z, xg, yg);
    if (pc->kind) xin = pc->z;
  } else {
    LAUNCH_ND((k_tanop_expand<2>), (k_tanop_expand<3>), nblk(nn), nn, (const int*)h->n2m_d, d2m, v, xg);
    HIPCHK(hipMemsetAsync(yg, 0, (size_t)nn * ND * sizeof(double), h->stream));
  }
  if (h->top_np > 0 && scatter_tiles<2, 3>(h, "nlps_gpu_tangent_apply", 1, yg, [&](auto NT, const TileD td) {
        LAUNCH_ND_BLK((k_tanop_apply<2, CT(NT)>), (k_tanop_apply<3, CT(NT)>), h->ntw, CT(NT), h->P, h->g, td,
                      (const double*)h->top_d, h->top_np, (const double*)xg, yg);
      }))
    return 1;
  HIPCHK(hipGetLastError());
  if (halo(h, yg, ND, 8, 0)) return 1;
  LAUNCH_ND((k_tanop_nodal<2>), (k_tanop_nodal<3>), nblk(nn), nn, (const int*)h->n2m_d, d2m, (const double*)yg, xin,
            h->top_mass ? (const double*)h->top_m : (const double*)nullptr, y);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int nlps_gpu_tangent_apply(nlps_gpu* h, const double* x, double* y) {
  if (tanop_valid(h, "nlps_gpu_tangent_apply")) return 1;
  if (!x || !y) {
    h->err = "nlps_gpu_tangent_apply: x and y are required";
    return 1;
  }
  VecIO io;
  if (vec_begin(h, "nlps_gpu_tangent_apply", io)) return 1;
  if (io.n == 0) return 0;
  const double* xd = io.in(x);
  double* yd = io.out(y, false);
  if (tanop_product(h, xd, yd, nullptr)) return 1;
  if (io.finish()) {
    h->err = "nlps_gpu_tangent_apply: HIP error";
    return 1;
  }
  if (io.back.empty()) HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// the N_A masked diagonal blocks into the device array out (stream order, no synchronisation); 0 or 1
static int tanop_bdiag(nlps_gpu* h, double* out) {
  const int ND = h->nd, E = ND * ND, nn = h->g.nnodes;
  int st = hipMemsetAsync(h->top_g, 0, (size_t)nn * E * sizeof(double), h->stream) != hipSuccess;
  if (!st && h->top_np > 0) {
    if (scatter_tiles<4, 9>(h, "nlps_gpu_tangent_block_diagonal", 1, h->top_g.get(), [&](auto NT, const TileD td) {
          LAUNCH_ND_BLK((k_tanop_bdiag<2, CT(NT)>), (k_tanop_bdiag<3, CT(NT)>), h->ntw, CT(NT), h->P, h->g, td,
                        (const double*)h->top_d, h->top_np, h->top_g.get());
        }))
      return 1;
    st = hipGetLastError() != hipSuccess;
  }
  if (!st) st = halo(h, h->top_g, E, 8, 0);
  if (!st) {
    LAUNCH_ND((k_tanop_bdiag_nodal<2>), (k_tanop_bdiag_nodal<3>), nblk(nn), nn, (const int*)h->n2m_d,
              h->top_dir ? (const int*)h->d2m_d : (const int*)nullptr, (const double*)h->top_g,
              h->top_mass ? (const double*)h->top_m : (const double*)nullptr, out);
    st = hipGetLastError() != hipSuccess;
  }
  return st;
}

extern "C" int nlps_gpu_tangent_block_diagonal(nlps_gpu* h, double* blocks) {
  if (tanop_valid(h, "nlps_gpu_tangent_block_diagonal")) return 1;
  if (!blocks) {
    h->err = "nlps_gpu_tangent_block_diagonal: blocks is required";
    return 1;
  }
  const int ND = h->nd, E = ND * ND;
  const size_t nb = (size_t)h->nactive * E;
  if (nb == 0) return 0;
  double* out = blocks;
  const bool host = !is_device_ptr(blocks);
  // staging of a host destination: kept on the handle (hipMalloc synchronises)
  if (host && reserve(h, "nlps_gpu_tangent_block_diagonal", h->top_b, nb, "the staging of the blocks")) return 1;
  if (host) out = h->top_b;
  int st = tanop_bdiag(h, out);
  if (!st && host) st = hipMemcpyAsync(blocks, out, nb * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess;
  if (hipStreamSynchronize(h->stream) != hipSuccess) st = 1;
  if (st && h->err.find("nlps_gpu_tangent_block_diagonal") == std::string::npos)
    h->err = "nlps_gpu_tangent_block_diagonal: HIP error (or halo exchange failure)";
  return st;
}

// ------------------------------------------------------------------------------------------------
// the tangent in CSR, assembled row by row without float atomics (nlps_tangent_csr.hpp)
// ------------------------------------------------------------------------------------------------
static size_t tancsr_bytes(int nd, size_t np, size_t nnodes, size_t nactive) {
  const size_t E = (size_t)nd * nd, mw = nd == 3 ? 12 : 2;
  return 8 * np * (E * E + 6 * (size_t)nd + 2) + 4 * (nnodes + 1) + 8 * mw * nnodes + 8 * (nactive + 1);
}

static int tancsr_one_rank(nlps_gpu* h, const char* who) {
  if (h->halo || h->rccl) {
    h->err = std::string(who) + ": the CSR assembly is built for one rank: not with a halo callback or an RCCL exchange "
             "attached (a row's owner would need the particles of the neighbouring rank that hold its node)";
    return 1;
  }
  return 0;
}

// off = the exclusive scan of the N_A + 1 counts cnt, *total = its last entry (synchronises).  The sort's workspace
// serves the scan; one of this call only where it is too small
static int tancsr_scan(nlps_gpu* h, const char* who, int* cnt, int* off, int* total) {
  const int n = h->nactive + 1;
  size_t bytes = 0;
  HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, cnt, off, n, h->stream));
  DevBuf<char> own;
  void* tmp = h->cub_tmp.get();
  if (bytes > h->cub_tmp_bytes) {
    if (reserve(h, who, own, bytes + 16, "the scan")) {
      (void)hipStreamSynchronize(h->stream);  // (a copy the caller queued into a variable of its own lands first)
      return 1;
    }
    tmp = own.get();
  }
  HIPCHK(hipcub::DeviceScan::ExclusiveSum(tmp, bytes, cnt, off, n, h->stream));
  HIPCHK(hipMemcpyAsync(total, off + n - 1, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// the row pointer and the indices of the arrays are int
static int tancsr_fits_int(nlps_gpu* h, const char* who, const char* what, long long n, const char* arrays) {
  if (n <= (long long)INT_MAX) return 0;
  char buf[200];
  snprintf(buf, sizeof buf, "%s: %s = %lld does not fit the int %s (INT_MAX = %d)", who, what, n, arrays, INT_MAX);
  h->err = buf;
  return 1;
}

// the records, runs, masks and block counts of the current linearisation, shared by the CSR and the block-CSR form:
// built by the first pattern call of either kind since the operator (they depend on the linearisation alone)
static int tancsr_records(nlps_gpu* h, const char* who) {
  if (h->csr_rec_serial != 0 && h->csr_rec_serial == h->top_serial) return 0;
  h->csr_rec_serial = 0;  // (no records until this call succeeds)
  const int ND = h->nd, E = ND * ND, np = h->top_np, nn = h->g.nnodes, na = h->nactive;
  const int mw = ND == 3 ? CsrCfg<3>::MW : CsrCfg<2>::MW;
  h->csr_blocks = 0;
  if (np > 0 && na > 0) {
    if (reserve(h, who, h->csr_e, (size_t)np * E * E, ND == 3 ? "81 doubles per particle" : "16 doubles per particle")) return 1;
    if (reserve(h, who, h->csr_f, (size_t)np * 6 * ND, "the shape-function factors")) return 1;
    if (reserve(h, who, h->csr_mk, (size_t)np * 2, "the membership masks")) return 1;
    if (reserve(h, who, h->csr_run, (size_t)nn + 1, "the run starts")) return 1;
    if (reserve(h, who, h->csr_mask, (size_t)nn * mw, "the visited-offset masks")) return 1;
    if (reserve(h, who, h->csr_cnt, (size_t)na + 1, "the block counts")) return 1;
    if (reserve(h, who, h->csr_off, (size_t)na + 1, "the block offsets")) return 1;
    // particles grouped by closest node: the (I0, p) sort of the atomic assembly (a stable radix sort of slots in
    // ascending order, so a run holds its particles by ascending memory slot)
    hipLaunchKernelGGL(k_tangent_keys, dim3(nblk(np)), dim3(BLK), 0, h->stream, h->P, h->skey_d, h->sval_d);
    size_t sort_bytes = h->cub_tmp_bytes;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(h->cub_tmp.get(), sort_bytes, h->skey_d.get(), h->skey2_d.get(), h->sval_d.get(),
                                              h->sval2_d.get(), np, 0, 32, h->stream));
    hipLaunchKernelGGL(k_tancsr_runs, dim3(nblk(np)), dim3(BLK), 0, h->stream, np, nn, (const unsigned long long*)h->skey2_d,
                       h->csr_run.get());
    // (the records of E, factors and masks in that order: the sorted list itself is not kept)
    LAUNCH_ND_BLK(k_tancsr_setup<2>, k_tancsr_setup<3>, (np + 63) / 64, 64, h->P, h->g, (const double*)h->top_d, np,
                  (const int*)h->sval2_d, h->csr_e.get(), h->csr_f.get(), h->csr_mk.get(), h->gstatus_d);
    HIPCHK(hipMemsetAsync(h->csr_cnt, 0, ((size_t)na + 1) * sizeof(int), h->stream));
    LAUNCH_ND((k_tancsr_pattern<2>), (k_tancsr_pattern<3>), (nn + 3) / 4, h->g, (const int*)h->csr_run,
              (const unsigned long long*)h->csr_mk, (const int*)h->n2m_d, h->csr_mask.get(), h->csr_cnt.get());
    HIPCHK(hipGetLastError());
    int total = 0;
    if (tancsr_scan(h, who, h->csr_cnt.get(), h->csr_off.get(), &total)) return 1;
    if (check_status(h, ST_NEWTON, (std::string(who) + "()").c_str())) return 1;  // (synchronises)
    h->csr_blocks = total;
  }
  h->csr_rec_serial = h->top_serial;
  return 0;
}

extern "C" int nlps_gpu_tangent_csr_pattern(nlps_gpu* h, long long* nnz, size_t* bytes) {
  if (fbar_refuse(h, "nlps_gpu_tangent_csr_pattern")) return 1;
  const char* who = "nlps_gpu_tangent_csr_pattern";
  if (tanop_valid(h, who)) return 1;
  if (tancsr_one_rank(h, who)) return 1;
  h->csr_serial = 0;  // (no pattern until this call succeeds)
  const int ND = h->nd, E = ND * ND;
  if (bytes) *bytes = tancsr_bytes(ND, (size_t)h->top_np, (size_t)h->g.nnodes, (size_t)h->nactive);
  if (tancsr_records(h, who)) return 1;
  const long long n = h->csr_blocks * E;
  if (nnz) *nnz = n;
  if (tancsr_fits_int(h, who, "nnz", n, "row_ptr and cols of the CSR arrays")) return 1;
  h->csr_serial = h->top_serial;
  return 0;
}

// The three arrays of an assembled form as the caller gave them: the row pointer [nr], the indices [ni], the values
// [nv].  Destinations on the device are written in place, host ones through staging of this call only.
struct TanOut {
  nlps_gpu* h;
  int *row_ptr, *idx;
  double* vals;
  size_t nr, ni, nv;
  bool dev = false;
  DevBuf<int> row_d, idx_d;
  DevBuf<double> vals_d;
  int *rp = nullptr, *ip = nullptr;  // what the kernels write
  double* vp = nullptr;
  // after the caller's launches.  row_src: the device array that is the row pointer as it stands (nullptr: a kernel
  // wrote rp)
  int finish(const int* row_src) {
    HIPCHK(hipGetLastError());
    if (row_src || !dev) HIPCHK(hipMemcpyAsync(row_ptr, row_src ? row_src : rp, nr * sizeof(int), hipMemcpyDefault, h->stream));
    if (!dev) {
      HIPCHK(hipMemcpyAsync(idx, ip, ni * sizeof(int), hipMemcpyDefault, h->stream));
      HIPCHK(hipMemcpyAsync(vals, vp, nv * sizeof(double), hipMemcpyDefault, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));  // (the copies land in the caller's memory before the staging goes)
    return 0;
  }
};
// Refuses the call (returns 1) or readies io for the launches.  serial: the pattern's, of the call `pattern`; rname and
// iname: what the caller's header calls the row pointer and the indices; stage_row: a kernel writes the row pointer.
// An empty matrix is finished here (the row pointer zeroed): the caller returns 0 where io.ni == 0.
static int tanout_begin(nlps_gpu* h, const char* who, unsigned long long serial, const char* pattern, const char* rname,
                        const char* iname, bool stage_row, TanOut& io) {
  if (tanop_valid(h, who)) return 1;
  if (tancsr_one_rank(h, who)) return 1;
  if (serial == 0 || serial != h->top_serial) {
    h->err = std::string(who) + ": call " + pattern + "() after nlps_gpu_tangent_operator() first";
    return 1;
  }
  if (!io.row_ptr || (io.ni > 0 && (!io.idx || !io.vals))) {
    h->err = std::string(who) + ": " + rname + ", " + iname + " and vals are required";
    return 1;
  }
  if (io.ni == 0) {
    if (is_device_ptr(io.row_ptr)) {
      HIPCHK(hipMemsetAsync(io.row_ptr, 0, io.nr * sizeof(int), h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));
    } else {
      memset(io.row_ptr, 0, io.nr * sizeof(int));
    }
    return 0;
  }
  io.dev = is_device_ptr(io.row_ptr) && is_device_ptr(io.idx) && is_device_ptr(io.vals);
  io.rp = io.row_ptr;
  io.ip = io.idx;
  io.vp = io.vals;
  if (!io.dev) {
    const std::string stage = "the staging of ";
    if ((stage_row && reserve(h, who, io.row_d, io.nr, (stage + rname).c_str())) ||
        reserve(h, who, io.idx_d, io.ni, (stage + iname).c_str()) || reserve(h, who, io.vals_d, io.nv, "the staging of vals"))
      return 1;
    io.rp = io.row_d.get();
    io.ip = io.idx_d.get();
    io.vp = io.vals_d.get();
  }
  return 0;
}

extern "C" int nlps_gpu_tangent_csr(nlps_gpu* h, int* row_ptr, int* cols, double* vals) {
  const char* who = "nlps_gpu_tangent_csr";
  const int ND = h->nd, E = ND * ND, nn = h->g.nnodes, na = h->nactive;
  const size_t ne = (size_t)h->csr_blocks * E;
  TanOut io{h, row_ptr, cols, vals, (size_t)na * ND + 1, ne, ne};
  if (tanout_begin(h, who, h->csr_serial, "nlps_gpu_tangent_csr_pattern", "row_ptr", "cols", true, io)) return 1;
  if (ne == 0) return 0;
  LAUNCH_ND((k_tancsr_rowptr<2>), (k_tancsr_rowptr<3>), nblk((int)io.nr), na, (const int*)h->csr_cnt, (const int*)h->csr_off,
            io.rp);
  const int* d2m = h->top_dir ? (const int*)h->d2m_d : nullptr;
  const double* aM = h->top_mass ? (const double*)h->top_m : nullptr;
  LAUNCH_ND_BLK((k_tancsr_rows<2>), (k_tancsr_rows<3>), nn, (ND == 3 ? CsrCfg<3>::NT : CsrCfg<2>::NT), h->g,
                (const int*)h->csr_run, (const double*)h->csr_e, (const double*)h->csr_f,
                (const unsigned long long*)h->csr_mk, (const unsigned long long*)h->csr_mask, (const int*)h->n2m_d, d2m, aM, (const int*)h->csr_cnt,
                (const int*)h->csr_off, io.ip, io.vp);
  return io.finish(nullptr);
}

// ------------------------------------------------------------------------------------------------
// the tangent in block CSR, every block or the upper blocks of a symmetric tangent (nlps_tangent_bsr.hpp)
// ------------------------------------------------------------------------------------------------
static size_t tanbsr_bytes(int nd, size_t np, size_t nnodes, size_t nactive) {
  return tancsr_bytes(nd, np, nnodes, nactive) + 8 * (nactive + 1) + 4;
}

extern "C" int nlps_gpu_tangent_bsr_pattern(nlps_gpu* h, int kind, long long* nblocks, size_t* bytes) {
  if (fbar_refuse(h, "nlps_gpu_tangent_bsr_pattern")) return 1;
  const char* who = "nlps_gpu_tangent_bsr_pattern";
  if (tanop_valid(h, who)) return 1;
  if (tancsr_one_rank(h, who)) return 1;
  h->bsr_serial = 0;  // (no pattern until this call succeeds)
  if (kind != NLPS_BSR_FULL && kind != NLPS_BSR_UPPER) {
    h->err = std::string(who) + ": kind " + std::to_string(kind) + " is neither NLPS_BSR_FULL (0) nor NLPS_BSR_UPPER (1)";
    return 1;
  }
  if (kind == NLPS_BSR_UPPER && h->uniform_law != NLPS_MAT_NEO_HOOKEAN) {
    // (the rule of the atomic path's half rows: nlps_gpu_tangent_assemble)
    static const char* const names[] = {"Neo-Hookean", "Hencky", "Drucker-Prager", "Von-Mises", "Matsuoka-Nakai / Lade-Duncan",
                                        "Newtonian-Fluid-Compressible"};
    std::string laws;
    for (int k = 1; k <= NLPS_KLAW_FLUID; k++)
      if (h->law_present & (1 << k)) laws += (laws.empty() ? "" : ", ") + std::string(names[k]);
    h->err = std::string(who) + ": NLPS_BSR_UPPER needs a symmetric tangent, which only a cloud of Neo-Hookean particles "
             "has; this cloud holds " + (laws.empty() ? "no material" : laws) + " (use NLPS_BSR_FULL)";
    return 1;
  }
  const int ND = h->nd, nn = h->g.nnodes, na = h->nactive;
  if (bytes) *bytes = tanbsr_bytes(ND, (size_t)h->top_np, (size_t)nn, (size_t)na);
  if (tancsr_records(h, who)) return 1;
  h->bsr_blocks = h->csr_blocks;  // (every block: the counts and offsets of the CSR pattern serve as they stand)
  h->bsr_half = false;
  if (h->csr_blocks > 0) {
    // [0, N_A]: the counts of the upper block rows; [N_A + 1]: some row's upper blocks are not its offsets >= 0
    if (reserve(h, who, h->bsr_cnt, (size_t)na + 2, "the block counts")) return 1;
    if (reserve(h, who, h->bsr_off, (size_t)na + 1, "the block offsets")) return 1;
  }
  if (h->csr_blocks > 0 && kind == NLPS_BSR_UPPER) {
    HIPCHK(hipMemsetAsync(h->bsr_cnt, 0, ((size_t)na + 2) * sizeof(int), h->stream));
    LAUNCH_ND((k_tanbsr_count<2>), (k_tanbsr_count<3>), (nn + 3) / 4, h->g, (const unsigned long long*)h->csr_mask,
              (const int*)h->n2m_d, h->bsr_cnt.get(), h->bsr_cnt.get() + na + 1);
    HIPCHK(hipGetLastError());
    int total = 0, mixed = 0;
    HIPCHK(hipMemcpyAsync(&mixed, h->bsr_cnt + na + 1, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (tancsr_scan(h, who, h->bsr_cnt.get(), h->bsr_off.get(), &total)) return 1;
    h->bsr_blocks = total;
    h->bsr_half = !mixed;
  }
  if (nblocks) *nblocks = h->bsr_blocks;
  if (tancsr_fits_int(h, who, "nblocks", h->bsr_blocks, "brow_ptr and bcols of the arrays")) return 1;
  h->bsr_kind = kind;
  h->bsr_serial = h->top_serial;
  return 0;
}

extern "C" int nlps_gpu_tangent_bsr(nlps_gpu* h, int col_major, int* brow_ptr, int* bcols, double* vals) {
  const char* who = "nlps_gpu_tangent_bsr";
  const int ND = h->nd, E = ND * ND, nn = h->g.nnodes;
  const size_t nb = (size_t)h->bsr_blocks;
  TanOut io{h, brow_ptr, bcols, vals, (size_t)h->nactive + 1, nb, nb * E};
  if (tanout_begin(h, who, h->bsr_serial, "nlps_gpu_tangent_bsr_pattern", "brow_ptr", "bcols", false, io)) return 1;
  if (nb == 0) return 0;
  const int* d2m = h->top_dir ? (const int*)h->d2m_d : nullptr;
  const double* aM = h->top_mass ? (const double*)h->top_m : nullptr;
  const int upper = h->bsr_kind == NLPS_BSR_UPPER ? 1 : 0, nt = ND == 3 ? CsrCfg<3>::NT : CsrCfg<2>::NT;
  const int* cnt = upper ? (const int*)h->bsr_cnt : (const int*)h->csr_cnt;
  const int* off = upper ? (const int*)h->bsr_off : (const int*)h->csr_off;
#define TANBSR_ROWS(HALF)                                                                                                   \
  LAUNCH_ND_BLK((k_tanbsr_rows<2, HALF>), (k_tanbsr_rows<3, HALF>), nn, nt, h->g, (const int*)h->csr_run,                   \
                (const double*)h->csr_e, (const double*)h->csr_f, (const unsigned long long*)h->csr_mk,                     \
                (const unsigned long long*)h->csr_mask, (const int*)h->n2m_d, d2m, aM, cnt, off, upper,                     \
                col_major ? 1 : 0, io.ip, io.vp)
  if (h->bsr_half)
    TANBSR_ROWS(true);
  else
    TANBSR_ROWS(false);
#undef TANBSR_ROWS
  return io.finish(off);  // (brow_ptr is the scan of the block counts as it stands)
}

// ------------------------------------------------------------------------------------------------
// device GMRES on the matrix-free tangent (nlps_krylov.hpp): the driver's KSPSolve in one call
// ------------------------------------------------------------------------------------------------
// the values the kernels left in the host word (one synchronisation)
static int ksp_wait(nlps_gpu* h) {
  HIPCHK(h->ksp_h.fetch(h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// the refusal of the solves whose reductions (what: "dot products", "norms") stay on one rank
static int single_rank_only(nlps_gpu* h, const char* who, const char* what) {
  if (!h->halo && !(h->rccl && h->rccl->world > 1)) return 0;
  h->err = std::string(who) + ": single rank only: this handle exchanges halos (a halo callback or an RCCL world > 1), and " +
           what + " across ranks would need an owner mask and an allreduce";
  return 1;
}

// the pinned word(s) the kernels of a solve report through: allocated and zeroed on first use (without a device alias
// the kernels write a device copy and the solve's wait brings it over)
template <class T>
static int ensure_host_word(nlps_gpu* h, Mirrored<T>& w, size_t n = 1) {
  if (w.host()) return 0;
  HIPCHK(w.alloc(n));
  memset(w.host(), 0, n * sizeof(T));
  return 0;
}

// the copies back to the caller's host vectors that close a solve; the caller of a solve on device vectors gets its
// synchronisation all the same
static int vec_end(nlps_gpu* h, const char* who, VecIO& io) {
  if (io.finish()) {
    h->err = std::string(who) + ": HIP error";
    return 1;
  }
  if (io.back.empty()) HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// the preconditioner of the current linearisation: built from the diagonal blocks once per successful
// nlps_gpu_tangent_operator (top_serial) and kind, reused by the solves that follow
static int ksp_pc_build(nlps_gpu* h, int kind) {
  if (kind == NLPS_PC_NONE || (h->ksp_pc_serial == h->top_serial && h->ksp_pc_kind == kind)) return 0;
  const int ND = h->nd, nA = h->nactive;
  h->ksp_pc_kind = -1;
  const char* who = "nlps_gpu_tangent_solve";
  if (reserve(h, who, h->ksp_pc, (size_t)nA * ND * ND, "the preconditioner")) return 1;
  if (reserve(h, who, h->ksp_bad_d, 1, "the preconditioner check")) return 1;
  if (tanop_bdiag(h, h->ksp_pc)) {
    if (h->err.find("nlps_gpu_tangent_solve") == std::string::npos)
      h->err = "nlps_gpu_tangent_solve: HIP error in the diagonal blocks of the preconditioner";
    return 1;
  }
  HIPCHK(hipMemsetAsync(h->ksp_bad_d, 0x7f, sizeof(int), h->stream));  // (0x7f7f7f7f: no node failed)
  LAUNCH_ND((k_ksp_pc_build<2>), (k_ksp_pc_build<3>), nblk(nA), nA, kind, h->ksp_pc, h->ksp_bad_d);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&h->ksp_h.host()->flags, h->ksp_bad_d, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  const int bad = *(volatile int*)&h->ksp_h.host()->flags;
  if (bad < nA) {
    char buf[240];
    snprintf(buf, sizeof buf,
             "nlps_gpu_tangent_solve: the %s of masked node %d does not invert (%s at or below 1e-14 of the block's norm): "
             "no %s preconditioner for this operator",
             kind == NLPS_PC_JACOBI ? "diagonal" : "diagonal block", bad, kind == NLPS_PC_JACOBI ? "an entry" : "a pivot",
             kind == NLPS_PC_JACOBI ? "Jacobi" : "point-block Jacobi");
    h->err = buf;
    return 1;
  }
  h->ksp_pc_serial = h->top_serial;
  h->ksp_pc_kind = kind;
  return 0;
}

// ---- what the Krylov drivers share ("One scaffold under the Krylov drivers") ----
static int ksp_tiles(size_t n) { return (int)((n + KSP_TILE - 1) / KSP_TILE); }

// where the two-pass Gram-Schmidt keeps its scalars in a driver's small state (KspSmall and EigSmall name them alike)
struct GsSmall {
  int h1, h2, wn2, refine;
};

// classical Gram-Schmidt of w against the first ncol columns of V (leading dimension n): pass 1 (with w.w for DGKS),
// then pass 2 when the refine word says so; eight launches, no wait
static void krylov_orthogonalise(nlps_gpu* h, size_t n, const double* V, int ncol, double* w, const GsSmall o, double* part,
                                 int nb, double* s) {
  const dim3 gs(nb), bs(KSP_NT);
  const double* const nul = nullptr;
  double* const nulw = nullptr;
  const double* const refine = s + o.refine;
  hipLaunchKernelGGL(k_ksp_mdot, gs, bs, 0, h->stream, (int)n, V, n, ncol, 1, (const double*)w, part, nb, nul);
  hipLaunchKernelGGL(k_ksp_finish, dim3(ncol + 1), bs, 0, h->stream, (const double*)part, nb, s + o.h1, nulw, nul, nulw, nul);
  hipLaunchKernelGGL(k_ksp_maxpy, gs, bs, 0, h->stream, (int)n, V, n, ncol, (const double*)(s + o.h1), w, part, nul);
  hipLaunchKernelGGL(k_ksp_finish, dim3(1), bs, 0, h->stream, (const double*)part, nb, s + o.wn2, nulw, nul, s + o.refine,
                     (const double*)(s + o.h1 + ncol));
  hipLaunchKernelGGL(k_ksp_mdot, gs, bs, 0, h->stream, (int)n, V, n, ncol, 0, (const double*)w, part, nb, refine);
  hipLaunchKernelGGL(k_ksp_finish, dim3(ncol), bs, 0, h->stream, (const double*)part, nb, s + o.h2, nulw, refine, nulw, nul);
  hipLaunchKernelGGL(k_ksp_maxpy, gs, bs, 0, h->stream, (int)n, V, n, ncol, (const double*)(s + o.h2), w, part, refine);
  hipLaunchKernelGGL(k_ksp_finish, dim3(1), bs, 0, h->stream, (const double*)part, nb, s + o.wn2, nulw, refine, nulw, nul);
}

// the workspace of one linear solver: vectors of n in ksp_v, partial sums, small state, what reserve() calls the first
// and the last, and the columns of ksp_v that r0 = b - K x0 goes to (r0) and K x0 goes through (scratch)
struct KspSpace {
  size_t nvec, npart, nsmall;
  const char *vectors, *small;
  int r0, scratch;
};

// what ksp_begin leaves to the recurrence; rnorm and reason move with the solve
struct KspRun {
  size_t n;
  int nb;
  const double* bd;
  double* xd;
  double bnorm, rnorm, tol;
  int reason;  // NLPS_KSP_CONVERGED_BZERO when the opening decided, else 0
};

// the opening of a linear solve: the footprint, the workspace, the preconditioner, ||b|| and r0 = b - K x0 with its
// norm (one wait).  n == 0 is decided here, ahead of every allocation (the caller returns 0); b == 0 is run.reason
static int ksp_begin(nlps_gpu* h, VecIO& io, const double* b, double* x, nlps_ksp* ksp, const KspSpace& sp, KspRun& run) {
  const char* who = "nlps_gpu_tangent_solve";
  const size_t n = io.n;
  const int ND = h->nd, nA = h->nactive, kind = ksp->pc, nb = ksp_tiles(n);
  ksp->bytes = sizeof(double) * (sp.nvec * n + sp.npart + sp.nsmall + (kind != NLPS_PC_NONE ? (size_t)nA * ND * ND : 0));
  double* hist = ksp->history;
  run = KspRun{n, nb, nullptr, nullptr, 0.0, 0.0, 0.0, 0};
  if (n == 0) {
    ksp->reason = NLPS_KSP_CONVERGED_BZERO;
    if (hist) hist[0] = 0.0;
    return 0;
  }
  if (reserve(h, who, h->ksp_v, sp.nvec * n, sp.vectors) || reserve(h, who, h->ksp_part, sp.npart, "the partial sums") ||
      reserve(h, who, h->ksp_s, sp.nsmall, sp.small))
    return 1;
  if (ensure_host_word(h, h->ksp_h)) return 1;
  if (ksp_pc_build(h, kind)) return 1;
  const double* bd = run.bd = io.in(b);
  double* xd = run.xd = io.out(x, ksp->x_is_guess != 0);
  double* const r0 = h->ksp_v + (size_t)sp.r0 * n;
  double* const t = h->ksp_v + (size_t)sp.scratch * n;
  double* const part = h->ksp_part;
  KspHost* const hw = h->ksp_h.target();
  const dim3 gs(nb), bs(KSP_NT);
  const double* const nul = nullptr;
  double* const nulw = nullptr;
  hipLaunchKernelGGL(k_ksp_resid, gs, bs, 0, h->stream, (int)n, bd, nul, nulw, part);
  hipLaunchKernelGGL(k_ksp_finish, dim3(1), bs, 0, h->stream, (const double*)part, nb, nulw, &hw->bn2, nul, nulw, nul);
  if (ksp->x_is_guess) {
    if (tanop_product(h, xd, t, nullptr)) return 1;
  } else {
    HIPCHK(hipMemsetAsync(xd, 0, n * sizeof(double), h->stream));
  }
  hipLaunchKernelGGL(k_ksp_resid, gs, bs, 0, h->stream, (int)n, bd, ksp->x_is_guess ? (const double*)t : nul, r0, part);
  hipLaunchKernelGGL(k_ksp_finish, dim3(1), bs, 0, h->stream, (const double*)part, nb, nulw, &hw->rn2, nul, nulw, nul);
  HIPCHK(hipGetLastError());
  if (ksp_wait(h)) return 1;
  run.bnorm = sqrt(h->ksp_h.host()->bn2);
  run.rnorm = sqrt(h->ksp_h.host()->rn2);
  run.tol = std::max(ksp->rtol * run.bnorm, ksp->atol);
  if (hist) hist[0] = run.rnorm;
  if (run.bnorm == 0.0) {  // x = 0 (also over a guess), as KSPSolve
    HIPCHK(hipMemsetAsync(xd, 0, n * sizeof(double), h->stream));
    run.rnorm = 0.0;
    if (hist) hist[0] = 0.0;
    run.reason = NLPS_KSP_CONVERGED_BZERO;
  }
  return 0;
}

// the stopping rule of a true residual after its iterations, in KSPSolve's order; broke: the recurrence cannot go on
static int ksp_stop(const KspRun& run, const nlps_ksp* ksp, int its, bool broke) {
  if (!std::isfinite(run.rnorm) || !std::isfinite(run.bnorm)) return NLPS_KSP_DIVERGED_NANORINF;
  if (run.rnorm <= run.tol) return run.rnorm < ksp->atol ? NLPS_KSP_CONVERGED_ATOL : NLPS_KSP_CONVERGED_RTOL;
  if (run.rnorm > ksp->dtol * run.bnorm) return NLPS_KSP_DIVERGED_DTOL;
  if (its >= ksp->max_it) return NLPS_KSP_DIVERGED_ITS;
  return broke ? NLPS_KSP_DIVERGED_BREAKDOWN : 0;
}

// run.rnorm = ||b - K x|| of the current x, the product through scratch, the residual into r_out (or nowhere): one wait
static int ksp_true_residual(nlps_gpu* h, KspRun& run, double* scratch, double* r_out) {
  const dim3 gs(run.nb), bs(KSP_NT);
  const double* const nul = nullptr;
  double* const nulw = nullptr;
  double* const part = h->ksp_part;
  if (tanop_product(h, run.xd, scratch, nullptr)) return 1;
  hipLaunchKernelGGL(k_ksp_resid, gs, bs, 0, h->stream, (int)run.n, run.bd, (const double*)scratch, r_out, part);
  hipLaunchKernelGGL(k_ksp_finish, dim3(1), bs, 0, h->stream, (const double*)part, run.nb, nulw, &h->ksp_h.target()->rn2, nul,
                     nulw, nul);
  HIPCHK(hipGetLastError());
  if (ksp_wait(h)) return 1;
  run.rnorm = sqrt(h->ksp_h.host()->rn2);
  return 0;
}

// the close of a linear solve: the results, the copies back to host vectors, the synchronisation
static int ksp_end(nlps_gpu* h, VecIO& io, nlps_ksp* ksp, const KspRun& run, int its) {
  ksp->reason = run.reason;
  ksp->iterations = its;
  ksp->rnorm = run.rnorm;
  ksp->bnorm = run.bnorm;
  return vec_end(h, "nlps_gpu_tangent_solve", io);
}

static size_t minres_nbn(size_t nA) { return (nA + KSP_NT - 1) / KSP_NT; }

// nlps_gpu_tangent_solve with NLPS_KSP_TYPE_MINRES (nlps_minres.hpp), after the checks the two solvers share: the
// algorithm of include/nlps_gpu.h, one host wait per step (|eta| and the flags) and one per confirmation
static int minres_solve(nlps_gpu* h, VecIO& io, const double* b, double* x, nlps_ksp* ksp) {
  const size_t n = io.n;
  const int nA = h->nactive, kind = ksp->pc, max_it = ksp->max_it, nb = ksp_tiles(n), nbn = (int)minres_nbn((size_t)nA);
  const KspSpace sp{7, (size_t)nb + (size_t)nbn, MINRES_SMALL, "the MINRES vectors", "the rotation state", 1, 6};
  KspRun run;  // (r0 into v, K x through p)
  if (ksp_begin(h, io, b, x, ksp, sp, run)) return 1;
  if (n == 0) return 0;
  double* const hist = ksp->history;
  double* const base = h->ksp_v;
  double *vp = base, *v = base + n, *wp = base + 2 * n, *w = base + 3 * n;  // (the pairs that rotate)
  double *const z = base + 4 * n, *const q = base + 5 * n, *const p = base + 6 * n;
  double* const part = h->ksp_part;    // [nb]: p . q and the residual norms
  double* const partn = part + nb;     // [nbn]: v_new . z
  double* const s = h->ksp_s;
  const double* const Minv = h->ksp_pc;
  KspHost* const hw = h->ksp_h.target();
  const dim3 gs(nb), bs(KSP_NT);
  // one step from src (r0 on the first, p = K q after it): v_new, z, the rotation and the update of w and x; the
  // wait brings |eta| and the flags
  auto step = [&](int first, const double* src) -> int {
    if (!first) hipLaunchKernelGGL(k_minres_dot, gs, bs, 0, h->stream, (int)n, (const double*)p, (const double*)q, part);
    LAUNCH_ND_BLK((k_minres_lanczos<2>), (k_minres_lanczos<3>), nbn, KSP_NT, nA, kind, Minv, first, src, (const double*)v,
                  vp, z, (const double*)part, nb, s, partn);
    hipLaunchKernelGGL(k_minres_rotate, dim3(1), dim3(64), 0, h->stream, first, (const double*)partn, nbn, s, hw);
    hipLaunchKernelGGL(k_minres_update, gs, bs, 0, h->stream, (int)n, first, (const double*)s, (const double*)z, q, wp,
                       (const double*)w, run.xd);
    HIPCHK(hipGetLastError());
    return ksp_wait(h);
  };
  int its = 0;
  if (!run.reason) run.reason = ksp_stop(run, ksp, its, false);
  double scale = 0.0;
  if (!run.reason) {  // z = M^-1 r0, g = sqrt(r0 . z), q = z / g; v_prev = w_prev = w = 0
    HIPCHK(hipMemsetAsync(vp, 0, n * sizeof(double), h->stream));
    HIPCHK(hipMemsetAsync(wp, 0, 2 * n * sizeof(double), h->stream));
    if (step(1, v)) return 1;
    const int flags = h->ksp_h.host()->flags;
    if (flags & MINRES_FLAG_INDEFINITE) run.reason = NLPS_KSP_DIVERGED_INDEFINITE_PC;
    else if (flags & KSP_FLAG_NONFINITE) run.reason = NLPS_KSP_DIVERGED_NANORINF;
    else scale = run.rnorm / h->ksp_h.host()->est;
  }
  while (!run.reason) {
    if (tanop_product(h, q, p, nullptr)) return 1;
    if (step(0, p)) return 1;
    const int flags = h->ksp_h.host()->flags;
    const double eta = h->ksp_h.host()->est;  // (|eta|: the estimate is scale |eta|)
    if (flags & (MINRES_FLAG_INDEFINITE | KSP_FLAG_NONFINITE | KSP_FLAG_SINGULAR)) {  // (x is the one of step its)
      run.reason = (flags & MINRES_FLAG_INDEFINITE) ? NLPS_KSP_DIVERGED_INDEFINITE_PC
                   : (flags & KSP_FLAG_NONFINITE)   ? NLPS_KSP_DIVERGED_NANORINF
                                                    : NLPS_KSP_DIVERGED_BREAKDOWN;
      if (ksp_true_residual(h, run, p, nullptr)) return 1;
      break;
    }
    std::swap(vp, v);  // (v_new and w_new were written over v_prev and w_prev)
    std::swap(wp, w);
    its++;
    const double est = scale * eta;
    if (hist) hist[its] = est;
    if (!std::isfinite(est)) {
      run.reason = NLPS_KSP_DIVERGED_NANORINF;
      if (ksp_true_residual(h, run, p, nullptr)) return 1;
      break;
    }
    const bool gzero = (flags & MINRES_FLAG_GZERO) != 0;
    if (est <= run.tol || its >= max_it || gzero) {  // the confirmation: read-only for the recurrence
      if (ksp_true_residual(h, run, p, nullptr)) return 1;
      run.reason = ksp_stop(run, ksp, its, gzero);
      if (!run.reason) scale = run.rnorm / eta;
    }
  }
  return ksp_end(h, io, ksp, run, its);
}

extern "C" int nlps_gpu_set_linear_solver(nlps_gpu* h, int type) {
  const char* who = "nlps_gpu_set_linear_solver";
  if (type != NLPS_KSP_TYPE_GMRES && type != NLPS_KSP_TYPE_MINRES) {
    h->err = std::string(who) + ": type " + std::to_string(type) + " is neither NLPS_KSP_TYPE_GMRES (0) nor NLPS_KSP_TYPE_MINRES (1)";
    return 1;
  }
  if (type == NLPS_KSP_TYPE_MINRES && h->uniform_law != NLPS_MAT_NEO_HOOKEAN) {  // (the rule of NLPS_BSR_UPPER)
    static const char* const names[] = {"Neo-Hookean", "Hencky", "Drucker-Prager", "Von-Mises", "Matsuoka-Nakai / Lade-Duncan",
                                        "Newtonian-Fluid-Compressible"};
    std::string laws;
    for (int k = 0; k <= NLPS_KLAW_FLUID; k++)
      if (h->law_present & (1 << k)) laws += (laws.empty() ? "" : ", ") + std::string(names[k]);
    h->err = std::string(who) + ": NLPS_KSP_TYPE_MINRES needs a symmetric tangent, which only a cloud of Neo-Hookean particles "
             "has; this cloud holds " + (laws.empty() ? "no material" : laws) + " (the handle stays on its previous solver)";
    return 1;
  }
  h->ksp_type = type;
  return 0;
}

extern "C" int nlps_gpu_tangent_solve(nlps_gpu* h, const double* b, double* x, nlps_ksp* ksp) {
  const char* who = "nlps_gpu_tangent_solve";
  if (!ksp) {
    h->err = "nlps_gpu_tangent_solve: ksp is required";
    return 1;
  }
  ksp->reason = 0;
  ksp->iterations = 0;
  ksp->rnorm = ksp->bnorm = 0.0;
  ksp->bytes = 0;
  if (tanop_valid(h, who)) return 1;
  if (single_rank_only(h, who, "dot products")) return 1;
  if (!b || !x) {
    h->err = "nlps_gpu_tangent_solve: b and x are required";
    return 1;
  }
  const int m = ksp->restart, kind = ksp->pc, max_it = ksp->max_it;
  if (kind != NLPS_PC_NONE && kind != NLPS_PC_JACOBI && kind != NLPS_PC_PBJACOBI) {
    h->err = "nlps_gpu_tangent_solve: pc must be NLPS_PC_NONE, NLPS_PC_JACOBI or NLPS_PC_PBJACOBI";
    return 1;
  }
  const bool minres = h->ksp_type == NLPS_KSP_TYPE_MINRES;  // (restart is not read)
  if ((!minres && (m < 1 || m > NLPS_KSP_MAX_RESTART)) || max_it < 0) {
    h->err = "nlps_gpu_tangent_solve: restart must be 1 .. NLPS_KSP_MAX_RESTART and max_it >= 0";
    return 1;
  }
  if (!(ksp->rtol >= 0.0) || !(ksp->atol >= 0.0) || !(ksp->dtol > 0.0)) {
    h->err = "nlps_gpu_tangent_solve: rtol and atol must be >= 0 and dtol > 0";
    return 1;
  }
  VecIO io;
  if (vec_begin(h, who, io)) return 1;
  if (minres) return minres_solve(h, io, b, x, ksp);
  const size_t n = io.n;
  const int nA = h->nactive, nb = ksp_tiles(n);
  const KspSmall L{m};
  const KspSpace sp{(size_t)m + 3, (size_t)(m + 2) * nb, L.size(), "the Krylov basis", "the Hessenberg state", 0, m + 2};
  KspRun run;  // (r0 into V[0], K x through t)
  if (ksp_begin(h, io, b, x, ksp, sp, run)) return 1;
  if (n == 0) return 0;
  double* const hist = ksp->history;
  double* const V = h->ksp_v;  // V[c] at V + c n
  double* const z = V + (size_t)(m + 1) * n;
  double* const t = z + n;
  double* const part = h->ksp_part;
  double* const s = h->ksp_s;
  KspHost* const hw = h->ksp_h.target();
  const KspPc pcd{kind, h->ksp_pc, z};
  const GsSmall gso{L.h1(), L.h2(), L.wn2(), L.refine()};
  const dim3 gs(nb), bs(KSP_NT);
  int its = 0;
  bool broke = false;
  while (!run.reason) {
    if ((run.reason = ksp_stop(run, ksp, its, broke))) break;
    // one cycle: V[0] = r / ||r||, Arnoldi steps on K M^-1 until the estimate converges, the cycle is full, max_it or
    // a breakdown; one host synchronisation per step (the estimate and the flags)
    hipLaunchKernelGGL(k_ksp_scale, gs, bs, 0, h->stream, (int)n, (const double*)V, V, 1.0 / run.rnorm, (const double*)nullptr);
    int k = 0;
    bool nonfinite = false;
    for (int j = 0; j < m; j++) {
      double* const w = V + (size_t)(j + 1) * n;
      if (tanop_product(h, V + (size_t)j * n, w, &pcd)) return 1;
      krylov_orthogonalise(h, n, V, j + 1, w, gso, part, nb, s);
      hipLaunchKernelGGL(k_ksp_arnoldi, dim3(1), dim3(64), 0, h->stream, L, s, j, run.rnorm, hw);
      hipLaunchKernelGGL(k_ksp_scale, gs, bs, 0, h->stream, (int)n, (const double*)w, w, 1.0, (const double*)(s + L.wn2()));
      HIPCHK(hipGetLastError());
      if (ksp_wait(h)) return 1;
      const double est = h->ksp_h.host()->est;
      const int flags = h->ksp_h.host()->flags;
      its++;
      if (hist) hist[its] = est;
      if ((flags & KSP_FLAG_NONFINITE) || !std::isfinite(est)) {
        nonfinite = true;
        break;
      }
      if (flags & KSP_FLAG_SINGULAR) {  // (column j does not enter the update)
        broke = true;
        break;
      }
      k = j + 1;
      if (est <= run.tol || (flags & KSP_FLAG_HAPPY) || its >= max_it) break;
    }
    if (nonfinite) {
      run.reason = NLPS_KSP_DIVERGED_NANORINF;
      break;
    }
    if (k > 0) {  // x += M^-1 V y, R y = g
      hipLaunchKernelGGL(k_ksp_hsolve, dim3(1), dim3(64), 0, h->stream, L, s, k);
      LAUNCH_ND((k_ksp_update<2>), (k_ksp_update<3>), nblk(nA), nA, kind, (const double*)h->ksp_pc, (const double*)V, n, k,
                (const double*)(s + L.y()), run.xd);
    }
    // the true residual of the new x: confirms the estimate, or starts the next cycle from V[0]
    if (ksp_true_residual(h, run, t, V)) return 1;
  }
  return ksp_end(h, io, ksp, run, its);
}

// ------------------------------------------------------------------------------------------------
// device Lanczos on the matrix-free tangent (nlps_eigen.hpp): the stable step of the explicit scheme
// ------------------------------------------------------------------------------------------------
extern "C" double nlps_host_critical_dt(double omega2, double gamma, double safety) {
  if (gamma < 0.5) return -1.0;
  if (!(omega2 > 0.0)) return INFINITY;
  return safety * sqrt(2.0 / gamma) / sqrt(omega2);  // Omega_crit = (gamma / 2 - beta)^-1/2 at beta = 0
}

// w = A q = ps (K (ps q)) on device masked vectors (xs: the scaled input, kept for the mass term); apart: the block
// partial sums of q . w, or nullptr
static int eig_product(nlps_gpu* h, const double* ps, const double* q, double* xs, double* w, double* apart) {
  const int ND = h->nd, nn = h->g.nnodes;
  double *xg = h->top_g, *yg = h->top_g + (size_t)nn * ND;
  LAUNCH_ND((k_eig_expand<2>), (k_eig_expand<3>), nblk(nn), nn, (const int*)h->n2m_d, ps, q, xs, xg, yg);
  if (h->top_np > 0 && scatter_tiles<2, 3>(h, "nlps_gpu_tangent_lambda_max", 1, yg, [&](auto NT, const TileD td) {
        LAUNCH_ND_BLK((k_tanop_apply<2, CT(NT)>), (k_tanop_apply<3, CT(NT)>), h->ntw, CT(NT), h->P, h->g, td,
                      (const double*)h->top_d, h->top_np, (const double*)xg, yg);
      }))
    return 1;
  HIPCHK(hipGetLastError());
  LAUNCH_ND_BLK((k_eig_nodal<2>), (k_eig_nodal<3>), nblk(nn, KSP_NT), KSP_NT, nn, (const int*)h->n2m_d, (const double*)yg,
                (const double*)xs, h->top_mass ? (const double*)h->top_m : (const double*)nullptr, ps,
                apart ? q : (const double*)nullptr, w, apart);
  HIPCHK(hipGetLastError());
  return 0;
}

static int eig_wait(nlps_gpu* h) {
  HIPCHK(h->eig_h.fetch(h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int nlps_gpu_tangent_lambda_max(nlps_gpu* h, const double* lumped_mass, const double* v0, nlps_eig* eig,
                                           double* mode) {
  if (fbar_refuse(h, "nlps_gpu_tangent_lambda_max")) return 1;
  const char* who = "nlps_gpu_tangent_lambda_max";
  if (!eig) {
    h->err = "nlps_gpu_tangent_lambda_max: eig is required";
    return 1;
  }
  eig->reason = 0;
  eig->iterations = 0;
  eig->theta = eig->resid = eig->asymmetry = 0.0;
  eig->bytes = 0;
  if (tanop_valid(h, who)) return 1;
  if (single_rank_only(h, who, "dot products")) return 1;
  if (!lumped_mass) {
    h->err = "nlps_gpu_tangent_lambda_max: lumped_mass is required";
    return 1;
  }
  const int m = eig->max_it;
  if (m < 1 || m > NLPS_KSP_MAX_RESTART) {
    h->err = "nlps_gpu_tangent_lambda_max: max_it must be 1 .. NLPS_KSP_MAX_RESTART";
    return 1;
  }
  if (!(eig->rtol >= 0.0)) {
    h->err = "nlps_gpu_tangent_lambda_max: rtol must be >= 0";
    return 1;
  }
  VecIO io;
  if (vec_begin(h, who, io)) return 1;
  const size_t n = io.n;
  const int nA = h->nactive, nn = h->g.nnodes, nb = ksp_tiles(n), nbg = nblk(nn, KSP_NT);
  const EigSmall L{m};
  eig->bytes = sizeof(double) * ((size_t)(m + 4) * n + (size_t)(m + 2) * nb + nbg + L.size());
  if (n == 0) {
    eig->reason = NLPS_EIG_EMPTY;
    return 0;
  }
  if (reserve(h, who, h->ksp_v, (size_t)(m + 4) * n, "the Lanczos basis") ||
      reserve(h, who, h->ksp_part, (size_t)(m + 2) * nb + nbg, "the partial sums") ||
      reserve(h, who, h->ksp_s, L.size(), "the tridiagonal state") ||
      reserve(h, who, h->ksp_bad_d, 1, "the mass check"))
    return 1;
  if (ensure_host_word(h, h->eig_h)) return 1;
  const double* md = io.in(lumped_mass);
  const double* v0d = io.in(v0);
  double* moded = io.out(mode, false);
  double* const Q = h->ksp_v;  // Q[c] at Q + c n, c <= m
  double* const ps = Q + (size_t)(m + 1) * n;
  double* const xs = ps + n;
  double* const y = xs + n;
  double* const part = h->ksp_part;
  double* const apart = part + (size_t)(m + 2) * nb;
  double* const s = h->ksp_s;
  EigHost* const hw = h->eig_h.target();
  EigHost* const hh = h->eig_h.host();
  const GsSmall gso{L.h1(), L.h2(), L.wn2(), L.refine()};
  const dim3 gs(nb), bs(KSP_NT);
  const double* const nul = nullptr;
  double* const nulw = nullptr;
  // ps = P S, q_1 = P v0 / ||P v0||; the one wait ahead of the loop brings the norm and the mass check
  HIPCHK(hipMemsetAsync(h->ksp_bad_d, 0x7f, sizeof(int), h->stream));  // (0x7f7f7f7f: no node failed)
  hipLaunchKernelGGL(k_eig_start, gs, bs, 0, h->stream, (int)n, h->nd, h->top_dir ? (const int*)h->d2m_d : (const int*)nullptr,
                     md, v0d, eig->seed, ps, Q, part, h->ksp_bad_d.get());
  hipLaunchKernelGGL(k_ksp_finish, dim3(1), bs, 0, h->stream, (const double*)part, nb, s + L.n2(), &hw->n2, nul, nulw, nul);
  hipLaunchKernelGGL(k_ksp_scale, gs, bs, 0, h->stream, (int)n, (const double*)Q, Q, 1.0, (const double*)(s + L.n2()));
  HIPCHK(hipGetLastError());
  HIPCHK(h->eig_h.fetch(h->stream));
  HIPCHK(hipMemcpyAsync(&hh->bad, h->ksp_bad_d, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  const int bad = *(volatile int*)&hh->bad;
  if (bad < nA) {
    char buf[240];
    snprintf(buf, sizeof buf,
             "nlps_gpu_tangent_lambda_max: the lumped mass of masked node %d is not positive and finite on a free dof: "
             "M^-1/2 does not exist there",
             bad);
    h->err = buf;
    return 1;
  }
  const double n2 = hh->n2;
  int its = 0, reason = 0;
  double theta = 0.0, asym = 0.0;
  if (n2 == 0.0) reason = NLPS_EIG_EMPTY;
  else if (!std::isfinite(n2)) reason = NLPS_EIG_DIVERGED_NANORINF;
  for (int j = 0; !reason; j++) {
    double* const w = Q + (size_t)(j + 1) * n;
    if (eig_product(h, ps, Q + (size_t)j * n, xs, w, apart)) return 1;
    hipLaunchKernelGGL(k_ksp_finish, dim3(1), bs, 0, h->stream, (const double*)apart, nbg, s + L.aj(), nulw, nul, nulw, nul);
    krylov_orthogonalise(h, n, Q, j + 1, w, gso, part, nb, s);  // (against q_1 .. q_j)
    hipLaunchKernelGGL(k_eig_ritz, dim3(1), dim3(64), 0, h->stream, L, s, j, hw);
    hipLaunchKernelGGL(k_ksp_scale, gs, bs, 0, h->stream, (int)n, (const double*)w, w, 1.0, (const double*)(s + L.wn2()));
    HIPCHK(hipGetLastError());
    if (eig_wait(h)) return 1;
    theta = hh->theta;
    asym = hh->asym;
    const double est = hh->est;
    its = j + 1;
    if (eig->history) eig->history[j] = theta;
    if ((hh->flags & EIG_FLAG_NONFINITE) || !std::isfinite(theta) || !std::isfinite(est)) reason = NLPS_EIG_DIVERGED_NANORINF;
    else if (est <= eig->rtol * fabs(theta)) reason = NLPS_EIG_CONVERGED;  // (beta_j == 0 gives est == 0)
    else if (its == m) reason = NLPS_EIG_DIVERGED_ITS;
  }
  eig->reason = reason;
  eig->iterations = its;
  eig->theta = theta;
  eig->asymmetry = asym;
  if (its > 0 && reason != NLPS_EIG_DIVERGED_NANORINF) {  // y = Q s, the true residual from one product, mode = S y
    double* const t = Q + (size_t)its * n;
    hipLaunchKernelGGL(k_eig_ritzvec, gs, bs, 0, h->stream, (int)n, (const double*)Q, n, its, (const double*)(s + L.s()), y);
    if (eig_product(h, ps, y, xs, t, nullptr)) return 1;
    hipLaunchKernelGGL(k_eig_resid, gs, bs, 0, h->stream, (int)n, (const double*)t, (const double*)y,
                       (const double*)(s + L.theta()), (const double*)ps, moded, part);
    hipLaunchKernelGGL(k_ksp_finish, dim3(1), bs, 0, h->stream, (const double*)part, nb, nulw, &hw->rn2, nul, nulw, nul);
    HIPCHK(hipGetLastError());
    if (eig_wait(h)) return 1;
    eig->resid = sqrt(hh->rn2);
  } else {
    if (moded) HIPCHK(hipMemsetAsync(moded, 0, n * sizeof(double), h->stream));
    if (reason == NLPS_EIG_DIVERGED_NANORINF) eig->resid = NAN;
  }
  return vec_end(h, who, io);
}

// ------------------------------------------------------------------------------------------------
// Newton solve (nlps_newton.hpp): the driver's SNESSolve (NEWTONLS, basic or bt line search) in one call
// ------------------------------------------------------------------------------------------------

// queues F . F of a device residual towards the host word (stream order, no wait)
static int snes_fnorm_launch(nlps_gpu* h, const double* F) {
  const int n = h->nactive * h->nd, nb = h->snes_nb;
  double* const hw = h->snes_h.target();
  double* const part = h->snes_part + (size_t)3 * nb;
  hipLaunchKernelGGL(k_snes_dots, dim3(nb), dim3(KSP_NT), 0, h->stream, n, F, (const double*)nullptr, part, nb);
  hipLaunchKernelGGL(k_snes_finish, dim3(1), dim3(KSP_NT), 0, h->stream, (const double*)part, nb, -1, hw + SNES_H_FF);
  HIPCHK(hipGetLastError());
  HIPCHK(h->snes_h.fetch(h->stream));
  h->snes_tail = false;
  return 0;
}

// what every residual evaluation of one solve shares (device pointers)
struct SnesResidual {
  const double *v, *a, *m, *alpha, *gravity;
  const nlps_bcc* loads;
  int nloads, step;
  double thickness;
  const double* area0;
};

// F = R(x) and its norm: the fused evaluation queues the norm ahead of its own synchronisation (snes_tail), the
// composition of the separate stages is followed by the norm and a wait
static int snes_residual(nlps_gpu* h, const SnesResidual& r, const double* x, double* F, nlps_snes* snes, double* fnorm) {
  h->snes_tail = true;
  const int st = nlps_gpu_lagrangian_evaluation(h, F, x, r.v, r.a, r.m, r.alpha, r.gravity, r.loads, r.nloads, r.step,
                                                r.thickness, r.area0, 0);
  const bool queued = !h->snes_tail;
  h->snes_tail = false;
  if (st) return 1;
  if (!queued) {
    if (snes_fnorm_launch(h, F)) return 1;
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  snes->function_evaluations++;
  *fnorm = sqrt(((volatile double*)h->snes_h.host())[SNES_H_FF]);
  return 0;
}

extern "C" int nlps_gpu_newton_solve(nlps_gpu* h, double* dU, const double* Un_dt, const double* Un_dt2, const double* M,
                                     const double* alpha, const double* gravity, const nlps_bcc* loads, int nloads, int step,
                                     double thickness, const double* area0, nlps_snes* snes) {
  if (fbar_refuse(h, "nlps_gpu_newton_solve")) return 1;
  const char* who = "nlps_gpu_newton_solve";
  if (!snes) {
    h->err = "nlps_gpu_newton_solve: snes is required";
    return 1;
  }
  snes->reason = snes->iterations = snes->function_evaluations = snes->linear_iterations = 0;
  snes->fnorm0 = snes->fnorm = snes->snorm = snes->xnorm = 0.0;
  if (need_masks(h, who)) return 1;
  if (single_rank_only(h, who, "norms")) return 1;
  if (!dU || !Un_dt || !Un_dt2 || !M || !alpha) {
    h->err = "nlps_gpu_newton_solve: dU, Un_dt, Un_dt2, M and alpha are required";
    return 1;
  }
  if (!(snes->atol >= 0.0) || !(snes->rtol >= 0.0) || !(snes->stol >= 0.0) || !(snes->divtol >= 0.0) || snes->max_it < 0) {
    h->err = "nlps_gpu_newton_solve: atol, rtol, stol, divtol and max_it must be >= 0";
    return 1;
  }
  h->tan_alpha4 = alpha[3];  // the fluid law's tangent reads alpha_4 (Constitutive.c:298-314)
  const bool bt = snes->linesearch == NLPS_LS_BT;
  if (!bt && snes->linesearch != NLPS_LS_BASIC) {
    h->err = "nlps_gpu_newton_solve: linesearch must be NLPS_LS_BASIC or NLPS_LS_BT";
    return 1;
  }
  if (bt && (snes->ls_max_it < 0 || !(snes->ls_alpha >= 0.0) || !(snes->ls_steptol >= 0.0) || !(snes->ls_maxstep > 0.0))) {
    h->err = "nlps_gpu_newton_solve: ls_max_it, ls_alpha and ls_steptol must be >= 0 and ls_maxstep > 0";
    return 1;
  }
  const size_t n = (size_t)h->nactive * h->nd;
  const int nb = (int)std::max<size_t>((n + KSP_TILE - 1) / KSP_TILE, 1);
  if (reserve(h, who, h->snes_v, 8 * std::max<size_t>(n, 1), "the work vectors") ||
      reserve(h, who, h->snes_part, (size_t)5 * nb, "the partial sums"))
    return 1;
  h->snes_nb = nb;
  if (ensure_host_word(h, h->snes_h, SNES_H_N)) return 1;
  volatile double* const hv = h->snes_h.host();
  double* const hw = h->snes_h.target();
  double *X = h->snes_v, *Y = X + n, *W = Y + n, *F = W + n, *T = F + n;
  // host vectors cross once: dU into X, the three constant vectors into their slots
  if (n > 0) HIPCHK(hipMemcpyAsync(X, dU, n * sizeof(double), hipMemcpyDefault, h->stream));
  const double* cst[3] = {Un_dt, Un_dt2, M};
  for (int q = 0; q < 3; q++) {
    if (is_device_ptr(cst[q]) || n == 0) continue;
    double* d = T + (size_t)(q + 1) * n;
    HIPCHK(hipMemcpyAsync(d, cst[q], n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    cst[q] = d;
  }
  const SnesResidual res{cst[0], cst[1], cst[2], alpha, gravity, loads, nloads, step, thickness, area0};
  const dim3 gs(nb), bs(KSP_NT);
  // W = X - lambda Y with its three scalars towards the host word (stream order)
  auto trial = [&](double lambda) -> int {
    hipLaunchKernelGGL(k_snes_trial, gs, bs, 0, h->stream, (int)n, (const double*)X, (const double*)Y, lambda, W, h->snes_part, nb);
    hipLaunchKernelGGL(k_snes_finish, dim3(3), bs, 0, h->stream, (const double*)h->snes_part, nb, 2, hw + SNES_H_WW);
    HIPCHK(hipGetLastError());
    return 0;
  };
  double fnorm = 0.0;
  if (snes_residual(h, res, X, F, snes, &fnorm)) return 1;
  snes->fnorm0 = snes->fnorm = fnorm;
  if (snes->fnorm_history) snes->fnorm_history[0] = fnorm;
  int reason = 0;
  if (!std::isfinite(fnorm)) reason = NLPS_SNES_DIVERGED_FNORM_NAN;
  else if (fnorm < snes->atol) reason = NLPS_SNES_CONVERGED_FNORM_ABS;
  const double fnorm0 = fnorm;
  while (!reason && snes->iterations < snes->max_it) {
    const int it = snes->iterations;
    if (nlps_gpu_tangent_operator(h, alpha[0], res.m, snes->apply_dirichlet, nullptr)) return 1;
    nlps_ksp k = snes->ksp;
    k.x_is_guess = 0;
    const int kst = nlps_gpu_tangent_solve(h, F, Y, &k);
    snes->ksp.reason = k.reason;
    snes->ksp.iterations = k.iterations;
    snes->ksp.rnorm = k.rnorm;
    snes->ksp.bnorm = k.bnorm;
    snes->ksp.bytes = k.bytes;
    if (kst) return 1;
    snes->linear_iterations += k.iterations;
    if (snes->ksp_iterations) snes->ksp_iterations[it] = k.iterations;
    if (k.reason < 0) {  // (the state is still the one of the evaluation at X)
      reason = NLPS_SNES_DIVERGED_LINEAR_SOLVE;
      break;
    }
    double lambda = 1.0, ynorm = 0.0, gnorm = 0.0;
    bool accepted = true;
    if (!bt) {
      if (trial(1.0) || snes_residual(h, res, W, F, snes, &gnorm)) return 1;
      ynorm = sqrt(hv[SNES_H_YY]);
    } else {
      // the slope F . (K Y) on the snapshotted operator, then the full step: its evaluation brings every scalar over
      if (n > 0 && tanop_product(h, Y, T, nullptr)) return 1;
      double* const part = h->snes_part + (size_t)3 * nb;
      hipLaunchKernelGGL(k_snes_dots, gs, bs, 0, h->stream, (int)n, (const double*)F, n > 0 ? (const double*)T : (const double*)nullptr, part, nb);
      hipLaunchKernelGGL(k_snes_finish, dim3(n > 0 ? 2 : 1), bs, 0, h->stream, (const double*)part, nb, -1, hw + SNES_H_FF);
      HIPCHK(hipGetLastError());
      if (trial(1.0) || snes_residual(h, res, W, F, snes, &gnorm)) return 1;
      double s = n > 0 ? hv[SNES_H_FT] : 0.0, ratio = hv[SNES_H_RATIO], ysc = 1.0;
      ynorm = sqrt(hv[SNES_H_YY]);
      if (ynorm > snes->ls_maxstep) {  // Y is too long: the full step was evaluated for nothing (it counts), the scaled one follows
        ysc = snes->ls_maxstep / ynorm;
        s *= ysc;
        ratio *= ysc;
        ynorm = snes->ls_maxstep;
        if (trial(ysc) || snes_residual(h, res, W, F, snes, &gnorm)) return 1;
      }
      if (s > 0.0) s = -s;
      if (s == 0.0) s = -1.0;
      const double minlambda = snes->ls_steptol / ratio, f2 = fnorm * fnorm;
      auto accept = [&](double g, double lam) { return std::isfinite(g) && 0.5 * g * g <= 0.5 * f2 + snes->ls_alpha * lam * s; };
      auto clamp = [](double lt, double lam) { return lt > 0.5 * lam ? 0.5 * lam : (lt <= 0.1 * lam ? 0.1 * lam : lt); };
      if (ynorm != 0.0 && !accept(gnorm, lambda)) {
        accepted = false;
        if (snes->ls_max_it > 0) {
          // the quadratic step through f, the slope and the full step
          double g2 = gnorm * gnorm;
          double lprev = lambda, g2prev = g2;
          lambda = std::isfinite(g2) ? clamp(-s / (g2 - f2 - 2.0 * lambda * s), lambda) : 0.5 * lambda;
          if (trial(lambda * ysc) || snes_residual(h, res, W, F, snes, &gnorm)) return 1;
          accepted = accept(gnorm, lambda);
          for (int c = 0; !accepted && c < snes->ls_max_it; c++) {
            if (lambda < minlambda) break;
            g2 = gnorm * gnorm;
            double lt = 0.5 * lambda;
            if (std::isfinite(g2) && std::isfinite(g2prev)) {  // the cubic through the last two trials
              const double t1 = 0.5 * (g2 - f2) - lambda * s, t2 = 0.5 * (g2prev - f2) - lprev * s;
              const double a = (t1 / (lambda * lambda) - t2 / (lprev * lprev)) / (lambda - lprev);
              const double b = (-lprev * t1 / (lambda * lambda) + lambda * t2 / (lprev * lprev)) / (lambda - lprev);
              double d = b * b - 3.0 * a * s;
              if (d < 0.0) d = 0.0;
              lt = a == 0.0 ? -s / (2.0 * b) : (-b + sqrt(d)) / (3.0 * a);
              lt = clamp(lt, lambda);
            }
            lprev = lambda;
            g2prev = g2;
            lambda = lt;
            if (trial(lambda * ysc) || snes_residual(h, res, W, F, snes, &gnorm)) return 1;
            accepted = accept(gnorm, lambda);
          }
        }
      }
    }
    if (!accepted) {  // X is restored: the state of a rejected trial must not be the one the call leaves
      if (snes_residual(h, res, X, F, snes, &fnorm)) return 1;
      reason = NLPS_SNES_DIVERGED_LINE_SEARCH;
      break;
    }
    std::swap(X, W);
    fnorm = gnorm;
    snes->iterations = it + 1;
    snes->fnorm = fnorm;
    snes->snorm = lambda * ynorm;
    snes->xnorm = sqrt(hv[SNES_H_WW]);
    if (snes->fnorm_history) snes->fnorm_history[it + 1] = fnorm;
    if (snes->lambda_history) snes->lambda_history[it] = lambda;
    if (!std::isfinite(fnorm)) reason = NLPS_SNES_DIVERGED_FNORM_NAN;
    else if (fnorm < snes->atol) reason = NLPS_SNES_CONVERGED_FNORM_ABS;
    else if (snes->function_evaluations > snes->max_funcs) reason = NLPS_SNES_DIVERGED_FUNCTION_COUNT;
    else if (fnorm <= snes->rtol * fnorm0) reason = NLPS_SNES_CONVERGED_FNORM_RELATIVE;
    else if (snes->snorm < snes->stol * snes->xnorm) reason = NLPS_SNES_CONVERGED_SNORM_RELATIVE;
    else if (fnorm > snes->divtol * fnorm0) reason = NLPS_SNES_DIVERGED_DTOL;
  }
  if (!reason) reason = NLPS_SNES_DIVERGED_MAX_IT;
  snes->reason = reason;
  snes->fnorm = fnorm;
  if (n > 0) HIPCHK(hipMemcpyAsync(dU, X, n * sizeof(double), hipMemcpyDefault, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// ------------------------------------------------------------------------------------------------
// the body of the implicit driver's time loop (U-Newmark-beta.c:192-404) in one call
// ------------------------------------------------------------------------------------------------
extern "C" int nlps_gpu_newmark_step(nlps_gpu* h, const nlps_bcc* bcc, int nbcc, int step, const nlps_newmark* nm,
                                     const double* gravity, const nlps_bcc* loads, int nloads, double thickness,
                                     const double* area0, nlps_snes* snes, int* nactive, double* dU_out) {
  if (fbar_refuse(h, "nlps_gpu_newmark_step")) return 1;
  const char* who = "nlps_gpu_newmark_step";
  if (!nm || !snes) {
    h->err = "nlps_gpu_newmark_step: nm and snes are required";
    return 1;
  }
  if (!(nm->dt > 0.0) || !(nm->beta > 0.0)) {
    h->err = "nlps_gpu_newmark_step: dt and beta must be positive";
    return 1;
  }
  if (nlps_gpu_local_search(h)) return 1;                                               // :197
  int na = 0;
  if (nlps_gpu_active_masks(h, bcc, nbcc, step, &na, nullptr, nullptr, nullptr)) return 1;  // :205-209
  if (nactive) *nactive = na;
  const size_t n = (size_t)na * h->nd;
  if (reserve(h, who, h->nm_v, 6 * std::max<size_t>(n, 1), "the nodal vectors of the step")) return 1;
  double *M = h->nm_v, *V = M + n, *A = V + n, *dU = A + n, *dV = dU + n, *dA = dV + n;
  if (nlps_gpu_lumped_mass(h, M)) return 1;                                             // :223
  if (nlps_gpu_nodal_field_n(h, V, A, M)) return 1;                                     // :241
  const double beta = nm->beta, gamma = nm->gamma, dt = nm->dt;                         // :497-514
  const double alpha[6] = {1.0 / (beta * dt * dt), 1.0 / (beta * dt), (1.0 - 2.0 * beta) / (2.0 * beta), gamma / (beta * dt),
                           1.0 - gamma / beta, (1.0 - gamma / (2.0 * beta)) * dt};
  if (n > 0) HIPCHK(hipMemsetAsync(dU, 0, n * sizeof(double), h->stream));
  if (nlps_gpu_form_initial_guess(h, dU, V, A, dt, nm->use_explicit_trial, bcc, nbcc, step)) return 1;  // :255
  if (nlps_gpu_newton_solve(h, dU, V, A, M, alpha, gravity, loads, nloads, step, thickness, area0, snes)) return 1;  // :356
  if (dU_out && n > 0) {
    HIPCHK(hipMemcpyAsync(dU_out, dU, n * sizeof(double), hipMemcpyDefault, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  if (snes->reason <= 0) return 0;  // (not converged: the particles stay at the last evaluated state, not rolled)
  if (nlps_gpu_nodal_kinetic_increments(h, dV, dA, dU, V, A, alpha)) return 1;          // :380
  if (nlps_gpu_roll_state(h)) return 1;                                                 // :393
  if (nlps_gpu_update_kinetics(h, nm->alpha_blend, dU, V, dV, dA)) return 1;            // :396
  if (h->rec.on) {  // the step record (nlps_gpu_set_step_record): a converged step, behind the particle update
    if (rec_check(h, who)) return 1;
    return rec_step(h, NLPS_REC_KIND_NEWMARK, step, dt, nullptr, 0);
  }
  return 0;
}
