// Device side of the particle snapshot (nlps_gpu_set_snapshots): k_snap_pack gathers the selected fields of
// every particle into a slot's staging block -- field after field, each in the caller's particle order and in the layout
// of nlps_gpu_download_state -- on the handle's stream; one asynchronous copy then takes the block to pinned memory on
// the snapshot stream.  The shape of nlps_record.hpp: the kernel reads THROUGH the pending state (a deferred move, the
// tau / W a folded step did not store, the density the fused scheme leaves as rho J) and forms in registers what
// materialise_move / materialise_roll would have stored, with their expressions.  Nothing here writes a particle array.
#pragma once

static constexpr int SNAP_NT = 256;     // threads per block of k_snap_pack
static constexpr int SNAP_NFIELDS = 20;  // the NLPS_SNAP_ bits; the last one (I0) is the block of ints behind the doubles

// components per particle of the field of bit b (doubles; 1 int for NLPS_SNAP_I0)
__host__ __device__ constexpr int snap_ncomp(int b, int nd) {
  return (b < 4 || b == 17) ? nd                    // x, dis, vel, acc, lambda
         : (b == 4 || b == 5 || b == 6) ? (nd == 2 ? 5 : 9)  // F_n, Stress, b_e_n
         : b == 14 ? 3                              // Back_stress
                   : 1;
}
// doubles per particle in front of the field of bit b (b = SNAP_NFIELDS - 1: all the doubles of a particle)
static inline int snap_doubles_before(unsigned fields, int b, int nd) {
  int n = 0;
  for (int q = 0; q < b && q < SNAP_NFIELDS - 1; q++)
    if ((fields >> q) & 1u) n += snap_ncomp(q, nd);
  return n;
}

struct SnapArgs {
  unsigned fields;
  int rolled;  // explicit steps renamed the n / n+1 slots since the last materialise_roll: rho is (rho J) / J_n
  int lazy;    // ... and the last one did not store tau and W of the hyperelastic laws (rec_stress_energy)
  const unsigned char* moved;  // the marks of a pending move, nullptr without one
  const int* perm;             // memory slot -> caller's index, or its inverse (k_snap_pack BY_CALLER)
  double* out;                 // the slot's staging block
};

// BY_CALLER (the shipped form): one thread per caller's index, perm = caller's index -> memory slot (k_inverse_perm): the
// columns are gathered, the rows of a wave are written side by side.  Otherwise one thread per memory slot, perm = slot ->
// caller's index: coalesced column reads, every caller's row written in one piece (ndim, 5 | 9, 3 or 1 consecutive
// doubles) wherever it lies.  Measured in DESIGN.md 5l.  Every branch on `fields` is uniform over the grid.
template <int ND, bool BY_CALLER = false>
__global__ __launch_bounds__(SNAP_NT) void k_snap_pack(PView P, const MatD* __restrict__ mats, SnapArgs a) {
  constexpr int T = ND == 2 ? 5 : 9;
  const int i = blockIdx.x * SNAP_NT + threadIdx.x;
  if (i >= P.np) return;
  const int p = BY_CALLER ? a.perm[i] : i;
  const size_t np = (size_t)P.np, q = BY_CALLER ? (size_t)i : (size_t)a.perm[i];
  const unsigned f = a.fields;
  double* __restrict__ o = a.out;
  const bool mv = a.moved && a.moved[p];
  if (f & (NLPS_SNAP_X | NLPS_SNAP_DIS)) {  // the additions of apply_move for a marked particle
    double dd[ND];
#pragma unroll
    for (int c = 0; c < ND; c++) dd[c] = mv ? PF(P, F_DDIS + c, p) : 0.0;
    if (f & NLPS_SNAP_X) {
#pragma unroll
      for (int c = 0; c < ND; c++) {
        const double v = PF(P, F_X + c, p);
        o[q * ND + c] = mv ? v + dd[c] : v;
      }
      o += np * ND;
    }
    if (f & NLPS_SNAP_DIS) {
#pragma unroll
      for (int c = 0; c < ND; c++) {
        const double v = PF(P, F_DIS + c, p);
        o[q * ND + c] = mv ? v + dd[c] : v;
      }
      o += np * ND;
    }
  }
  if (f & NLPS_SNAP_VEL) {
#pragma unroll
    for (int c = 0; c < ND; c++) o[q * ND + c] = PF(P, F_VEL + c, p);
    o += np * ND;
  }
  if (f & NLPS_SNAP_ACC) {
#pragma unroll
    for (int c = 0; c < ND; c++) o[q * ND + c] = PF(P, F_ACC + c, p);
    o += np * ND;
  }
  if (f & NLPS_SNAP_F_N) {
    const int fn = fFN(P);
#pragma unroll
    for (int s = 0; s < T; s++) o[q * T + s] = PF(P, fn + s, p);
    o += np * T;
  }
  double W = 0.0;
  if (f & (NLPS_SNAP_STRESS | NLPS_SNAP_W)) {
    double tau[ND * ND], tzz = 0.0;
    rec_stress_energy<ND>(P, mats, a.lazy, p, tau, tzz, W, (f & NLPS_SNAP_STRESS) != 0);
    if (f & NLPS_SNAP_STRESS) {
#pragma unroll
      for (int s = 0; s < ND * ND; s++) o[q * T + s] = tau[s];
      if (ND == 2) o[q * T + 4] = tzz;
      o += np * T;
    }
  }
  if (f & NLPS_SNAP_B_E_N) {
    const int fb = fBEN(P);
#pragma unroll
    for (int s = 0; s < T; s++) o[q * T + s] = PF(P, fb + s, p);
    o += np * T;
  }
  if (f & NLPS_SNAP_J_N) {
    o[q] = PF(P, F_JN, p);
    o += np;
  }
  if (f & NLPS_SNAP_RHO) {  // (k_copy_n_to_n1)
    o[q] = a.rolled ? PF(P, F_RHOJ, p) / PF(P, F_JN, p) : PF(P, F_RHO, p);
    o += np;
  }
  if (f & NLPS_SNAP_MASS) {
    o[q] = PF(P, F_MASS, p);
    o += np;
  }
  if (f & NLPS_SNAP_VOL0) {
    o[q] = PF(P, F_VOL0, p);
    o += np;
  }
  if (f & NLPS_SNAP_W) {
    o[q] = W;
    o += np;
  }
  if (f & NLPS_SNAP_KAPPA_N) {
    o[q] = PF(P, F_KN, p);
    o += np;
  }
  if (f & NLPS_SNAP_EPS_N) {
    o[q] = PF(P, F_EN, p);
    o += np;
  }
  if (f & NLPS_SNAP_BACK_STRESS) {
#pragma unroll
    for (int c = 0; c < 3; c++) o[q * 3 + c] = PF(P, F_BACK + c, p);
    o += np * 3;
  }
  if (f & NLPS_SNAP_DAMAGE_N) {
    o[q] = PF(P, F_DMG, p);
    o += np;
  }
  if (f & NLPS_SNAP_STRAIN_F_N) {
    o[q] = PF(P, F_STRF, p);
    o += np;
  }
  if (f & NLPS_SNAP_LAMBDA) {
#pragma unroll
    for (int c = 0; c < ND; c++) o[q * ND + c] = PF(P, F_LAM + c, p);
    o += np * ND;
  }
  if (f & NLPS_SNAP_BETA) {
    o[q] = PF(P, F_BETA, p);
    o += np;
  }
  if (f & NLPS_SNAP_I0) reinterpret_cast<int*>(o)[q] = P.I0[p];
}
