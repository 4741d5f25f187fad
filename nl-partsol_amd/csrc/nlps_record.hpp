// Device side of the step record (nlps_gpu_set_step_record): one row per recorded step, made behind the
// step on the handle's stream.  k_rec_particles folds the cloud into one partial per block and quantity (wave shuffles
// and LDS, no float atomics), k_rec_finish combines a quantity's partials in a fixed order and writes the global block
// of the ring's row, k_rec_reactions sums the reactions of the Dirichlet sets of an explicit step from the kept nodal
// sums, k_rec_probes copies the selected fields of the probed particles.  The shape of nlps_newton.hpp: a row is
// bit-reproducible for a given memory order of the particles.  Nothing here writes a particle or a nodal array.
#pragma once

// the quantities of k_rec_particles: sums first, then maxima (J_min travels as the maximum of -J)
enum {
  REC_Q_MASS = 0, REC_Q_MOM = 1, REC_Q_ANG = 4, REC_Q_MX = 7, REC_Q_KIN = 10, REC_Q_STRAIN = 11, REC_Q_VOL = 12,
  REC_Q_FAILED = 13, REC_NSUM = 14,
  REC_M_VCOMP = 0, REC_M_VV = 1, REC_M_NEGJ = 2, REC_M_J = 3, REC_M_EPS = 4, REC_M_DMG = 5, REC_NMAX = 6,
  REC_NQ = REC_NSUM + REC_NMAX
};
static constexpr int REC_NT = 256;            // threads per block of every k_rec_ kernel
static constexpr int REC_MAX_BLOCKS = 2048;   // k_rec_particles: above REC_NT * REC_MAX_BLOCKS particles a thread folds several
static constexpr int REC_SETS_PER_LAUNCH = 8; // Dirichlet sets that travel as one kernel argument

// tau, tau_zz and W of a particle as nlps_gpu_download_state would return them: the stored values, or -- after a folded
// explicit step, which does not store them for the hyperelastic laws (stress_update LAZY) -- re-formed in registers from
// the stored F_n and J_n with the code of k_copy_n_to_n1
template <int ND>
__device__ __forceinline__ void rec_stress_energy(const PView& P, const MatD* __restrict__ mats, int lazy, int p, double* tau,
                                                  double& tau_zz, double& W, bool want_tau) {
  if (lazy) {
    const MatD m = mats[P.mat[p]];
    if (m.type == NLPS_MAT_NEO_HOOKEAN || m.type == NLPS_MAT_HENCKY) {
      double F[ND * ND], z;
      load_block<ND>(P, fFN(P), p, F, z);
      StressIO<ND> o;
      o.fail = 0;
      if (m.type == NLPS_MAT_NEO_HOOKEAN) law_neo_hookean<ND>(m, F, PF(P, F_JN, p), o);
      else law_hencky<ND>(m, F, o);
#pragma unroll
      for (int s = 0; s < ND * ND; s++) tau[s] = o.tau[s];
      tau_zz = o.tau_zz;
      W = o.W;
      return;
    }
  }
  if (want_tau) load_block<ND>(P, F_TAU, p, tau, tau_zz);
  W = PF(P, F_W, p);
}

template <int ND>
__global__ __launch_bounds__(REC_NT) void k_rec_particles(PView P, const MatD* __restrict__ mats, int lazy,
                                                          double* __restrict__ partials, int nb) {
  __shared__ double red[REC_NQ][REC_NT / 64];
  double s[REC_NSUM], m[REC_NMAX];
#pragma unroll
  for (int q = 0; q < REC_NSUM; q++) s[q] = 0.0;
#pragma unroll
  for (int q = 0; q < REC_NMAX; q++) m[q] = -INFINITY;
  for (int p = blockIdx.x * REC_NT + threadIdx.x; p < P.np; p += nb * REC_NT) {
    const double mass = PF(P, F_MASS, p), J = PF(P, F_JN, p), dmg = PF(P, F_DMG, p);
    double x[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < ND; a++) {
      x[a] = PF(P, F_X + a, p);
      v[a] = PF(P, F_VEL + a, p);
    }
    double tau[ND * ND], tzz, W;
    rec_stress_energy<ND>(P, mats, lazy, p, tau, tzz, W, false);
    double vv = 0.0, vc = 0.0;
#pragma unroll
    for (int a = 0; a < ND; a++) {
      vv += v[a] * v[a];
      vc = fmax(vc, fabs(v[a]));
    }
    s[REC_Q_MASS] += mass;
#pragma unroll
    for (int a = 0; a < ND; a++) {
      s[REC_Q_MOM + a] += mass * v[a];
      s[REC_Q_MX + a] += mass * x[a];
    }
    if (ND == 3) {
      s[REC_Q_ANG + 0] += mass * (x[1] * v[2] - x[2] * v[1]);
      s[REC_Q_ANG + 1] += mass * (x[2] * v[0] - x[0] * v[2]);
    }
    s[REC_Q_ANG + 2] += mass * (x[0] * v[1] - x[1] * v[0]);
    s[REC_Q_KIN] += 0.5 * mass * vv;
    s[REC_Q_STRAIN] += W * PF(P, F_VOL0, p);
    s[REC_Q_VOL] += PF(P, F_VOL0, p) * J;
    s[REC_Q_FAILED] += dmg == 1.0 ? 1.0 : 0.0;
    m[REC_M_VCOMP] = fmax(m[REC_M_VCOMP], vc);
    m[REC_M_VV] = fmax(m[REC_M_VV], vv);
    m[REC_M_NEGJ] = fmax(m[REC_M_NEGJ], -J);
    m[REC_M_J] = fmax(m[REC_M_J], J);
    m[REC_M_EPS] = fmax(m[REC_M_EPS], PF(P, F_EN, p));
    m[REC_M_DMG] = fmax(m[REC_M_DMG], dmg);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int q = 0; q < REC_NSUM; q++) s[q] += __shfl_down(s[q], off);
#pragma unroll
    for (int q = 0; q < REC_NMAX; q++) m[q] = fmax(m[q], __shfl_down(m[q], off));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < REC_NSUM; q++) red[q][wave] = s[q];
#pragma unroll
    for (int q = 0; q < REC_NMAX; q++) red[REC_NSUM + q][wave] = m[q];
  }
  __syncthreads();
  if (threadIdx.x < REC_NQ) {
    const int q = threadIdx.x;
    const double a = red[q][0], b = red[q][1], c = red[q][2], d = red[q][3];
    partials[(size_t)q * nb + blockIdx.x] = q < REC_NSUM ? ((a + b) + c) + d : fmax(fmax(a, b), fmax(c, d));
  }
}

// what the host knows of a row
struct RecHead {
  double step, kind, dt, time, np;
};

// one block per quantity: its partials in a fixed order (a thread takes every REC_NT-th, then the tree of the block) into
// the slot of the row; block 0 also writes the head, the status word and the reserved slots
__global__ __launch_bounds__(REC_NT) void k_rec_finish(const double* __restrict__ partials, int nb, RecHead hd,
                                                       const int* __restrict__ gstatus, double* __restrict__ row) {
  __shared__ double red[REC_NT / 64];
  const int q = blockIdx.x;
  const bool sum = q < REC_NSUM;
  double a = sum ? 0.0 : -INFINITY;
  for (int i = threadIdx.x; i < nb; i += REC_NT) {
    const double v = partials[(size_t)q * nb + i];
    a = sum ? a + v : fmax(a, v);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_down(a, off);
    a = sum ? a + o : fmax(a, o);
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x != 0) return;
  a = sum ? ((red[0] + red[1]) + red[2]) + red[3] : fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  const int m = q - REC_NSUM;
  if (q < REC_Q_FAILED) row[NLPS_REC_MASS + q] = a;  // mass, momentum, angular, mass_x, kinetic, strain, volume
  else if (q == REC_Q_FAILED) row[NLPS_REC_FAILED] = a;
  else if (m == REC_M_VCOMP) row[NLPS_REC_VMAX_COMP] = nb > 0 ? a : 0.0;  // (empty cloud: the identities of the header)
  else if (m == REC_M_VV) row[NLPS_REC_VMAX_NORM] = nb > 0 ? sqrt(a) : 0.0;
  else if (m == REC_M_NEGJ) row[NLPS_REC_J_MIN] = -a;
  else if (m == REC_M_J) row[NLPS_REC_J_MAX] = a;
  else if (m == REC_M_EPS) row[NLPS_REC_EPS_MAX] = nb > 0 ? a : 0.0;
  else row[NLPS_REC_DAMAGE_MAX] = nb > 0 ? a : 0.0;
  if (q == 0) {
    row[NLPS_REC_STEP] = hd.step;
    row[NLPS_REC_KIND] = hd.kind;
    row[NLPS_REC_DT] = hd.dt;
    row[NLPS_REC_TIME] = hd.time;
    row[NLPS_REC_NP] = hd.np;
    row[NLPS_REC_STATUS] = (double)*gstatus;
    for (int r = NLPS_REC_STATUS + 1; r < NLPS_REC_NGLOBAL; r++) row[r] = 0.0;
  }
}

// the Dirichlet sets of one launch: the node lists ensure_bcs keeps on the device, and the directions switched on at the step
struct RecSets {
  const int* nodes[REC_SETS_PER_LAUNCH];
  int n[REC_SETS_PER_LAUNCH], bits[REC_SETS_PER_LAUNCH], dim[REC_SETS_PER_LAUNCH];
  int nlive;  // blocks < nlive sum their set, the others write NaN (sets the step did not have; rows of other kinds)
};

// One block per set.  The reaction of a dof (node, k) of the set with dir[k][step] == 1 is what k_nodal_accel stores for a
// fixed dof: the kept force sum where the node is active and has mass, 0 elsewhere (an active node of the set IS fixed in
// every direction the set switches on, whichever later set overrides its value).  Reads N.active, N.nm, N.force only.
template <int ND>
__global__ __launch_bounds__(REC_NT) void k_rec_reactions(NView N, RecSets sets, int n0, int nwn, double* __restrict__ out) {
  __shared__ double red[3][REC_NT / 64];
  const int s = blockIdx.x;
  if (s >= sets.nlive) {
    if (threadIdx.x < 3) out[(size_t)s * 3 + threadIdx.x] = NAN;
    return;
  }
  const int* __restrict__ nodes = sets.nodes[s];
  const int n = sets.n[s], bits = sets.bits[s], dim = sets.dim[s];
  double r[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < n; i += REC_NT) {
    const int A = nodes[i];
    if (A < n0 || A >= n0 + nwn) continue;  // (outside the node window nothing of the step exists)
    const double M = N.nm[(size_t)A * (1 + ND)];
    if (!N.active[A] || M == 0.0) continue;
#pragma unroll
    for (int k = 0; k < ND; k++)
      if (k < dim && ((bits >> k) & 1)) r[k] += N.force[(size_t)A * ND + k];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < 3; k++) r[k] += __shfl_down(r[k], off);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 3; k++) red[k][threadIdx.x >> 6] = r[k];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    out[(size_t)s * 3 + k] = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
  }
}

// One thread per probe and field group (the ten NLPS_PROBE_ bits); a probe's block holds the selected groups in ascending
// bit order, in the layout of nlps_gpu_download_state.  inv: caller's index -> memory slot (k_inverse_perm).
template <int ND>
__global__ __launch_bounds__(REC_NT) void k_rec_probes(PView P, const MatD* __restrict__ mats, int lazy, const int* __restrict__ ids,
                                                       const int* __restrict__ inv, int nprobes, unsigned fields, int probe_doubles,
                                                       double* __restrict__ out) {
  constexpr int T = ND == 2 ? 5 : 9, NG = 10;
  const int t = blockIdx.x * REC_NT + threadIdx.x;
  const int q = t / NG, g = t - q * NG;
  if (q >= nprobes || !((fields >> g) & 1u)) return;
  int off = 0;
#pragma unroll
  for (int b = 0; b < NG; b++)
    if (b < g && ((fields >> b) & 1u)) off += b < 4 ? ND : (b < 6 ? T : 1);
  const int p = inv[ids[q]];
  double* __restrict__ o = out + (size_t)q * probe_doubles + off;
  if (g < 4) {  // x, dis, vel, acc
    const int f = g == 0 ? F_X : (g == 1 ? F_DIS : (g == 2 ? F_VEL : F_ACC));
#pragma unroll
    for (int a = 0; a < ND; a++) o[a] = PF(P, f + a, p);
  } else if (g == 4) {  // F_n
#pragma unroll
    for (int s = 0; s < T; s++) o[s] = PF(P, fFN(P) + s, p);
  } else if (g == 5 || g == 9) {  // Stress, W
    double tau[ND * ND], tzz = 0.0, W;
    rec_stress_energy<ND>(P, mats, lazy, p, tau, tzz, W, g == 5);
    if (g == 9) {
      o[0] = W;
    } else {
#pragma unroll
      for (int s = 0; s < ND * ND; s++) o[s] = tau[s];
      if (ND == 2) o[4] = tzz;
    }
  } else {
    o[0] = PF(P, g == 6 ? F_JN : (g == 7 ? F_EN : F_DMG), p);
  }
}
