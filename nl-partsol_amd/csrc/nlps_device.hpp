// nlps_device.hpp — device-side building blocks (gfx950): separable LME evaluation on the
// structured background grid, <=3x3 tensor algebra in registers, the three Kirchhoff-stress laws.
//
// Reference semantics (file:line relative to nl-partsol/src of migmolper/NL-PartSol):
//   p_a, r, J, grad p_a ........ Nodes/LME.c:676-891
//   Newton for lambda .......... Nodes/LME.c:272-353
//   Neo-Hookean ................ Constitutive/Hyperelastic/Neo-Hookean.c:18-85
//   Hencky ..................... Constitutive/Hyperelastic/Hencky.c:40-94,233-285
//   Drucker-Prager ............. Constitutive/Plasticity/Drucker-Prager.c:319-1084
//
// MI355X-first formulation: on a lattice, x_a = x_I0 + h*(i,j,k), so
//   exp(-beta |l_a|^2 + lambda.l_a) = Ex(i) * Ey(j) * Ez(k)
// with 5 one-dimensional factors per axis: 15 exp() per evaluation instead of 5^3 = 125, every
// factor and every partial sum held in registers by one lane (one particle per lane, no cross-lane
// traffic).  Neighbourhood membership (active node AND |l_a| <= Ra, LME.c:1062-1082) is a 125-bit
// mask per particle in lexicographic stencil order (bit = i + 5*j + 25*k).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nlps {

typedef unsigned long long u64;

struct GridD {
  int nd;
  int n[3];
  int nnodes;
  double o[3];
  double h;
};

// per-material constants, precomputed on the host with libm so they carry the bits the CPU path has
struct MatD {
  int type;
  double E, nu;
  double G, lame, K;                 // shear, Lame, bulk (E/(3(1-2nu)))
  double alpha_F, alpha_Q, beta_dp;  // Drucker-Prager.c:362-375
  double kappa_0, exp_param, eps_0, p_ref;
  double H, theta, K_0, K_inf, delta;  // Von-Mises.c:246-253 (sigma_y = kappa_0)
  double Ceps, Gf;                     // eigenerosion (EigenErosion.c:63-64)
  double ft, heps, wcrit;              // eigensoftening (EigenSoftening.c:67-69)
  // Matsuoka-Nakai (surface 0) / Lade-Duncan (surface 1): type = NLPS_KLAW_FRICTIONAL for both
  int surface;
  // (one law per material: the fluid's constants share the slots of the frictional laws', so the table keeps its row size
  // and the kernels of the other laws the addresses they were compiled with)
  union {
    struct {
      double c_cotphi, alpha_b, a_b[3];
    };
    // compressible Newtonian fluid (Newtonian-Fluid.c:31-34; ReferencePressure is p_ref): type = NLPS_KLAW_FLUID
    struct {
      double viscosity, K_fluid, n_macdonald;
    };
  };
};
#define NLPS_KLAW_FRICTIONAL 4
#define NLPS_KLAW_FLUID 5  // NLPS_MAT_NEWTONIAN_FLUID: the one law that reads the rate tensors

struct ParamsD {
  double gamma_lme, neg_log_tol_zero, tol_wrapper;
  int max_iter_lme;
  double tol_radial;
  int max_iter_radial;
};

#define NLPS_TOL_NR 10E-6  // Macros.h:40

// a * b + c contracted to fma inside the constitutive laws and their 3 x 3 helpers (the library is built
// -ffp-contract=off for the index maps)
#define NLPS_FP_CONTRACT _Pragma("clang fp contract(fast)")

__device__ __forceinline__ double dsqr(double a) { return a == 0.0 ? 0.0 : a * a; }  // Macros.h:49-50

// ------------------------------------------------------------------------------------------------
// small tensors (row-major, N = 2|3)
// ------------------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ double det(const double* A) {  // I3__TensorLib__, TensorLib.c:154-168
  NLPS_FP_CONTRACT
  if (N == 2) return A[0] * A[3] - A[1] * A[2];
  return A[0] * A[4] * A[8] - A[0] * A[5] * A[7] + A[1] * A[5] * A[6] - A[1] * A[3] * A[8] +
         A[2] * A[3] * A[7] - A[2] * A[4] * A[6];
}

// inverse__MatrixLib__ (MatrixOp.c:320, LAPACK dgetrf/dgetri in the reference): adjugate / det
template <int N>
__device__ __forceinline__ bool inverse(double* Am1, const double* A) {
  NLPS_FP_CONTRACT
  if (N == 2) {
    double d = A[0] * A[3] - A[1] * A[2];
    if (d == 0.0) return false;
    double id = 1.0 / d;
    Am1[0] = A[3] * id;
    Am1[1] = -A[1] * id;
    Am1[2] = -A[2] * id;
    Am1[3] = A[0] * id;
    return true;
  }
  double c00 = A[4] * A[8] - A[5] * A[7];
  double c01 = A[5] * A[6] - A[3] * A[8];
  double c02 = A[3] * A[7] - A[4] * A[6];
  double d = A[0] * c00 + A[1] * c01 + A[2] * c02;
  if (d == 0.0) return false;
  double id = 1.0 / d;
  Am1[0] = c00 * id;
  Am1[1] = (A[2] * A[7] - A[1] * A[8]) * id;
  Am1[2] = (A[1] * A[5] - A[2] * A[4]) * id;
  Am1[3] = c01 * id;
  Am1[4] = (A[0] * A[8] - A[2] * A[6]) * id;
  Am1[5] = (A[2] * A[3] - A[0] * A[5]) * id;
  Am1[6] = c02 * id;
  Am1[7] = (A[1] * A[6] - A[0] * A[7]) * id;
  Am1[8] = (A[0] * A[4] - A[1] * A[3]) * id;
  return true;
}

// rcond__TensorLib__ as the reference really evaluates it (TensorLib.c:966-990: dgecon on the
// unfactored matrix): 1 / (||A||_1 * ||(L_A U_A)^-1||_1).  Gate only (LME.c:308).
template <int N>
__device__ __forceinline__ double rcond_ref(const double* A) {
  double anorm = 0.0;
#pragma unroll
  for (int j = 0; j < N; j++) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < N; i++) s += fabs(A[i * N + j]);
    anorm = s > anorm ? s : anorm;
  }
  double LU[N * N], inv[N * N];
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = 0; j < N; j++) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < N; k++) {
        double l = (k < i) ? A[i * N + k] : (k == i ? 1.0 : 0.0);
        double u = (k <= j) ? A[k * N + j] : 0.0;
        s += l * u;
      }
      LU[i * N + j] = s;
    }
  if (anorm == 0.0) return 0.0;
  if (!inverse<N>(inv, LU)) return 0.0;
  double inorm = 0.0;
#pragma unroll
  for (int j = 0; j < N; j++) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < N; i++) s += fabs(inv[i * N + j]);
    inorm = s > inorm ? s : inorm;
  }
  if (!(inorm > 0.0) || isinf(inorm) || isnan(inorm)) return 0.0;
  return (1.0 / inorm) / anorm;
}

// The gate `rcond__TensorLib__(J) < 1E-8` of the Newton iteration (LME.c:308) without evaluating rcond_ref, whenever
// a rigorous lower bound of it already clears the threshold.  With L = unit lower part of A, U = upper part of A
// (what dgecon sees in the unfactored matrix), m = min |diagonal|, q = max |strict upper| / m:
//   ||(L U)^-1||_1 <= ||U^-1||_1 ||L^-1||_1,   ||U^-1||_1 <= (1 + q)^(N-1) / m,
//   ||L^-1||_1 <= 1 + sum |strict lower| + |a10 a21|  (N = 3; 1 + |a10| for N = 2),
// hence rcond_ref >= m^N / (||A||_1 NL (m + qmax)^(N-1)).  Twice the threshold pays for the rounding of the bound
// itself; NaNs, zeros and badly scaled matrices fail the comparison and take the exact evaluation.  The result is
// the boolean the reference computes, for ~25 instructions instead of ~150 per Newton pass.
template <int N>
__device__ __forceinline__ bool rcond_below_gate(const double* A) {
  double anorm = 0.0;
#pragma unroll
  for (int j = 0; j < N; j++) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < N; i++) s += fabs(A[i * N + j]);
    anorm = s > anorm ? s : anorm;
  }
  double m = fabs(A[0]), qmax = 0.0, nl = 1.0;
#pragma unroll
  for (int i = 1; i < N; i++) m = fmin(m, fabs(A[i * N + i]));
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = 0; j < N; j++) {
      if (j > i) qmax = fmax(qmax, fabs(A[i * N + j]));
      if (j < i) nl += fabs(A[i * N + j]);
    }
  if (N == 3) nl += fabs(A[3 % (N * N)] * A[7 % (N * N)]);
  const double mq = m + qmax;
  const double lhs = (N == 3) ? m * m * m : m * m;
  const double rhs = 2.0e-8 * anorm * nl * ((N == 3) ? mq * mq : mq);
  const bool sure = (lhs >= rhs) && (m > 1.0e-90) && (anorm < 1.0e90);
  if (__builtin_amdgcn_ballot_w64(!sure) == 0ull) return false;  // wave-uniform: every lane is surely above the gate
  return rcond_ref<N>(A) < 1E-8;
}

// Symmetric eigen-decomposition by cyclic Jacobi, all in registers (replaces LAPACKE_dsyev,
// TensorLib.c:208 / Drucker-Prager.c:635).  Eigenvector A = COLUMN A of v, eigenvalues ascending like dsyev.
template <int N>
__device__ __forceinline__ void sym_eigen(double* w, double* v, const double* Ain) {
  NLPS_FP_CONTRACT
  // cyclic Jacobi on the upper triangle (Rutishauser's update formulas): per rotation two reciprocal
  // square roots; the rotated pair is annihilated exactly.
  double d[N], o[N == 3 ? 3 : 1];  // diagonal; off-diagonals o[0] = a01, o[1] = a02, o[2] = a12
#pragma unroll
  for (int i = 0; i < N; i++) {
    d[i] = Ain[i * N + i];
#pragma unroll
    for (int j = 0; j < N; j++) v[i * N + j] = (i == j) ? 1.0 : 0.0;
  }
  o[0] = Ain[1];
  if (N == 3) {
    o[1 % (N == 3 ? 3 : 1)] = Ain[2 % (N * N)];
    o[2 % (N == 3 ? 3 : 1)] = Ain[5 % (N * N)];
  }
#pragma unroll 1
  for (int sweep = 0; sweep < 12; sweep++) {
    double off = 0.0, dg = 0.0;
#pragma unroll
    for (int i = 0; i < N; i++) dg += d[i] * d[i];
#pragma unroll
    for (int i = 0; i < (N == 3 ? 3 : 1); i++) off += 2.0 * o[i] * o[i];
    if (off <= 1e-32 * dg || off == 0.0) break;
#pragma unroll
    for (int r = 0; r < (N == 3 ? 3 : 1); r++) {
      // pair (p,q) and the third index m: r = 0 -> (0,1) m=2 ; r = 1 -> (0,2) m=1 ; r = 2 -> (1,2) m=0
      const int p = (r == 2) ? 1 : 0, q = (r == 0) ? 1 : 2;
      const double apq = o[r];
      // An entry below 1e-145 is passed over, not rotated away.  Its square is a subnormal that has lost bits, or zero,
      // so beside a df that small (two equal diagonal entries, or a matrix that small altogether: a stress that is
      // rounding noise) h^2 below is wrong or zero, rh wrong or inf, and the rotation not orthogonal or NaN
      // (c^2 = 0 * inf, c = inf * 0).  Ignoring it moves the matrix by less than 1e-145, far below the rounding of
      // anything a caller reads from the result, and every entry that is rotated has h^2 >= 4e-290.  The entry stays
      // where it is (zeroing it on this path costs the Von-Mises K3 kernels 8 to 12 bytes of scratch): it
      // adds less than 2e-290 to `off`, so the sweeps end as they would without it, at the latest at the twelfth.
      // A NaN fails the comparison, is rotated and stays NaN.
      if (!(fabs(apq) < 1e-145)) {
        const double df = d[q] - d[p];
        // the rotation (|theta| <= 45 degrees, the inner one) from two reciprocal square roots (no division, no sqrt):
        // with h = sqrt(df^2 + 4 apq^2), cos 2 theta = |df| / h, so c^2 = (1 + |df| / h) / 2 in [1/2, 1],
        // s = sgn(df) apq / (h c), t = s / c
        const double rh = rsqrt(fma(df, df, 4.0 * apq * apq));
        const double c2 = fma(0.5 * fabs(df), rh, 0.5), ic = rsqrt(c2);
        const double c = c2 * ic, sn = (df >= 0.0 ? apq : -apq) * rh * ic, t = sn * ic;
        d[p] -= t * apq;
        d[q] += t * apq;
        o[r] = 0.0;
        if (N == 3) {
          // the two other off-diagonals couple p and q with the third index m
          const int ip = (r == 0) ? 1 : (r == 1 ? 0 : 0);  // index in o[] of a_{p m}
          const int iq = (r == 0) ? 2 : (r == 1 ? 2 : 1);  // index in o[] of a_{q m}
          const double apm = o[ip % (N == 3 ? 3 : 1)], aqm = o[iq % (N == 3 ? 3 : 1)];
          o[ip % (N == 3 ? 3 : 1)] = c * apm - sn * aqm;
          o[iq % (N == 3 ? 3 : 1)] = sn * apm + c * aqm;
        }
#pragma unroll
        for (int k = 0; k < N; k++) {
          const double vkp = v[k * N + p], vkq = v[k * N + q];
          v[k * N + p] = c * vkp - sn * vkq;
          v[k * N + q] = sn * vkp + c * vkq;
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < N; i++) w[i] = d[i];
  // ascending eigenvalues like LAPACK's dsyev (Matlib/LAPACK.c): the stress is order-invariant, but the
  // Drucker-Prager tangent moduli C_ep are stored per principal direction
#pragma unroll
  for (int i = 0; i < N - 1; i++)
#pragma unroll
    for (int j = 0; j < N - 1 - i; j++)
      if (w[j] > w[j + 1]) {
        double t = w[j];
        w[j] = w[j + 1];
        w[j + 1] = t;
#pragma unroll
        for (int k = 0; k < N; k++) {
          t = v[k * N + j];
          v[k * N + j] = v[k * N + j + 1];
          v[k * N + j + 1] = t;
        }
      }
}

template <int N>
__device__ __forceinline__ void left_cauchy_green(double* b, const double* F) {  // compute-Strains.c:365-384
  NLPS_FP_CONTRACT
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = 0; j < N; j++) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < N; k++) s += F[i * N + k] * F[j * N + k];
      b[i * N + j] = s;
    }
}

// sum_A T_A n_A (x) n_A with n_A = column A (Hencky.c:248-265; Drucker-Prager.c:755-776, 663-710)
template <int N>
__device__ __forceinline__ void ppal_to_xyz(double* T, const double* Tp, const double* v) {
  NLPS_FP_CONTRACT
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = 0; j < N; j++) {
      double s = 0.0;
#pragma unroll
      for (int A = 0; A < N; A++) s += Tp[A] * v[A + i * N] * v[A + j * N];
      T[i * N + j] = s;
    }
}

// ------------------------------------------------------------------------------------------------
// Kirchhoff-stress laws.  Tensors are passed as the d x d block t[N*N] plus the 2-D zz slot.
// ------------------------------------------------------------------------------------------------
template <int N>
struct StressIO {
  double tau[N * N];
  double tau_zz;  // 2-D slot 4
  double W;
  double be[N * N];
  double be_zz;
  double kappa, eps;
  double cep[N * N];  // elastoplastic tangent moduli in principal space (Drucker-Prager.c:1088-1198)
  double back[3];     // principal back stress (Von-Mises), in/out
  int fail;
  bool cep_keep;      // Matsuoka-Nakai / Lade-Duncan in 3-D after a plastic step: the stored C_ep is left alone
};

template <int N>
__device__ __forceinline__ void law_neo_hookean(const MatD& m, const double* F, double J, StressIO<N>& o) {
  NLPS_FP_CONTRACT
  double c0 = m.lame * 0.5 * (J * J - 1.0);
  double b[N * N];
  left_cauchy_green<N>(b, F);
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = 0; j < N; j++) {
      double Id = (i == j) ? 1.0 : 0.0;
      o.tau[i * N + j] = c0 * Id + m.G * (b[i * N + j] - Id);
    }
  o.tau_zz = c0;
  double I1 = 0.0;
#pragma unroll
  for (int i = 0; i < N; i++) I1 += b[i * N + i];
  double lj = log(J);
  double f_J = 0.25 * m.lame * (J * J - 1) - 0.5 * m.lame * lj - m.G * lj;
  o.W = f_J + 0.5 * m.G * (I1 - (double)N);
}

template <int N>
__device__ __forceinline__ void law_hencky(const MatD& m, const double* F, StressIO<N>& o) {
  NLPS_FP_CONTRACT
  double b[N * N], v[N * N], w[3] = {0.0, 0.0, 1.0};  // 2-D: third eigenvalue fixed at 1 (Hencky.c:48)
  left_cauchy_green<N>(b, F);
  sym_eigen<N>(w, v, b);
  double Eh[3], Tp[3];
#pragma unroll
  for (int a = 0; a < 3; a++) Eh[a] = 0.5 * log(w[a]);
  double d = m.lame + 2 * m.G;
  Tp[0] = d * Eh[0] + m.lame * Eh[1] + m.lame * Eh[2];
  Tp[1] = m.lame * Eh[0] + d * Eh[1] + m.lame * Eh[2];
  Tp[2] = m.lame * Eh[0] + m.lame * Eh[1] + d * Eh[2];
  ppal_to_xyz<N>(o.tau, Tp, v);
  o.tau_zz = Tp[2];
  o.W = 0.5 * (Tp[0] * Eh[0] + Tp[1] * Eh[1] + Tp[2] * Eh[2]);
  if (isnan(w[0]) || isnan(w[1])) o.fail = 1;
}

// Compressible Newtonian fluid, statement order of Fluid/Newtonian-Fluid.c:17-79: L = dt_F F^-1
// (spatial_velocity_gradient__Particles__, compute-Strains.c:249-341), E = sym L, Macdonald pressure.  As upstream: in 2-D
// the "trace" is E[0] + E[2], i.e. xx + yx (:59), and the out-of-plane entry is -pressure - (2/3) c0 trace (:74).  Writes
// neither W nor an internal variable.  L (when asked for) and E are left for the tangent.  false: F does not invert.
struct FluidCoef {
  double pressure, c0;
};
__device__ double pow_cold(double x, double y);  // (out of line, below: pow's registers stay out of the caller's budget)
__device__ __forceinline__ FluidCoef fluid_coefficients(const MatD& m, double J) {
  FluidCoef k;
  k.pressure = J * (m.p_ref + (m.K_fluid / m.n_macdonald) * (pow_cold(J, -m.n_macdonald) - 1.0));
  k.c0 = J * m.viscosity;
  return k;
}
template <int N>
__device__ __forceinline__ bool law_newtonian_fluid(const MatD& m, const double* F, const double* dFdt, double J, double* tau,
                                                    double& tau_zz, double* L_out = nullptr, double* E_out = nullptr) {
  NLPS_FP_CONTRACT
  double Fm1[N * N], L[N * N], E[N * N];
  if (!inverse<N>(Fm1, F)) return false;
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = 0; j < N; j++) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < N; k++) s += dFdt[i * N + k] * Fm1[k * N + j];
      L[i * N + j] = s;
    }
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = 0; j < N; j++) E[i * N + j] = 0.5 * (L[i * N + j] + L[j * N + i]);
  const FluidCoef k = fluid_coefficients(m, J);
  const double trace_E = (N == 2) ? E[0] + E[2] : E[0] + E[4 % (N * N)] + E[8 % (N * N)];
  const double dev = (2.0 / 3.0) * k.c0 * trace_E;
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = 0; j < N; j++) tau[i * N + j] = ((i == j) ? -k.pressure - dev : 0.0) + 2.0 * k.c0 * E[i * N + j];
  tau_zz = -k.pressure - dev;
  if (L_out) {
#pragma unroll
    for (int q = 0; q < N * N; q++) L_out[q] = L[q];
  }
  if (E_out) {
#pragma unroll
    for (int q = 0; q < N * N; q++) E_out[q] = E[q];
  }
  return true;
}

// Von-Mises (J2) plasticity with combined isotropic (linear + Voce) / kinematic hardening in principal Hencky
// strains, statement order of Von-Mises.c:212-392 (helpers :396-757); eigenvectors by column everywhere.
template <int N>
__device__ __forceinline__ void law_von_mises(const MatD& m, const ParamsD& prm, const double* d_phi, const double* b_e_n,
                                              double b_e_n_zz, double eps_n, StressIO<N>& o) {
  NLPS_FP_CONTRACT
  double btr[N * N], v[N * N], w[3] = {0, 0, 0};
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = 0; j < N; j++) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < N; k++)
#pragma unroll
        for (int l = 0; l < N; l++) s += d_phi[i * N + k] * b_e_n[k * N + l] * d_phi[j * N + l];
      btr[i * N + j] = s;
    }
  sym_eigen<N>(w, v, btr);
  if (N == 2) w[2] = b_e_n_zz;
  double Etr[3] = {0.5 * log(w[0]), 0.5 * log(w[1]), 0.5 * log(w[2])};
  const double K = m.K, G = m.G, sigma_y = m.kappa_0, H = m.H, theta = m.theta, K_0 = m.K_0, K_inf = m.K_inf,
               delta = m.delta;
  double n[3] = {0, 0, 0}, dEp[3] = {0, 0, 0}, Tp[3], Tvol[3], Tdev[3];
  double kappa_n[2], kappa_k[2], d_kappa_k[2];
  double PHI, PHI_0, d_PHI, J2, eps_k = eps_n, d_gamma_k = 0.0;
  const double TOL = prm.tol_radial;
  const int MaxIter = prm.max_iter_radial;
  int Iter = 0;
  o.eps = eps_n;
  const double Evol = (1.0 / 3.0) * (Etr[0] + Etr[1] + Etr[2]);
#pragma unroll
  for (int a = 0; a < 3; a++) {
    Tvol[a] = K * Evol;
    Tdev[a] = 2 * G * (Etr[a] - Evol) - o.back[a];
  }
  J2 = sqrt(Tdev[0] * Tdev[0] + Tdev[1] * Tdev[1] + Tdev[2] * Tdev[2]);
#define NLPS_VM_KAPPA(k, e)                                                         \
  {                                                                                 \
    if ((e) < 0.0) o.fail = 1;                                                      \
    (k)[0] = sigma_y + theta * H * (e) + (K_inf - K_0) * (1 - exp(-delta * (e)));   \
    (k)[1] = (1 - theta) * H * (e);                                                 \
  }
#define NLPS_VM_YIELD(kk, dg) (J2 - sqrt(2. / 3.) * ((kk)[0] + (kk)[1] - kappa_n[1]) - 2.0 * G * (dg))
  NLPS_VM_KAPPA(kappa_n, eps_n);
  PHI_0 = NLPS_VM_YIELD(kappa_n, d_gamma_k);
  kappa_k[0] = kappa_n[0];
  kappa_k[1] = kappa_n[1];
  if (PHI_0 <= 0.0) {
#pragma unroll
    for (int a = 0; a < 3; a++) Tp[a] = Tvol[a] + Tdev[a];
  } else {
#pragma unroll
    for (int a = 0; a < 3; a++) n[a] = Tdev[a] / J2;
    PHI = PHI_0;
    while (fabs(PHI / PHI_0) >= TOL) {
      Iter++;
      if (Iter == MaxIter) break;
      if (eps_k < 0.0) {
        o.fail = 1;
        break;
      }
      d_kappa_k[0] = theta * H + delta * (K_inf - K_0) * exp(-delta * eps_k);
      d_kappa_k[1] = (1 - theta) * H;
      d_PHI = -2.0 * G * (1.0 + (d_kappa_k[0] + d_kappa_k[1]) / (3 * G));
      d_gamma_k += -PHI / d_PHI;
      eps_k = eps_n + sqrt(2. / 3.) * d_gamma_k;
      NLPS_VM_KAPPA(kappa_k, eps_k);
      if (o.fail) break;
      PHI = NLPS_VM_YIELD(kappa_k, d_gamma_k);
    }
    const double d_K_kin = kappa_k[1] - kappa_n[1];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      Tp[a] = Tvol[a] + Tdev[a] + o.back[a] - d_gamma_k * 2 * G * n[a];
      dEp[a] = d_gamma_k * n[a];
    }
#pragma unroll
    for (int a = 0; a < 3; a++) o.back[a] += sqrt(2. / 3.) * d_K_kin * n[a];
    o.eps = eps_k;
  }
#undef NLPS_VM_KAPPA
#undef NLPS_VM_YIELD
  ppal_to_xyz<N>(o.tau, Tp, v);
  o.tau_zz = Tp[2];
  Etr[0] -= dEp[0];
  Etr[1] -= dEp[1];
  Etr[2] -= dEp[2];
  const double lam[3] = {exp(2 * Etr[0]), exp(2 * Etr[1]), exp(2 * Etr[2])};
  ppal_to_xyz<N>(o.be, lam, v);
  o.be_zz = lam[2];
  {  // __tangent_moduli :717-757
    double th = 0.0;
    if (J2 > NLPS_TOL_NR) th = 1.0 - 2.0 * G * d_gamma_k / J2;
    const double theta_bar = 1.0 / (1.0 + (kappa_k[0] + kappa_k[1]) / (3.0 * G)) - (1.0 - th);
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
      for (int j = 0; j < N; j++)
        o.cep[i * N + j] = K * 1.0 * 1.0 + 2.0 * G * th * ((i == j ? 1.0 : 0.0) - (1.0 / 3.0) * 1.0 * 1.0) -
                           2.0 * G * theta_bar * n[i] * n[j];
  }
  o.W = 0.5 * (Tp[0] * Etr[0] + Tp[1] * Etr[1] + Tp[2] * Etr[2]);
  if (isnan(w[0]) || isnan(w[1])) o.fail = 1;
}

// Drucker-Prager backward Euler in principal log-strain space.  Statement order follows
// Drucker-Prager.c:319-613 (elastic :410-432, classical return :457-530, apex return :532-590,
// corrector :593-610); eigenvectors by column everywhere.
// libm's pow as a real call: inlined, its register demand sets the allocation of the whole kernel and makes the HOT path
// spill around a branch that linear hardening (m = 1) never takes (Drucker-Prager K3 at three waves per SIMD: 51 scratch
// reloads sat inside the inlined pow, their stores at the head of the particle loop).
__device__ __attribute__((noinline)) double pow_cold(double x, double y) { return pow(x, y); }

template <int N>
__device__ __forceinline__ void law_drucker_prager(const MatD& m, const ParamsD& prm, const double* d_phi,
                                                   const double* b_e_n, double b_e_n_zz, double kappa_n,
                                                   double eps_n, StressIO<N>& o) {
  NLPS_FP_CONTRACT
  double btr[N * N], v[N * N], w[3] = {0, 0, 0};
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = 0; j < N; j++) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < N; k++)
#pragma unroll
        for (int l = 0; l < N; l++) s += d_phi[i * N + k] * b_e_n[k * N + l] * d_phi[j * N + l];
      btr[i * N + j] = s;
    }
  sym_eigen<N>(w, v, btr);
  if (N == 2) w[2] = b_e_n_zz;  // :655-657

  double Etr[3] = {0.5 * log(w[0]), 0.5 * log(w[1]), 0.5 * log(w[2])};
  const double K = m.K, G = m.G, p_ref = m.p_ref;
  const double alpha_F = m.alpha_F, alpha_Q = m.alpha_Q, beta = m.beta_dp;
  const double exp_param = m.exp_param, kappa_0 = m.kappa_0, eps_0 = m.eps_0;

  double n[3] = {0, 0, 0}, dEp[3] = {0, 0, 0}, Tp[3];
  double PHI, PHI_0, d_PHI;
  double d_gamma_k = 0.0;
  double eps_k = eps_n, kappa_k = kappa_n, d_kappa_k = 0.0;
  const double TOL = prm.tol_radial;
  const int MaxIter = prm.max_iter_radial;
  int Iter = 0;
  o.kappa = kappa_n;  // Constitutive.c:160-168: n+1 state starts from n
  o.eps = eps_n;

  double tr = Etr[0] + Etr[1] + Etr[2];
  double Evol = (1.0 / 3.0) * tr;
  double Tvol[3], Tdev[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    Tvol[a] = -p_ref - K * Evol;
    Tdev[a] = 2 * G * (Etr[a] - Evol);
  }
  double pressure = (Tvol[0] + Tvol[1] + Tvol[2]) / 3.0;
  double J2 = sqrt(Tdev[0] * Tdev[0] + Tdev[1] * Tdev[1] + Tdev[2] * Tdev[2]);

#define NLPS_YIELD(dg, kap) \
  (J2 - 2.0 * G * (dg)-3.0 * alpha_F * (pressure - 3.0 * K * alpha_Q * (dg)) - beta * (kap))

  PHI = PHI_0 = NLPS_YIELD(d_gamma_k, kappa_k);

  if (PHI_0 <= NLPS_TOL_NR) {
#pragma unroll
    for (int a = 0; a < 3; a++) Tp[a] = -Tvol[a] + Tdev[a];
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
      for (int j = 0; j < N; j++)
        o.cep[i * N + j] = (1.0 / 3.0) * K * 1.0 * 1.0 + 2.0 * G * ((i == j ? 1.0 : 0.0) - (1.0 / 3.0) * 1.0 * 1.0);
  } else {
    if (J2 > NLPS_TOL_NR) {
      n[0] = Tdev[0] / J2;
      n[1] = Tdev[1] / J2;
      n[2] = Tdev[2] / J2;
    }
    // Hardening law kappa = kappa_0 base^(1/m), kappa' = kappa_0 / (m eps_0) base^(1/m - 1) (Drucker-Prager.c:835-860).
    // m = 1 (linear hardening, the reference's own test values and BASELINE configs[4]): pow(x, 1) = x and pow(x, 0) = 1
    // exactly, so the branch below returns the bits of the two libm calls without making them -- three pow per yielding
    // particle and iterate otherwise, executed by every wave that holds one yielding lane.
    const bool linear_hardening = exp_param == 1.0;
    const double dk_coef = kappa_0 / (exp_param * eps_0);
    {
      double base = 1.0 + eps_n / eps_0;
      if (base < 0.0) o.fail = 1;
      d_kappa_k = linear_hardening ? dk_coef * 1.0 : dk_coef * pow_cold(base, 1.0 / exp_param - 1.0);
    }
    double ads = sqrt(1.0 + 3.0 * alpha_Q * alpha_Q);
    if (alpha_F == 0.0) o.fail = 1;
    double pressure_limit = 3.0 * alpha_Q * K / (2.0 * G) * J2 +
                            beta / (3.0 * alpha_F) * ((J2 / (2.0 * G)) * d_kappa_k * ads + kappa_k);
    if (-pressure < pressure_limit) {
      while (fabs(PHI / PHI_0) >= TOL) {
        Iter++;
        if (Iter == MaxIter) break;
        d_PHI = 9.0 * K * alpha_F * alpha_Q - 2.0 * G - beta * d_kappa_k * ads;
        if (fabs(d_PHI) < TOL) { o.fail = 1; break; }
        d_gamma_k += -PHI / d_PHI;
        if (d_gamma_k < 0.0) { o.fail = 1; break; }
        eps_k = eps_n + d_gamma_k * sqrt(3.0 * alpha_Q * alpha_Q + 1.0);
        if (eps_k < 0.0) { o.fail = 1; break; }
        double base = 1.0 + eps_k / eps_0;
        if (base < 0.0) { o.fail = 1; break; }
        kappa_k = linear_hardening ? kappa_0 * base : kappa_0 * pow_cold(base, 1.0 / exp_param);
        if (kappa_k < 0.0) { o.fail = 1; break; }
        d_kappa_k = linear_hardening ? dk_coef * 1.0 : dk_coef * pow_cold(base, 1.0 / exp_param - 1.0);
        PHI = NLPS_YIELD(d_gamma_k, kappa_k);
      }
#pragma unroll
      for (int a = 0; a < 3; a++) {
        Tp[a] = -Tvol[a] + Tdev[a] + d_gamma_k * (3 * K * alpha_Q - 2 * G * n[a]);
        dEp[a] = d_gamma_k * (alpha_Q + n[a]);
      }
      o.eps = eps_k;
      o.kappa = kappa_k;
      {
        const double c0 = 9 * alpha_F * alpha_Q * K + 2 * G + beta * d_kappa_k * sqrt(2. / 3. * (1 + 3 * alpha_Q * alpha_Q));
        const double c1 = 1.0 - 9.0 * alpha_F * alpha_Q * K / c0;
        double c2 = 0.0;
        if (J2 > NLPS_TOL_NR) c2 = d_gamma_k / J2;
#pragma unroll
        for (int i = 0; i < N; i++)
#pragma unroll
          for (int j = 0; j < N; j++)
            o.cep[i * N + j] = c1 * K * 1.0 * 1.0 +
                               2 * G * ((i == j ? 1.0 : 0.0) - (1. / 3.) * (1.0 - 2.0 * G * c2) * 1.0 * 1.0) -
                               (6.0 * alpha_Q * K * G / c0) * 1.0 * n[j] - (6.0 * alpha_Q * K * G / c0) * n[i] * 1.0 -
                               4 * G * G * (1.0 / c0 - c2) * n[i] * n[j];
      }
    } else {
      double d_gamma_1 = J2 / (2.0 * G);
      double d_gamma_2_k = 0.0;
      d_gamma_k = d_gamma_1 + d_gamma_2_k;
      while (fabs(PHI / PHI_0) >= TOL) {
        Iter++;
        if (Iter == MaxIter) break;
        double rt = sqrt((d_gamma_1 * d_gamma_1) + 3.0 * (alpha_Q * alpha_Q) * (d_gamma_k * d_gamma_k));
        d_PHI = 3.0 * alpha_Q * K + 3.0 * d_kappa_k * beta * (alpha_Q * alpha_Q) * d_gamma_k / (3.0 * alpha_F * rt);
        if (fabs(d_PHI) < TOL) break;
        d_gamma_2_k += -PHI / d_PHI;
        if (d_gamma_2_k < 0.0) {
          d_gamma_k = 0.0;
          d_gamma_2_k = 0.0;
          break;
        } else {
          d_gamma_k = d_gamma_1 + d_gamma_2_k;
        }
        PHI = (beta / (3.0 * alpha_F) *
                   (kappa_k + d_kappa_k * sqrt((d_gamma_1 * d_gamma_1) +
                                               3.0 * (alpha_Q * alpha_Q) * (d_gamma_k * d_gamma_k))) -
               pressure + 3.0 * K * alpha_Q * d_gamma_k);
      }
      eps_k = eps_n + d_gamma_k * sqrt(3.0 * alpha_Q * alpha_Q + 1.0);
      if (eps_k < 0.0) o.fail = 1;
#pragma unroll
      for (int a = 0; a < 3; a++) {
        Tp[a] = -Tvol[a] + d_gamma_k * 3 * K * alpha_Q;
        dEp[a] = d_gamma_k * alpha_Q + d_gamma_1 * n[a];
      }
      o.eps = eps_k;
      o.kappa = kappa_k;
      {
        double c0 = 0.0, c1 = 0.0;
        if (d_gamma_k > 0.0) {
          c0 = (alpha_Q * beta * sqrt(2. / 3.) * d_kappa_k * d_gamma_k) /
               (3.0 * alpha_F * K * sqrt(d_gamma_1 * d_gamma_1 + 3.0 * alpha_Q * alpha_Q * d_gamma_k * d_gamma_k) +
                alpha_Q * beta * sqrt(2. / 3.) * d_kappa_k * d_gamma_k);
          c1 = c0 * K / (2.0 * alpha_Q * G * d_gamma_k);
        }
#pragma unroll
        for (int i = 0; i < N; i++)
#pragma unroll
          for (int j = 0; j < N; j++) o.cep[i * N + j] = c0 * K * 1.0 * 1.0 + c1 * 1.0 * n[j];
      }
    }
  }
#undef NLPS_YIELD
  ppal_to_xyz<N>(o.tau, Tp, v);
  o.tau_zz = Tp[2];
  Etr[0] -= dEp[0];
  Etr[1] -= dEp[1];
  Etr[2] -= dEp[2];
  o.W = 0.5 * (Tp[0] * Etr[0] + Tp[1] * Etr[1] + Tp[2] * Etr[2]);
  double ev[3] = {exp(2 * Etr[0]), exp(2 * Etr[1]), exp(2 * Etr[2])};
  ppal_to_xyz<N>(o.be, ev, v);
  o.be_zz = ev[2];
  if (isnan(w[0]) || isnan(w[1]) || isnan(w[2])) o.fail = 1;
}

// ------------------------------------------------------------------------------------------------
// Matsuoka-Nakai / Lade-Duncan: the monolithic three-invariant return mapping with line search of
// Matsuoka-Nakai.c:300-700 and Lade-Duncan.c:290-692.  One routine for both: the files differ in the surfaces
// (Matsuoka-Nakai.c:961-1053 | Lade-Duncan.c:959-1035) and in which of E_trial / E_k1 the plastic branch overwrites
// (:432-434 | Lade-Duncan.c:430-432).  Kept as written upstream: the residual added to the diagonal of the 5 x 5 tangent
// (:505-510), the line search along the NEW residual (:583-587), b_e = 1 after an elastic step (E_hencky_k1 stays zero,
// :410-424 and :694), C_ep stored in 2-D only after a plastic step (:1285-1290).  Eigenvectors by column everywhere.
// ------------------------------------------------------------------------------------------------
struct FricInv {
  double I1, I2, I3;
  bool ld;
  __device__ __forceinline__ void set(const double* T) {
    I1 = T[0] + T[1] + T[2];
    I2 = T[0] * T[1] + T[1] * T[2] + T[0] * T[2];
    I3 = T[0] * T[1] * T[2];
  }
  __device__ __forceinline__ double K(double kap) const { return (ld ? 27.0 : 9.0) + kap; }
  __device__ __forceinline__ double F(double kappa_phi) const {
    return ld ? cbrt(K(kappa_phi) * I3) - I1 : cbrt(K(kappa_phi) * I3) - cbrt(I1 * I2);
  }
  __device__ __forceinline__ double grad_g(const double* T, int A) const {
    const double c = cbrt(I1 * I2);
    return (I1 * (I1 - T[A]) + I2) / (3.0 * (c * c));
  }
  __device__ __forceinline__ void dsurf(double* d, const double* T, double kap) const {
    const double c = cbrt(K(kap) * I3);
#pragma unroll
    for (int A = 0; A < 3; A++) d[A] = c / (3.0 * T[A]) - (ld ? 1.0 : grad_g(T, A));
  }
  __device__ __forceinline__ double dF_dkappa(double kappa_phi) const {
    const double c = cbrt(K(kappa_phi));
    return (1.0 / 3.0) * (1.0 / (c * c)) * cbrt(I3);
  }
  __device__ __forceinline__ void ddG(double* dd, const double* T, double kappa_psi) const {
    const double c = cbrt(K(kappa_psi) * I3), q = cbrt(I1 * I2);
    double g[3] = {0, 0, 0};
    if (!ld) {
#pragma unroll
      for (int A = 0; A < 3; A++) g[A] = grad_g(T, A);
    }
#pragma unroll
    for (int A = 0; A < 3; A++)
#pragma unroll
      for (int B = 0; B < 3; B++) {
        const double dAB = (A == B) ? 1.0 : 0.0;
        double v = (1.0 / 3.0) * c * (1.0 / (3.0 * T[A] * T[B]) - 1.0 * dAB / (T[A] * T[A]));
        if (!ld) v -= (1.0 / (q * q)) / 3.0 * (3.0 * I1 - T[A] - T[B] - I1 * dAB) - (2.0 / q) * g[A] * g[B];
        dd[A * 3 + B] = v;
      }
  }
  __device__ __forceinline__ void ddG_dkappa(double* d, const double* T, double kappa_psi) const {
    const double c3 = cbrt(I3), ck = cbrt(9.0 + kappa_psi);
#pragma unroll
    for (int A = 0; A < 3; A++) {
      d[A] = c3 / (3.0 * T[A]);
      if (!ld) d[A] = d[A] / (3.0 * (ck * ck));
    }
  }
};

// A x = b in place (row-major 5 x 5), partial pivoting on the first maximum like dgetrf; all indices static
__device__ __forceinline__ bool lu_solve5(double (&A)[25], double (&b)[5]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 5; k++) {
    int piv = k;
    double big = fabs(A[k * 5 + k]);
#pragma unroll
    for (int r = k + 1; r < 5; r++) {
      const double v = fabs(A[r * 5 + k]);
      if (v > big) {
        big = v;
        piv = r;
      }
    }
#pragma unroll
    for (int r = k + 1; r < 5; r++) {
      if (piv == r) {
#pragma unroll
        for (int c = 0; c < 5; c++) {
          const double t = A[k * 5 + c];
          A[k * 5 + c] = A[r * 5 + c];
          A[r * 5 + c] = t;
        }
        const double t = b[k];
        b[k] = b[r];
        b[r] = t;
      }
    }
    if (A[k * 5 + k] == 0.0) ok = false;
#pragma unroll
    for (int r = k + 1; r < 5; r++) {
      const double f = A[r * 5 + k] / A[k * 5 + k];
#pragma unroll
      for (int c = k + 1; c < 5; c++) A[r * 5 + c] -= f * A[k * 5 + c];
      b[r] -= f * b[k];
    }
  }
#pragma unroll
  for (int k = 4; k >= 0; k--) {
    double t = b[k];
#pragma unroll
    for (int c = k + 1; c < 5; c++) t -= A[k * 5 + c] * b[c];
    b[k] = t / A[k * 5 + k];
  }
  return ok;
}

// in place inverse of a 3 x 3 with partial pivoting (dgetrf_ + dgetri_, Matsuoka-Nakai.c:1241-1283)
__device__ __forceinline__ bool inverse3_pivot(double (&A)[9]) {
  double M[3][6];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      M[i][j] = A[i * 3 + j];
      M[i][3 + j] = (i == j) ? 1.0 : 0.0;
    }
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    int piv = k;
    {  // first maximum of column k among rows k..2 (static indices only)
      double big = fabs(M[k][k]);
#pragma unroll
      for (int r = k + 1; r < 3; r++) {
        const double v = fabs(M[r][k]);
        if (v > big) {
          big = v;
          piv = r;
        }
      }
    }
#pragma unroll
    for (int r = k + 1; r < 3; r++)
      if (piv == r) {
#pragma unroll
        for (int c = 0; c < 6; c++) {
          const double t = M[k][c];
          M[k][c] = M[r][c];
          M[r][c] = t;
        }
      }
    if (M[k][k] == 0.0) ok = false;
    const double d = M[k][k];
#pragma unroll
    for (int c = 0; c < 6; c++) M[k][c] /= d;
#pragma unroll
    for (int r = 0; r < 3; r++) {
      if (r == k) continue;
      const double f = M[r][k];
#pragma unroll
      for (int c = 0; c < 6; c++) M[r][c] -= f * M[k][c];
    }
  }
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) A[i * 3 + j] = M[i][3 + j];
  return ok;
}

template <int N>
__device__ __forceinline__ void law_frictional(const MatD& m, const ParamsD& prm, const double* d_phi, const double* b_e_n,
                                            double b_e_n_zz, double kappa_in, double eps_in, StressIO<N>& o) {
  double btr[N * N], v[N * N], w[3] = {0, 0, 0};
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = 0; j < N; j++) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < N; k++)
#pragma unroll
        for (int l = 0; l < N; l++) s += d_phi[i * N + k] * b_e_n[k * N + l] * d_phi[j * N + l];
      btr[i * N + j] = s;
    }
  sym_eigen<N>(w, v, btr);
  if (N == 2) w[2] = b_e_n_zz;
  double E_tr[3] = {0.5 * log(w[0]), 0.5 * log(w[1]), 0.5 * log(w[2])};
  double E_k1[3] = {0, 0, 0}, E_k2[3] = {0, 0, 0};
  FricInv s;
  s.ld = m.surface != 0;
  const double E = m.E, nu = m.nu, c_cotphi = m.c_cotphi, alpha = m.alpha_b;
  const double a0 = m.a_b[0], a1 = m.a_b[1], a2 = m.a_b[2];
  const double cd = 1.0 / E, co = -nu / E;                   // compliance CC (:799-810)
  const double sd = m.lame + 2 * m.G, so = m.lame;           // stiffness AA (:812-822)
#define NLPS_FRIC_E(Eo, Tk)                                                                        \
  {                                                                                                \
    const double t0_ = (Tk)[0] + c_cotphi, t1_ = (Tk)[1] + c_cotphi, t2_ = (Tk)[2] + c_cotphi;     \
    (Eo)[0] = cd * t0_ + co * t1_ + co * t2_;                                                      \
    (Eo)[1] = co * t0_ + cd * t1_ + co * t2_;                                                      \
    (Eo)[2] = co * t0_ + co * t1_ + cd * t2_;                                                      \
  }
#define NLPS_FRIC_KHAT(Lam) (a0 * (Lam)*exp(a1 * s.I1) * exp(-a2 * (Lam)))
#define NLPS_FRIC_RES(R, Ek, kph, khat, Fk, dl)                          \
  ((R)[0] = (Ek)[0] - E_tr[0] + (dl)*dG[0], (R)[1] = (Ek)[1] - E_tr[1] + (dl)*dG[1], \
   (R)[2] = (Ek)[2] - E_tr[2] + (dl)*dG[2], (R)[3] = (kph) - (khat), (R)[4] = (Fk),  \
   sqrt((R)[0] * (R)[0] + (R)[1] * (R)[1] + (R)[2] * (R)[2] + (R)[3] * (R)[3] + (R)[4] * (R)[4]))
#define NLPS_FRIC_APEX(Tk) (fabs(((Tk)[0] + (Tk)[1] + (Tk)[2]) / 3.0) < 0.1)
  const double Lambda_n = eps_in, kappa_n0 = kappa_in, kappa_n1 = alpha * kappa_in;
  const double TOL = prm.tol_radial;
  const int MaxIter_k1 = prm.max_iter_radial, MaxIter_k2 = 10 * prm.max_iter_radial;
  double T_tr[3], T_k1[3], T_k2[3] = {0, 0, 0};
  o.kappa = kappa_in;
  o.eps = eps_in;
  o.cep_keep = false;
  T_tr[0] = sd * E_tr[0] + so * E_tr[1] + so * E_tr[2] - c_cotphi;
  T_tr[1] = so * E_tr[0] + sd * E_tr[1] + so * E_tr[2] - c_cotphi;
  T_tr[2] = so * E_tr[0] + so * E_tr[1] + sd * E_tr[2] - c_cotphi;
  s.set(T_tr);
  const double F_0 = s.F(kappa_n0);
#pragma unroll
  for (int r = 0; r < 3; r++) T_k1[r] = T_tr[r];
  if (F_0 <= NLPS_TOL_NR) {
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
      for (int j = 0; j < N; j++) o.cep[i * N + j] = (i == j) ? sd : so;
  } else {
    double dG[3], ddG[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, R1[5], R2[5] = {0, 0, 0, 0, 0};
    double kappa_k1 = kappa_n0, kappa_k2 = 0.0, F_k1 = F_0, F_k2 = 0.0, dl1 = 0.0, dl2 = 0.0;
    double Lambda_k1 = Lambda_n, Lambda_k2 = 0.0, N1, N2 = 0.0, delta;
    NLPS_FRIC_E(E_k1, T_k1);
#pragma unroll
    for (int r = 0; r < 3; r++) {
      if (s.ld) E_k1[r] = E_tr[r];
      else E_tr[r] = E_k1[r];
    }
    double kappa_hat = NLPS_FRIC_KHAT(Lambda_n);
    s.dsurf(dG, T_tr, kappa_n1);
    const double N0 = NLPS_FRIC_RES(R1, E_k1, kappa_n0, kappa_hat, F_0, 0.0);
    N1 = N0;
    int Iter_k1 = 0;
#pragma unroll 1
    while ((fabs(N1 / N0) >= TOL) && (fabs(F_k1 / F_0) >= TOL)) {
      delta = 1.0;
      const double dkappa_ds = a0 * a1 * Lambda_k1 * exp(a1 * s.I1) * exp(-a2 * Lambda_k1);
      const double dkappa_dl = (1 - a2 * Lambda_k1) * a0 * exp(a1 * s.I1) * exp(-a2 * Lambda_k1);
      double dF[3], ddG_dk[3], TM[25];
      s.dsurf(dF, T_k1, kappa_k1);
      const double dF_dk = s.dF_dkappa(kappa_k1);
      s.ddG(ddG, T_k1, alpha * kappa_k1);
      s.ddG_dkappa(ddG_dk, T_k1, alpha * kappa_k1);
#pragma unroll
      for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) TM[r * 5 + c] = ((r == c) ? cd : co) + dl1 * ddG[r * 3 + c];
        TM[r * 5 + 3] = alpha * dl1 * ddG_dk[r];
        TM[r * 5 + 4] = dG[r];
        TM[15 + r] = -dkappa_ds;
        TM[20 + r] = dF[r];
      }
      TM[18] = 1.0;
      TM[19] = -dkappa_dl;
      TM[23] = dF_dk;
      TM[24] = 0.0;
#pragma unroll
      for (int r = 0; r < 5; r++) TM[r * 5 + r] += R1[r];
      if (!lu_solve5(TM, R1)) {
        o.fail = 1;
        break;
      }
      dl2 = dl1 - delta * R1[4];
      if (Lambda_n + dl2 < 0.0) break;
      Lambda_k2 = Lambda_n + dl2;
#pragma unroll
      for (int r = 0; r < 3; r++) T_k2[r] = T_k1[r] - delta * R1[r];
      kappa_k2 = kappa_k1 - delta * R1[3];
      if (NLPS_FRIC_APEX(T_k2)) break;
      int Iter_k2 = 0;
#define NLPS_FRIC_EVAL_K2()                                              \
  {                                                                      \
    s.set(T_k2);                                                         \
    NLPS_FRIC_E(E_k2, T_k2);                                             \
    kappa_hat = NLPS_FRIC_KHAT(Lambda_k2);                               \
    s.dsurf(dG, T_k2, alpha * kappa_k2);                                 \
    F_k2 = s.F(kappa_k2);                                                \
    N2 = NLPS_FRIC_RES(R2, E_k2, kappa_k2, kappa_hat, F_k2, dl2);        \
  }
      NLPS_FRIC_EVAL_K2();
#pragma unroll 1
      while ((fabs(N2 - N1) > TOL) && (fabs(F_k2 / F_0) >= TOL)) {
        delta = (delta * delta) * 0.5 * N1 / (N2 - delta * N1 + N1);
        if ((delta > 1.0) || (delta < 0.0)) break;
        dl2 = dl1 - delta * R2[4];
        if (Lambda_n + dl2 < 0.0) break;
        Lambda_k2 = Lambda_n + dl2;
#pragma unroll
        for (int r = 0; r < 3; r++) T_k2[r] = T_k1[r] - delta * R2[r];
        kappa_k2 = kappa_k1 - delta * R2[3];
        if (NLPS_FRIC_APEX(T_k2)) {
          Lambda_k2 = Lambda_n;
          kappa_k2 = kappa_n0;
          T_k2[0] = T_k2[1] = T_k2[2] = 0.0;
          break;
        }
        NLPS_FRIC_EVAL_K2();
        Iter_k2++;
        if (Iter_k2 == MaxIter_k2) break;
      }
#undef NLPS_FRIC_EVAL_K2
#pragma unroll
      for (int r = 0; r < 3; r++) {
        T_k1[r] = T_k2[r];
        E_k1[r] = E_k2[r];
      }
      kappa_k1 = kappa_k2;
      Lambda_k1 = Lambda_k2;
      F_k1 = F_k2;
      dl1 = dl2;
#pragma unroll
      for (int r = 0; r < 5; r++) R1[r] = R2[r];
      N1 = N2;
      Iter_k1++;
      if (NLPS_FRIC_APEX(T_k1)) {
        Lambda_k1 = Lambda_n;
        kappa_k1 = kappa_n0;
        T_k1[0] = T_k1[1] = T_k1[2] = 0.0;
        break;
      }
      if (Iter_k1 == MaxIter_k1) break;
    }
    o.eps = Lambda_k1;
    o.kappa = kappa_k1;
    {
      double aux[9];
#pragma unroll
      for (int q = 0; q < 9; q++) aux[q] = ((q % 4 == 0) ? cd : co) + dl1 * ddG[q];
      if (!inverse3_pivot(aux)) o.fail = 1;
      if (N == 2) {
        o.cep[0] = aux[0];
        o.cep[1] = aux[1];
        o.cep[2 % (N * N)] = aux[3];
        o.cep[3 % (N * N)] = aux[4];
      } else {
        o.cep_keep = true;
      }
    }
  }
#undef NLPS_FRIC_E
#undef NLPS_FRIC_KHAT
#undef NLPS_FRIC_RES
#undef NLPS_FRIC_APEX
  const double Tp[3] = {T_k1[0] + c_cotphi, T_k1[1] + c_cotphi, T_k1[2] + c_cotphi};
  ppal_to_xyz<N>(o.tau, Tp, v);
  o.tau_zz = Tp[2];
  const double lam[3] = {exp(2 * E_k1[0]), exp(2 * E_k1[1]), exp(2 * E_k1[2])};
  ppal_to_xyz<N>(o.be, lam, v);
  o.be_zz = lam[2];
  o.W = 0.5 * (Tp[0] * E_tr[0] + Tp[1] * E_tr[1] + Tp[2] * E_tr[2]);
  if (isnan(w[0]) || isnan(w[1]) || isnan(w[2])) o.fail = 1;
}

// exp() for the bounded LME exponents (|x| < 700, no NaN/Inf handling): n = rint(x log2 e),
// r = x - n ln2 (two-piece ln2), degree-13 Taylor on |r| <= 0.347 (truncation 4e-18), ldexp.
// ~20 instructions against ~45 for the general-purpose library routine; error < 1 ulp + 1e-17.
__device__ __forceinline__ double exp_bounded(double x) {
  const double L2E = 1.4426950408889634074, LN2H = 6.93147180369123816490e-01, LN2L = 1.90821492927058770002e-10;
  const double n = rint(x * L2E);
  double r = fma(-n, LN2H, x);
  r = fma(-n, LN2L, r);
  double p = 1.0 / 6227020800.0;
  p = fma(p, r, 1.0 / 479001600.0);
  p = fma(p, r, 1.0 / 39916800.0);
  p = fma(p, r, 1.0 / 3628800.0);
  p = fma(p, r, 1.0 / 362880.0);
  p = fma(p, r, 1.0 / 40320.0);
  p = fma(p, r, 1.0 / 5040.0);
  p = fma(p, r, 1.0 / 720.0);
  p = fma(p, r, 1.0 / 120.0);
  p = fma(p, r, 1.0 / 24.0);
  p = fma(p, r, 1.0 / 6.0);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return ldexp(p, (int)n);
}

// ------------------------------------------------------------------------------------------------
// Separable LME context of one particle (one lane).
// ------------------------------------------------------------------------------------------------
template <int ND>
struct Lme {
  static constexpr int KN = (ND == 3) ? 5 : 1;
  double lx[5], ly[5], lz[KN];  // l_a components per stencil offset: x_p - x_a
  double ex[5], ey[5], ez[KN];  // separable factors exp(-beta l^2 + lambda l)
  int ijk[3];                   // lattice index of I0
  int I0;
  u64 mlo, mhi;                 // neighbourhood mask, bit = i + 5*j + 25*k

  __device__ __forceinline__ bool on(int b) const {
    return b < 64 ? ((mlo >> b) & 1ull) : ((mhi >> (b - 64)) & 1ull);
  }

  // l_a = x_p - Coordinates[a], with Coordinates = origin + h*idx evaluated exactly like the host
  // mesh builder does (no FMA contraction: the file is compiled with -ffp-contract=off)
  __device__ __forceinline__ void geom(const GridD& g, const double* x, int I0_) {
    I0 = I0_;
    ijk[0] = I0_ % g.n[0];
    ijk[1] = (I0_ / g.n[0]) % g.n[1];
    ijk[2] = I0_ / (g.n[0] * g.n[1]);
#pragma unroll
    for (int i = 0; i < 5; i++) {
      lx[i] = x[0] - (g.o[0] + g.h * (double)(ijk[0] + i - 2));
      ly[i] = x[1] - (g.o[1] + g.h * (double)(ijk[1] + i - 2));
      if (ND == 3) lz[i % KN] = x[2 % ND] - (g.o[2] + g.h * (double)(ijk[2] + i - 2));
    }
  }

  // The 5 factors of one axis sit on a lattice line: with l_o = l_0 - h o (o = -2..2),
  //   f(o) = -beta l_o^2 + lambda l_o = f(0) + o h (2 beta l_0 - lambda) - o^2 beta h^2
  // so  E(o) = E(0) G^o Q^(o^2),  G = exp(h (2 beta l_0 - lambda)),  Q = exp(-beta h^2):
  // 3 exp per axis (E(0), G, 1/G) + one shared Q instead of 5 per axis.
  __device__ __forceinline__ void axis_factors(double* e, double l0, double lam, double beta, double h, double Q,
                                               double Q4) const {
    const double e0 = exp_bounded(fma(-beta * l0, l0, lam * l0));
    const double t = h * fma(2.0 * beta, l0, -lam);
    const double G = exp_bounded(t), Gi = exp_bounded(-t);
    const double e0q = e0 * Q, e0q4 = e0 * Q4;
    e[2] = e0;
    e[3] = e0q * G;
    e[1] = e0q * Gi;
    e[4] = e0q4 * (G * G);
    e[0] = e0q4 * (Gi * Gi);
  }
  __device__ __forceinline__ void factors(const double* lam, double beta, double h) {
  NLPS_FP_CONTRACT
    const double Q = exp_bounded(-beta * h * h), Q2 = Q * Q, Q4 = Q2 * Q2;
    axis_factors(ex, lx[2], lam[0], beta, h, Q, Q4);
    axis_factors(ey, ly[2], lam[1], beta, h, Q, Q4);
    if (ND == 3) {
      double e5[5];
      axis_factors(e5, lz[2 % KN], lam[2 % ND], beta, h, Q, Q4);
#pragma unroll
      for (int i = 0; i < 5; i++) ez[i % KN] = e5[i];
    }
  }

  __device__ __forceinline__ int node_offset(const GridD& g, int i, int j, int k) const {
    return (i - 2) + g.n[0] * ((j - 2) + (ND == 3 ? g.n[1] * (k - 2) : 0));
  }
};

// ------------------------------------------------------------------------------------------------
// Hierarchical (row -> plane -> total) evaluation.  The weights are separable, only the membership
// mask is not: the innermost loop over i touches three masked adds per member, everything that does
// not depend on i is applied once per (j,k) row, everything that only depends on k once per plane.
// ------------------------------------------------------------------------------------------------

// 25 membership bits of plane k (k may be a run-time, wave-uniform loop counter)
template <int ND>
__device__ __forceinline__ unsigned plane_bits(const Lme<ND>& c, int k) {
  const int s = 25 * k;
  u64 v;
  if (s == 0) v = c.mlo;
  else if (s < 64) v = (c.mlo >> s) | (c.mhi << (64 - s));
  else v = c.mhi >> (s - 64);
  return (unsigned)v & 0x1FFFFFFu;
}

// y/z factors and offsets as plain LOCAL arrays (not struct members: only those are promoted to
// registers): the (j,k) row loops are real loops whose wave-uniform counters index them through
// v_cndmask chains instead of scratch.
#define NLPS_YZ_LOCALS(c)                                         \
  double ey5[5], ly5[5], ez5[5], lz5[5];                          \
  _Pragma("unroll") for (int i_ = 0; i_ < 5; i_++) {              \
    ey5[i_] = (c).ey[i_];                                         \
    ly5[i_] = (c).ly[i_];                                         \
    ez5[i_] = (ND == 3) ? (c).ez[i_ % Lme<ND>::KN] : 1.0;         \
    lz5[i_] = (ND == 3) ? (c).lz[i_ % Lme<ND>::KN] : 0.0;         \
  }

// Weight of stencil member i of a row: e when bit i of `bits` is set, otherwise e with its high word cleared
// (one v_bfe_i32 + one v_and_b32 instead of a bit test and two v_cndmask).  What is left of a non-member is
// a denormal below 2^-1042; every sum it enters also holds members of relative weight >= TOL_zero (or is itself
// discarded), so no bit of any result changes with respect to an exact zero.
__device__ __forceinline__ double masked_weight(double e, unsigned bits, int i) {
  const int m = __builtin_amdgcn_sbfe((int)bits, (unsigned)i, 1u);
  return __hiloint2double(__double2hiint(e) & m, __double2loint(e));
}

// The five weights of a row in two vector instructions per member: the row's membership bits go to the top of a word,
// word + word shifts the next one into the carry (v_add_co_u32 writes the carry's lane mask to a scalar pair), and that
// pair is the condition of ONE v_cndmask_b32 on the high word.  The back end turns masked_weight's bfe + and into
// and + compare + select (three instructions): 125 members x (two Newton evaluations | gather + moments | the K5 gather)
// are 250 / 250 / 125 vector instructions per particle less in K2 / K3 / K5.
__device__ __forceinline__ double masked_weight_pop(double e, unsigned& b) {
  unsigned long long m;
  asm("v_add_co_u32 %0, %1, %0, %0" : "+v"(b), "=s"(m));
  const int hi = __builtin_amdgcn_inverse_ballot_w64(m) ? __double2hiint(e) : 0;
  return __hiloint2double(hi, __double2loint(e));
}
__device__ __forceinline__ void masked_row(double* m, const double* ex, unsigned bits) {
  unsigned b = bits << 27;  // bit 4 of the row first
#pragma unroll
  for (int i = 4; i >= 0; i--) m[i] = masked_weight_pop(ex[i], b);
}

// Membership test of the scatter loops in ONE vector instruction per stencil node: the 25 bits of a plane sit at the top
// of `b` (bit 24 of plane_bits at bit 31), b + b shifts the next one out into the carry, whose lane mask is the branch
// condition as it stands (v_add_co_u32 writes it to a scalar pair; inverse_ballot hands that pair to the branch without
// a compare).  Nodes therefore come in descending order, (j, i) = (4, 4) first.  The bit test it replaces was
// v_and_b32 + v_cmp_ne_u32: 125 vector instructions less per particle in each of the two scatter loops.
__device__ __forceinline__ bool pop_member(unsigned& b) {
  unsigned long long m;
  asm("v_add_co_u32 %0, %1, %0, %0" : "+v"(b), "=s"(m));
  return __builtin_amdgcn_inverse_ballot_w64(m);
}

// Z^-1, r = sum p l, J = sum p l(x)l - r(x)r  (LME.c:766-832) by rows and planes.
// The moments are accumulated in INDEX space: with l_x(i) = a_x - u h, u = i - 2 in {-2..2} (a = l of the
// centre node) the weights of a row are the small integers u and u^2, so a row costs 8 additions / FMAs on its 5
// masked factors instead of 4 per member; the conversion to moments of l is a handful of operations at the end:
//   sum e l_x = a_x M0 - h M1x ,  sum e l_x l_y = a_x a_y M0 - h (a_x M1y + a_y M1x) + h^2 M2xy .
template <int ND>
__device__ __forceinline__ void lme_moments_h(const Lme<ND>& c, double& Zinv, double* r, double* Jm) {
  NLPS_FP_CONTRACT
  NLPS_YZ_LOCALS(c);
  (void)ly5;
  (void)lz5;
  double M0 = 0.0, M1x = 0.0, M1y = 0.0, M1z = 0.0, M2xx = 0.0, M2xy = 0.0, M2xz = 0.0, M2yy = 0.0, M2yz = 0.0, M2zz = 0.0;
  // real (not unrolled) plane loop, unrolled rows: compact code, short live ranges (the unrolled plane loop spills)
#pragma unroll 1
  for (int k = 0; k < Lme<ND>::KN; k++) {
    const unsigned pb = plane_bits<ND>(c, k);
    double P00 = 0.0, P10 = 0.0, P20 = 0.0, P01 = 0.0, P11 = 0.0, P02 = 0.0;
#pragma unroll 5
    for (int j = 0; j < 5; j++) {
      const unsigned bits = (pb >> (5 * j)) & 31u;
      double mw[5];
      masked_row(mw, c.ex, bits);
      const double m0 = mw[0], m1 = mw[1], m2 = mw[2], m3 = mw[3], m4 = mw[4];
      const double s13 = m1 + m3, s04 = m0 + m4;
      const double A0 = m2 + s13 + s04;                  // sum e
      const double A1 = fma(2.0, m4 - m0, m3 - m1);      // sum e u
      const double A2 = fma(4.0, s04, s13);              // sum e u^2
      const double cj = (double)(j - 2);
      const double y0 = ey5[j], y1 = y0 * cj, y2 = y1 * cj;
      P00 = fma(y0, A0, P00);
      P10 = fma(y0, A1, P10);
      P20 = fma(y0, A2, P20);
      P01 = fma(y1, A0, P01);
      P11 = fma(y1, A1, P11);
      P02 = fma(y2, A0, P02);
    }
    if (ND == 3) {
      const double ck = (double)(k - 2);
      const double z0 = ez5[k], z1 = z0 * ck, z2 = z1 * ck;
      M0 = fma(z0, P00, M0);
      M1x = fma(z0, P10, M1x);
      M1y = fma(z0, P01, M1y);
      M1z = fma(z1, P00, M1z);
      M2xx = fma(z0, P20, M2xx);
      M2xy = fma(z0, P11, M2xy);
      M2xz = fma(z1, P10, M2xz);
      M2yy = fma(z0, P02, M2yy);
      M2yz = fma(z1, P01, M2yz);
      M2zz = fma(z2, P00, M2zz);
    } else {
      M0 = P00;
      M1x = P10;
      M1y = P01;
      M2xx = P20;
      M2xy = P11;
      M2yy = P02;
    }
  }
  Zinv = 1.0 / M0;
  // l = a - u h per axis (Lme::geom: lx[i] = x - (o + h (I0 + i - 2)), so a = lx[2] and h = lx[2] - lx[3])
  const double hx = c.lx[2] - c.lx[3];
  const double ax = c.lx[2], ay = c.ly[2], az = (ND == 3) ? c.lz[2 % Lme<ND>::KN] : 0.0;
  const double e1x = M1x * Zinv, e1y = M1y * Zinv, e1z = M1z * Zinv;  // <u>
  const double rx = ax - hx * e1x, ry = ay - hx * e1y, rz = az - hx * e1z;
  r[0] = rx;
  r[1] = ry;
  if (ND == 3) r[ND - 1] = rz;
  // J = <l l> - r r = h^2 (<u u> - <u><u>)   (the a-terms cancel identically)
  const double h2 = hx * hx;
  const double cxx = M2xx * Zinv - e1x * e1x, cxy = M2xy * Zinv - e1x * e1y, cyy = M2yy * Zinv - e1y * e1y;
  if (ND == 2) {
    Jm[0] = h2 * cxx;
    Jm[1] = Jm[2] = h2 * cxy;
    Jm[3] = h2 * cyy;
  } else {
    const double cxz = M2xz * Zinv - e1x * e1z, cyz = M2yz * Zinv - e1y * e1z, czz = M2zz * Zinv - e1z * e1z;
    Jm[0] = h2 * cxx;
    Jm[1] = Jm[3 % (ND * ND)] = h2 * cxy;
    Jm[2] = Jm[6 % (ND * ND)] = h2 * cxz;
    Jm[4 % (ND * ND)] = h2 * cyy;
    Jm[5 % (ND * ND)] = Jm[7 % (ND * ND)] = h2 * cyz;
    Jm[8 % (ND * ND)] = h2 * czz;
  }
}

// Largest t with fl(sqrt(t)) <= Ra: the reference's test `sqrt(|l|^2) <= Ra` (LME.c:1076,
// MatrixOp.c:895-920) is then exactly `|l|^2 <= t`, without 125 square roots per particle.
__device__ __forceinline__ double sqrt_threshold(double Ra) {
  double t = Ra * Ra;
  if (isinf(Ra) || isnan(t)) return Ra;
#pragma unroll 1
  for (int it = 0; it < 8 && sqrt(t) > Ra; it++) t = __longlong_as_double(__double_as_longlong(t) - 1);
#pragma unroll 1
  for (int it = 0; it < 8; it++) {
    double tn = __longlong_as_double(__double_as_longlong(t) + 1);
    if (sqrt(tn) <= Ra) t = tn;
    else break;
  }
  return t;
}

}  // namespace nlps
