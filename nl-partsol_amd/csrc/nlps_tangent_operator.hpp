// Matrix-free tangent of the implicit driver: y = K x and the d x d diagonal blocks of K without the assembled matrix
// (the MatShell counterpart of nlps_tangent_kernels.hpp; MATOP_MULT / MATOP_GET_DIAGONAL).
//
// Every block the assembly adds is bilinear in the particle's two LME gradients.  With gn_B the gradient of member B
// in the reference frame and g1_B = DF^-T gn_B, the assembly's phase B adds K_AB[i][j] = sum_kl g1_A[k] g1_B[l] D[k][l][i][j]
// (V0 folded in; Neo-Hookean D = V0 (c0 d_ki d_lj + c1 d_kj d_li + G d_ij (DF b_n DF^T)[l][k]), the spectral laws spD).
// Pulling DF^-1 into the tensor, Dh[m][n][i][j] = sum_kl DFm1[m][k] DFm1[n][l] D[k][l][i][j], gives one form for every law:
//   K_AB[i][j] = sum_mn gn_A[m] gn_B[n] Dh[m][n][i][j]
//   (K x)_A[i] = sum_m gn_A[m] T[m][i],  T[m][i] = sum_nj Dh[m][n][i][j] G[n][j],  G[n][j] = sum_B gn_B[n] x_B[j]
// G is the gather of the compatibility stage (grad dU), the scatter of T through gn_A is the internal-force scatter; B
// runs over the particle's members, which are exactly the pairs the assembly visits.
//
// k_tanop_setup writes Dh per particle, structure of arrays [d^4][np] (the apply reads it coalesced in tile order);
// k_tanop_apply and k_tanop_bdiag are tile-binned like kb_fint_tile: an LDS gather window of x in grid numbering, the
// LME factors regenerated in registers, an LDS accumulator window flushed with f64 atomics (run-to-run summation order
// may differ) or, in deterministic mode, copied to window slabs that k_slab_gather sums in a fixed order.  With gn_B = -N_B Jm1 l_B (l_B = x_B - x_p):
//   G = -Jm1 H,  H[b][j] = sum_B N_B l_B[b] x_B[j]     and     (K x)_A[i] = N_A sum_b l_A[b] Q[i][b],  Q = -(Jm1^T T)^T,
// so both ends are separable sums over the stencil rows.
#pragma once

// Dh of one particle, or zeros (no neighbourhood, or J / DF singular: flagged like the assembly's phase A)
static constexpr int TANOP_SETUP_NT = 64;
template <int ND>
__global__ __launch_bounds__(TANOP_SETUP_NT) void k_tanop_setup(PView P, GridD g, const MatD* __restrict__ mats,
                                                                double* __restrict__ Dh, int ld, int* __restrict__ gstatus,
                                                                double alpha4) {
  constexpr int E = ND * ND;
  __shared__ double sh_tanop[7 * E][TANOP_SETUP_NT];
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P.np) return;
  Lme<ND> c;
  double lam[ND], beta;
  bool ok = load_lme<ND>(P, g, p, c, lam, beta);  // (no neighbourhood: flagged by the search already)
  double Zinv, r[ND], J[E], Jm1[E], DF[E], Fi[E], zz;
  if (ok) {
    lme_moments_h<ND>(c, Zinv, r, J);
    load_block<ND>(P, F_DF, p, DF, zz);
    if (!inverse<ND>(Jm1, J) || !inverse<ND>(Fi, DF)) {
      atomicOr(&P.status[p], ST_NEWTON);
      atomicOr(gstatus, ST_NEWTON);
      ok = false;
    }
  }
  if (!ok) {
#pragma unroll
    for (int e = 0; e < E * E; e++) Dh[(size_t)e * ld + p] = 0.0;
    return;
  }
  const MatD m = mats[P.mat[p]];
  const double V0 = tangent_vol(P, p);
  if (m.type == NLPS_MAT_NEO_HOOKEAN) {
    // Dh = V0 (c0 Fi[m][i] Fi[n][j] + c1 Fi[m][j] Fi[n][i] + G d_ij b_n[n][m])   (Neo-Hookean.c:107-110; Fi DF = I)
    double Fn[E], bn[E];
    load_block<ND>(P, fFN(P), p, Fn, zz);
    left_cauchy_green<ND>(bn, Fn);
    const double Jp = PF(P, F_JN1, p), sqrJ = Jp * Jp;
    const double c0 = V0 * (m.lame * sqrJ), c1 = V0 * (m.G - 0.5 * m.lame * (sqrJ - 1)), cG = V0 * m.G;
#pragma unroll
    for (int mm = 0; mm < ND; mm++)
#pragma unroll
      for (int n = 0; n < ND; n++)
#pragma unroll
        for (int i = 0; i < ND; i++)
#pragma unroll
          for (int j = 0; j < ND; j++) {
            const double v = c0 * Fi[mm * ND + i] * Fi[n * ND + j] + c1 * Fi[mm * ND + j] * Fi[n * ND + i] +
                             (i == j ? cG * bn[n * ND + mm] : 0.0);
            Dh[(size_t)(((mm * ND + n) * ND + i) * ND + j) * ld + p] = v;
          }
    return;
  }
  if (m.type == NLPS_KLAW_FLUID) {
    // Newtonian-Fluid.c:83-190 with a1 = DF^-T gn_A, b1 = DF^-T gn_B pulled into the tensor:
    // Dh = V0 ( -c1 Fi[m][i] Fi[n][j] + c2 Fi[m][j] Fi[n][i] + 2 c0 (E Fi^T)[i][m] Fi[n][j] - 2 c0 (E Fi^T)[i][n] Fi[m][j]
    //           + (alpha4 c0 d_ij - c0 L[i][j]) b_n[n][m] - c0 Fi[n][i] (Fi L)[m][j] + 2/3 c0 Fi[m][i] (Fi L)[n][j] )
    double Fn[E], bn[E], F1[E], dF1[E], tau[E], tzz, L[E], Es[E];
    load_block<ND>(P, fFN(P), p, Fn, zz);
    left_cauchy_green<ND>(bn, Fn);
    load_block<ND>(P, fFN1(P), p, F1, zz);
    load_block<ND>(P, F_DTFN1, p, dF1, zz);
    const double Jp = PF(P, F_JN1, p);
    if (!law_newtonian_fluid<ND>(m, F1, dF1, Jp, tau, tzz, L, Es)) {
      atomicOr(&P.status[p], ST_CONSTITUTIVE);
      atomicOr(gstatus, ST_CONSTITUTIVE);
#pragma unroll
      for (int e = 0; e < E * E; e++) Dh[(size_t)e * ld + p] = 0.0;
      return;
    }
    const FluidCoef k = fluid_coefficients(m, Jp);
    const double dp = -m.K_fluid * pow(Jp, 1.0 - m.n_macdonald);  // :109
    const double c0 = k.c0, c1 = k.pressure + dp + (2.0 / 3.0) * alpha4 * c0, c2 = k.pressure + alpha4 * c0;
    double EFt[E], FL[E];
#pragma unroll
    for (int a = 0; a < ND; a++)
#pragma unroll
      for (int b = 0; b < ND; b++) {
        double u = 0.0, v = 0.0;
#pragma unroll
        for (int q = 0; q < ND; q++) {
          u = fma(Es[a * ND + q], Fi[b * ND + q], u);
          v = fma(Fi[a * ND + q], L[q * ND + b], v);
        }
        EFt[a * ND + b] = u;
        FL[a * ND + b] = v;
      }
#pragma unroll
    for (int mm = 0; mm < ND; mm++)
#pragma unroll
      for (int n = 0; n < ND; n++)
#pragma unroll
        for (int i = 0; i < ND; i++)
#pragma unroll
          for (int j = 0; j < ND; j++) {
            const double v = -c1 * Fi[mm * ND + i] * Fi[n * ND + j] + c2 * Fi[mm * ND + j] * Fi[n * ND + i] +
                             2.0 * c0 * (EFt[i * ND + mm] * Fi[n * ND + j] - EFt[i * ND + n] * Fi[mm * ND + j]) +
                             ((i == j ? alpha4 * c0 : 0.0) - c0 * L[i * ND + j]) * bn[n * ND + mm] -
                             c0 * Fi[n * ND + i] * FL[mm * ND + j] + (2.0 / 3.0) * c0 * Fi[mm * ND + i] * FL[n * ND + j];
            Dh[(size_t)(((mm * ND + n) * ND + i) * ND + j) * ld + p] = V0 * v;
          }
    return;
  }
  // spectral laws: the tensor of the assembly's phase A (Hencky.c:98-229, Elastoplastic-Tangent-Matrix.c:42-163),
  //   D[k][l][i][j] = V0 ( -d_kj tau_il + sum_AB C_AB N_kA N_lB N_iA N_jB
  //                        + sum_{A != B, |lam_B - lam_A| > 1e-14} hq_AB (lam_A N_lA N_kB N_iA N_jB + lam_B N_kB N_lB N_iA N_jA) ),
  // pulled back with U_A = DF^-1 N_A (k, l -> m, n):
  //   Dh[m][n][i][j] = V0 ( -Fi[m][j] (Fi tau^T)[n][i] + sum_AB C_AB U_A[m] U_B[n] N_iA N_jB
  //                         + Y_AB U_B[m] N_jB U_A[n] N_iA + Z_AB U_B[m] U_B[n] N_iA N_jA ),  Y_AB = hq_AB lam_A, Z_AB = hq_AB lam_B.
  // The 7 d^2 per-particle factors wait in LDS (one column per lane, read back by the lane itself), so that the 81
  // outputs are a run-time loop (fully unrolled, the 3-D kernel held them all in registers and spilled 756 bytes)
  double bmat[E], tau[E], lamb[3] = {0, 0, 0}, tauv[3] = {0, 0, 0}, nv[E], tv[E], Cm[E];
  load_block<ND>(P, F_TAU, p, tau, zz);
  if (m.type == NLPS_MAT_HENCKY) {
    double F1[E];
    load_block<ND>(P, fFN1(P), p, F1, zz);
    left_cauchy_green<ND>(bmat, F1);
#pragma unroll
    for (int i = 0; i < ND; i++)
#pragma unroll
      for (int j = 0; j < ND; j++) Cm[i * ND + j] = m.lame + (i == j ? 2 * m.G : 0.0);
  } else {
    load_block<ND>(P, fBEN1(P), p, bmat, zz);
#pragma unroll
    for (int q = 0; q < E; q++) Cm[q] = PF(P, F_CEP + q, p);
  }
  sym_eigen<ND>(lamb, nv, bmat);
  sym_eigen<ND>(tauv, tv, tau);
  double* const U = &sh_tanop[0][threadIdx.x];  // [A][m], stride TANOP_SETUP_NT
  double* const Nv = U + E * TANOP_SETUP_NT;     // [A][i]
  double* const Cs = Nv + E * TANOP_SETUP_NT;    // [A][B]
  double* const Ys = Cs + E * TANOP_SETUP_NT;
  double* const Zs = Ys + E * TANOP_SETUP_NT;
  double* const Ft = Zs + E * TANOP_SETUP_NT;    // [n][i] = sum_l Fi[n][l] tau[i][l]
  double* const Fs = Ft + E * TANOP_SETUP_NT;    // [m][j]
#define TS(arr, q) arr[(q) * TANOP_SETUP_NT]
#pragma unroll
  for (int A = 0; A < ND; A++)
#pragma unroll
    for (int a = 0; a < ND; a++) {
      double u = 0.0, f = 0.0;
#pragma unroll
      for (int k = 0; k < ND; k++) {
        u = fma(Fi[a * ND + k], nv[A + k * ND], u);
        f = fma(Fi[A * ND + k], tau[a * ND + k], f);
      }
      TS(U, A * ND + a) = u;
      TS(Nv, A * ND + a) = nv[A + a * ND];
      TS(Ft, A * ND + a) = f;
      TS(Fs, A * ND + a) = Fi[A * ND + a];
      TS(Cs, A * ND + a) = Cm[A * ND + a];
      const int B = a;
      const double dl = lamb[B] - lamb[A];
      const bool on = A != B && fabs(dl) > 1E-14;
      const double hq = on ? 0.5 * ((tauv[B] - tauv[A]) / dl) : 0.0;
      TS(Ys, A * ND + B) = hq * lamb[A];
      TS(Zs, A * ND + B) = hq * lamb[B];
    }
#pragma unroll 1
  for (int e4 = 0; e4 < E * E; e4++) {
    const int j = e4 % ND, i = (e4 / ND) % ND, n = (e4 / E) % ND, mm = e4 / (E * ND);
    double v = -TS(Fs, mm * ND + j) * TS(Ft, n * ND + i);
#pragma unroll
    for (int A = 0; A < ND; A++) {
      const double UAm = TS(U, A * ND + mm), UAn = TS(U, A * ND + n), NAi = TS(Nv, A * ND + i), NAj = TS(Nv, A * ND + j);
#pragma unroll
      for (int B = 0; B < ND; B++) {
        const double UBm = TS(U, B * ND + mm), UBn = TS(U, B * ND + n), NBj = TS(Nv, B * ND + j);
        v = fma(TS(Cs, A * ND + B) * UAm * UBn, NAi * NBj, v);
        v = fma(TS(Ys, A * ND + B) * UBm * NBj, UAn * NAi, v);
        v = fma(TS(Zs, A * ND + B) * UBm * UBn, NAi * NAj, v);
      }
    }
    Dh[(size_t)e4 * ld + p] = V0 * v;
  }
#undef TS
}

// y_grid += K x_grid over the particles of one tile (x: grid numbering [nnodes][d], Dirichlet dofs already zeroed)
// NT = 64 (here and in k_tanop_bdiag): the deterministic form -- one wave per tile over the exact canonical list, the
// accumulator window copied to the tile's slab (window_to_slab), y_grid written by k_slab_gather; y is then unused
template <int ND, int NT = BLK>
__global__ __launch_bounds__(NT) void k_tanop_apply(PView P, GridD g, TileD td, const double* __restrict__ Dh, int ld,
                                                     const double* __restrict__ x, double* __restrict__ y) {
  constexpr int W = TileCfg<ND>::W, PS = TileCfg<ND>::PS, NW = TileCfg<ND>::NW, KN = Lme<ND>::KN, E = ND * ND;
  __shared__ double win[NW * ND];  // x of the window, node-major
  __shared__ double acc[ND * NW];  // (K x) of the window, field-major (kb_fint_tile's layout)
  TileWork tw;
  if (!tile_work_item(td, tw)) return;
  const int tile = tw.tile, cnt = td.count[tile];
  int w0[3];
  tile_origin<ND>(td, tile, w0);
  for (int idx = threadIdx.x; idx < NW; idx += NT) {
    bool in;
    const int node = window_node<ND>(g, w0, idx, in);
#pragma unroll
    for (int a = 0; a < ND; a++) {
      win[idx * ND + a] = in ? x[(size_t)node * ND + a] : 0.0;
      acc[a * NW + idx] = 0.0;
    }
  }
  __syncthreads();
  const int start = td.start[tile];
  for (int s = threadIdx.x; s < cnt; s += NT) {
    const int p = tile_list<NT>(td)[start + s];
    Lme<ND> c;
    double lam[ND], beta;
    if (!load_lme<ND>(P, g, p, c, lam, beta)) continue;
    double Zinv, r[ND], J[E], Jm1[E];
    lme_moments_h<ND>(c, Zinv, r, J);
    if (!inverse<ND>(Jm1, J)) continue;  // (flagged by the setup)
    const int base = window_base<ND>(c.ijk, w0);
    NLPS_YZ_LOCALS(c);
    // gather: H[b][a] = sum_B (N_B / Zinv) l_B[b] x_B[a]
    double H[E];
#pragma unroll
    for (int q = 0; q < E; q++) H[q] = 0.0;
#pragma unroll 1
    for (int k = 0; k < KN; k++) {
      const unsigned pb = plane_bits<ND>(c, k);
      const int basek = base + (ND == 3 ? PS * (k - 2) : 0);
#pragma unroll 1
      for (int j = 0; j < 5; j++) {
        const unsigned bits = (pb >> (5 * j)) & 31u;
        double S0[ND], S1[ND];
#pragma unroll
        for (int a = 0; a < ND; a++) S0[a] = S1[a] = 0.0;
#pragma unroll
        for (int i = 0; i < 5; i++)
          if ((bits >> i) & 1u) {
            const int li = basek + (i - 2) + W * (j - 2);
            const double e = c.ex[i], el = e * c.lx[i];
#pragma unroll
            for (int a = 0; a < ND; a++) {
              const double xv = win[li * ND + a];
              S0[a] = fma(e, xv, S0[a]);
              S1[a] = fma(el, xv, S1[a]);
            }
          }
        const double w = ey5[j] * ez5[k], wy = w * ly5[j], wz = w * lz5[k];
#pragma unroll
        for (int a = 0; a < ND; a++) {
          H[0 * ND + a] = fma(w, S1[a], H[0 * ND + a]);
          H[1 * ND + a] = fma(wy, S0[a], H[1 * ND + a]);
          if (ND == 3) H[(2 % ND) * ND + a] = fma(wz, S0[a], H[(2 % ND) * ND + a]);
        }
      }
    }
    // G[n][a] = -Zinv sum_b Jm1[n][b] H[b][a]
    double G[E];
#pragma unroll
    for (int n = 0; n < ND; n++)
#pragma unroll
      for (int a = 0; a < ND; a++) {
        double v = 0.0;
#pragma unroll
        for (int b = 0; b < ND; b++) v = fma(Jm1[n * ND + b], H[b * ND + a], v);
        G[n * ND + a] = -Zinv * v;
      }
    // T[m][i] = sum_nj Dh[m][n][i][j] G[n][j]  (all reads of the particle's Dh first)
    double T[E];
#pragma unroll
    for (int q = 0; q < E; q++) T[q] = 0.0;
#pragma unroll
    for (int mm = 0; mm < ND; mm++)
#pragma unroll
      for (int n = 0; n < ND; n++)
#pragma unroll
        for (int i = 0; i < ND; i++)
#pragma unroll
          for (int j = 0; j < ND; j++)
            T[mm * ND + i] = fma(Dh[(size_t)(((mm * ND + n) * ND + i) * ND + j) * ld + p], G[n * ND + j], T[mm * ND + i]);
    // Q[i][b] = -sum_m Jm1[m][b] T[m][i]: (K x)_A[i] = N_A sum_b l_A[b] Q[i][b]
    double Q[E];
#pragma unroll
    for (int i = 0; i < ND; i++)
#pragma unroll
      for (int b = 0; b < ND; b++) {
        double v = 0.0;
#pragma unroll
        for (int mm = 0; mm < ND; mm++) v = fma(Jm1[mm * ND + b], T[mm * ND + i], v);
        Q[i * ND + b] = -v;
      }
#pragma unroll 1
    for (int k = 0; k < KN; k++) {
      const unsigned pb = plane_bits<ND>(c, k);
      const int basek = base + (ND == 3 ? PS * (k - 2) : 0);
      const double wz = Zinv * ez5[k];
      const double lzk = lz5[k];
#pragma unroll 1
      for (int j = 0; j < 5; j++) {
        const unsigned bits = (pb >> (5 * j)) & 31u;
        const double w = wz * ey5[j];
        double cr[ND];
#pragma unroll
        for (int a = 0; a < ND; a++)
          cr[a] = (ND == 3) ? fma(Q[a * ND + 1], ly5[j], Q[a * ND + (2 % ND)] * lzk) : Q[a * ND + 1] * ly5[j];
#pragma unroll
        for (int i = 0; i < 5; i++)
          if ((bits >> i) & 1u) {
            const int li = basek + (i - 2) + W * (j - 2);
            const double we = w * c.ex[i];
#pragma unroll
            for (int a = 0; a < ND; a++) atomicAdd(&acc[a * NW + li], we * fma(Q[a * ND + 0], c.lx[i], cr[a]));
          }
      }
    }
  }
  __syncthreads();
  window_leave<ND, ND, NT>(g, td, tile, w0, acc, y);
}

// out_grid[A][i][j] += sum_p sum_mn gn_A[m] gn_A[n] Dh_p[m][n][i][j]: the diagonal blocks, d^2 accumulator fields per node
template <int ND, int NT = BLK>
__global__ __launch_bounds__(NT) void k_tanop_bdiag(PView P, GridD g, TileD td, const double* __restrict__ Dh, int ld,
                                                     double* __restrict__ out) {
  constexpr int W = TileCfg<ND>::W, PS = TileCfg<ND>::PS, NW = TileCfg<ND>::NW, KN = Lme<ND>::KN, E = ND * ND;
  __shared__ double acc[E * NW];
  TileWork tw;
  if (!tile_work_item(td, tw)) return;
  const int tile = tw.tile, cnt = td.count[tile];
  int w0[3];
  tile_origin<ND>(td, tile, w0);
  for (int idx = threadIdx.x; idx < NW * E; idx += NT) acc[idx] = 0.0;
  __syncthreads();
  const int start = td.start[tile];
  for (int s = threadIdx.x; s < cnt; s += NT) {
    const int p = tile_list<NT>(td)[start + s];
    Lme<ND> c;
    double lam[ND], beta;
    if (!load_lme<ND>(P, g, p, c, lam, beta)) continue;
    double Zinv, r[ND], J[E], Jm1[E];
    lme_moments_h<ND>(c, Zinv, r, J);
    if (!inverse<ND>(Jm1, J)) continue;
    // with gn_A[m] = -N_A sum_b Jm1[m][b] l_A[b] the block of member A is N_A^2 sum_bc l_b l_c Dt[b][c][i][j],
    // Dt[b][c][i][j] = sum_mn Jm1[m][b] Jm1[n][c] Dh[m][n][i][j]; kept as its d (d + 1) / 2 pairs b <= c (symmetrised)
    constexpr int NBC = ND * (ND + 1) / 2;
    double Dt[NBC * E];
#pragma unroll
    for (int ij = 0; ij < E; ij++) {
      double Dm[E], X[E];  // slice Dh[.][.][ij], then Jm1^T slice Jm1
#pragma unroll
      for (int mn = 0; mn < E; mn++) Dm[mn] = Dh[(size_t)(mn * E + ij) * ld + p];
#pragma unroll
      for (int b = 0; b < ND; b++)
#pragma unroll
        for (int n = 0; n < ND; n++) {
          double v = 0.0;
#pragma unroll
          for (int mm = 0; mm < ND; mm++) v = fma(Jm1[mm * ND + b], Dm[mm * ND + n], v);
          X[b * ND + n] = v;
        }
      int q = 0;
#pragma unroll
      for (int b = 0; b < ND; b++)
#pragma unroll
        for (int cc = b; cc < ND; cc++) {
          double v = 0.0, vt = 0.0;
#pragma unroll
          for (int n = 0; n < ND; n++) {
            v = fma(X[b * ND + n], Jm1[n * ND + cc], v);
            vt = fma(X[cc * ND + n], Jm1[n * ND + b], vt);
          }
          Dt[q * E + ij] = (b == cc) ? v : v + vt;
          q++;
        }
    }
    const int base = window_base<ND>(c.ijk, w0);
    NLPS_YZ_LOCALS(c);
#pragma unroll 1
    for (int k = 0; k < KN; k++) {
      const unsigned pb = plane_bits<ND>(c, k);
      const int basek = base + (ND == 3 ? PS * (k - 2) : 0);
      const double wz = Zinv * ez5[k];
#pragma unroll 1
      for (int j = 0; j < 5; j++) {
        const unsigned bits = (pb >> (5 * j)) & 31u;
        const double w = wz * ey5[j];
#pragma unroll
        for (int i = 0; i < 5; i++)
          if ((bits >> i) & 1u) {
            const int li = basek + (i - 2) + W * (j - 2);
            const double NA = w * c.ex[i];
            const double l[3] = {c.lx[i], ly5[j], lz5[k]};
            double lb[NBC];
            int q = 0;
#pragma unroll
            for (int b = 0; b < ND; b++)
#pragma unroll
              for (int cc = b; cc < ND; cc++) lb[q++] = NA * NA * l[b] * l[cc];
#pragma unroll
            for (int ij = 0; ij < E; ij++) {
              double v = 0.0;
#pragma unroll
              for (int t = 0; t < NBC; t++) v = fma(lb[t], Dt[t * E + ij], v);
              atomicAdd(&acc[ij * NW + li], v);
            }
          }
      }
    }
  }
  __syncthreads();
  window_leave<ND, E, NT>(g, td, tile, w0, acc, out);
}

// x (masked) -> grid numbering, the dofs fixed at the step of nlps_gpu_active_masks zeroed when d2m is given
template <int ND>
__global__ void k_tanop_expand(int nnodes, const int* __restrict__ n2m, const int* __restrict__ d2m, const double* __restrict__ x,
                               double* __restrict__ xg) {
  const int A = blockIdx.x * blockDim.x + threadIdx.x;
  if (A >= nnodes) return;
  const int m = n2m[A];
#pragma unroll
  for (int f = 0; f < ND; f++) {
    const size_t i = (size_t)m * ND + f;
    xg[(size_t)A * ND + f] = (m >= 0 && !(d2m && d2m[i] == -1)) ? x[i] : 0.0;
  }
}

// y = K x + alpha_1 M x on the free dofs, y = x on the fixed ones (identity rows, MatZeroRowsColumnsIS)
template <int ND>
__global__ void k_tanop_nodal(int nnodes, const int* __restrict__ n2m, const int* __restrict__ d2m, const double* __restrict__ yg,
                              const double* __restrict__ x, const double* __restrict__ aM, double* __restrict__ y) {
  const int A = blockIdx.x * blockDim.x + threadIdx.x;
  if (A >= nnodes) return;
  const int m = n2m[A];
  if (m < 0) return;
#pragma unroll
  for (int f = 0; f < ND; f++) {
    const size_t i = (size_t)m * ND + f;
    if (d2m && d2m[i] == -1) {
      y[i] = x[i];
      continue;
    }
    double v = yg[(size_t)A * ND + f];
    if (aM) v = fma(aM[i], x[i], v);
    y[i] = v;
  }
}

// the masked diagonal blocks, row-major, with alpha_1 M on their diagonal and the Dirichlet identity rows / columns
template <int ND>
__global__ void k_tanop_bdiag_nodal(int nnodes, const int* __restrict__ n2m, const int* __restrict__ d2m,
                                    const double* __restrict__ bg, const double* __restrict__ aM, double* __restrict__ blocks) {
  constexpr int E = ND * ND;
  const int A = blockIdx.x * blockDim.x + threadIdx.x;
  if (A >= nnodes) return;
  const int m = n2m[A];
  if (m < 0) return;
#pragma unroll
  for (int i = 0; i < ND; i++)
#pragma unroll
    for (int j = 0; j < ND; j++) {
      const size_t ri = (size_t)m * ND + i, cj = (size_t)m * ND + j;
      double v = bg[(size_t)A * E + i * ND + j];
      if (i == j && aM) v += aM[ri];
      if (d2m && (d2m[ri] == -1 || d2m[cj] == -1)) v = (i == j) ? 1.0 : 0.0;
      blocks[(size_t)m * E + i * ND + j] = v;
    }
}

// M <- alpha_1 * M, in place (the snapshot of the mass term)
__global__ void k_tanop_scale(size_t n, double a, double* M) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) M[i] = a * M[i];
}
