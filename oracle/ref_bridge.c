/* ref_bridge.c -- flat-array entry points into the REFERENCE's own 2-D objects (oracle/_ref/libnlps_ref2d.so).
 *
 * TEST INFRASTRUCTURE ONLY.  This file is the project's own text.  It includes the reference's headers by -I at
 * compile time (like integration/nlps_glue.c) and is linked with the reference's unmodified sources of src/Matlib,
 * src/Nodes, src/Particles and src/Constitutive, compiled with -DUSE_PLAINSTRAIN by oracle/orc.py::build_ref().
 * Nothing of the reference is copied here.  It does three things:
 *   1. defines the globals of Globals.h those objects leave undefined, with setters;
 *   2. builds the reference's Matrix / ChainPtr / Particle / Mesh / Material values from flat arrays, calls ONE
 *      reference function per entry point and exposes the results;
 *   3. stands in for `parse` (InOutFun/Parser.c), which only the mesh readers call and nothing here reaches.
 * The reference exit()s on several failure paths: callers run this library in a child process (tests/ref.py).
 *
 * One cloud lives in the library at a time (ref_cloud_new); its fields are read and written in place through
 * ref_field().  Tensors are rows of 5 in 2-D (xx, xy, yx, yy, zz), like the reference's. */
#include <math.h>
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "Macros.h"
#include "Types.h"
#include "Globals.h"
#include "Matlib.h"
#include "Particles.h"
#include "Nodes/Shape-Functions.h"
#include "Nodes/LME.h"
#include "Nodes/Q4.h"
#include "Constitutive/Constitutive.h"

#if NumberDimensions != 2
#error "the reference bridge is 2-D only (the reference's 3-D TensorLib.c does not compile)"
#endif

#define ND 2
#define TW 5 /* tensor row width in 2-D */
#define CW 9 /* row width given to C_ep and Back_stress (the laws use the first 4 and 3) */

/* ---- 1. globals of Globals.h ---- */
char ShapeFunctionGP[MAXC] = "LME";
char wrapper_LME[MAXC] = "Newton-Raphson";
bool Driver_EigenErosion = false;
bool Driver_EigenSoftening = false;
double gamma_LME = 3.0;
double TOL_zero_LME = 1e-6;
double TOL_wrapper_LME = 1e-10;
int max_iter_LME = 10;
double TOL_Radial_Returning = 1e-14;
int Max_Iterations_Radial_Returning = 10;
int NumberDOF = ND;

#ifndef REF_HAVE_PARSER /* build_ref() links the reference's own InOutFun/Parser.c when it compiles alone */
int parse(char **out, char *text, char *separators) {
  (void)out, (void)text, (void)separators;
  fprintf(stderr, "ref_bridge: parse() is a stand-in, the readers are not on the path\n");
  exit(EXIT_FAILURE);
}
#endif

void ref_set_lme(double gamma, double tol_zero, double tol_wrapper, int max_iter) {
  gamma_LME = gamma;
  TOL_zero_LME = tol_zero;
  TOL_wrapper_LME = tol_wrapper;
  max_iter_LME = max_iter;
}

void ref_set_radial_returning(double tol, int max_it) {
  TOL_Radial_Returning = tol;
  Max_Iterations_Radial_Returning = max_it;
}

void ref_set_drivers(int erosion, int softening) {
  Driver_EigenErosion = erosion != 0;
  Driver_EigenSoftening = softening != 0;
}

/* ---- helpers ---- */
static Matrix mk(int rows, int cols) { /* zeroed, contiguous nV with row pointers nM */
  Matrix A;
  memset(&A, 0, sizeof(A));
  A.N_rows = rows;
  A.N_cols = cols;
  A.nV = (double *)calloc((size_t)rows * cols + 1, sizeof(double));
  A.nM = (double **)calloc((size_t)rows + 1, sizeof(double *));
  for (int i = 0; i < rows; i++) A.nM[i] = A.nV + (size_t)i * cols;
  return A;
}

static Matrix view(int rows, int cols, double *mem, double **rowbuf) {
  Matrix A;
  memset(&A, 0, sizeof(A));
  A.N_rows = rows;
  A.N_cols = cols;
  A.nV = mem;
  A.nM = rowbuf;
  for (int i = 0; i < rows; i++) rowbuf[i] = mem + (size_t)i * cols;
  return A;
}

/* chain whose walk order is v[0], v[1], ...: push__SetLib__ prepends */
static ChainPtr chain_of(const int *v, int n) {
  ChainPtr c = NULL;
  for (int a = n - 1; a >= 0; a--) push__SetLib__(&c, v[a]);
  return c;
}

static int chain_out(ChainPtr c, int *out, int cap) {
  int n = 0;
  for (; c != NULL; c = c->next) {
    if (n < cap) out[n] = c->Idx;
    n++;
  }
  return n;
}

/* ---- 2a. Matlib, batched over n matrices of 4 (row-major 2 x 2) ---- */
int ref_sym_eigen(int n, const double *A, double *w, double *V) {
  int st = 0;
  for (int k = 0; k < n; k++) {
    double A5[TW] = {A[4 * k], A[4 * k + 1], A[4 * k + 2], A[4 * k + 3], 0.0};
    double wk[3] = {0, 0, 0};
    st |= sym_eigen_analysis__TensorLib__(wk, &V[4 * k], A5);
    w[2 * k] = wk[0];
    w[2 * k + 1] = wk[1];
  }
  return st;
}

int ref_inverse(int n, const double *A, double *Am1_lapack, double *Am1_tensor) {
  int st = 0;
  for (int k = 0; k < n; k++) {
    double A5[TW] = {A[4 * k], A[4 * k + 1], A[4 * k + 2], A[4 * k + 3], 1.0};
    st |= compute_inverse__TensorLib__(&Am1_lapack[4 * k], A5);
    Tensor At = memory_to_tensor__TensorLib__(A5, 2);
    Tensor Bt = Inverse__TensorLib__(At);
    for (int i = 0; i < ND; i++)
      for (int j = 0; j < ND; j++) Am1_tensor[4 * k + i * ND + j] = Bt.N[i][j];
    free__TensorLib__(Bt);
  }
  return st;
}

void ref_rcond(int n, const double *A, double *out) {
  for (int k = 0; k < n; k++) out[k] = rcond__TensorLib__(&A[4 * k]);
}

/* ---- 2b. LME pointwise ---- */
double ref_beta_lme(double gamma, double h_avg) { return beta__LME__(gamma, h_avg); }

void ref_p_lme(int na, const double *l, const double *lambda, double beta, double *p) {
  double **rows = (double **)malloc(sizeof(double *) * (size_t)na);
  double *rl[ND];
  double lam[ND] = {lambda[0], lambda[1]};
  Matrix L = view(na, ND, (double *)l, rows);
  Matrix Lam = view(ND, 1, lam, rl);
  Matrix P = p__LME__(L, Lam, beta);
  memcpy(p, P.nV, sizeof(double) * (size_t)na);
  free__MatrixLib__(P);
  free(rows);
}

void ref_dp_lme(int na, const double *l, const double *p, double *dp) {
  double **rows = (double **)malloc(sizeof(double *) * (size_t)na);
  double *rp[1];
  Matrix L = view(na, ND, (double *)l, rows);
  Matrix P = view(1, na, (double *)p, rp);
  Matrix D = dp__LME__(L, P);
  for (int a = 0; a < na; a++)
    for (int i = 0; i < ND; i++) dp[a * ND + i] = D.nM[a][i];
  free__MatrixLib__(D);
  free(rows);
}

/* ---- 2c. one cloud: the reference's own Particle and Mesh ---- */
static Particle g_P;
static Mesh g_M;
static int g_np = 0, g_nnodes = 0, g_nelem = 0, g_nmat = 0;

typedef struct {
  const char *name;
  Matrix *m;   /* Matrix field */
  double **v;  /* or a plain double* field */
  int cols;
} field_t;

static field_t g_fields[40];
static int g_nfields = 0;

static void add_m(const char *name, Matrix *m, int cols) {
  *m = mk(g_np, cols);
  g_fields[g_nfields++] = (field_t){name, m, NULL, cols};
}

static void add_v(const char *name, double **v) {
  *v = (double *)calloc((size_t)g_np + 1, sizeof(double));
  g_fields[g_nfields++] = (field_t){name, NULL, v, 1};
}

int ref_cloud_new(int np, int nnodes, int nelem, int nmat) {
  memset(&g_P, 0, sizeof(g_P));
  memset(&g_M, 0, sizeof(g_M));
  g_np = np, g_nnodes = nnodes, g_nelem = nelem, g_nmat = nmat, g_nfields = 0;
  Fields *F = &g_P.Phi;
  g_P.NumGP = np;
  g_P.I0 = (int *)calloc((size_t)np, sizeof(int));
  g_P.Element_p = (int *)calloc((size_t)np, sizeof(int));
  g_P.NumberNodes = (int *)calloc((size_t)np, sizeof(int));
  g_P.ListNodes = (ChainPtr *)calloc((size_t)np, sizeof(ChainPtr));
  g_P.Beps = (ChainPtr *)calloc((size_t)np, sizeof(ChainPtr));
  g_P.MatIdx = (int *)calloc((size_t)np, sizeof(int));
  g_P.NumberMaterials = nmat;
  g_P.Mat = (Material *)calloc((size_t)nmat, sizeof(Material));
  add_m("x_GC", &F->x_GC, ND);
  add_m("dis", &F->dis, ND);
  add_m("Vol_0", &F->Vol_0, 1);
  add_m("mass", &F->mass, 1);
  add_m("Stress", &F->Stress, TW);
  add_m("F_n", &F->F_n, TW);
  add_m("F_n1", &F->F_n1, TW);
  add_m("DF", &F->DF, TW);
  add_m("dt_F_n", &F->dt_F_n, TW);
  add_m("dt_F_n1", &F->dt_F_n1, TW);
  add_m("dt_DF", &F->dt_DF, TW);
  add_m("J_n", &F->J_n, 1);
  add_m("J_n1", &F->J_n1, 1);
  add_m("b_e_n", &F->b_e_n, TW);
  add_m("b_e_n1", &F->b_e_n1, TW);
  add_m("C_ep", &F->C_ep, CW);
  add_m("Back_stress", &F->Back_stress, CW);
  add_m("lambda", &g_P.lambda, ND);
  add_m("Beta", &g_P.Beta, 1);
  add_v("W", &F->W);
  add_v("Damage_n", &F->Damage_n);
  add_v("Damage_n1", &F->Damage_n1);
  add_v("Strain_f_n", &F->Strain_f_n);
  add_v("Strain_f_n1", &F->Strain_f_n1);
  add_v("EPS_n", &F->EPS_n);
  add_v("EPS_n1", &F->EPS_n1);
  add_v("Kappa_n", &F->Kappa_n);
  add_v("Kappa_n1", &F->Kappa_n1);
  F->Status_particle = (bool *)calloc((size_t)np + 1, sizeof(bool));

  g_M.NumNodesMesh = nnodes;
  g_M.NumElemMesh = nelem;
  g_M.Coordinates = mk(nnodes, ND);
  g_M.NumNodesElem = (int *)calloc((size_t)nelem + 1, sizeof(int));
  g_M.Connectivity = (ChainPtr *)calloc((size_t)nelem + 1, sizeof(ChainPtr));
  g_M.NumNeighbour = (int *)calloc((size_t)nnodes, sizeof(int));
  g_M.NodeNeighbour = (ChainPtr *)calloc((size_t)nnodes, sizeof(ChainPtr));
  g_M.SizeNodalLocality_0 = (int *)calloc((size_t)nnodes, sizeof(int));
  g_M.SizeNodalLocality = (int *)calloc((size_t)nnodes, sizeof(int));
  g_M.NodalLocality_0 = (ChainPtr *)calloc((size_t)nnodes, sizeof(ChainPtr));
  g_M.NodalLocality = (ChainPtr *)calloc((size_t)nnodes, sizeof(ChainPtr));
  g_M.ActiveNode = (bool *)calloc((size_t)nnodes, sizeof(bool));
  g_M.BoundaryNode = (bool *)calloc((size_t)nnodes, sizeof(bool));
  g_M.h_avg = (double *)calloc((size_t)nnodes, sizeof(double));
  g_M.Num_Particles_Node = (int *)calloc((size_t)nnodes, sizeof(int));
  g_M.List_Particles_Node = (ChainPtr *)calloc((size_t)nnodes, sizeof(ChainPtr));
  g_M.Dimension = ND;
  g_M.Locking_Control_Fbar = false;
  strcpy(g_M.TypeElem, "Quadrilateral");
  g_M.N_ref = N__Q4__;
  g_M.dNdX = dN__Q4__;
  g_M.dNdX_ref = dN_Ref__Q4__;
  g_M.volume_Element = volume__Q4__;
  g_M.In_Out_Element = in_out__Q4__;
  return 0;
}

/* pointer to the storage of a particle field, [np][cols] */
double *ref_field(const char *name, int *cols) {
  for (int k = 0; k < g_nfields; k++)
    if (strcmp(g_fields[k].name, name) == 0) {
      if (cols) *cols = g_fields[k].cols;
      return g_fields[k].m ? g_fields[k].m->nV : *g_fields[k].v;
    }
  return NULL;
}

int *ref_ifield(const char *name) {
  if (strcmp(name, "I0") == 0) return g_P.I0;
  if (strcmp(name, "NumberNodes") == 0) return g_P.NumberNodes;
  if (strcmp(name, "MatIdx") == 0) return g_P.MatIdx;
  if (strcmp(name, "Element_p") == 0) return g_P.Element_p;
  return NULL;
}

/* Mesh tables from a lattice: element connectivity and both nodal localities arrive in CHAIN (walk) order */
void ref_mesh_fill(const double *coords, const int *elem, int nodes_per_elem, const int *r1_ptr, const int *r1,
                   const int *r2_ptr, const int *r2, const double *h_avg, double DeltaX) {
  memcpy(g_M.Coordinates.nV, coords, sizeof(double) * (size_t)g_nnodes * ND);
  for (int e = 0; e < g_nelem; e++) {
    g_M.NumNodesElem[e] = nodes_per_elem;
    g_M.Connectivity[e] = chain_of(&elem[(size_t)e * nodes_per_elem], nodes_per_elem);
  }
  for (int I = 0; I < g_nnodes; I++) {
    g_M.SizeNodalLocality_0[I] = r1_ptr[I + 1] - r1_ptr[I];
    g_M.NodalLocality_0[I] = chain_of(&r1[r1_ptr[I]], r1_ptr[I + 1] - r1_ptr[I]);
    g_M.SizeNodalLocality[I] = r2_ptr[I + 1] - r2_ptr[I];
    g_M.NodalLocality[I] = chain_of(&r2[r2_ptr[I]], r2_ptr[I + 1] - r2_ptr[I]);
    g_M.h_avg[I] = h_avg[I];
  }
  g_M.DeltaX = DeltaX;
}

/* params: E nu ReferencePressure Ceps Gf ft heps wcrit kappa_0 Hardening_modulus Plastic_Strain_0 Cohesion
 *         phi_Frictional psi_Frictional Exponent_Hardening_Ortiz K_0_Voce K_inf_Voce delta_Voce theta_Voce
 *         a_Borja[0..2] alpha_Borja atmospheric_pressure  (24 numbers) */
void ref_set_material(int idx, const char *type, const double *q) {
  Material *m = &g_P.Mat[idx];
  memset(m, 0, sizeof(*m));
  m->Id = idx;
  strncpy(m->Type, type, sizeof(m->Type) - 1);
  m->E = q[0], m->nu = q[1], m->ReferencePressure = q[2], m->Ceps = q[3], m->Gf = q[4], m->ft = q[5];
  m->heps = q[6], m->wcrit = q[7], m->kappa_0 = q[8], m->Hardening_modulus = q[9], m->Plastic_Strain_0 = q[10];
  m->Cohesion = q[11], m->phi_Frictional = q[12], m->psi_Frictional = q[13];
  m->Exponent_Hardening_Ortiz = q[14], m->K_0_Hardening_Voce = q[15], m->K_inf_Hardening_Voce = q[16];
  m->delta_Hardening_Voce = q[17], m->theta_Hardening_Voce = q[18];
  m->a_Hardening_Borja[0] = q[19], m->a_Hardening_Borja[1] = q[20], m->a_Hardening_Borja[2] = q[21];
  m->alpha_Hardening_Borja = q[22], m->atmospheric_pressure = q[23];
  m->Locking_Control_Fbar = false;
}

void ref_initialise_shapefun(void) { initialise_shapefun__MeshTools__(g_P, g_M); }

int ref_local_search(void) { return local_search__MeshTools__(g_P, g_M); }

/* ListNodes in chain order, NumberNodes, ActiveNode */
int ref_get_lists(int *list, int stride, int *active) {
  int worst = 0;
  for (int p = 0; p < g_np; p++) {
    int n = chain_out(g_P.ListNodes[p], &list[(size_t)p * stride], stride);
    if (n > worst) worst = n;
  }
  for (int I = 0; I < g_nnodes; I++) active[I] = g_M.ActiveNode[I] ? 1 : 0;
  return worst;
}

/* compute_N__MeshTools__ / compute_dN__MeshTools__ of every particle, rows of `stride` slots */
void ref_shape_functions(double *N, double *dN, int stride) {
  for (int p = 0; p < g_np; p++) {
    Element e = nodal_set__Particles__(p, g_P.ListNodes[p], g_P.NumberNodes[p]);
    Matrix Np = compute_N__MeshTools__(e, g_P, g_M);
    Matrix dNp = compute_dN__MeshTools__(e, g_P, g_M);
    for (int a = 0; a < e.NumberNodes && a < stride; a++) {
      N[(size_t)p * stride + a] = Np.nV[a];
      for (int i = 0; i < ND; i++) dN[((size_t)p * stride + a) * ND + i] = dNp.nM[a][i];
    }
    free__MatrixLib__(Np);
    free__MatrixLib__(dNp);
    free(e.Connectivity);
  }
}

/* The four functions of Particles/compute-Strains.c and I3__TensorLib__ per particle, on nodal increments given per
 * MESH node (dU[nnodes][2], dV likewise or NULL).  The gather by the particle's list and the loop are the bridge's. */
void ref_compatibility(const double *dU, const double *dV) {
  for (int p = 0; p < g_np; p++) {
    Element e = nodal_set__Particles__(p, g_P.ListNodes[p], g_P.NumberNodes[p]);
    Matrix g = compute_dN__MeshTools__(e, g_P, g_M);
    int nn = e.NumberNodes;
    double *Ua = (double *)malloc(sizeof(double) * (size_t)nn * ND);
    double *Va = (double *)malloc(sizeof(double) * (size_t)nn * ND);
    for (int a = 0; a < nn; a++)
      for (int i = 0; i < ND; i++) {
        Ua[a * ND + i] = dU[e.Connectivity[a] * ND + i];
        Va[a * ND + i] = dV ? dV[e.Connectivity[a] * ND + i] : 0.0;
      }
    Fields *F = &g_P.Phi;
    update_increment_Deformation_Gradient__Particles__(F->DF.nM[p], Ua, g.nV, (unsigned)nn);
    update_Deformation_Gradient_n1__Particles__(F->F_n1.nM[p], F->F_n.nM[p], F->DF.nM[p]);
    if (dV) {
      update_rate_increment_Deformation_Gradient__Particles__(F->dt_DF.nM[p], Va, g.nV, (unsigned)nn);
      update_rate_Deformation_Gradient_n1__Particles__(F->dt_F_n1.nM[p], F->dt_DF.nM[p], F->F_n.nM[p], F->DF.nM[p],
                                                       F->dt_F_n.nM[p]);
    }
    F->J_n1.nV[p] = I3__TensorLib__(F->F_n1.nM[p]);
    free(Ua);
    free(Va);
    free__MatrixLib__(g);
    free(e.Connectivity);
  }
}

/* Stress_integration__Constitutive__ per particle; status[p] = its return, failed[p] = Status_particle.  With a damage
 * driver on, a failed particle (Damage_n == 1) is left alone, as the driver's loop does (U-Newmark-beta.c:1218-1224:
 * that loop is the driver's, restated here). */
int ref_stress_integration(int *status, int *failed) {
  int st = 0;
  for (int p = 0; p < g_np; p++) {
    status[p] = 0;
    if ((Driver_EigenErosion || Driver_EigenSoftening) && g_P.Phi.Damage_n[p] == 1.0)
      g_P.Phi.W[p] = 0.0; /* :1221 */
    else
      status[p] = Stress_integration__Constitutive__(p, g_P, g_P.Mat[g_P.MatIdx[p]]);
    failed[p] = g_P.Phi.Status_particle[p] ? 1 : 0;
    st |= status[p];
  }
  return st;
}

/* Every pair (A, B) of particle p's list: the gradient of compute_dN__MeshTools__ pushed to n+1 by the reference's
 * push_forward_dN__MeshTools__ with the particle's DF, then stiffness_density__Constitutive__ per pair.  The pair
 * loop is the bridge's (the reference's lives inside the PETSc driver); Kd[nn][nn][4], gradients out as [nn][2]. */
int ref_particle_stiffness(int p, double alpha_4, double *Kd, double *dN_n, double *dN_n1) {
  int st = 0;
  Element e = nodal_set__Particles__(p, g_P.ListNodes[p], g_P.NumberNodes[p]);
  Matrix g0 = compute_dN__MeshTools__(e, g_P, g_M);
  int nn = e.NumberNodes;
  double *g1 = push_forward_dN__MeshTools__(g0.nV, g_P.Phi.DF.nM[p], (unsigned)nn, &st);
  if (st == EXIT_SUCCESS) {
    for (int A = 0; A < nn; A++)
      for (int B = 0; B < nn; B++)
        st |= stiffness_density__Constitutive__(p, &Kd[((size_t)A * nn + B) * 4], &g1[A * ND], &g1[B * ND],
                                                &g0.nV[A * ND], &g0.nV[B * ND], alpha_4, g_P, g_P.Mat[g_P.MatIdx[p]]);
    memcpy(dN_n, g0.nV, sizeof(double) * (size_t)nn * ND);
    memcpy(dN_n1, g1, sizeof(double) * (size_t)nn * ND);
  }
  free(g1);
  free__MatrixLib__(g0);
  free(e.Connectivity);
  return st;
}

/* ---- 2g. fracture ---- */
int ref_compute_beps(int initialize, int *beps_n, int *beps, int stride) {
  compute_Beps__Constitutive__(g_P, g_M, initialize != 0);
  int worst = 0;
  for (int p = 0; p < g_np; p++) {
    beps_n[p] = chain_out(g_P.Beps[p], &beps[(size_t)p * stride], stride);
    if (beps_n[p] > worst) worst = beps_n[p];
  }
  return worst;
}

/* Eigenerosion__Constitutive__ with the arguments its definition names (EigenErosion.c:29-33), per particle */
int ref_eigenerosion(double DeltaX) {
  int st = 0;
  Fields *F = &g_P.Phi;
  for (int p = 0; p < g_np; p++)
    st |= Eigenerosion__Constitutive__((unsigned)p, F->Damage_n, F->Damage_n1, F->W, F->J_n1.nV, F->Vol_0.nV,
                                       F->Stress.nM[p], g_P.Mat[g_P.MatIdx[p]], g_P.Beps[p], DeltaX);
  return st;
}

/* compute_damage__Constitutive__ per particle with Driver_EigenSoftening (-> eulerian_almansi__Particles__ and
 * Eigensoftening__Constitutive__), one particle after the other, each followed by the in-place scaling of its Kirchhoff
 * stress by (1 - Damage_n1[p]).  The loop and the scaling are the driver's (U-Newmark-beta.c:1313-1331), restated here:
 * a neighbour that came earlier in the loop is read already scaled. */
int ref_softening_hook(double DeltaX) {
  int st = 0;
  Fields *F = &g_P.Phi;
  for (int p = 0; p < g_np; p++) {
    st |= compute_damage__Constitutive__((unsigned)p, g_P, DeltaX);
    for (int i = 0; i < TW; i++) F->Stress.nM[p][i] *= (1.0 - F->Damage_n1[p]);
  }
  return st;
}
