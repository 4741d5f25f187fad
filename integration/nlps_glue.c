/* nlps_glue.c — the reference-side binding of include/nlps_gpu.h.
 *
 * This file is meant to be dropped into nl-partsol/src/Formulations/Displacements/ and compiled WITH the
 * reference (it includes the reference's own headers; nothing of them is copied here).  It marshals the
 * reference's Particle / Mesh / Material / Boundaries structures (Types.h:14-797) into the plain-pointer
 * structures of the C-ABI, so that U-Newmark-beta.c / U-Static.c can replace their static stage functions by
 * the nlps_gpu_* calls listed in INTEGRATION.md.  It cannot be linked into the reference here (the reference needs
 * PETSc and LAPACK); tests/test_abi.py::test_glue_compiles_against_the_reference_headers compiles it to an object
 * against the real Types.h in both dimensions whenever the reference tree is present and checks the nlps_gpu_* symbols
 * it leaves undefined against the library's exports.
 *
 * Node numbering: the library indexes every nodal array in LATTICE numbering (x fastest).  A GiD box mesh may number
 * its nodes differently, so the glue keeps canon[file node] = lattice node (nlps_host_lattice_from_nodes) and maps
 * I0, the Dirichlet node lists, h_avg and Nodes2Mask through it, both ways.
 *
 *   cc -std=gnu99 [-DUSE_PLAINSTRAIN] -I<nl-partsol>/src -I<this repo>/include -c nlps_glue.c
 */
#include <math.h>
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "Macros.h"
#include "Types.h"
#include "Globals.h"

#include "nlps_gpu.h"

/* law ids of the C-ABI from Material.Type, the strings of Constitutive.c:28-258 */
static int nlps_glue_law(const Material *M) {
  if (strcmp(M->Type, "Neo-Hookean-Wriggers") == 0) return NLPS_MAT_NEO_HOOKEAN;
  if (strcmp(M->Type, "Hencky") == 0) return NLPS_MAT_HENCKY;
  if (strcmp(M->Type, "Drucker-Prager") == 0) return NLPS_MAT_DRUCKER_PRAGER;
  if (strcmp(M->Type, "Von-Mises") == 0) return NLPS_MAT_VON_MISES;
  if (strcmp(M->Type, "Matsuoka-Nakai") == 0) return NLPS_MAT_MATSUOKA_NAKAI;
  if (strcmp(M->Type, "Lade-Duncan") == 0) return NLPS_MAT_LADE_DUNCAN;
  if (strcmp(M->Type, "Newtonian-Fluid-Compressible") == 0) return NLPS_MAT_NEWTONIAN_FLUID;
  return -1;
}

/* what the binding keeps between calls */
typedef struct {
  nlps_gpu *gpu;
  int N;          /* FEM_Mesh.NumNodesMesh */
  int identity;   /* the mesh file already numbers its nodes x fastest */
  int *canon;     /* [N] file node -> lattice node */
  int *file_of;   /* [N] lattice node -> file node */
  int *I0_l;      /* [NumGP] closest nodes in lattice numbering (upload / download staging) */
  double *h_avg_l; /* [N] FEM_Mesh.h_avg in lattice numbering */
} nlps_glue;

void nlps_glue_free(nlps_glue *G) {
  if (G == NULL) return;
  if (G->gpu) nlps_gpu_destroy(G->gpu);
  free(G->canon);
  free(G->file_of);
  free(G->I0_l);
  free(G->h_avg_l);
  memset(G, 0, sizeof *G);
}

/* The GramsBox lattice behind FEM_Mesh.Coordinates: spacing, nodes per axis, origin and the node map.  Fails loudly
 * when the background mesh is not a structured lattice (such meshes stay on the CPU path). */
static int nlps_glue_lattice(nlps_glue *G, const Mesh *FEM_Mesh, nlps_grid *g) {
  const int Ndim = NumberDimensions;
  const int N = FEM_Mesh->NumNodesMesh;
  G->N = N;
  G->canon = (int *)malloc((size_t)N * sizeof(int));
  G->file_of = (int *)malloc((size_t)N * sizeof(int));
  G->h_avg_l = (double *)malloc((size_t)N * sizeof(double));
  if (G->canon == NULL || G->file_of == NULL || G->h_avg_l == NULL) return EXIT_FAILURE;
  memset(g, 0, sizeof *g);
  g->ndim = Ndim;
  /* Coordinates.nV is the contiguous [N][Ndim] storage of the Matrix (MatrixOp.c:128-181) */
  if (nlps_host_lattice_from_nodes(Ndim, N, FEM_Mesh->Coordinates.nV, &g->h, g->n, g->origin, G->canon) != 0) {
    fprintf(stderr, "" RED "nlps_glue: the background mesh is not a structured lattice: %s" RESET "\n",
            nlps_host_io_last_error());
    return EXIT_FAILURE;
  }
  G->identity = 1;
  for (int A = 0; A < N; A++) {
    if (G->canon[A] < 0 || G->canon[A] >= N) return EXIT_FAILURE;
    G->file_of[G->canon[A]] = A;
    G->identity &= (G->canon[A] == A);
    G->h_avg_l[G->canon[A]] = FEM_Mesh->h_avg[A];
  }
  g->h_avg = G->h_avg_l;
  return EXIT_SUCCESS;
}

/* The particle arrays the reference already owns (Matrix.nV is the contiguous row-major storage,
 * Matlib/MatrixOp.c:128-181). */
static nlps_particles nlps_glue_particles(Particle MPM_Mesh) {
  nlps_particles p;
  memset(&p, 0, sizeof p);
  p.np = MPM_Mesh.NumGP;
  p.x_GC = MPM_Mesh.Phi.x_GC.nV;
  p.dis = MPM_Mesh.Phi.dis.nV;
  p.vel = MPM_Mesh.Phi.vel.nV;
  p.acc = MPM_Mesh.Phi.acc.nV;
  p.F_n = MPM_Mesh.Phi.F_n.nV;
  p.F_n1 = MPM_Mesh.Phi.F_n1.nV;
  p.DF = MPM_Mesh.Phi.DF.nV;
  p.Stress = MPM_Mesh.Phi.Stress.nV;
  p.b_e_n = MPM_Mesh.Phi.b_e_n.nV;
  p.b_e_n1 = MPM_Mesh.Phi.b_e_n1.nV;
  p.J_n = MPM_Mesh.Phi.J_n.nV;
  p.J_n1 = MPM_Mesh.Phi.J_n1.nV;
  p.rho = MPM_Mesh.Phi.rho.nV;
  p.mass = MPM_Mesh.Phi.mass.nV;
  p.Vol_0 = MPM_Mesh.Phi.Vol_0.nV;
  p.W = MPM_Mesh.Phi.W;
  p.Kappa_n = MPM_Mesh.Phi.Kappa_n;
  p.Kappa_n1 = MPM_Mesh.Phi.Kappa_n1;
  p.EPS_n = MPM_Mesh.Phi.EPS_n;
  p.EPS_n1 = MPM_Mesh.Phi.EPS_n1;
  p.MatIdx = MPM_Mesh.MatIdx;
  p.I0 = MPM_Mesh.I0;
  p.lambda = MPM_Mesh.lambda.nV;
  p.Beta = MPM_Mesh.Beta.nV;
  p.dt_F_n = MPM_Mesh.Phi.dt_F_n.nV;
  p.dt_F_n1 = MPM_Mesh.Phi.dt_F_n1.nV;
  p.dt_DF = MPM_Mesh.Phi.dt_DF.nV;
  p.C_ep = MPM_Mesh.Phi.C_ep.nV;
  p.Back_stress = MPM_Mesh.Phi.Back_stress.nV;
  p.Damage_n = MPM_Mesh.Phi.Damage_n;
  p.Damage_n1 = MPM_Mesh.Phi.Damage_n1;
  p.Strain_f_n = MPM_Mesh.Phi.Strain_f_n;
  p.Strain_f_n1 = MPM_Mesh.Phi.Strain_f_n1;
  return p;
}

/* after initialise_shapefun__MeshTools__ (driver-nl-partsol.c:344): upload everything once */
int nlps_glue_create(nlps_glue *G, Mesh FEM_Mesh, Particle MPM_Mesh, Time_Int_Params Parameters_Solver) {
  nlps_grid g;
  memset(G, 0, sizeof *G);
  if (strcmp(wrapper_LME, "Newton-Raphson") != 0) { /* LME.c:97-101: Nelder-Mead also changes the initial lambda */
    fprintf(stderr, "" RED "nlps_glue: wrapper_LME = %s stays on the CPU path (the GPU path restates Newton-Raphson)" RESET "\n",
            wrapper_LME);
    return EXIT_FAILURE;
  }
  if (nlps_glue_lattice(G, &FEM_Mesh, &g) == EXIT_FAILURE) return EXIT_FAILURE;
  /* snapshot of the globals the level-A functions read implicitly (Globals.h:33-58) */
  nlps_params prm = {gamma_LME, TOL_zero_LME, TOL_wrapper_LME, max_iter_LME, TOL_Radial_Returning,
                     Max_Iterations_Radial_Returning, Driver_EigenErosion ? 1 : 0, Driver_EigenSoftening ? 1 : 0};
  const int Nmat = MPM_Mesh.NumberMaterials;
  nlps_material *mats = (nlps_material *)calloc((size_t)Nmat, sizeof(nlps_material));
  if (mats == NULL) return EXIT_FAILURE;
  for (int m = 0; m < Nmat; m++) {
    const Material *M = &MPM_Mesh.Mat[m];
    const int law = nlps_glue_law(M);
    if (law < 0) {
      fprintf(stderr, "" RED "nlps_glue: material %s stays on the CPU path" RESET "\n", M->Type);
      free(mats);
      return EXIT_FAILURE;
    }
    mats[m].type = law;
    mats[m].E = M->E;
    mats[m].nu = M->nu;
    mats[m].phi_deg = M->phi_Frictional;
    mats[m].psi_deg = M->psi_Frictional;
    mats[m].kappa_0 = M->kappa_0;
    mats[m].exponent_ortiz = M->Exponent_Hardening_Ortiz;
    mats[m].eps_0 = M->Plastic_Strain_0;
    mats[m].p_ref = M->ReferencePressure;
    mats[m].hardening_modulus = M->Hardening_modulus;
    mats[m].theta_voce = M->theta_Hardening_Voce;
    mats[m].K0_voce = M->K_0_Hardening_Voce;
    mats[m].Kinf_voce = M->K_inf_Hardening_Voce;
    mats[m].delta_voce = M->delta_Hardening_Voce;
    mats[m].Ceps = M->Ceps;
    mats[m].Gf = M->Gf;
    mats[m].ft = M->ft;
    mats[m].heps = M->heps;
    mats[m].wcrit = M->wcrit;
    mats[m].cohesion = M->Cohesion;
    mats[m].alpha_borja = M->alpha_Hardening_Borja;
    for (int k = 0; k < 3; k++) mats[m].a_borja[k] = M->a_Hardening_Borja[k];
    mats[m].viscosity = M->Viscosity;
    mats[m].compressibility = M->Compressibility;
    mats[m].n_macdonald = M->n_Macdonald_model;
  }
  nlps_particles p = nlps_glue_particles(MPM_Mesh);
  /* closest nodes in lattice numbering */
  G->I0_l = (int *)malloc((size_t)(p.np > 0 ? p.np : 1) * sizeof(int));
  if (G->I0_l == NULL) {
    free(mats);
    return EXIT_FAILURE;
  }
  for (int q = 0; q < p.np; q++) G->I0_l[q] = G->canon[MPM_Mesh.I0[q]];
  p.I0 = G->I0_l;
  const int STATUS = nlps_gpu_create(&G->gpu, &g, &prm, mats, Nmat, &p, Parameters_Solver.NumTimeStep, NULL);
  free(mats);
  if (STATUS != EXIT_SUCCESS) {
    fprintf(stderr, "" RED "%s" RESET "\n", G->gpu ? nlps_gpu_last_error(G->gpu) : "nlps_gpu_create");
    return STATUS;
  }
  /* a mesh file that is not numbered x-fastest: the masked numbering follows the FILE's node order (Nodes-Tools.c:46-66) */
  if (!G->identity && nlps_gpu_set_node_numbering(G->gpu, G->canon) != EXIT_SUCCESS) {
    fprintf(stderr, "" RED "%s" RESET "\n", nlps_gpu_last_error(G->gpu));
    return EXIT_FAILURE;
  }
  return STATUS;
}

/* FEM_Mesh.Bounds (Types.h:296-351) flattened to the value[k*NumTimeStep + t] layout of nlps_bcc, node lists in
 * lattice numbering.  The caller frees bcc[i].nodes, bcc[i].value and bcc. */
nlps_bcc *nlps_glue_boundaries(const nlps_glue *G, Mesh FEM_Mesh, int NumTimeStep, int *nbcc) {
  const int NumBounds = FEM_Mesh.Bounds.NumBounds;
  nlps_bcc *bcc = (nlps_bcc *)calloc((size_t)(NumBounds > 0 ? NumBounds : 1), sizeof(nlps_bcc));
  if (bcc == NULL) return NULL;
  for (int i = 0; i < NumBounds; i++) {
    const Load *L = &FEM_Mesh.Bounds.BCC_i[i];
    double *value = (double *)calloc((size_t)L->Dim * NumTimeStep, sizeof(double));
    if (value == NULL) return NULL;
    for (int k = 0; k < L->Dim; k++)
      for (int t = 0; t < NumTimeStep && t < L->Value[k].Num; t++) value[(size_t)k * NumTimeStep + t] = L->Value[k].Fx[t];
    int *nodes = (int *)malloc((size_t)(L->NumNodes > 0 ? L->NumNodes : 1) * sizeof(int));
    if (nodes == NULL) return NULL;
    for (int q = 0; q < L->NumNodes; q++) nodes[q] = G->canon[L->Nodes[q]];
    bcc[i].nnodes = L->NumNodes;
    bcc[i].nodes = nodes;
    bcc[i].dim = L->Dim;
    bcc[i].dir = L->Dir; /* Dir[k*NumTimeStep + t], Nodes-Tools.c:130 */
    bcc[i].value = value;
  }
  *nbcc = NumBounds;
  return bcc;
}

/* get_active_nodes__MeshTools__ + get_active_dofs__MeshTools__ (U-Newmark-beta.c:205-209): the Mask structures
 * the host still needs for the PETSc sizes.  Nodes2Mask arrays are malloc'd like the reference's (caller frees). */
int nlps_glue_masks(const nlps_glue *G, Mesh FEM_Mesh, const nlps_bcc *bcc, int nbcc, int TimeStep, Mask *ActiveNodes,
                    Mask *ActiveDOFs) {
  const int Ndim = NumberDimensions;
  nlps_gpu *GPU = G->gpu;
  int Nactivenodes = 0, Nfree = 0;
  ActiveNodes->Nodes2Mask = (int *)malloc((size_t)FEM_Mesh.NumNodesMesh * sizeof(int));
  ActiveDOFs->Nodes2Mask = (int *)malloc((size_t)FEM_Mesh.NumNodesMesh * Ndim * sizeof(int));
  if (ActiveNodes->Nodes2Mask == NULL || ActiveDOFs->Nodes2Mask == NULL) return EXIT_FAILURE;
  if (nlps_gpu_active_masks(GPU, bcc, nbcc, TimeStep, &Nactivenodes, &Nfree, ActiveNodes->Nodes2Mask,
                            ActiveDOFs->Nodes2Mask) != EXIT_SUCCESS) {
    fprintf(stderr, "" RED "%s" RESET "\n", nlps_gpu_last_error(GPU));
    return EXIT_FAILURE;
  }
  /* (for a mesh file that is not numbered x-fastest nlps_glue_create has handed the file's node order to the library,
   * nlps_gpu_set_node_numbering: Nodes2Mask arrives indexed by file node with the running index in file order, exactly
   * the array of get_active_nodes__MeshTools__, and the dof mask -- indexed by MASKED node, Nodes-Tools.c:96-135 -- with it) */
  ActiveNodes->Nactivenodes = Nactivenodes;
  ActiveDOFs->Nactivenodes = Nfree;
  return EXIT_SUCCESS;
}

/* before particle_results_vtk__InOutFun__ (U-Newmark-beta.c:409) or any host-side use of MPM_Mesh.Phi */
int nlps_glue_download(const nlps_glue *G, Particle MPM_Mesh) {
  nlps_particles p = nlps_glue_particles(MPM_Mesh);
  p.I0 = G->I0_l;
  const int STATUS = nlps_gpu_download_state(G->gpu, &p);
  if (STATUS != EXIT_SUCCESS) fprintf(stderr, "" RED "%s" RESET "\n", nlps_gpu_last_error(G->gpu));
  for (int q = 0; q < p.np && STATUS == EXIT_SUCCESS; q++) MPM_Mesh.I0[q] = G->file_of[G->I0_l[q]];
  return STATUS;
}

/* U-Static.c:1380-1470, __update_Particles(dU, MPM_Mesh, FEM_Mesh, ActiveNodes): the roll of the internal variables
 * and x_GC, dis += sum_A N_pA dU_A; the quasi-static driver has no velocities to update (NULL rate vectors). */
int nlps_glue_update_particles_static(const nlps_glue *G, const double *dU /* VecGetArrayRead(dU) */) {
  if (nlps_gpu_roll_state(G->gpu) != EXIT_SUCCESS || nlps_gpu_update_kinetics(G->gpu, 1.0, dU, NULL, NULL, NULL) != EXIT_SUCCESS) {
    fprintf(stderr, "" RED "%s" RESET "\n", nlps_gpu_last_error(G->gpu));
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}

/* U-Newmark-beta.c:970-1058, the body of __lagrangian_evaluation(snes, dU, Lagrangian, ctx) between its VecGetArray and
 * VecRestoreArray calls: the reference's
 *     VecZeroEntries(Lagrangian); dU_dt = __compute_nodal_velocity_increments(...);
 *     __local_compatibility_conditions(...); __constitutive_update(...); __nodal_internal_forces(...);
 *     __nodal_traction_forces(...); __nodal_inertial_forces(...);
 * becomes ONE library call.  The pointers are the driver's own (VecGetArray / VecGetArrayRead of Lagrangian, dU and of
 * ctx->Lumped_Mass, U_n_dt, U_n_dt2); alpha[6] = {alpha_1 .. alpha_6} of ctx->Time_Integration_Params (:497-514);
 * neumann[] = MPM_Mesh.Neumann_Contours flattened like the Dirichlet boundaries (nodes = particle indices);
 * first_evaluation_of_the_step != 0 for the first residual of a time step (the three vectors that do not change during
 * the SNES solve are then copied to the device, afterwards reused).  Returns EXIT_SUCCESS / EXIT_FAILURE like the static. */
int nlps_glue_lagrangian_evaluation(const nlps_glue *G, Particle MPM_Mesh, double *Lagrangian_ptr, const double *dU_ptr,
                                    const double *Un_dt_ptr, const double *Un_dt2_ptr, const double *Lumped_Mass_ptr,
                                    const double alpha[6], const double *gravity /* b of :1519-1557, or NULL */,
                                    const nlps_bcc *neumann, int nneumann, int TimeStep, int first_evaluation_of_the_step) {
#if NumberDimensions == 2
  const double thickness = Thickness_Plain_Stress;
  const double *area0 = NULL;
#else
  const double thickness = 1.0;
  const double *area0 = MPM_Mesh.Phi.Area_0.nV; /* :1440-1444 */
#endif
  const int flags = first_evaluation_of_the_step ? 0 : NLPS_LAGR_SAME_STEP;
  const int STATUS = nlps_gpu_lagrangian_evaluation(G->gpu, Lagrangian_ptr, dU_ptr, Un_dt_ptr, Un_dt2_ptr, Lumped_Mass_ptr, alpha,
                                                    gravity, neumann, nneumann, TimeStep, thickness, area0, flags);
  if (STATUS != EXIT_SUCCESS) fprintf(stderr, "" RED "%s" RESET "\n", nlps_gpu_last_error(G->gpu));
  return STATUS;
}

/* U-Static.c:492-551, the same callback of the quasi-static driver: no rate vectors, the inertial term is - M b
 * (:1005-1033).  The dynamic call with alpha = 0 gives exactly that (0 * dU - 0 * v - 0 * a - b); dU stands in for the
 * two rate vectors, which are multiplied by zero. */
int nlps_glue_lagrangian_evaluation_static(const nlps_glue *G, Particle MPM_Mesh, double *Lagrangian_ptr, const double *dU_ptr,
                                           const double *Lumped_Mass_ptr, const double *b /* gravity or NULL */,
                                           const nlps_bcc *neumann, int nneumann, int TimeStep) {
  static const double alpha0[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  return nlps_glue_lagrangian_evaluation(G, MPM_Mesh, Lagrangian_ptr, dU_ptr, dU_ptr, dU_ptr, Lumped_Mass_ptr, alpha0, b, neumann,
                                         nneumann, TimeStep, 1);
}

/* compute_Nodal_Nominal_traction_Forces (U-Verlet.c:805-902) of the explicit drivers: call once behind nlps_glue_create
 * (and again when the contours change); every nlps_gpu_explicit_step then adds Forces[A] += N_pA T A0_p of its TimeStep
 * behind the internal forces (:695).  neumann[] = MPM_Mesh.Neumann_Contours flattened as for nlps_glue_lagrangian_evaluation
 * (nodes = particle indices); the library copies it, the caller may free it afterwards.  nneumann = 0 removes the loads. */
int nlps_glue_set_explicit_loads(const nlps_glue *G, Particle MPM_Mesh, const nlps_bcc *neumann, int nneumann) {
#if NumberDimensions == 2
  const double thickness = Thickness_Plain_Stress;
  const double *area0 = NULL;
  (void)MPM_Mesh;
#else
  const double thickness = 1.0;
  const double *area0 = MPM_Mesh.Phi.Area_0.nV; /* :851-857 */
#endif
  const int STATUS = nlps_gpu_set_explicit_loads(G->gpu, neumann, nneumann, thickness, area0);
  if (STATUS != EXIT_SUCCESS) fprintf(stderr, "" RED "%s" RESET "\n", nlps_gpu_last_error(G->gpu));
  return STATUS;
}

/* F-bar of the explicit drivers on patches of block[] cells of the GramsBox lattice (the reference's own patches exist on
 * T6 / T10 meshes only): call once behind nlps_glue_create.  The flags come from the materials --
 * Mat[m].Locking_Control_Fbar switches a material in, Mat[m].alpha_Fbar is its alpha (Neo-Hookean.c:133-146,
 * Compressible-Newtonian-Fluid.c:107-118) -- and travel as the alpha array of nlps_fbar_cfg; Fbar_n / Jbar_n start as
 * F_n / J_n on the device.  No material with the flag: nothing is set (EXIT_SUCCESS). */
int nlps_glue_set_explicit_fbar(const nlps_glue *G, Particle MPM_Mesh, const int block[3]) {
  const int Nmat = MPM_Mesh.NumberMaterials;
  double *alpha = (double *)malloc((size_t)(Nmat > 0 ? Nmat : 1) * sizeof(double));
  if (alpha == NULL) return EXIT_FAILURE;
  int any = 0;
  for (int m = 0; m < Nmat; m++) {
    alpha[m] = MPM_Mesh.Mat[m].Locking_Control_Fbar ? MPM_Mesh.Mat[m].alpha_Fbar : -1.0;
    any |= MPM_Mesh.Mat[m].Locking_Control_Fbar ? 1 : 0;
  }
  int STATUS = EXIT_SUCCESS;
  if (any) {
    nlps_fbar_cfg cfg = {{block[0], block[1], block[2]}, alpha, NULL, NULL};
    STATUS = nlps_gpu_set_explicit_fbar(G->gpu, &cfg);
    if (STATUS != EXIT_SUCCESS) fprintf(stderr, "" RED "%s" RESET "\n", nlps_gpu_last_error(G->gpu));
  }
  free(alpha);
  return STATUS;
}

/* __jacobian_evaluation (U-Newmark-beta.c:1646-1830) as a MatShell instead of an assembled MATAIJ: the matrix-free
 * counterpart of nlps_gpu_tangent_assemble + nlps_gpu_tangent_coo.  Call it where the driver assembles the Jacobian
 * (the SNES Jacobian callback): it linearises at the state the last residual evaluation left, with alpha_1 M on the
 * diagonal (Lumped_Mass_ptr = VecGetArrayRead(ctx->Lumped_Mass)) and the Dirichlet dofs as identity rows / columns
 * (MatZeroRowsColumnsIS, :1822).  The operator stays fixed through the line-search trials that follow. */
int nlps_glue_tangent_operator(const nlps_glue *G, double alpha_1, const double *Lumped_Mass_ptr) {
  const int STATUS = nlps_gpu_tangent_operator(G->gpu, alpha_1, Lumped_Mass_ptr, 1, NULL);
  if (STATUS != EXIT_SUCCESS) fprintf(stderr, "" RED "%s" RESET "\n", nlps_gpu_last_error(G->gpu));
  return STATUS;
}

/* __create_sparsity_pattern + __jacobian_evaluation (U-Newmark-beta.c:1568-1830; the PCCHOLESKY / CHOLMOD branch of
 * U-Static.c:229-241) as the three arrays of MatCreateSeqAIJWithArrays(PETSC_COMM_SELF, n, n, *row_ptr, *cols, *vals, &K),
 * n = nactive * NumberDimensions: sorted CSR of the linearisation of the last nlps_glue_tangent_operator, assembled on the
 * device row by row without float atomics (it repeats bit for bit), columns ascending in every row.  The arrays are
 * malloc()ed here and belong to the caller (free() them after MatDestroy: the matrix does not copy them); *nnz = the
 * stored entries.  PetscInt must be a 32-bit int (the default configuration); nnz > INT_MAX is refused by the library. */
int nlps_glue_jacobian_csr(const nlps_glue *G, int nactive, int **row_ptr, int **cols, double **vals, long long *nnz) {
  long long n = 0;
  *row_ptr = NULL;
  *cols = NULL;
  *vals = NULL;
  int STATUS = nlps_gpu_tangent_csr_pattern(G->gpu, &n, NULL);
  if (STATUS == EXIT_SUCCESS) {
    *row_ptr = (int *)malloc(((size_t)nactive * NumberDimensions + 1) * sizeof(int));
    *cols = (int *)malloc((size_t)(n > 0 ? n : 1) * sizeof(int));
    *vals = (double *)malloc((size_t)(n > 0 ? n : 1) * sizeof(double));
    if (*row_ptr == NULL || *cols == NULL || *vals == NULL) {
      fprintf(stderr, "" RED "nlps_glue_jacobian_csr: out of memory for %lld entries" RESET "\n", n);
      STATUS = EXIT_FAILURE;
    } else {
      STATUS = nlps_gpu_tangent_csr(G->gpu, *row_ptr, *cols, *vals);
      if (STATUS != EXIT_SUCCESS) fprintf(stderr, "" RED "%s" RESET "\n", nlps_gpu_last_error(G->gpu));
    }
  } else {
    fprintf(stderr, "" RED "%s" RESET "\n", nlps_gpu_last_error(G->gpu));
  }
  if (STATUS != EXIT_SUCCESS) {
    free(*row_ptr);
    free(*cols);
    free(*vals);
    *row_ptr = NULL;
    *cols = NULL;
    *vals = NULL;
  }
  if (nnz) *nnz = n;
  return STATUS;
}

/* The same tangent as the three arrays of MatCreateSeqSBAIJWithArrays / MatCreateSeqBAIJWithArrays(PETSC_COMM_SELF, bs, n,
 * n, *brow_ptr, *bcols, *vals, &K) with bs = NumberDimensions, n = nactive * bs: block rows per masked node, bcols
 * ascending, every block in PETSc's column-major values(bs,bs,nblocks) (col_major = 1).  kind = NLPS_BSR_UPPER: the blocks
 * B >= A of a Neo-Hookean cloud's symmetric tangent, what the Cholesky factorisations and CHOLMOD take without the AIJ ->
 * SBAIJ conversion of every Newton iterate (refused by the library for a cloud of another law).  Ownership and
 * PetscInt as in nlps_glue_jacobian_csr; *nblocks = the stored blocks. */
static int nlps_glue_jacobian_blocks(const nlps_glue *G, int kind, const char *who, int nactive, int **brow_ptr, int **bcols,
                                     double **vals, long long *nblocks) {
  const size_t bs2 = (size_t)NumberDimensions * NumberDimensions;
  long long n = 0;
  *brow_ptr = NULL;
  *bcols = NULL;
  *vals = NULL;
  int STATUS = nlps_gpu_tangent_bsr_pattern(G->gpu, kind, &n, NULL);
  if (STATUS == EXIT_SUCCESS) {
    *brow_ptr = (int *)malloc(((size_t)nactive + 1) * sizeof(int));
    *bcols = (int *)malloc((size_t)(n > 0 ? n : 1) * sizeof(int));
    *vals = (double *)malloc((size_t)(n > 0 ? n : 1) * bs2 * sizeof(double));
    if (*brow_ptr == NULL || *bcols == NULL || *vals == NULL) {
      fprintf(stderr, "" RED "%s: out of memory for %lld blocks" RESET "\n", who, n);
      STATUS = EXIT_FAILURE;
    } else {
      STATUS = nlps_gpu_tangent_bsr(G->gpu, 1, *brow_ptr, *bcols, *vals);
      if (STATUS != EXIT_SUCCESS) fprintf(stderr, "" RED "%s" RESET "\n", nlps_gpu_last_error(G->gpu));
    }
  } else {
    fprintf(stderr, "" RED "%s" RESET "\n", nlps_gpu_last_error(G->gpu));
  }
  if (STATUS != EXIT_SUCCESS) {
    free(*brow_ptr);
    free(*bcols);
    free(*vals);
    *brow_ptr = NULL;
    *bcols = NULL;
    *vals = NULL;
  }
  if (nblocks) *nblocks = n;
  return STATUS;
}

int nlps_glue_jacobian_sbaij(const nlps_glue *G, int nactive, int **brow_ptr, int **bcols, double **vals, long long *nblocks) {
  return nlps_glue_jacobian_blocks(G, NLPS_BSR_UPPER, "nlps_glue_jacobian_sbaij", nactive, brow_ptr, bcols, vals, nblocks);
}

int nlps_glue_jacobian_baij(const nlps_glue *G, int nactive, int **brow_ptr, int **bcols, double **vals, long long *nblocks) {
  return nlps_glue_jacobian_blocks(G, NLPS_BSR_FULL, "nlps_glue_jacobian_baij", nactive, brow_ptr, bcols, vals, nblocks);
}

/* The body of the MatShell's MATOP_MULT after VecGetArrayRead(x, &x_ptr) / VecGetArray(y, &y_ptr): y = K x. */
int nlps_glue_tangent_mult(const nlps_glue *G, const double *x_ptr, double *y_ptr) {
  const int STATUS = nlps_gpu_tangent_apply(G->gpu, x_ptr, y_ptr);
  if (STATUS != EXIT_SUCCESS) fprintf(stderr, "" RED "%s" RESET "\n", nlps_gpu_last_error(G->gpu));
  return STATUS;
}

/* MATOP_GET_DIAGONAL after VecGetArray(d, &d_ptr): the diagonal of K (nactive * NumberDimensions doubles), taken from
 * the point blocks; blocks_ptr = caller's scratch of nactive * NumberDimensions^2 doubles, or NULL to skip the
 * blocks (they are what a point-block Jacobi preconditioner, PCPBJACOBI, inverts). */
int nlps_glue_tangent_diagonal(const nlps_glue *G, double *d_ptr, double *blocks_ptr, int nactive) {
  const int d = NumberDimensions;
  double *b = blocks_ptr ? blocks_ptr : (double *)malloc((size_t)(nactive > 0 ? nactive : 1) * d * d * sizeof(double));
  if (b == NULL) return EXIT_FAILURE;
  const int STATUS = nlps_gpu_tangent_block_diagonal(G->gpu, b);
  if (STATUS != EXIT_SUCCESS) fprintf(stderr, "" RED "%s" RESET "\n", nlps_gpu_last_error(G->gpu));
  for (int A = 0; A < nactive && STATUS == EXIT_SUCCESS && d_ptr; A++)
    for (int i = 0; i < d; i++) d_ptr[A * d + i] = b[((size_t)A * d + i) * d + i];
  if (b != blocks_ptr) free(b);
  return STATUS;
}

/* The whole linear solve of the SNES iterate as one library call: the body of a PCShellSetApply after
 * VecGetArrayRead(b, &b_ptr) / VecGetArray(x, &x_ptr), with KSPSetType(ksp, KSPPREONLY), so that SNES's
 * KSPSolve (U-Newmark-beta.c:270-336; U-Static.c) hands its right-hand side straight to the device GMRES on the
 * operator of nlps_glue_tangent_operator.  pc = NLPS_PC_JACOBI is the driver's PCJACOBI, NLPS_PC_PBJACOBI the point
 * blocks; restart 30, rtol / atol / max_it as KSPGetTolerances returns them (dtol 1e5).  The stopping test sees the
 * true residual ||b - K x||, not PETSc's left-preconditioned one.  *iterations (may be NULL) = the Arnoldi steps
 * taken; a solve that ran without converging prints its reason and returns EXIT_FAILURE, as a failed KSPSolve makes
 * SNES stop the step. */
int nlps_glue_linear_solve(const nlps_glue *G, const double *b_ptr, double *x_ptr, int pc, double rtol, double atol,
                           int max_it, int *iterations) {
  nlps_ksp K;
  memset(&K, 0, sizeof K);
  K.pc = pc;
  K.restart = 30;
  K.max_it = max_it;
  K.x_is_guess = 0;
  K.rtol = rtol;
  K.atol = atol;
  K.dtol = 1e5;
  K.history = NULL;
  const int STATUS = nlps_gpu_tangent_solve(G->gpu, b_ptr, x_ptr, &K);
  if (iterations) *iterations = K.iterations;
  if (STATUS != EXIT_SUCCESS) {
    fprintf(stderr, "" RED "%s" RESET "\n", nlps_gpu_last_error(G->gpu));
    return STATUS;
  }
  if (K.reason < 0) {
    fprintf(stderr, "" RED "nlps_gpu_tangent_solve: no convergence (reason %d) after %d iterations, ||r|| = %e of ||b|| = %e" RESET "\n",
            K.reason, K.iterations, K.rnorm, K.bnorm);
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}

/* the driver's SNES settings (U-Newmark-beta.c:170-172, :328-334): SNESSetTolerances(100 TOL, TOL, default stol 1e-8,
 * MaxIter, default 10000 evaluations), divergence tolerance 1e4, the bt line search with PETSc's defaults, PCJACOBI and
 * GMRES(30) with KSP's default tolerances (rtol 1e-5, atol 1e-50, dtol 1e5, 10000 iterations) */
static nlps_snes nlps_glue_snes(double TOL, int MaxIter) {
  nlps_snes S;
  memset(&S, 0, sizeof S);
  S.max_it = MaxIter;
  S.max_funcs = 10000;
  S.atol = 100.0 * TOL;
  S.rtol = TOL;
  S.stol = 1e-8;
  S.divtol = 1e4;
  S.linesearch = NLPS_LS_BT;
  S.ls_alpha = 1e-4;
  S.ls_steptol = 1e-12;
  S.ls_maxstep = 1e8;
  S.ls_max_it = 40;
  S.apply_dirichlet = 1;
  S.ksp.pc = NLPS_PC_JACOBI;
  S.ksp.restart = 30;
  S.ksp.max_it = 10000;
  S.ksp.rtol = 1e-5;
  S.ksp.atol = 1e-50;
  S.ksp.dtol = 1e5;
  return S;
}

static int nlps_glue_snes_report(const nlps_glue *G, int STATUS, const nlps_snes *S) {
  if (STATUS != EXIT_SUCCESS) {
    fprintf(stderr, "" RED "%s" RESET "\n", nlps_gpu_last_error(G->gpu));
    return EXIT_FAILURE;
  }
  if (S->reason < 0) {
    fprintf(stderr, "" RED "nlps_gpu_newton_solve: no convergence (reason %d) after %d iterations, ||F|| = %e of %e" RESET "\n",
            S->reason, S->iterations, S->fnorm, S->fnorm0);
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}

/* The SNESSolve(snes, NULL, dU) of U-Newmark-beta.c:356 as one library call, after VecGetArray(dU, &dU_ptr) (the
 * initial guess of __form_initial_guess in, the converged increment out) and VecGetArrayRead of ctx->U_n_dt, U_n_dt2 and
 * Lumped_Mass: neither SNES nor KSP nor a Jacobian matrix is needed any more.  TOL = Parameters_Solver.TOL_Newmark_beta,
 * MaxIter = Parameters_Solver.MaxIter; the other arguments as nlps_glue_lagrangian_evaluation.  *snes_iterations /
 * *ksp_iterations (may be NULL) are what print_convergence_stats reports (:2078).  A solve that does not converge prints
 * its reason and returns EXIT_FAILURE, where the driver tests SNESGetConvergedReason. */
int nlps_glue_newton_solve(const nlps_glue *G, Particle MPM_Mesh, double *dU_ptr, const double *Un_dt_ptr,
                           const double *Un_dt2_ptr, const double *Lumped_Mass_ptr, const double alpha[6],
                           const double *gravity, const nlps_bcc *neumann, int nneumann, int TimeStep, double TOL,
                           int MaxIter, int *snes_iterations, int *ksp_iterations) {
#if NumberDimensions == 2
  const double thickness = Thickness_Plain_Stress;
  const double *area0 = NULL;
#else
  const double thickness = 1.0;
  const double *area0 = MPM_Mesh.Phi.Area_0.nV;
#endif
  nlps_snes S = nlps_glue_snes(TOL, MaxIter);
  const int STATUS = nlps_gpu_newton_solve(G->gpu, dU_ptr, Un_dt_ptr, Un_dt2_ptr, Lumped_Mass_ptr, alpha, gravity, neumann,
                                           nneumann, TimeStep, thickness, area0, &S);
  if (snes_iterations) *snes_iterations = S.iterations;
  if (ksp_iterations) *ksp_iterations = S.linear_iterations;
  return nlps_glue_snes_report(G, STATUS, &S);
}

/* The body of the time loop, U-Newmark-beta.c:192-404, as one library call: local search, masks, lumped mass, nodal
 * field, Newmark parameters, initial guess, SNESSolve, kinetic increments and the particle update, with every nodal
 * vector on the device.  bcc / nbcc from nlps_glue_boundaries; beta, gamma, Use_explicit_trial of Parameters_Solver
 * (:144-147), DeltaTimeStep of __compute_deltat (:180); alpha_blend = 1 is the driver's FLIP / PIC blend (:148).
 * *Nactivenodes (may be NULL) = the active nodes of the step.  Returns EXIT_FAILURE when the solve did not converge: the
 * particles are then left at the last evaluated state, not updated. */
int nlps_glue_newmark_step(const nlps_glue *G, Particle MPM_Mesh, const nlps_bcc *bcc, int nbcc, int TimeStep, double beta,
                           double gamma, double DeltaTimeStep, bool Use_explicit_trial, const double *gravity,
                           const nlps_bcc *neumann, int nneumann, double TOL, int MaxIter, int *Nactivenodes,
                           int *snes_iterations, int *ksp_iterations) {
#if NumberDimensions == 2
  const double thickness = Thickness_Plain_Stress;
  const double *area0 = NULL;
#else
  const double thickness = 1.0;
  const double *area0 = MPM_Mesh.Phi.Area_0.nV;
#endif
  nlps_snes S = nlps_glue_snes(TOL, MaxIter);
  nlps_newmark NM;
  NM.beta = beta;
  NM.gamma = gamma;
  NM.dt = DeltaTimeStep;
  NM.alpha_blend = 1.0;
  NM.use_explicit_trial = Use_explicit_trial ? 1 : 0;
  const int STATUS = nlps_gpu_newmark_step(G->gpu, bcc, nbcc, TimeStep, &NM, gravity, neumann, nneumann, thickness, area0, &S,
                                           Nactivenodes, NULL);
  if (snes_iterations) *snes_iterations = S.iterations;
  if (ksp_iterations) *ksp_iterations = S.linear_iterations;
  return nlps_glue_snes_report(G, STATUS, &S);
}

/* The step record from one of the reference's particle-path events (Out-particles-path-csv (i_start; i_step; i_end),
 * NLPS-Out-particle-path-csv.c:62-71, 401-457): the particles of Event.Idx_Path as probes, the Out_csv_particles_path_*
 * selectors as probe fields, Event.i_step as the interval -- the library records the steps that are multiples of it, so
 * the reader keeps the rows with i_start <= row[NLPS_REC_STEP] <= i_end.  capacity: rows kept between two reads (the
 * driver reads when it writes its csv files); nsets: reaction totals for the first nsets Dirichlet sets of
 * nlps_glue_boundaries (a load-displacement curve), 0 for none.  Energy-Kinetic / Energy-Potential of WriteVtk.c:816-841
 * are the sums NLPS_REC_KINETIC / NLPS_REC_STRAIN of the same row.  Event == NULL switches the record off. */
int nlps_glue_set_step_record(const nlps_glue *G, const Event *Out, int capacity, int nsets) {
  if (Out == NULL) return nlps_gpu_set_step_record(G->gpu, NULL) ? EXIT_FAILURE : EXIT_SUCCESS;
  nlps_record_cfg cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.every = Out->i_step > 0 ? Out->i_step : 1;
  cfg.capacity = capacity;
  cfg.nsets = nsets;
  cfg.nprobes = Out->Lenght_Path;
  cfg.probes = Out->Idx_Path;
  cfg.probe_fields = NLPS_PROBE_X;
  if (Out->Out_csv_particles_path_Damage) cfg.probe_fields |= NLPS_PROBE_DAMAGE;
  if (Out->Out_csv_particles_path_Velocity) cfg.probe_fields |= NLPS_PROBE_VEL;
  if (Out->Out_csv_particles_path_Acceleration) cfg.probe_fields |= NLPS_PROBE_ACC;
  if (Out->Out_csv_particles_path_Displacement) cfg.probe_fields |= NLPS_PROBE_DIS;
  if (Out->Out_csv_particles_path_Stress) cfg.probe_fields |= NLPS_PROBE_STRESS;
  if (Out->Out_csv_particles_path_Deformation_gradient) cfg.probe_fields |= NLPS_PROBE_F;
  if (nlps_gpu_set_step_record(G->gpu, &cfg) != 0) {
    fprintf(stderr, "" RED "nlps_glue_set_step_record: %s" RESET "\n", nlps_gpu_last_error(G->gpu));
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
