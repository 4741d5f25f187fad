/*
 * nlps_gpu.h — C-ABI of the MI355X (gfx950) implementation of NL-PartSol's particle<->grid transfer
 * and per-particle stress-update hot path.
 *
 * Plain C, plain pointers and sizes.  Every entry point names the reference interface it replaces
 * (file:line relative to nl-partsol/src of migmolper/NL-PartSol @ v1).  The reference passes its fat
 * `Particle` / `Mesh` structs by value (Types.h:548-760); here the same data crosses the boundary as
 * the contiguous row-major arrays those structs already own (`Matrix.nV`, MatrixOp.c:128-181), so the
 * glue a maintainer adds in U-Newmark-beta.c / U-Static.c is pointer plumbing only.
 *
 * Conventions
 *  - return value: 0 = EXIT_SUCCESS, 1 = EXIT_FAILURE (reference convention, U-Newmark-beta.c:199-204);
 *    the library never exit()s; nlps_gpu_last_error() returns the message the reference would have
 *    printed in red on stderr.  A missing GPU / failed HIP call is a failure, never a CPU fallback.
 *  - arithmetic is FP64; index maps are 32-bit int and bit-identical to the reference's.
 *  - particle state is device resident between calls (SoA, sorted by background-grid cell); host
 *    arrays are stale until nlps_gpu_download_state().
 *  - nodal vectors ("Vec" arrays of the PETSc driver) use the reference's masked numbering
 *    [Nactivenodes*Ndim], index = Nodes2Mask[node]*Ndim + i.  Each such pointer may be a HOST pointer
 *    (VecGetArray) or a DEVICE pointer (hipMalloc / torch tensor); the library detects which.
 *  - threading: one host thread per handle (the PETSc thread); all work is issued on one HIP stream.
 */
#ifndef NLPS_GPU_H
#define NLPS_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: these are its exports */
#endif

typedef struct nlps_gpu nlps_gpu; /* opaque: device buffers, stream, tables */

#define NLPS_MAXNB 128 /* row stride of downloaded neighbour lists (>= 5^3) */

/* Material.Type strings of Constitutive/Constitutive.c:28-258 that are on the path */
enum {
  NLPS_MAT_NEO_HOOKEAN = 0,   /* "Neo-Hookean-Wriggers", Hyperelastic/Neo-Hookean.c:38-85 */
  NLPS_MAT_HENCKY = 1,        /* "Hencky",               Hyperelastic/Hencky.c:40-94       */
  NLPS_MAT_DRUCKER_PRAGER = 2, /* "Drucker-Prager",      Plasticity/Drucker-Prager.c:319-613 */
  NLPS_MAT_VON_MISES = 3,      /* "Von-Mises",           Plasticity/Von-Mises.c:212-392 */
  NLPS_MAT_MATSUOKA_NAKAI = 4, /* "Matsuoka-Nakai",      Plasticity/Matsuoka-Nakai.c:300-700 */
  NLPS_MAT_LADE_DUNCAN = 5,    /* "Lade-Duncan",         Plasticity/Lade-Duncan.c:290-692 */
  NLPS_MAT_NEWTONIAN_FLUID = 6 /* "Newtonian-Fluid-Compressible", Fluid/Newtonian-Fluid.c:17-79: reads the rate tensor dt_F_n1.
                                  Implicit path; nlps_gpu_explicit_step refuses a cloud that holds it unless
                                  nlps_gpu_set_explicit_fluid is on, which defines the rate of that step */
};

/* Structured background grid (GramsBox mesh, InOutFun/Read_GramsBox.c:54): Q4 / H8 lattice, nodes
 * numbered x-fastest, elements x-fastest with GiD connectivity order.  h_avg = FEM_Mesh.h_avg
 * (Read_GramsBox.c:460-507) or NULL to have the library compute it with the same rule. */
typedef struct {
  int ndim;          /* NumberDimensions, Macros.h:33-37 */
  int n[3];          /* nodes per axis */
  double origin[3];
  double h;          /* lattice spacing (FEM_Mesh.DeltaX) */
  const double *h_avg;
} nlps_grid;

/* Snapshot of the globals the path reads implicitly (Globals.h:21,33-58);
 * defaults InOutFun/Read_GramsShapeFun.c:100-104. */
typedef struct {
  double gamma_lme;        /* gamma_LME        (3.0)   */
  double tol_zero_lme;     /* TOL_zero_LME     (1e-6)  */
  double tol_wrapper_lme;  /* TOL_wrapper_LME  (1e-10) */
  int max_iter_lme;        /* max_iter_LME     (10)    */
  double tol_radial_returning;   /* TOL_Radial_Returning            */
  int max_iter_radial_returning; /* Max_Iterations_Radial_Returning */
  int driver_eigenerosion;       /* Driver_EigenErosion (Globals.h): the damage hooks of the level-B stages (0 = off) */
  int driver_eigensoftening;     /* Driver_EigenSoftening: the same hooks with Eigensoftening__Constitutive__ (0 = off;
                                    both on = eigenerosion, like the if / else if of Constitutive.c:395-412) */
} nlps_params;

/* Material, Types.h:359-458 (members read by the three laws) */
typedef struct {
  int type;
  double E, nu;
  double phi_deg, psi_deg; /* phi_Frictional, psi_Frictional */
  double kappa_0, exponent_ortiz, eps_0 /* Plastic_Strain_0 */, p_ref /* ReferencePressure */;
  /* Von-Mises (Von-Mises.c:246-253): sigma_y = kappa_0, Hardening_modulus, theta / K_0 / K_inf / delta _Hardening_Voce */
  double hardening_modulus, theta_voce, K0_voce, Kinf_voce, delta_voce;
  double Ceps, Gf; /* eigenerosion (Constitutive/Fracture/EigenErosion.c:63-64): normalising constant, Griffith energy */
  /* Matsuoka-Nakai / Lade-Duncan (Matsuoka-Nakai.c:330-341): Cohesion, alpha_Hardening_Borja, a_Hardening_Borja[3];
   * they also read phi_deg; Kappa_n starts at kappa_0 and EPS_n of Matsuoka-Nakai at eps_0 (caller's arrays,
   * Generate-One-Phase-Analysis.c:620-626).  Their readers set TOL_Radial_Returning / Max_Iterations_Radial_Returning
   * to 1e-10 / 20 (Matsuoka-Nakai) and 1e-14 / 10 (Lade-Duncan): nlps_params carries them */
  double cohesion, alpha_borja, a_borja[3];
  double ft, heps, wcrit; /* eigensoftening (Types.h:386-390, EigenSoftening.c:67-69): tensile strength, band width of the
                             cohesive fracture, critical opening displacement */
  /* Newtonian-Fluid-Compressible (Newtonian-Fluid.c:31-34): Viscosity, Compressibility, n_Macdonald_model; the law also
   * reads p_ref (ReferencePressure).  Appended: the members above keep their offsets */
  double viscosity, compressibility, n_macdonald;
} nlps_material;

/* Particle fields, Types.h:184-283 / 548-623: HOST pointers to the reference's row-major arrays
 * (MPM_Mesh.Phi.<field>.nV).  T = 5 in 2-D (xx,xy,yx,yy,zz), 9 in 3-D.  Optional members may be NULL. */
typedef struct {
  int np;               /* NumGP */
  double *x_GC;         /* [np][ndim] */
  double *dis;          /* [np][ndim] */
  double *vel;          /* [np][ndim] */
  double *acc;          /* [np][ndim] */
  double *F_n;          /* [np][T] */
  double *F_n1;         /* [np][T]  optional on upload (defaults to F_n) */
  double *DF;           /* [np][T]  optional on upload (identity) */
  double *Stress;       /* [np][T]  optional on upload (0): Kirchhoff stress */
  double *b_e_n;        /* [np][T]  optional (identity) */
  double *b_e_n1;       /* [np][T]  optional */
  double *J_n;          /* [np] */
  double *J_n1;         /* [np]     optional (J_n) */
  double *rho;          /* [np] */
  double *mass;         /* [np] */
  double *Vol_0;        /* [np] */
  double *W;            /* [np]     optional */
  double *Kappa_n, *Kappa_n1, *EPS_n, *EPS_n1; /* [np] optional (0) */
  int *MatIdx;          /* [np] */
  int *I0;              /* [np]      NULL on upload => nlps_gpu_initialize_lme() must be called */
  double *lambda;       /* [np][ndim] (MPM_Mesh.lambda.nV) optional */
  double *Beta;         /* [np]       (MPM_Mesh.Beta.nV)   optional */
  double *dt_F_n;       /* [np][T]  optional (0): rate of F, consumed only by the fluid law upstream */
  double *dt_F_n1;      /* [np][T]  optional */
  double *dt_DF;        /* [np][T]  optional */
  double *C_ep;         /* [np][ndim*ndim] download only: elastoplastic tangent moduli (Drucker-Prager, Von-Mises) */
  double *Back_stress;  /* [np][3] optional (0): principal back stress of Von-Mises (Phi.Back_stress), in/out */
  double *Damage_n;     /* [np] optional (0): Phi.Damage_n  (eigenerosion, driver_eigenerosion != 0) */
  double *Damage_n1;    /* [np] optional (Damage_n): Phi.Damage_n1 */
  double *Strain_f_n;   /* [np] optional (0): Phi.Strain_f_n  (eigensoftening: strain at the onset of fracture) */
  double *Strain_f_n1;  /* [np] optional (Strain_f_n): Phi.Strain_f_n1 -- the one Eigensoftening reads AND writes */
} nlps_particles;

/* Dirichlet boundary = Load of FEM_Mesh.Bounds (Types.h:296-351), flattened:
 * dir[k*nsteps + t] = Dir[k*NumTimeStep+t], value[k*nsteps + t] = Value[k].Fx[t]. */
typedef struct {
  int nnodes;
  const int *nodes;
  int dim;
  const int *dir;
  const double *value;
} nlps_bcc;

/* ------------------------------------------------------------------ lifetime */

/* Uploads the particle set (AoS -> cell-sorted SoA) and builds the grid tables.
 * hip_stream: a hipStream_t to issue all work on (NULL = the library creates its own). */
int nlps_gpu_create(nlps_gpu **h, const nlps_grid *grid, const nlps_params *prm,
                    const nlps_material *mats, int nmats, const nlps_particles *host, int nsteps,
                    void *hip_stream);
int nlps_gpu_destroy(nlps_gpu *h);
const char *nlps_gpu_last_error(const nlps_gpu *h);
int nlps_gpu_synchronize(nlps_gpu *h);

/* Copies the device state back into the caller's arrays in the caller's particle order (before VTK/CSV
 * output, Outputs/WriteVtk.c:95-266, or host tangent assembly).  NULL members are skipped. */
int nlps_gpu_download_state(nlps_gpu *h, nlps_particles *host);
/* MPM_Mesh.NumberNodes[p] and ListNodes[p] as arrays (chain order = nodal_set__Particles__ order,
 * Particles/Particles-Tools.c:71-82): nn[np], list[np][NLPS_MAXNB]. */
int nlps_gpu_download_lists(nlps_gpu *h, int *nn, int *list);
/* The shape functions and their gradients of particles first .. first + count - 1 (caller's order) in the order of
 * ListNodes[p]: what compute_N__ShapeFun__ / compute_dN__ShapeFun__ return for the LME family (Shape-Functions.c:145-262;
 * p__LME__ LME.c:716-762, dp__LME__ LME.c:836-891, with the particle's current lambda and beta).  N[count][NLPS_MAXNB],
 * dN[count][NLPS_MAXNB][ndim], entries behind NumberNodes[p] are 0; either may be NULL.  A level-A entry for callers that
 * interpolate fields of their own (outputs, contact, diagnostics); the step kernels never store these values. */
int nlps_gpu_shape_functions(nlps_gpu *h, int first, int count, double *N, double *dN);
/* FEM_Mesh.ActiveNode[nnodes] as bytes */
int nlps_gpu_download_active(nlps_gpu *h, unsigned char *active);
/* OR of the per-particle failure flags (1 Newton, 2 connectivity, 4 J<=0, 8 constitutive, 16 halo) */
int nlps_gpu_status_flags(nlps_gpu *h, int *flags);

/* ------------------------------------------------------------------ level-B stage calls */

/* initialise_shapefun__MeshTools__ -> initialize__LME__, Nodes/LME.c:45-173 */
int nlps_gpu_initialize_lme(nlps_gpu *h);

/* local_search__MeshTools__ (Nodes/Shape-Functions.c:31-90) -> local_search__LME__ (Nodes/LME.c:895-1015):
 * I0 update, 1-ring activation, neighbour lists, beta, lambda Newton. */
int nlps_gpu_local_search(nlps_gpu *h);

/* get_active_nodes__MeshTools__ + get_active_dofs__MeshTools__ (Nodes/Nodes-Tools.c:46-156).
 * nodes2mask[nnodes] / dofs2mask[nactive*ndim] may be NULL (kept on the device only). */
/* Node order of the masked numbering.  get_active_nodes__MeshTools__ hands out its running index in the order of the
 * mesh file's nodes (Nodes/Nodes-Tools.c:46-66); the library works in lattice numbering (x fastest), which is the same
 * thing only for a file numbered that way.  lattice_of_file[A] = lattice node of file node A (the map
 * nlps_host_lattice_from_nodes returns; nnodes entries, copied): from now on Nodes2Mask -- and with it every masked
 * vector, the dof mask and the COO rows / columns of the tangent -- counts the active nodes in FILE order, and the
 * nodes2mask array of nlps_gpu_active_masks is indexed by file node.  Everything else of this interface that names a
 * node (I0, lists, Dirichlet node sets, h_avg, active flags) stays in lattice numbering.  NULL = lattice order. */
int nlps_gpu_set_node_numbering(nlps_gpu *h, const int *lattice_of_file);
int nlps_gpu_active_masks(nlps_gpu *h, const nlps_bcc *bcc, int nbcc, int step, int *nactive,
                          int *nfree_dofs, int *nodes2mask, int *dofs2mask);

/* __compute_nodal_lumped_mass, U-Newmark-beta.c:528-597.  M[nactive*ndim] is overwritten. */
int nlps_gpu_lumped_mass(nlps_gpu *h, double *M);

/* __get_nodal_field_n, U-Newmark-beta.c:615-696.  V, A overwritten; needs M from the call above. */
int nlps_gpu_nodal_field_n(nlps_gpu *h, double *V, double *A, const double *M);

/* __local_compatibility_conditions, U-Newmark-beta.c:1064-1160: DF, F_n1, J_n1 and, when dU_dt is given,
 * the rate tensors dt_DF, dt_F_n1 (compute-Strains.c:48-72,176-207; they feed only the Newtonian-fluid law,
 * Constitutive.c:84-108, so dU_dt may be NULL for a cloud without that law; with it the caller gives dU_dt
 * (nlps_gpu_nodal_kinetic_increments) and a NULL is refused: the stress would be made from stale rates). */
int nlps_gpu_compatibility(nlps_gpu *h, const double *dU, const double *dU_dt);

/* __constitutive_update -> Stress_integration__Constitutive__, U-Newmark-beta.c:1208-1242,
 * Constitutive/Constitutive.c:18-258 */
int nlps_gpu_constitutive(nlps_gpu *h);

/* __nodal_internal_forces, U-Newmark-beta.c:1257-1374 (+ push_forward_dN__MeshTools__,
 * Shape-Functions.c:405-448).  R[nactive*ndim] is ACCUMULATED into; Dirichlet dofs are skipped. */
int nlps_gpu_internal_forces(nlps_gpu *h, double *R);
/* __nodal_traction_forces (U-Newmark-beta.c:1376-1500): R_A -= N_pA T A0_p over the particles of the Neumann contours
 * (the reference runs it serially on the host between the internal and the inertial forces).  loads[l]
 * is a Load like the Dirichlet ones with nodes = PARTICLE indices in the caller's order; the traction of the current
 * step is value where dir is 1 and, as upstream, the previous contour's value where it is 0.  A0_p is Vol_0 / thickness
 * in 2-D (Thickness_Plain_Stress) and area0[p] (Phi.Area_0, caller's order) in 3-D.  R: masked, host or device. */
int nlps_gpu_nodal_traction_forces(nlps_gpu *h, double *R, const nlps_bcc *loads, int nloads, int step,
                                   double thickness, const double *area0);

/* __update_particles_internal_variables, U-Newmark-beta.c:1917-1978 */
int nlps_gpu_roll_state(nlps_gpu *h);

/* __update_particles_kinetics_FLIP_PIC, U-Newmark-beta.c:1993-2072 */
int nlps_gpu_update_kinetics(nlps_gpu *h, double alpha_blend, const double *dU, const double *Un_dt,
                             const double *dU_dt, const double *dU_dt2);

/* Fused explicit predictor-corrector step (stage order and formulas of U-Verlet.c:229-253, 301-367,
 * 455-527, 530-676, 919-1010, 1024-1084; internal force in the Kirchhoff form of
 * U-Newmark-beta.c:1257-1374; the contour tractions of :805-902 once nlps_gpu_set_explicit_loads has given them).
 * gravity[ndim] may be NULL.  One P2G+stress+G2P particle step.
 * A cloud that holds Newtonian-Fluid-Compressible is refused at the start of the call (return 1, the law named in
 * nlps_gpu_last_error): the law reads dt_F_n1 and the reference has no working explicit driver that defines that rate.
 * nlps_gpu_set_explicit_fluid (below) defines it and lifts the refusal for the handle it is set on. */
int nlps_gpu_explicit_step(nlps_gpu *h, const nlps_bcc *bcc, int nbcc, int step, double dt,
                           double gamma, const double *gravity);
/* The explicit step of a cloud that holds Newtonian-Fluid-Compressible.  Off by default: nlps_gpu_explicit_step then
 * refuses such a cloud, as above.  With on != 0 the step of such a cloud is the explicit composition above (stage order
 * of U-Verlet.c) with the rate tensors of the reference's own formulas (compute-Strains.c:48-72, 176-207) under two
 * choices:
 *   - the nodal rate vector is the increment's mean rate over the step, dV_A = dU_A / dt;
 *   - the rate carried over from the last step is zero.
 * That gives
 *   dt_DF   = sum_A (dU_A / dt) (x) grad N_A   = (DF - I) / dt,
 *   dt_F_n1 = dt_DF F_n                        = (F_n1 - F_n) / dt,
 *   L       = dt_F_n1 F_n1^-1                  = (I - DF^-1) / dt.
 * The carried term DF dt_F_n of the Newmark path is dropped on purpose: there dV is a velocity INCREMENT and the term
 * accumulates it; here dV is the full mean velocity of the step, and keeping the term would make the viscous stress grow
 * step by step.
 * The fluid stress is Newtonian-Fluid.c:17-79 from F_n1, dt_F_n1, J_n1 (in 2-D the trace is xx + yx, as upstream).  The
 * density update rho / det DF, the internal forces, gravity, the Dirichlet sets, the contour loads, the equilibrium, G2P
 * and the corrector are the step's own, shared with the solid laws of a mixed cloud (one K3 launch per law present).
 * The roll includes dt_F_n <- dt_F_n1: a download after the step returns the step's rate in both dt_F_n and dt_F_n1 for
 * the fluid particles, and a nlps_gpu_newmark_step that follows explicit steps starts from that rate; particles of other
 * laws keep what they had.  The step does not write dt_DF: a download returns for it what it returned before the step.
 * W of a fluid particle is not touched (Constitutive.c:84-108 writes Stress and nothing else).
 * A particle with J_n1 <= 0 raises the Jacobian flag as in every explicit step; one whose F_n1 does not invert raises the
 * constitutive flag and contributes neither stress nor force.
 * With the switch on a step returns 1 with the reason in nlps_gpu_last_error, launches nothing and leaves the handle
 * usable when a halo callback or an RCCL exchange is attached (one rank only), for a cloud created with
 * driver_eigenerosion / driver_eigensoftening (the state half of the damage step is cut for the solid laws), and for
 * dt <= 0 (the rate is the increment over dt).
 * nlps_gpu_set_law_launch_mode(2) stays refused for such a cloud.  The step runs the non-folded form on the handle's
 * stream, in deterministic mode too.
 * The setter returns 1, with the reason in nlps_gpu_last_error, for a cloud that holds no fluid material. */
int nlps_gpu_set_explicit_fluid(nlps_gpu *h, int on);
/* The damage hooks inside the explicit step (clouds created with driver_eigenerosion or driver_eigensoftening).  Off
 * by default: nlps_gpu_explicit_step then refuses such a cloud (the hooks of the level-B stages are its only form).
 * With on != 0 the step of such a cloud is the composition of the explicit step above with the hooks of the maintained
 * driver at the places U-Newmark-beta.c puts them (the reference's explicit drivers are stubs):
 *   1. search, active nodes, lumped mass, predictor, nodal dU with the Dirichlet sets, compatibility (DF, F_n1, J_n1,
 *      rho), all as above;
 *   2. after the search compute_Beps__Constitutive__(.., false): the epsilon-neighbourhoods of the particles whose total
 *      displacement exceeds 1e-6 (Beps.c:30-36).  Eigenerosion: the other particles keep the lists of
 *      Initialize_Beps = true, taken before the first step (U-Newmark-beta.c:182-183); eigensoftening: their lists are
 *      empty (:213-215);
 *   3. the constitutive update, which skips failed particles (Damage_n == 1: W = 0, stress untouched, :1218-1224);
 *   4. the damage hook (:1313-1331): Damage_n1 (and Strain_f_n1), then every Kirchhoff stress scaled in place by
 *      1 - Damage_n1; eigensoftening with the reference's sequential semantics (one particle after the other in the
 *      caller's order);
 *   5. internal forces from the scaled stress, nodal equilibrium, G2P, corrector;
 *   6. the roll of the explicit step, and Damage_n <- Damage_n1, Strain_f_n <- Strain_f_n1 (:1950-1956).
 * A download after such a step returns Stress = the scaled stress of that step, W = the unscaled energy (0 for a skipped
 * particle), Damage_n == Damage_n1 and both Strain_f slots, like the level-B roll.
 * The step runs on one rank, on the handle's stream, without sorts, synchronisation or allocation (in deterministic mode
 * with nlps_gpu_set_deterministic_damage one more kernel orders every node run in place).  It returns 1 with
 * the reason in nlps_gpu_last_error when a halo callback or an RCCL exchange is attached (an epsilon-neighbourhood across
 * a slab face needs ghost particles), in deterministic mode unless nlps_gpu_set_deterministic_damage is on, and for the
 * fluid law (as above).
 * The setter returns 1 for a cloud created without either driver. */
int nlps_gpu_set_explicit_damage(nlps_gpu *h, int on);
/* F-bar, the reference's volumetric-locking control, inside the explicit step, on patches of background-lattice cells.
 * Upstream: Neo-Hookean-Wriggers and Newtonian-Fluid-Compressible carry Fbar / Fbar-alpha
 * (InOutFun/Material/Hyperelastic/Neo-Hookean.c:133-146, Fluid/Compressible-Newtonian-Fluid.c:107-118); the compatibility
 * stage sums J Vol_0 over patches of elements (U-Newmark-beta.c:1146-1193);
 * get_locking_free_Deformation_Gradient_n1__Particles__ (compute-Strains.c:109-172) turns the patch ratio into Fbar; the
 * law reads (Fbar, Jbar) in place of (F_n1, J_n1) (Constitutive.c:32-38, 66-72, 89-95).  Upstream defines its patches on
 * T6 / T10 meshes only, overwrites Fbar_n in place at every residual evaluation and starts Phi.Fbar from zeros, so the
 * definition is stated here and only the formulas are upstream's.
 *
 * Off by default: a step then launches exactly what it launches without this call.  With a configuration set, a step is
 * the explicit composition above with one insertion between the compatibility and the constitutive update:
 *   - The patch of a particle.  Its cell is c_k = clamp(floor((x_k - origin_k) / h), 0, n_k - 2) per axis k, with x the
 *     position nlps_gpu_download_state would return in front of the step and n_k the nodes of the lattice along k; its
 *     patch is c_k / block[k] (integer division) per axis.
 *   - Patch sums, behind the step's compatibility (DF, F_n1 = DF F_n, J_n1 as always), over ALL particles of a patch
 *     whatever their material, as upstream does: Vn = sum J_n Vol_0, Vn1 = sum J_n1 Vol_0, J_patch = Vn1 / Vn.
 *   - Per particle, with alpha the entry of its material (a material with alpha < 0 forms its values with alpha = 0):
 *       DJ = det DF (2-D: of the in-plane 2 x 2 block),   c = (J_patch / DJ)^(1 / ndim),
 *       Fbar_n1 = alpha F_n1 + (1 - alpha) c DF Fbar_n    (2-D: the in-plane block; the zz entry is F_n1's),
 *       Jbar_n1 = Jbar_n J_patch.
 *     Both are formed for every particle.
 *   - The law.  A material with alpha >= 0 receives (Fbar_n1, Jbar_n1) where it would receive (F_n1, J_n1).  The rate of
 *     the fluid law stays the unbarred dt_F_n1 of nlps_gpu_set_explicit_fluid (Constitutive.c:87).  Everything else in the
 *     step is unchanged -- for a material with alpha < 0 the whole step: density, internal force in the Kirchhoff form
 *     with the step's own gradients (DF, not a barred one), gravity, Dirichlet sets, contour loads, equilibrium, G2P,
 *     corrector.
 *   - The roll adds Fbar_n <- Fbar_n1, Jbar_n <- Jbar_n1.  F_n, J_n, rho and the rates stay unbarred; Stress and W of a
 *     download behind the step are the law's values at the state it received.
 * Fbar_n / Jbar_n belong to the particles: they move with them in nlps_gpu_resort, the periodic and the adaptive re-sort,
 * and nlps_gpu_download_fbar returns them in the caller's order ([np][5 | 9] like every tensor, [np]).  A run is restarted
 * from (the downloaded state, Fbar_n, Jbar_n).  Inside a step F-bar adds kernels on the handle's stream and nothing else:
 * no allocation, no synchronisation, no copy (the setter makes the patch array, 2 doubles per patch of the lattice).
 * Patch sums are taken by floating-point atomics: their summation order is not fixed.
 *
 * cfg == NULL switches F-bar off and frees everything it made.  The setter returns 1, with the reason in
 * nlps_gpu_last_error, stores nothing and leaves the handle as it was for: a block entry < 1; an alpha > 1; alpha >= 0 on a
 * material that is neither Neo-Hookean nor Newtonian-Fluid-Compressible; every alpha < 0; a cloud created with
 * driver_eigenerosion / driver_eigensoftening; a handle with a halo callback or an RCCL exchange attached; a migrated
 * handle.  A step returns 1 in the same way, launching nothing, when an exchange has been attached since, after a
 * migration, in deterministic mode (fixed-order patch sums are not built), and -- as without F-bar -- for a fluid material
 * without nlps_gpu_set_explicit_fluid.  While F-bar is set, the calls whose law would have to read it return 1:
 * nlps_gpu_compatibility, _constitutive, _lagrangian_evaluation, _newton_solve, _newmark_step, _tangent_assemble,
 * _tangent_operator, _tangent_csr_pattern, _tangent_bsr_pattern, _tangent_lambda_max (the consistent F-bar tangent couples
 * all particles of a patch).  The step runs the non-folded form on one rank. */
typedef struct {
  int block[3];         /* cells per patch along each axis, >= 1 (block[2] not read in 2-D) */
  const double *alpha;  /* [nmats] alpha_Fbar in [0,1] for materials whose law reads F-bar; < 0: the material does not */
  const double *Fbar_n; /* [np][T], caller's order, or NULL: F_n as it stands on the device */
  const double *Jbar_n; /* [np], caller's order, or NULL: J_n as it stands */
} nlps_fbar_cfg;
int nlps_gpu_set_explicit_fbar(nlps_gpu *h, const nlps_fbar_cfg *cfg);   /* NULL: off, frees everything */
int nlps_gpu_download_fbar(nlps_gpu *h, double *Fbar_n, double *Jbar_n); /* caller's order; either may be NULL */
/* The Neumann contours inside the explicit step: compute_Nodal_Nominal_traction_Forces (U-Verlet.c:805-902), which
 * compute_Nodal_Forces calls directly behind the internal forces (:680-699), Forces[A] += N_pA T A0_p over the particles
 * of MPM_Mesh.Neumann_Contours.  The arguments mean what they mean in nlps_gpu_nodal_traction_forces: loads[l].nodes are
 * PARTICLE indices in the caller's order, dir / value are [dim][nsteps] with the handle's nsteps, A0_p is Vol_0 / thickness
 * in 2-D and area0[p] (Phi.Area_0, caller's order, required) in 3-D.  Everything is copied to the device: the caller's
 * arrays may be freed after the call.  nloads == 0 removes the loads, a second call replaces the first; the loads survive
 * nlps_gpu_resort, the periodic and the adaptive re-sort (the caller's indices keep addressing the same particles).
 * From then on every nlps_gpu_explicit_step(.., step, ..) adds the contour tractions of `step` to the nodal force on every
 * dof, fixed or free, behind the internal forces and in front of the nodal equilibrium (:695): the accelerations of free
 * dofs and the reactions of fixed dofs (Reactions = Total_Forces, :955) contain them, and nlps_gpu_explicit_nodal returns
 * force = -f_int + sum N_pA T A0_p, accel and reaction with them.  The traction vector of a step starts at zero; each
 * contour in turn overwrites the directions whose dir is 1 at that step, a direction switched off keeps the value of the
 * contour before it (:865-869).  N_pA are the shape functions every other stage of the step uses.
 * The step stays free of allocation, synchronisation and copies: one more kernel on the handle's stream over the contour
 * particles, and one over the particles behind a re-sort (the caller's index -> slot map).  In deterministic mode one
 * wave adds the contributions in the caller's contour order behind the fixed-order sum of the force slabs: the step stays
 * bit-reproducible.  It works in every one-rank form of the step, nlps_gpu_set_explicit_damage included.
 * Returns 1, with the reason in nlps_gpu_last_error and nothing stored: a particle index outside the cloud; 3-D without
 * area0; 2-D with thickness <= 0; a handle with a halo callback or an RCCL exchange attached (slab ranks are not built:
 * a contour particle near a slab face adds to band nodes, and that sum would have to go in front of the exchange of the
 * nodal forces in every overlap form) -- a step returns 1 if one is attached later while loads are set; a migrated handle.
 * With loads set, nlps_gpu_explicit_step returns 1 for a step outside [0, nsteps), with or without Dirichlet sets. */
int nlps_gpu_set_explicit_loads(nlps_gpu *h, const nlps_bcc *loads, int nloads, double thickness, const double *area0);
/* The step record: one small row of doubles per recorded step, made on the device behind the step and kept in a ring on
 * the handle -- what a driver watches a run by (energy balance, momenta, min J, the largest velocity of the dynamic Courant
 * bound of Courant.c:26-45, the reaction on a Dirichlet set, the history of a few particles; the reference's
 * Energy-Kinetic / Energy-Potential blocks, WriteVtk.c:816-841, and its Out-particles-path-csv events) without
 * nlps_gpu_download_state.  Inside a step the record adds kernels on the handle's stream and nothing else: no allocation,
 * no synchronisation, no copy.  With no record set a step launches what it launched before.
 *
 * A row is [global block: NLPS_REC_NGLOBAL doubles][reactions: nsets x 3][probes: nprobes x probe_doubles]
 * (nlps_gpu_step_record_layout gives the offsets).
 * Global block: every quantity is the reduction over what nlps_gpu_download_state would return at that point --
 *   mass = sum m, momentum = sum m v, angular = sum m x cross v about the coordinate origin (2-D: slot +2 only), mass_x =
 *   sum m x, kinetic = 1/2 sum m |v|^2, strain = sum W Vol_0, volume = sum Vol_0 J_n, vmax_comp = max_p max_j |v_pj|,
 *   vmax_norm = max_p |v_p|, J_min / J_max over J_n, EPS_max over EPS_n, Damage_max over Damage_n, failed = the number of
 *   particles with Damage_n == 1, status = the handle's failure-flag word read in stream order.  Slots of the third
 *   dimension are 0 in 2-D.  An empty cloud: sums 0, maxima of non-negative quantities 0, J_min = +inf, J_max = -inf.
 *   step = the step argument (nlps_gpu_record_now: the tag), kind = NLPS_REC_KIND_*, dt = the step's (NOW: 0), time = the
 *   sum of the dt of every explicit step and every converged Newmark step since the record was set, recorded or not.
 *   After a folded explicit step the hyperelastic laws have not stored tau and W: the record re-forms them in registers
 *   from the stored F_n and J_n with the code the download uses, and writes nothing to the particle arrays; in every other
 *   state it reads the stored values.  The sums are made without float atomics in a fixed order: a row is bit-reproducible
 *   for a given memory order of the particles.
 * Reactions: after an explicit step, for set s < min(nsets, nbcc) and direction k, the sum over the nodes of bcc[s] of the
 *   reaction nlps_gpu_explicit_nodal would return for dof (node, k), over the dofs with dir[k][step] == 1 (contour tractions
 *   and gravity enter as they do there); formed from the kept nodal sums without making the lazy nodal arrays.  Slots of
 *   sets the step did not have, and every reaction slot of a row of another kind, are NaN.
 * Probes: per probed particle (caller's index; the indices survive every re-sort) the fields selected in probe_fields in
 *   ascending bit order, laid out as in nlps_gpu_download_state (ndim per vector, 5 or 9 per tensor): x_GC, dis, vel, acc,
 *   F_n, Stress, J_n, EPS_n, Damage_n, W.
 * Rows are written at the end of nlps_gpu_explicit_step (every one-rank form; on a slab rank the particle sums are that
 * rank's share: add the sums and take min / max across the ranks), at the end of a converged nlps_gpu_newmark_step, and
 * by nlps_gpu_record_now.  The setter returns 1 with the reason in nlps_gpu_last_error and stores nothing for every < 1,
 * capacity < 1, a negative count, a probe index outside the cloud, nprobes > 0 with probe_fields == 0 (or a bit outside
 * NLPS_PROBE_*), and nprobes > 0 or nsets > 0 on a handle with a halo callback or an RCCL exchange attached or on a
 * migrated handle -- a step returns 1 if one is attached later while such a record is set.  A second set replaces the
 * first (behind a device synchronise) and starts the row count and the time at zero; cfg == NULL switches the record off
 * and frees it. */
enum { NLPS_REC_KIND_NOW = 0, NLPS_REC_KIND_EXPLICIT = 1, NLPS_REC_KIND_NEWMARK = 2 };
enum { /* offsets into the global block of a row, doubles */
  NLPS_REC_STEP = 0, NLPS_REC_KIND = 1, NLPS_REC_DT = 2, NLPS_REC_TIME = 3, NLPS_REC_NP = 4, NLPS_REC_MASS = 5,
  NLPS_REC_MOMENTUM = 6 /*3*/, NLPS_REC_ANGULAR = 9 /*3*/, NLPS_REC_MASS_X = 12 /*3*/, NLPS_REC_KINETIC = 15,
  NLPS_REC_STRAIN = 16, NLPS_REC_VOLUME = 17, NLPS_REC_VMAX_COMP = 18, NLPS_REC_VMAX_NORM = 19, NLPS_REC_J_MIN = 20,
  NLPS_REC_J_MAX = 21, NLPS_REC_EPS_MAX = 22, NLPS_REC_DAMAGE_MAX = 23, NLPS_REC_FAILED = 24, NLPS_REC_STATUS = 25,
  NLPS_REC_NGLOBAL = 32 /* 26..31 reserved, 0 */ };
enum { NLPS_PROBE_X = 1, NLPS_PROBE_DIS = 2, NLPS_PROBE_VEL = 4, NLPS_PROBE_ACC = 8, NLPS_PROBE_F = 16,
       NLPS_PROBE_STRESS = 32, NLPS_PROBE_J = 64, NLPS_PROBE_EPS = 128, NLPS_PROBE_DAMAGE = 256, NLPS_PROBE_W = 512 };
typedef struct {
  int every;            /* >= 1: steps whose `step` argument is a multiple of it are recorded */
  int capacity;         /* >= 1: rows kept (a ring: the newest `capacity` rows survive) */
  int nsets;            /* >= 0: reaction totals for the first nsets Dirichlet sets of a step, 3 doubles each */
  int nprobes; const int *probes;   /* particle indices in the caller's order (copied) */
  unsigned probe_fields;            /* NLPS_PROBE_*, in ascending bit order inside a probe's block */
} nlps_record_cfg;
int nlps_gpu_set_step_record(nlps_gpu *h, const nlps_record_cfg *cfg);      /* NULL: off, frees everything */
/* doubles per row, offset of the reaction block and of the probe block inside a row, doubles per probe (any pointer may be
 * NULL); 1 with no record set */
int nlps_gpu_step_record_layout(nlps_gpu *h, int *row_doubles, int *reaction_offset, int *probe_offset, int *probe_doubles);
int nlps_gpu_record_now(nlps_gpu *h, int tag);                              /* one row of the state as it stands */
/* synchronises the handle's stream once.  *total: rows written since the set; *count = min(total, capacity, max_rows);
 * rows: the newest *count rows, oldest first (rows == NULL: the counts only).  1 with no record set. */
int nlps_gpu_read_step_records(nlps_gpu *h, long long *total, int *count, double *rows, int max_rows);
/* the time step of Courant.c: CFL h / Cel, or with a row CFL h / (Cel + row[NLPS_REC_VMAX_COMP]) (DynamicTimeStep) */
double nlps_host_courant_dt(double CFL, double h, double Cel, const double *row /* or NULL */);
/* The particle snapshot: what a driver WRITES a run out by (the particle VTK every N steps of GramsOutputs (i=N), the
 * state a restart starts from) without nlps_gpu_download_state and its stall.  nlps_gpu_snapshot_begin launches one pack
 * kernel on the handle's stream, which gathers the selected fields into a staging block on the device, and queues one
 * asynchronous copy of that block to pinned host memory on a stream of the snapshot's own; the steps that follow run
 * beside the copy.  The caller picks the snapshot up later with nlps_gpu_snapshot_wait.
 *
 * Values: the selected arrays are bit for bit what nlps_gpu_download_state would have returned, had it been called in
 *   place of nlps_gpu_snapshot_begin, in the same layout ([np][ndim] vectors, [np][5 | 9] tensors, Back_stress [np][3],
 *   caller's particle order) -- in every state the handle can be in between two calls: after an explicit step of any
 *   form (non-folded, folded, async lists, deferred move, deterministic, with the damage hooks, with contour loads),
 *   after the level-B stages, after nlps_gpu_newmark_step, after any re-sort, right after create.  The field set is the
 *   n state and the kinematics (what an output reads and what nlps_gpu_create takes back); the n+1 slots, DF, the rate
 *   tensors and C_ep stay with nlps_gpu_download_state.  Damage_n and Strain_f_n are defined for every cloud, as they
 *   are there (0, or what was uploaded, on a cloud without the damage drivers).
 * No writes: begin reads through the pending state and writes nothing to the particle arrays -- x + d_dis and dis +
 *   d_dis of the particles a deferred move has marked, tau and W of the hyperelastic laws after a folded step and rho =
 *   (rho J) / J_n inside the fused scheme are formed in registers with the expressions the download's kernels use, and the
 *   n slots of F and b_e are read under the current renaming.  The steps behind it launch exactly what they would have
 *   launched without it.
 * Cost of begin: the pack kernel and an event record on the handle's stream (in front of the first pack behind a re-sort,
 *   one more kernel that inverts the permutation of the slots), a wait for that event and ONE device-to-host copy on the
 *   snapshot stream.  No allocation (the setter makes every buffer), no synchronisation, no host copy.  The handle's
 *   stream never waits for the snapshot stream, which is not the side stream of the async lists.
 * nlps_gpu_snapshot_wait blocks on that slot's copy alone (not on the handle's stream), sets view->np and the pointers of
 *   the selected fields into the slot's pinned block (every other member NULL) and returns the tag; the pointers are
 *   valid until nlps_gpu_snapshot_release, which frees the slot for the next begin (and, for a slot nobody has waited
 *   for, waits for its copy first).  nlps_host_write_particles_vtk takes them as they are.  A slot may be waited for
 *   more than once.
 * Memory (nlps_gpu_snapshot_bytes): pinned = slots x max(8, np x (8 D + 4 I)) bytes, device = pinned + 4 max(np, 1) (the
 *   inverse permutation, shared with the explicit loads and the step record), np the particle count at the set, D the
 *   doubles per particle of the selected fields (ndim for x, dis, vel, acc, lambda; 5 | 9 for F_n, Stress, b_e_n; 3 for
 *   Back_stress; 1 for the others), I = 1 with NLPS_SNAP_I0.  A slot's block holds the selected fields one after the
 *   other in ascending bit order, the ints of I0 last.
 * Returns 1 with the reason in nlps_gpu_last_error, stores and launches nothing, and leaves the handle usable: the setter
 *   for slots outside [1, NLPS_SNAP_MAX_SLOTS], fields == 0 or a bit outside NLPS_SNAP_*, a failed allocation (the
 *   snapshots set before stay), a migrated handle (its rows are by global id); begin / wait / release / bytes with no
 *   snapshots set; begin with every slot in flight or unreleased, or on a handle that has migrated since the set; wait or
 *   release on a slot that was not begun.  A halo callback or an RCCL exchange changes nothing: the pack is rank-local.
 * A second set replaces the first; cfg == NULL switches the snapshots off.  Both, and nlps_gpu_destroy, wait for the
 * copies in flight before they free. */
enum { NLPS_SNAP_X = 1 << 0, NLPS_SNAP_DIS = 1 << 1, NLPS_SNAP_VEL = 1 << 2, NLPS_SNAP_ACC = 1 << 3,
       NLPS_SNAP_F_N = 1 << 4, NLPS_SNAP_STRESS = 1 << 5, NLPS_SNAP_B_E_N = 1 << 6, NLPS_SNAP_J_N = 1 << 7,
       NLPS_SNAP_RHO = 1 << 8, NLPS_SNAP_MASS = 1 << 9, NLPS_SNAP_VOL0 = 1 << 10, NLPS_SNAP_W = 1 << 11,
       NLPS_SNAP_KAPPA_N = 1 << 12, NLPS_SNAP_EPS_N = 1 << 13, NLPS_SNAP_BACK_STRESS = 1 << 14,
       NLPS_SNAP_DAMAGE_N = 1 << 15, NLPS_SNAP_STRAIN_F_N = 1 << 16, NLPS_SNAP_LAMBDA = 1 << 17,
       NLPS_SNAP_BETA = 1 << 18, NLPS_SNAP_I0 = 1 << 19 };
#define NLPS_SNAP_MAX_SLOTS 4
typedef struct { unsigned fields; int slots; } nlps_snapshot_cfg;       /* slots: snapshots that may be in flight or unreleased */
int nlps_gpu_set_snapshots(nlps_gpu *h, const nlps_snapshot_cfg *cfg);  /* NULL: off, waits for copies in flight, frees */
int nlps_gpu_snapshot_begin(nlps_gpu *h, int tag, int *slot);
int nlps_gpu_snapshot_wait(nlps_gpu *h, int slot, nlps_particles *view, int *tag);
int nlps_gpu_snapshot_release(nlps_gpu *h, int slot);
int nlps_gpu_snapshot_bytes(nlps_gpu *h, size_t *device, size_t *pinned);
/* The damage hooks inside the fused residual (clouds created with driver_eigenerosion or driver_eigensoftening).  Off by
 * default: nlps_gpu_lagrangian_evaluation then runs the separate stages for such a cloud (nlps_gpu_compatibility,
 * nlps_gpu_constitutive, nlps_gpu_internal_forces with its two sorts, the traction and inertial calls), exactly as before.
 * With on != 0 -- and neither NLPS_LAGR_SEPARATE nor NLPS_LAGR_RATES in flags -- the evaluation is the fused damage form,
 * and so are the evaluations of nlps_gpu_newton_solve and nlps_gpu_newmark_step, which call it.  What it computes, in the
 * order of U-Newmark-beta.c:1018-1036:
 *   1. compatibility for every particle: DF, F_n1, J_n1 from the caller's dU, J <= 0 clamped to 0 (:1137-1142);
 *   2. the constitutive update, which skips failed particles (Damage_n == 1: W = 0, stress and the n+1 internal
 *      variables untouched, :1218-1224, as the level-B constitutive stage does); every other particle gets tau, W, b_e,n+1,
 *      kappa_n+1, eps_n+1 and C_ep;
 *   3. the damage hook (:1313-1331): Damage_n1 (and Strain_f_n1) from the n state, then every Kirchhoff stress scaled in
 *      place by 1 - Damage_n1; eigensoftening with the reference's sequential semantics (one particle after the other in
 *      the caller's order);
 *   4. +f_int from the scaled stress, then the traction and inertial terms, 0 on the Dirichlet dofs.
 * The n state is never touched: the residual may be evaluated any number of times from it.  nlps_gpu_tangent_operator
 * scales with 1 - Damage_n1 of the state the evaluation left, nlps_gpu_roll_state rolls Damage and Strain_f, as before.
 * An evaluation runs on one rank, on the handle's stream, without sorts or allocation and with the one synchronisation
 * every fused evaluation ends in (inside nlps_gpu_newton_solve its norm arrives with that wait).  The node runs of the
 * hook are built at the first evaluation and reused until a call that makes the matrix-free operator stale (the list under
 * nlps_gpu_tangent_apply).  In deterministic mode with nlps_gpu_set_deterministic_damage on, the evaluation sums in a fixed
 * order (sorted runs, one wave per tile, slabs) and repeats bit for bit; otherwise a damage cloud sums with atomics.
 * The setter allocates every table (shared with nlps_gpu_set_explicit_damage).  It returns 1, with the reason in
 * nlps_gpu_last_error, for a cloud created without either driver, for a cloud that holds Newtonian-Fluid-Compressible
 * (the state half is cut for the solid laws), and when a halo callback or an RCCL exchange is attached (an
 * epsilon-neighbourhood across a slab face needs ghost particles); an evaluation returns 1 if one is attached later. */
int nlps_gpu_set_implicit_damage(nlps_gpu *h, int on);
/* Number of active nodes after the last search (computes Nodes2Mask on the device). */
int nlps_gpu_num_active(nlps_gpu *h, int *nactive);
/* Nodal results of the last explicit step in masked numbering (any pointer may be NULL).  On one GPU without a ghost
 * exchange the step itself keeps only the nodal sums (mass, momentum, force): dU, accelerations and reactions are made
 * from them by this call (or before a level-B stage overwrites the sums), two small kernels. */
int nlps_gpu_explicit_nodal(nlps_gpu *h, double *mass, double *dU, double *force, double *accel,
                            double *reaction);

/* Maintenance: physically re-sorts the device-resident particle arrays by (tile of the closest node,
 * corner type, closest node) so that memory order keeps matching the tile binning as particles move.
 * Results are unaffected (downloads always use the caller's particle order).  explicit_step calls it
 * every `every_n_steps` steps (default 50, 0 = never). */
int nlps_gpu_resort(nlps_gpu *h);
int nlps_gpu_set_resort_interval(nlps_gpu *h, int every_n_steps);
/* Adaptive re-sort of the fused explicit step (ON by default with budget 0.8, min_steps 4, whenever the interval above
 * is not 0; off in deterministic mode: the trigger reads a count the device publishes asynchronously, so the step that
 * re-sorts -- never a result beyond rounding -- can differ from run to run): the search stage counts the particles that are no
 * longer in the tile their memory slot was sorted into; every step adds that share of the cloud to a debt, and when
 * the debt since the last re-sort exceeds `budget` (and at least min_steps steps have passed) the step re-sorts ahead
 * of the interval above.  budget = 0 switches it off; an interval of 0 switches every re-sort off.  A budget of 0.6
 * is about the cost of one re-sort in units of the slowdown displaced particles cause.  No reference
 * counterpart (the CPU path has no memory order to keep). */
int nlps_gpu_set_adaptive_resort(nlps_gpu *gpu, double budget, int min_steps);

/* ------------------------------------------------------------------ multi-GPU: ghost-layer exchange over RCCL, owned by
 * the library.  One process per GPU; the particles are range-partitioned into slabs along the slowest grid
 * axis, rank r touches node layers [layer_lo[r], layer_hi[r]] (inclusive, every rank passes the ranges of ALL ranks).
 * After every nodal scatter of a stage function or of the fused explicit step the layers shared with rank r-1 / r+1
 * are summed (doubles) or OR-ed (activation flags): ncclSend / ncclRecv of the two contiguous slices on a
 * library-owned stream, behind the tiles that do not touch a shared layer (mode 0), or one ncclAllReduce of the whole
 * array (mode 1, BASELINE.json's wording).  librccl.so.1 is dlopen()ed at attach time.
 * nlps_gpu_rccl_unique_id: rank 0 makes the 128-byte ncclUniqueId, the host driver hands it to the other ranks
 * (MPI_Bcast, a file, ...).  _attach creates the communicator (ncclCommInitRank, collective), restricts the per-step
 * nodal work to the rank's layers (nlps_gpu_set_node_window) and declares the shared layers (nlps_gpu_set_ghost_bands);
 * _attach_comm takes an existing ncclComm_t.  Call before nlps_gpu_initialize_lme.
 * nlps_gpu_rccl_reduce: implicit driver on several ranks -- a masked vector (device pointer, n doubles: residual,
 * lumped mass) summed onto `root`, the rank that runs the PETSc solve, or onto all ranks (root < 0). */
int nlps_gpu_rccl_unique_id(void *id128);
int nlps_gpu_rccl_attach(nlps_gpu *h, const void *id128, int rank, int world, const int *layer_lo,
                         const int *layer_hi, int mode);
int nlps_gpu_rccl_attach_comm(nlps_gpu *h, void *nccl_comm, int rank, int world, const int *layer_lo,
                              const int *layer_hi, int mode);
int nlps_gpu_rccl_detach(nlps_gpu *h);
int nlps_gpu_rccl_reduce(nlps_gpu *h, double *vec, size_t n, int root);
/* What the attached communicator reports (ncclCommCount, ncclCommUserRank) and the overlap choreography in force
 * (0 blocking exchanges, 1 split launches, 2 one launch per stage); any pointer may be NULL. */
int nlps_gpu_rccl_info(nlps_gpu *h, int *nranks, int *rank, int *overlap_mode);
/* world-size-1 self-test of the exchange (one-GPU boxes): the rank is its own two neighbours -- the lowest three
 * layers of its range are exchanged with the highest three by ncclSend / ncclRecv to itself; overlap = the two-phase
 * (side-stream) form. */
int nlps_gpu_rccl_selftest_exchange(nlps_gpu *h, void *dptr, int nfield, int elem_bytes, int kind, int overlap);

/* Clouds whose materials follow several laws (Constitutive.c:28-258 dispatches per particle on MatProp.Type): the
 * fused stress stage runs either as one launch per law of the kernel compiled for that law (mode 1: right when the
 * materials sit in blocks, nearly every tile of closest nodes then holds one law) or as one kernel that dispatches on
 * the law at run time (mode 2: right when the laws are interleaved particle by particle).  nlps_gpu_create picks the
 * mode from the share of tiles that hold more than one law; results are identical.  Mode 2 is refused for a cloud that
 * holds Matsuoka-Nakai / Lade-Duncan or Newtonian-Fluid-Compressible: the dispatch kernel does not hold those laws. */
int nlps_gpu_set_law_launch_mode(nlps_gpu *h, int mode);

/* Run-to-run bit-reproducible results ("race detection"): with on != 0 every nodal sum is accumulated in a
 * FIXED order -- the per-tile particle lists are sorted exactly, one wave per tile accumulates its list into a window of
 * its own, the windows leave the workgroup as plain copies (slabs) and are combined per node in index order (no
 * floating-point atomics between workgroups).  Slower than the default path (atomic accumulation in arrival order);
 * same results to rounding.  Two runs from the same inputs then agree bit for bit, on one rank, with host or device
 * vectors, in:
 *   - nlps_gpu_explicit_step (the fused explicit step);
 *   - the implicit path: nlps_gpu_lumped_mass, nlps_gpu_nodal_field_n, nlps_gpu_internal_forces, the traction sums
 *     (nlps_gpu_nodal_traction_forces and the loads of the residual: one wave over the contour particles in the
 *     caller's order), nlps_gpu_lagrangian_evaluation (fused and NLPS_LAGR_SEPARATE), nlps_gpu_tangent_apply,
 *     nlps_gpu_tangent_block_diagonal, and what is built from them: nlps_gpu_tangent_solve, nlps_gpu_newton_solve,
 *     nlps_gpu_newmark_step (their norms, dot products and step lengths add per-block partials in a fixed order).
 * The mode may be switched between calls.  Tile lists that a search built with the mode off are not exact; the first
 * implicit-path call made with the mode on sorts them exactly before it sums over them (nothing to do for the caller).
 * The window slabs are allocated at the first call that needs them: 12 x 800 (3-D, per tile of 4^3 closest nodes) or
 * 8 x 400 (2-D, per tile of 16^2) doubles per tile of the grid.
 * The assembled tangent is inside the contract in its CSR form (nlps_gpu_tangent_csr_pattern / nlps_gpu_tangent_csr,
 * which hold no floating-point atomic in any mode).
 * Outside the contract, on their usual (atomic) path in every mode: the COO form of the assembled tangent
 * (nlps_gpu_tangent_assemble / nlps_gpu_tangent_coo); clouds created with driver_eigenerosion / driver_eigensoftening (the damage hooks, in the
 * separate stages and in the fused form of nlps_gpu_set_implicit_damage alike) unless nlps_gpu_set_deterministic_damage
 * is on -- without it the explicit step refuses such a cloud in the mode; handles
 * with a halo-exchange callback or an RCCL exchange attached; the folded, lazy and async-lists forms of the explicit
 * step, which the mode does not use.
 * Switching the mode drops the cached node runs of the damage hooks (they are rebuilt by the next step or evaluation). */
int nlps_gpu_set_deterministic(nlps_gpu *h, int on);
/* Deterministic mode for clouds created with driver_eigenerosion or driver_eigensoftening.  Off by default: such a cloud
 * then stays outside the contract above (the explicit step refuses it in the mode, the implicit path sums with atomics).
 * With on != 0 AND nlps_gpu_set_deterministic on, on one rank, the contract above also holds for a damage cloud in
 * nlps_gpu_explicit_step (with nlps_gpu_set_explicit_damage), nlps_gpu_lumped_mass, nlps_gpu_nodal_field_n,
 * nlps_gpu_internal_forces with its hook, nlps_gpu_lagrangian_evaluation (NLPS_LAGR_SEPARATE, the separate stages of
 * nlps_gpu_set_implicit_damage off, the fused damage form), nlps_gpu_tangent_apply, nlps_gpu_tangent_block_diagonal,
 * nlps_gpu_tangent_solve, nlps_gpu_newton_solve and nlps_gpu_newmark_step: the particles of every node run of the hooks
 * are visited in ascending memory slot, so the threshold decisions G_p > Gf and T_eps > ft read sums made in one order,
 * and the nodal forces under them come from one wave per tile and a fixed-order sum of window slabs.  Damage decisions
 * and every downloaded array then repeat bit for bit between two runs from the same inputs.
 * nlps_gpu_tangent_csr_pattern / nlps_gpu_tangent_csr repeat bit for bit for a damage cloud as well.
 * Still refused or outside the contract: a halo callback or an RCCL exchange, the fluid law, the COO form of the
 * assembled tangent (nlps_gpu_tangent_assemble / nlps_gpu_tangent_coo).
 * The setter allocates the run tables and the window slabs (no step or evaluation allocates) and drops the cached node
 * runs.  It returns 1, with the reason in nlps_gpu_last_error, for a cloud created without either driver. */
int nlps_gpu_set_deterministic_damage(nlps_gpu *h, int on);

/* ------------------------------------------------------------------ per-dof updates of the implicit driver (a21)
 * Vectors of N_A*d doubles in masked numbering, host (VecGetArray) or device pointers.  alpha = the six Newmark
 * parameters alpha_1..alpha_6 of __compute_Newmark_parameters (U-Newmark-beta.c:497-514). */
/* __form_initial_guess, :879-957: optional explicit trial dU = dt*Un_dt + dt^2/2*Un_dt2, then the Dirichlet
 * values of the active boundary dofs at `step` */
int nlps_gpu_form_initial_guess(nlps_gpu *h, double *dU, const double *Un_dt, const double *Un_dt2, double dt,
                                int use_explicit_trial, const nlps_bcc *bcc, int nbcc, int step);
/* __compute_nodal_velocity_increments / __compute_nodal_kinetic_increments, :1834-1906 (either output may be NULL) */
int nlps_gpu_nodal_kinetic_increments(nlps_gpu *h, double *dU_dt, double *dU_dt2, const double *dU,
                                      const double *Un_dt, const double *Un_dt2, const double *alpha);
/* __nodal_inertial_forces, :1519-1557: R += M (alpha_1 dU - alpha_2 Un_dt - alpha_3 Un_dt2 - b) on the free dofs */
int nlps_gpu_nodal_inertial_forces(nlps_gpu *h, double *R, const double *M, const double *dU, const double *Un_dt,
                                   const double *Un_dt2, const double *alpha, const double *gravity);

/* __lagrangian_evaluation, U-Newmark-beta.c:970-1058 -- the callback SNES runs at every Newton iterate and every
 * line-search trial of the maintained driver -- as ONE call: VecZeroEntries(R), then
 *   __compute_nodal_velocity_increments (:1018), __local_compatibility_conditions (:1021-1022),
 *   __constitutive_update (:1026), __nodal_internal_forces (:1028-1029), __nodal_traction_forces (:1031-1032),
 *   __nodal_inertial_forces (:1034-1036).
 * On the device: the caller's dU is gathered, DF / F_n1 / J_n1 (J <= 0 clamped to 0 like :1137-1142), the stress update
 * and the scatter of the internal force run as ONE pass over the particles with DF and tau handed over in registers
 * (what nlps_gpu_compatibility + _constitutive + _internal_forces do in three passes with DF, F_n1, tau through HBM in
 * between), then one nodal kernel adds the traction and inertial terms and leaves 0 on the Dirichlet dofs.
 * The particle state afterwards is what the three separate stages leave: DF, F_n1, J_n1, Stress, W, b_e_n1, Kappa_n1,
 * EPS_n1, C_ep (the n state is not touched: the residual is evaluated many times from it), so
 * nlps_gpu_tangent_assemble / nlps_gpu_roll_state / nlps_gpu_update_kinetics follow it exactly as they follow the stages.
 * R, dU, Un_dt, Un_dt2, M: masked [N_A*d], host (VecGetArray) or device pointers; R is OVERWRITTEN.  alpha[6] as for
 * the per-dof updates above, gravity[ndim] or NULL, loads / nloads / step / thickness / area0 as for
 * nlps_gpu_nodal_traction_forces (nloads = 0: none).  Needs nlps_gpu_local_search + nlps_gpu_active_masks first.
 * A cloud that holds the Newtonian-Fluid-Compressible law carries the rate tensors by itself, no flag needed: its
 * particles run the same one pass with a second gather window of dU_dt = alpha_4 dU + (alpha_5 - 1) Un_dt + alpha_6 Un_dt2
 * (:1834-1870), dt_DF and dt_F_n1 = dt_DF F_n + DF dt_F_n stay in registers for the stress and are stored with the rest;
 * in a mixed cloud the solids' launches are the ones above.
 * flags: NLPS_LAGR_RATES   also the rate tensors dt_DF, dt_F_n1 (compute-Strains.c:48-72,176-207) for a cloud WITHOUT the
 *                          fluid law, where nothing reads them: off by default -- runs the separate stages;
 *        NLPS_LAGR_SEPARATE the composition of the separate stage calls (same results; what the fused form is tested and
 *                          timed against).  The separate stages also run when the damage hooks are on
 *                          (driver_eigenerosion / _eigensoftening: every stress before any force).  A cloud of several laws
 *                          runs one fused launch per law present.
 *        NLPS_LAGR_SAME_STEP host vectors only: Un_dt, Un_dt2 and M are the ones of the previous evaluation (they do not
 *                          change inside one SNES solve, U-Newmark-beta.c:241-300): their device copies are reused, an
 *                          evaluation then moves dU in and R out and nothing else (2 of 5 transfers).  An error without an
 *                          earlier evaluation since nlps_gpu_active_masks. */
enum { NLPS_LAGR_RATES = 1, NLPS_LAGR_SEPARATE = 2, NLPS_LAGR_SAME_STEP = 4 };
int nlps_gpu_lagrangian_evaluation(nlps_gpu *h, double *R, const double *dU, const double *Un_dt, const double *Un_dt2,
                                   const double *M, const double *alpha, const double *gravity, const nlps_bcc *loads,
                                   int nloads, int step, double thickness, const double *area0, int flags);

/* ------------------------------------------------------------------ tangent assembly */

/* __jacobian_evaluation (U-Newmark-beta.c:1646-1830) with stiffness_density__Constitutive__
 * (Constitutive.c:262-381): Neo-Hookean (Hyperelastic/Neo-Hookean.c:89-141), Hencky (Hencky.c:98-229) and
 * Drucker-Prager (Plasticity/Elastoplastic-Tangent-Matrix.c:42-163, with the C_ep of the last constitutive
 * update).  The d x d blocks V0 * stiffness_density(A, B) of every node pair a particle connects are summed on
 * the device, from the state the compatibility + constitutive stages left (DF, F_n, F_n1, J_n1, tau, b_e,n+1,
 * C_ep) and the current lists / lambda.  The Newtonian-Fluid-Compressible law (Fluid/Newtonian-Fluid.c:83-190) is taken
 * too, from F_n, F_n1, dt_F_n1, J_n1 and alpha_4 (nlps_gpu_set_tangent_alpha4); its blocks are not symmetric.  *nnz = number of COO entries = d*d * (number of structurally visited node
 * pairs, the reference's sparsity pattern).  Needs nlps_gpu_active_masks() first. */
int nlps_gpu_tangent_assemble(nlps_gpu *h, long long *nnz);
/* grouped != 0 (default): one workgroup per closest node sums the blocks of the particles sharing it before the
 * atomics; 0: one wave per particle (kept for comparison, same result up to summation order). */
int nlps_gpu_tangent_set_grouped(nlps_gpu *h, int grouped);
/* The assembled matrix as COO triplets (masked dof numbering, every visited pair present even when its value is
 * zero, like MatSetValues ... ADD_VALUES): rows[nnz], cols[nnz], vals[nnz], host or device pointers.
 * lumped_mass (masked [N_A*d], may be NULL): alpha_1 * M is added on the diagonal (:1797-1807).
 * apply_dirichlet != 0: rows and columns of the dofs fixed at the step given to nlps_gpu_active_masks() become
 * identity rows (MatZeroRowsColumnsIS, :1822). */
int nlps_gpu_tangent_coo(nlps_gpu *h, double alpha_1, const double *lumped_mass, int apply_dirichlet, int *rows,
                         int *cols, double *vals);
/* __create_sparsity_pattern (U-Newmark-beta.c:1568-1632): visited columns per dof row, nnz_per_row[N_A*d] */
int nlps_gpu_sparsity_pattern(nlps_gpu *h, int *nnz_per_row);
/* alpha_4 of the Newmark scheme (gamma / (beta dt), __compute_Newmark_parameters :497-514) for the tangent of the
 * Newtonian-Fluid-Compressible law, the one law whose stiffness density reads it (Constitutive.c:298-314: the velocity
 * increment is alpha_4 dU, so the viscous stress depends on dU through it).  Read by nlps_gpu_tangent_assemble and
 * nlps_gpu_tangent_operator at their next call; default 0, the quasi-static value.  nlps_gpu_newton_solve and
 * nlps_gpu_newmark_step set it from alpha[3] themselves.  The other laws ignore it. */
int nlps_gpu_set_tangent_alpha4(nlps_gpu *h, double alpha_4);

/* ------------------------------------------------------------------ matrix-free tangent (MatShell of __jacobian_evaluation)
 * The same K as nlps_gpu_tangent_assemble + nlps_gpu_tangent_coo, never formed: every block is bilinear in the
 * particle's two LME gradients, K_AB[i][j] = sum_mn gn_A[m] gn_B[n] Dh[m][n][i][j] with ONE fourth-order tensor per
 * particle (Dh = V0 DF^-1 D DF^-T pulled into the reference frame; V0 -> V0 (1 - Damage_n1) with the damage hooks on),
 * so y = K x is a gather of x over the particle's members, a d^4 contraction and a scatter: O(members) work and memory
 * that grows with the particle count only.  Same laws as the assembly, per particle (mixed clouds included).
 * nlps_gpu_tangent_operator linearises at the current particle state (what the residual call or the compatibility +
 * constitutive stages left), same inputs as nlps_gpu_tangent_coo: lumped_mass (masked [N_A*d], host or device, may be
 * NULL) adds alpha_1 M on the diagonal, apply_dirichlet != 0 makes the dofs fixed at the step of nlps_gpu_active_masks
 * identity rows and columns.  It SNAPSHOTS the linearisation (Dh per particle, alpha_1 M, the Dirichlet choice): later
 * residual evaluations (line-search trials) do not change it.  Particles whose J or DF does not invert raise the flags
 * and the error of nlps_gpu_tangent_assemble.  *bytes (may be NULL) = device memory this linearisation needs, by the
 *   formula 8 * (d^4 np + N_A d + d^2 nnodes)  -- 81 doubles per particle in 3-D, 16 in 2-D, plus a masked vector and
 *   a d^2-field grid array (the assembled path: 8 d^2 (9^d nnodes + triplets) bytes and more).  The buffers are kept
 *   and only grow, so after a larger earlier linearisation the handle may hold more.  nlps_gpu_tangent_block_diagonal
 *   with a host destination also keeps a staging buffer of 8 N_A d^2 bytes on the handle (not in *bytes).
 * A failed allocation returns 1 with the reason in nlps_gpu_last_error.
 * nlps_gpu_tangent_apply: y = K x (MATOP_MULT), x and y masked [N_A*d], host or device pointers; y is overwritten, x is
 * not touched.  nlps_gpu_tangent_block_diagonal: the N_A d x d diagonal blocks of K, row-major, in masked node order,
 * blocks[N_A*d*d], host or device (MATOP_GET_DIAGONAL / point-block Jacobi).
 * Both fail with a message naming the cause, never with a stale result, before any nlps_gpu_tangent_operator and after
 * any call that moves, reorders or re-lists particles: nlps_gpu_local_search, nlps_gpu_active_masks, a re-sort
 * (nlps_gpu_resort, periodic or adaptive), a migration, nlps_gpu_update_kinetics, nlps_gpu_roll_state and
 * nlps_gpu_explicit_step.  Several ranks: the scattered K x (and the blocks) pass the halo exchange hook before the
 * nodal epilogue, like the residual call; every rank's x must agree on the shared nodes, as its dU does.
 * Sums use floating-point atomics, so results agree with the assembled matrix times x up to summation order; in
 * deterministic mode (nlps_gpu_set_deterministic, one rank) both calls sum in a fixed order and repeat bit for bit. */
int nlps_gpu_tangent_operator(nlps_gpu *h, double alpha_1, const double *lumped_mass, int apply_dirichlet, size_t *bytes);
int nlps_gpu_tangent_apply(nlps_gpu *h, const double *x, double *y);
int nlps_gpu_tangent_block_diagonal(nlps_gpu *h, double *blocks);

/* nlps_gpu_tangent_solve: K x = b for the operator of the last nlps_gpu_tangent_operator, by restarted GMRES(restart) on
 * the device -- the driver's KSPSolve (GMRES(30) + PCJACOBI, U-Newmark-beta.c:270-336) in one call.  b and x are masked
 * [N_A*d], host or device pointers (a host vector crosses PCIe once per solve); b is not touched.
 * Right preconditioning, K M^-1 u = b, x = M^-1 u: the stopping test sees the unpreconditioned residual ||b - K x||
 * (PETSc's default is left preconditioning and the preconditioned norm).  Classical Gram-Schmidt with one more pass when
 * the norm drops below 1/sqrt 2 of its value (DGKS, PETSc's refine_ifneeded).  Iterations are Arnoldi steps summed over
 * the restarts.  Every cycle ends with the true residual b - K x (one product): it confirms a converged estimate or
 * starts the next cycle.  history[0] = ||b - K x0||, history[k] = the estimate after step k.
 * Preconditioners: NLPS_PC_JACOBI the reciprocal diagonal of K (PCJACOBI), NLPS_PC_PBJACOBI the inverted d x d diagonal
 * blocks (PCPBJACOBI), built from nlps_gpu_tangent_block_diagonal's blocks once per successful
 * nlps_gpu_tangent_operator and reused by the solves that follow on the same linearisation.  A block whose pivot (or a
 * diagonal entry) is at or below 1e-14 of the block's Frobenius norm fails the call, naming the masked node.
 * Returns 1 for misuse, a HIP failure, a preconditioner that does not invert, before any nlps_gpu_tangent_operator and
 * after anything that makes the operator stale (as nlps_gpu_tangent_apply), and on a handle that exchanges halos (a halo
 * callback or an RCCL world > 1: single rank only).  Returns 0 when the solve ran, converged or not (ksp->reason).
 * bytes = 8 * ((restart + 3) n + (restart + 2) nb + 6 (restart + 2) + 8 + restart (restart + 1) + [pc] N_A d^2) with
 *   n = N_A d, nb = ceil(n / 512): the basis, two work vectors, per-block partial sums, the Hessenberg state and the
 *   preconditioner (pc != NLPS_PC_NONE).  Kept on the handle and only grown, like the operator's buffers. */
enum { NLPS_PC_NONE = 0, NLPS_PC_JACOBI = 1, NLPS_PC_PBJACOBI = 2 };
enum {
  NLPS_KSP_CONVERGED_BZERO = 1,     /* b == 0: x = 0 */
  NLPS_KSP_CONVERGED_RTOL = 2,      /* ||b - K x|| <= rtol ||b|| */
  NLPS_KSP_CONVERGED_ATOL = 3,      /* ||b - K x|| <= atol */
  NLPS_KSP_DIVERGED_ITS = -3,       /* max_it steps without convergence */
  NLPS_KSP_DIVERGED_DTOL = -4,      /* ||b - K x|| > dtol ||b|| */
  NLPS_KSP_DIVERGED_BREAKDOWN = -5, /* the Hessenberg matrix is singular (K M^-1 singular on the Krylov space) */
  NLPS_KSP_DIVERGED_INDEFINITE_PC = -8, /* MINRES only: v . M^-1 v < 0 (<= 0 at r0), M^-1 is not positive definite */
  NLPS_KSP_DIVERGED_NANORINF = -9   /* a non-finite value: x is the one of the last finished cycle */
};
#define NLPS_KSP_MAX_RESTART 256
typedef struct {
  /* in */
  int pc;         /* NLPS_PC_* */
  int restart;    /* Krylov vectors per cycle, 1 .. NLPS_KSP_MAX_RESTART (the driver's default 30) */
  int max_it;     /* Arnoldi steps over all cycles */
  int x_is_guess; /* 0: x0 = 0 (x is only written), else x holds the initial guess */
  double rtol, atol, dtol; /* converged: ||b - K x|| <= max(rtol ||b||, atol); diverged: > dtol ||b|| (at a cycle's end) */
  double *history;         /* host array of max_it + 1 residual norms, or NULL (KSPSetResidualHistory) */
  /* out */
  int reason;     /* NLPS_KSP_*: > 0 converged, < 0 not */
  int iterations; /* Arnoldi steps taken */
  double rnorm;   /* ||b - K x|| of the returned x (the true residual, from one product) */
  double bnorm;   /* ||b|| */
  size_t bytes;   /* device workspace this solve holds, by the formula above */
} nlps_ksp;
int nlps_gpu_tangent_solve(nlps_gpu *h, const double *b, double *x, nlps_ksp *ksp);

/* nlps_gpu_set_linear_solver: which Krylov method nlps_gpu_tangent_solve runs on this handle, and with it
 * nlps_gpu_newton_solve and nlps_gpu_newmark_step, which call it.  NLPS_KSP_TYPE_GMRES (the default) is the solve above,
 * unchanged.  NLPS_KSP_TYPE_MINRES is a preconditioned MINRES for a SYMMETRIC tangent: a short recurrence, one product
 * per step, no basis and no restart, and no need for K to be positive definite (the Neo-Hookean tangent at a general
 * Newton iterate is not).  The setter returns 1, names the cloud's laws in nlps_gpu_last_error and leaves the handle on
 * its previous solver unless every particle is Neo-Hookean (the rule of NLPS_BSR_UPPER; damage, alpha_1 M and the
 * Dirichlet choice keep K symmetric); it also returns 1 for a type other than the two.
 * With MINRES selected ksp->restart is not read; pc, max_it, x_is_guess, rtol, atol, dtol, history, reason, iterations,
 * rnorm, bnorm and bytes mean what they mean for GMRES, and the call refuses what the GMRES form refuses (no operator, a
 * stale operator, a halo callback or an RCCL world > 1, missing arguments, negative tolerances), with the same messages.
 * M^-1 is none, the reciprocal diagonal or the inverted diagonal blocks of the GMRES form (built once per linearisation
 * and shared with it); it must be positive definite.  tol = max(rtol ||b||, atol).  The algorithm:
 *
 *   x = x0 (0 unless x_is_guess);  r0 = b - K x (no product for x0 = 0);  rnorm = ||r0||;  history[0] = rnorm
 *   ahead of the first step, in GMRES's order: ||b|| == 0 -> BZERO, x = 0;  non-finite -> NANORINF;  rnorm <= tol ->
 *     ATOL / RTOL;  rnorm > dtol ||b|| -> DTOL;  max_it == 0 -> ITS
 *   v_prev = 0, v = r0, z = M^-1 v, g = sqrt(v.z)  (v.z <= 0: INDEFINITE_PC, not finite: NANORINF, 0 iterations)
 *   g_prev = 1, eta = g, scale = rnorm / g, c_prev = c = 1, s_prev = s = 0, w_prev = w = 0
 *   step k = 1, 2, ...:
 *     q = z / g;  p = K q;  d = p.q
 *     v_new = p - (d / g) v - (g / g_prev) v_prev;   z_new = M^-1 v_new;   gg = v_new.z_new
 *     gg < 0 -> INDEFINITE_PC;  d, gg not finite -> NANORINF   (in both the step's update of x is NOT applied)
 *     g_new = sqrt(gg)
 *     a0 = c d - c_prev s g;  a1 = sqrt(a0^2 + gg);  a2 = s d + c_prev c g;  a3 = s_prev g
 *     a1 == 0 -> BREAKDOWN (no update)
 *     (c_prev, c) = (c, a0 / a1);  (s_prev, s) = (s, g_new / a1)
 *     w_new = (q - a3 w_prev - a2 w) / a1;   x += c eta w_new;   eta = -s eta
 *     shift (v_prev, v, z, g_prev, g, w_prev, w);   iterations = k;   est = scale |eta|;   history[k] = est
 *     est not finite -> NANORINF
 *     if est <= tol or k == max_it or g_new == 0:           -- confirmation, one product, read-only for the recurrence
 *        rnorm = ||b - K x||;  not finite -> NANORINF;  rnorm <= tol -> ATOL (rnorm < atol) / RTOL;
 *        rnorm > dtol ||b|| -> DTOL;  k == max_it -> ITS;  g_new == 0 -> BREAKDOWN;
 *        otherwise scale = rnorm / |eta| and the SAME recurrence goes on
 *
 * est is the preconditioned residual norm ||r||_{M^-1}, which MINRES minimises and which never grows, calibrated to the
 * true norm at r0 and at every confirmation that did not end the solve (the history steps up there).  The recurrence is never restarted.  ksp->rnorm
 * is always the true residual ||b - K x|| of the returned x, from one product, also where a step ends the solve without a
 * confirmation (INDEFINITE_PC, BREAKDOWN and NANORINF inside a step); iterations counts the steps whose update x holds.
 * One host wait per step and one per confirmation; the rotation's coefficients stay on the device.
 * bytes = 8 * (7 n + nb + nbn + 16 + [pc] N_A d^2) with n = N_A d, nb = ceil(n / 512) and nbn = ceil(N_A / 256): two
 *   Lanczos vectors, z, q, p, two direction vectors, the per-block partial sums of the element and of the node kernels,
 *   the rotation state and the preconditioner.  The buffers are the ones of the GMRES form (shared, kept on the handle
 *   and only grown): for the same n less than GMRES(restart) from restart = 5 on.
 * Every sum is taken over per-block partials in a fixed order (no float atomics of its own): in deterministic mode
 * (nlps_gpu_set_deterministic) a solve repeats bit for bit. */
enum { NLPS_KSP_TYPE_GMRES = 0, NLPS_KSP_TYPE_MINRES = 1 };
int nlps_gpu_set_linear_solver(nlps_gpu *h, int type);

/* nlps_gpu_tangent_lambda_max: the largest Ritz value theta of the pencil (K, M) on the free dofs, by Lanczos on the
 * device -- the omega_max^2 that bounds the explicit step's stable dt (nlps_host_critical_dt), where the deck's
 * CFL h / Cel (nlps_host_courant_dt, Courant.c:6-56) knows nothing of the cloud's gradients or its light rim nodes.
 * K is the operator of the last nlps_gpu_tangent_operator, whatever alpha_1 and mass that was built with: with
 * alpha_1 != 0 and the same mass the result is omega^2 + alpha_1.  lumped_mass and v0 are masked [N_A*d], host or device
 * pointers, neither is touched; mode (masked [N_A*d], host or device, may be NULL) is written.
 * A = P S K S P, S = diag(M^-1/2), P zeroes the dofs the operator's Dirichlet snapshot fixes (apply_dirichlet = 0: P = I).
 *   1. q_1 = P v0 / ||P v0||.  v0 is used as it is, in the scaled space.  v0 == NULL: component i (i = masked node * d +
 *      direction) is 2 u - 1 in [-1, 1) with u = (z >> 11) * 2^-53 and z the splitmix64 output of 64-bit wrapping arithmetic
 *        z = seed + (i + 1) * 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *        z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z = z ^ (z >> 31).
 *   2. For j = 1 .. max_it:  w = A q_j;  alpha_j = q_j . w;  w is orthogonalised against every q_i, i <= j, by classical
 *      Gram-Schmidt with one more pass when ||w|| drops below 1/sqrt 2 of its value (DGKS, the rule and the kernels of
 *      nlps_gpu_tangent_solve);  beta_j = ||w||;  T_j = tridiag(alpha_1..alpha_j ; beta_1..beta_{j-1}) and (theta_j, s) its
 *      largest eigenpair, ||s|| = 1 (one wave on the device: Sturm-count multisection to the last bits of ||T||, the
 *      vector by the twisted factorisation);  est_j = beta_j |s_j|;  history[j-1] = theta_j.  Stop, in this order: a
 *      non-finite value NLPS_EIG_DIVERGED_NANORINF; est_j <= rtol |theta_j| (beta_j == 0 included) NLPS_EIG_CONVERGED;
 *      j == max_it NLPS_EIG_DIVERGED_ITS.  q_{j+1} = w / beta_j.  One host wait per step.
 *   3. y = Q s and resid = ||A y - theta y|| from one more product: the TRUE residual.  For a symmetric K an eigenvalue
 *      of the pencil lies within resid of theta, and theta <= lambda_max: pass theta + resid to nlps_host_critical_dt.
 *   4. mode = S y: M-normalised (mode^T M mode = 1) and exactly 0 on the fixed dofs.  Not a converged run
 *      (NLPS_EIG_DIVERGED_ITS) still returns its theta, resid and mode; NLPS_EIG_DIVERGED_NANORINF (resid = NaN) and
 *      NLPS_EIG_EMPTY write a zero mode.
 * asymmetry = max over j of sqrt(sum_{i<j-1} (q_i . w)^2 + ((q_{j-1} . w) - beta_{j-1})^2) / |theta_j|, from the first
 *   Gram-Schmidt pass of step j: what a symmetric A makes zero.  Rounding noise for a symmetric tangent (Neo-Hookean); of
 *   the order of the tangent's own asymmetry for the laws whose assembled tangent is not symmetric (Hencky,
 *   Drucker-Prager: max|K - K^T| / max|K| of a few 1e-3).  The iteration treats A as symmetric all the same: for such
 *   laws theta is the Ritz value of the symmetric recurrence, close to the largest eigenvalue of A's symmetric part, and
 *   the bracket of 3. does not hold to the letter.
 * No free dof, or P v0 == 0: returns 0 with reason NLPS_EIG_EMPTY, iterations 0, theta 0.
 * Returns 1, with the reason in nlps_gpu_last_error and the handle usable, where nlps_gpu_tangent_solve does (no
 * operator, a stale operator, a halo callback or an RCCL world > 1) and for lumped_mass == NULL, max_it outside
 * 1 .. NLPS_KSP_MAX_RESTART, rtol < 0, eig == NULL, and a mass entry <= 0 or not finite on a free dof (found by the kernel
 * that builds S, ahead of any product; the message names the masked node).
 * bytes = 8 * ((max_it + 4) n + (max_it + 2) nb + nbg + 5 (max_it + 2) + 8) with n = N_A d, nb = ceil(n / 512) and
 *   nbg = ceil(nnodes / 256): the basis, S P, two work vectors, per-block partial sums and T's state.  The buffers are the
 *   ones of nlps_gpu_tangent_solve (shared, kept on the handle and only grown): no allocation once a call has sized them.
 * In deterministic mode (nlps_gpu_set_deterministic) the call repeats bit for bit: the product does, and every sum here
 * is taken in a fixed order (no float atomics of its own). */
enum {
  NLPS_EIG_CONVERGED = 1,          /* est_j <= rtol |theta_j| */
  NLPS_EIG_EMPTY = 2,              /* no free dof or P v0 == 0: nothing to iterate on */
  NLPS_EIG_DIVERGED_ITS = -3,      /* max_it steps without convergence (rtol = 0: the run asked for) */
  NLPS_EIG_DIVERGED_NANORINF = -9  /* a non-finite value */
};
typedef struct {
  /* in */
  int max_it;              /* Lanczos steps, 1 .. NLPS_KSP_MAX_RESTART */
  double rtol;             /* stop when est_j <= rtol |theta_j|; 0: run max_it steps */
  unsigned long long seed; /* start vector when v0 == NULL */
  double *history;         /* host array of max_it values theta_j, or NULL */
  /* out */
  int reason, iterations;  /* NLPS_EIG_*: > 0 converged or empty, < 0 not; Lanczos steps taken */
  double theta;            /* largest Ritz value of the pencil (K, M) on the free dofs */
  double resid;            /* ||A y - theta y||, the true residual, from one product */
  double asymmetry;        /* see above */
  size_t bytes;            /* device workspace this call holds, by the formula above */
} nlps_eig;
int nlps_gpu_tangent_lambda_max(nlps_gpu *h, const double *lumped_mass, const double *v0 /* or NULL */, nlps_eig *eig,
                                double *mode /* or NULL */);
/* The stable step of the explicit scheme (K2 / K5: the Newmark family at beta = 0) from omega2 = omega_max^2:
 * safety * sqrt(2 / gamma) / sqrt(omega2), the undamped limit Omega_crit = (gamma / 2 - beta)^-1/2; 2 / omega at
 * gamma = 1/2.  +inf for omega2 <= 0, -1 for gamma < 0.5.  Callers pass theta + resid.  Host only. */
double nlps_host_critical_dt(double omega2, double gamma, double safety);

/* ------------------------------------------------------------------ nonlinear solve and the implicit time step
 * nlps_gpu_newton_solve: the SNESSolve of the maintained driver (U-Newmark-beta.c:270-356) in one call -- Newton with a
 * line search around nlps_gpu_lagrangian_evaluation (the residual R), nlps_gpu_tangent_operator and
 * nlps_gpu_tangent_solve, with every vector on the device from the first residual to the returned dU.
 * dU: the initial guess on entry and the solution on return, masked [N_A*d], host or device like every other vector of
 * the call.  Un_dt, Un_dt2, M, alpha, gravity, loads, nloads, step, thickness, area0: as for
 * nlps_gpu_lagrangian_evaluation; alpha[0] is the alpha_1 of the operator, zeros in alpha give the quasi-static driver.
 * The algorithm (it follows SNESSolve_NEWTONLS, SNESConvergedDefault and the bt line search with their defaults, and it
 * is the definition of this call):
 *   F = R(X), fnorm0 = ||F||.  fnorm0 not finite: FNORM_NAN.  fnorm0 < atol: FNORM_ABS after 0 iterations.
 *   While iterations < max_it:
 *     1. nlps_gpu_tangent_operator(alpha[0], M, apply_dirichlet) at the state the last residual left.
 *     2. K Y = F by nlps_gpu_tangent_solve with snes->ksp and x0 = 0.  ksp.reason < 0: DIVERGED_LINEAR_SOLVE (PETSc's
 *        default of one allowed failure); X stays as it is.
 *     3. The line search: X <- X - lambda Y, the new F and fnorm.
 *     4. iterations++.   5. snorm = lambda ||Y||, xnorm = ||X||.
 *     6. In this order: fnorm not finite -> FNORM_NAN; fnorm < atol -> FNORM_ABS; function_evaluations > max_funcs ->
 *        FUNCTION_COUNT; fnorm <= rtol fnorm0 -> FNORM_RELATIVE; snorm < stol xnorm -> SNORM_RELATIVE;
 *        fnorm > divtol fnorm0 -> DTOL.
 *   Leaving the loop without a reason: MAX_IT.
 *   Line search NLPS_LS_BASIC: lambda = 1, one evaluation.
 *   Line search NLPS_LS_BT (Dennis-Schnabel A6.3.1 as PETSc's bt does it), f = the current norm, g = a trial's norm:
 *     ||Y|| > ls_maxstep: Y is scaled down to that length.  ||Y|| = 0: lambda = 1 is taken as it is.
 *     s = F . (K Y), one product on the snapshotted operator; s > 0: s = -s; s == 0: s = -1.
 *     minlambda = ls_steptol / max_i(|y_i| / max(|x_i|, 1)).
 *     lambda = 1 is accepted when g^2 / 2 <= f^2 / 2 + ls_alpha lambda s (the test of every trial).
 *     Otherwise the quadratic step lambda_t = -s / (g^2 - f^2 - 2 s), clamped to [0.1 lambda, 0.5 lambda]; after that up
 *     to ls_max_it cubic steps through the last two trials, same clamp.  A trial whose norm is not finite halves lambda
 *     without interpolation (so does a cubic step one of whose two trials is not finite).
 *     lambda < minlambda ahead of a cubic step, or running out of steps: X is restored, DIVERGED_LINE_SEARCH (iterations
 *     does not count the failed iterate).  ls_max_it = 0 switches backtracking off: a rejected full step fails.
 * Differences from PETSc: right preconditioning and the true-residual norm in the linear solve (nlps_gpu_tangent_solve),
 * x0 = 0 for every linear solve, no Jacobian lagging (a new operator every iterate, PETSc's default).
 * State after the call, whatever the reason: the particle state (DF, F_n1, J_n1, Stress, W, b_e_n1, Kappa_n1, EPS_n1,
 * C_ep) is the one a residual evaluation at the returned dU leaves, so nlps_gpu_roll_state and nlps_gpu_update_kinetics
 * can follow directly.  A rejected trial is never the last evaluation: after a restore the residual is evaluated at X
 * again, and that evaluation counts in function_evaluations.
 * Returns 1 where nlps_gpu_lagrangian_evaluation, nlps_gpu_tangent_operator or nlps_gpu_tangent_solve return 1 (a handle
 * that exchanges halos included: single rank only), for snes == NULL, a negative tolerance, max_it < 0, ls_max_it < 0 or
 * an unknown line search; 0 when the solve ran, converged or not (snes->reason).
 * Host vectors cross PCIe once per call (dU in and out, the three constant vectors in).  The work vectors (X, Y, W, F,
 * K Y, the constant vectors) and the partial sums are kept on the handle and only grow: 8 * (8 n + 5 ceil(n / 512)) bytes,
 * n = N_A d, beside the workspace of the linear solve.  No allocation inside the loop.  One stream synchronisation per
 * residual evaluation (the scalars of the line search arrive with it), besides the operator's and the linear solve's. */
enum { NLPS_LS_BASIC = 0, NLPS_LS_BT = 1 };
enum {
  NLPS_SNES_CONVERGED_FNORM_ABS = 2, NLPS_SNES_CONVERGED_FNORM_RELATIVE = 3, NLPS_SNES_CONVERGED_SNORM_RELATIVE = 4,
  NLPS_SNES_DIVERGED_FUNCTION_COUNT = -2, NLPS_SNES_DIVERGED_LINEAR_SOLVE = -3, NLPS_SNES_DIVERGED_FNORM_NAN = -4,
  NLPS_SNES_DIVERGED_MAX_IT = -5, NLPS_SNES_DIVERGED_LINE_SEARCH = -6, NLPS_SNES_DIVERGED_DTOL = -9
}; /* PETSc's SNESConvergedReason values */
typedef struct {
  /* in */
  int max_it, max_funcs;           /* driver: Parameters_Solver.MaxIter, 10000 */
  double atol, rtol, stol, divtol; /* driver: 100*TOL_Newmark_beta, TOL_Newmark_beta, 1e-8, 1e4 */
  int linesearch;                  /* NLPS_LS_* */
  double ls_alpha, ls_steptol, ls_maxstep; /* bt defaults 1e-4, 1e-12, 1e8 */
  int ls_max_it;                           /* bt default 40 */
  int apply_dirichlet;             /* as nlps_gpu_tangent_operator; the driver: 1 */
  nlps_ksp ksp;                    /* settings of every linear solve (x_is_guess is ignored); on return the last solve's outputs */
  double *fnorm_history;           /* host, max_it + 1, or NULL */
  double *lambda_history;          /* host, max_it: the accepted step length of each iterate, or NULL */
  int *ksp_iterations;             /* host, max_it: Arnoldi steps of each iterate, or NULL */
  /* out */
  int reason, iterations, function_evaluations, linear_iterations;
  double fnorm0, fnorm, snorm, xnorm;
} nlps_snes;
int nlps_gpu_newton_solve(nlps_gpu *h, double *dU, const double *Un_dt, const double *Un_dt2, const double *M,
                          const double *alpha, const double *gravity, const nlps_bcc *loads, int nloads, int step,
                          double thickness, const double *area0, nlps_snes *snes);

/* nlps_gpu_newmark_step: the body of the driver's time loop (U-Newmark-beta.c:192-404) in one call, in the driver's
 * order: nlps_gpu_local_search, nlps_gpu_active_masks(bcc, nbcc, step), nlps_gpu_lumped_mass, nlps_gpu_nodal_field_n, the
 * Newmark parameters of :497-514 from beta, gamma, dt, nlps_gpu_form_initial_guess(dt, use_explicit_trial, bcc, step),
 * nlps_gpu_newton_solve, nlps_gpu_nodal_kinetic_increments, nlps_gpu_roll_state and
 * nlps_gpu_update_kinetics(alpha_blend).  The nodal vectors (M, Un_dt, Un_dt2, dU and the increments) are kept on the
 * handle; none leaves the device unless dU_out is a host pointer.  *nactive (may be NULL) = N_A of this step; dU_out
 * (may be NULL, host or device) receives the N_A*d converged increments and needs room for nnodes*d doubles.
 * The particle update runs only when snes->reason > 0.  Otherwise the call returns 0 with the reason set, and the
 * particles sit at the last evaluated state, not rolled and not moved: the caller decides what to do (a smaller step,
 * other tolerances, stop).  Returns 1 where one of the composed calls returns 1, and for a dt or beta that is not
 * positive. */
typedef struct { double beta, gamma, dt, alpha_blend; int use_explicit_trial; } nlps_newmark;
int nlps_gpu_newmark_step(nlps_gpu *h, const nlps_bcc *bcc, int nbcc, int step, const nlps_newmark *nm,
                          const double *gravity, const nlps_bcc *loads, int nloads, double thickness,
                          const double *area0, nlps_snes *snes, int *nactive, double *dU_out /* or NULL */);

/* ------------------------------------------------------------------ the tangent in CSR (MatCreateSeqAIJWithArrays)
 * The matrix of nlps_gpu_tangent_assemble + nlps_gpu_tangent_coo as sorted CSR, assembled row by row: every entry has one
 * owner, which adds the particles' contributions in a fixed order (closest nodes around the row node in grid order, the
 * particles of one closest node by ascending memory slot) with plain adds and writes the finished row once.  No kernel
 * of the path holds a floating-point atomic, and no dense stencil array is allocated.
 * Both calls work on the linearisation of the last successful nlps_gpu_tangent_operator, whose snapshot supplies Dh,
 * alpha_1 M and the Dirichlet choice; they fail with the messages and under the staleness rules of
 * nlps_gpu_tangent_apply (before any operator; after a search, nlps_gpu_active_masks, a re-sort, a migration,
 * nlps_gpu_update_kinetics, nlps_gpu_roll_state or nlps_gpu_explicit_step).  One rank: both are refused, with the reason,
 * while a halo callback or an RCCL exchange is attached.  A failed allocation returns 1 with the reason.
 * nlps_gpu_tangent_csr_pattern: the structure -- all d x d entries of a node pair (A, B) are present iff some particle
 * holds both nodes in its list (__create_sparsity_pattern, U-Newmark-beta.c:1568-1632; the set nlps_gpu_tangent_coo
 * emits).  *nnz (may be NULL) = the stored entries, equal to nlps_gpu_tangent_assemble's; nnz > INT_MAX returns 1 with a
 * message naming nnz.  *bytes (may be NULL) = the device memory the CSR path keeps on the handle for this
 * linearisation, by the formula
 *   8 np (d^4 + 6 d + 2) + 4 (nnodes + 1) + 8 w nnodes + 8 (N_A + 1),   w = 2 in 2-D, 12 in 3-D
 * -- per particle, in the order by closest node, the tensor E = Jm1^T Dh Jm1, the 5 d separable shape-function factors,
 * the position and the membership mask; the run starts and a bit mask of the visited column offsets per grid node
 * (81 / 729 bits); block counts and offsets per active node.  (The atomic path: 8 d^2 (9^d nnodes + nnz / d^2) bytes and more.)  The buffers are kept and
 * only grow.  Staging for host destinations and the scan's workspace live for one call and are not counted.
 * nlps_gpu_tangent_csr: row_ptr[N_A*d + 1], cols[nnz], vals[nnz], host or device pointers (all three on the device, or
 * staged).  Rows and columns in masked dof numbering; columns strictly ascending within each row, also under
 * nlps_gpu_set_node_numbering; every structural entry present even when its value is 0 (the zeroed entries of the
 * Dirichlet rows and columns included, which keep a 1 on the diagonal), as in nlps_gpu_tangent_coo.  Requires
 * nlps_gpu_tangent_csr_pattern since the current operator.  np == 0 or N_A == 0: nnz = 0, row_ptr all zero, return 0
 * (cols and vals may then be NULL).
 * Two calls on one linearisation return the same bits in any mode; with nlps_gpu_set_deterministic on (and
 * nlps_gpu_set_deterministic_damage for a damage cloud) two runs from the same inputs return bit-identical arrays. */
int nlps_gpu_tangent_csr_pattern(nlps_gpu *h, long long *nnz, size_t *bytes);
int nlps_gpu_tangent_csr(nlps_gpu *h, int *row_ptr, int *cols, double *vals);

/* ------------------------------------------------------------------ the tangent in block CSR (MatCreateSeq[S]BAIJWithArrays)
 * The matrix of nlps_gpu_tangent_csr with one column index and d x d contiguous values per node pair: block rows of the
 * N_A masked nodes, bs = d.  kind = NLPS_BSR_FULL keeps every block (MATSEQBAIJ), NLPS_BSR_UPPER the blocks (A, B) with
 * B >= A in masked numbering, the diagonal block whole (MATSEQSBAIJ, what a Cholesky factorisation takes).
 * Both calls work on the linearisation of the last successful nlps_gpu_tangent_operator and are refused exactly like
 * nlps_gpu_tangent_csr_pattern / nlps_gpu_tangent_csr: before any operator, when it is stale, with a halo callback or an
 * RCCL exchange attached, on a failed allocation; a refusal leaves the handle usable.  A block-CSR pattern and a CSR
 * pattern may both exist on one linearisation, neither invalidates the other, and the per-particle records, the runs
 * and the visited-offset masks are built once and shared.
 * nlps_gpu_tangent_bsr_pattern: block (A, B) is present iff the CSR pattern holds the entries of that node pair.
 * *nblocks (may be NULL): for FULL the nnz of nlps_gpu_tangent_csr_pattern divided by d^2; the pattern is structurally
 * symmetric, so FULL = 2 UPPER - (diagonal blocks present).  nblocks > INT_MAX returns 1 with a message naming nblocks;
 * a kind other than the two returns 1.  NLPS_BSR_UPPER is accepted for a cloud whose particles are all Neo-Hookean
 * (with or without the damage factor, alpha_1 M and the Dirichlet choice: all keep K symmetric), the rule of the half
 * rows of nlps_gpu_tangent_assemble; any other cloud -- the spectral and plastic laws, the fluid law, a mixed cloud
 * that holds another law -- is refused with the laws named, since its assembled tangent is not symmetric.  *bytes (may
 * be NULL) = the device memory the CSR / block-CSR path keeps on the handle for this linearisation, the same for both
 * kinds and whether or not a CSR pattern exists beside it:
 *   8 np (d^4 + 6 d + 2) + 4 (nnodes + 1) + 8 w nnodes + 8 (N_A + 1)  [the CSR formula]  + 8 (N_A + 1) + 4
 * -- the counts and offsets of the upper block rows and one flag (the full form reads those of the CSR pattern).
 * Nothing of the order 9^d nnodes doubles.
 * nlps_gpu_tangent_bsr: brow_ptr[N_A + 1], bcols[nblocks], vals[nblocks * d * d] of the kind of the last
 * nlps_gpu_tangent_bsr_pattern since the current operator (refused without one); host or device pointers (all three
 * on the device, or staged).  bcols strictly ascending within each block row, also under nlps_gpu_set_node_numbering,
 * where "upper" is decided by the masked numbers, not by the lattice offset.  vals[q][i][j] is row-major inside a block
 * like nlps_gpu_tangent_block_diagonal; col_major != 0 stores vals[q][j][i] (PETSc's values(bs,bs,nnz)).  Every value
 * has the bits of the entry (A d + i, B d + j) nlps_gpu_tangent_csr returns for this linearisation: the same sums in the
 * same order, alpha_1 M and the identity rows and columns of the Dirichlet choice included (zeroed entries kept).  No
 * floating-point atomic on the path; two calls return the same bits.  np == 0 or N_A == 0: nblocks = 0, brow_ptr all
 * zero, return 0 (bcols and vals may then be NULL). */
enum { NLPS_BSR_FULL = 0, NLPS_BSR_UPPER = 1 };
int nlps_gpu_tangent_bsr_pattern(nlps_gpu *h, int kind, long long *nblocks, size_t *bytes);
int nlps_gpu_tangent_bsr(nlps_gpu *h, int col_major, int *brow_ptr, int *bcols, double *vals);

/* ------------------------------------------------------------------ multi-GPU hooks */

/* Halo exchange callback, invoked by explicit_step / the P2G stages after a nodal scatter, on the
 * handle's stream order.  dptr = device array [nnodes_grid][nfield] of `elem_bytes`-sized elements in
 * GRID numbering (x fastest, slab axis slowest => a slab halo is one contiguous byte range);
 * kind: 0 = sum doubles, 1 = OR bytes.  The callee sums/ORs the halo layers with the neighbouring
 * ranks (RCCL send/recv or all-reduce).  NULL = single GPU.
 * phase: 0 = exchange now, in the order of the handle's stream; 1 = start the exchange (the callee may run it on
 * a stream of its own, after making that stream wait for the work queued on the handle's stream so far);
 * 2 = make the handle's stream wait for the exchange started by the matching phase-1 call.  Phases 1/2 are only
 * used by nlps_gpu_explicit_step when nlps_gpu_set_ghost_bands(..., overlap = 1) was called. */
typedef int (*nlps_halo_fn)(void *ctx, void *dptr, int nfield, int elem_bytes, int kind, int phase);
int nlps_gpu_set_halo_exchange(nlps_gpu *h, nlps_halo_fn fn, void *ctx);
/* Promise that the 5^d stencils of this rank's particles stay inside node layers [layer_lo, layer_hi] of the
 * slab (slowest) axis: the per-step nodal work of explicit_step / local_search (resets, nodal kernels, tile
 * launches) is limited to that window instead of the whole grid, so a rank's cost does not grow with the number
 * of ranks.  A particle that leaves the window raises status flag 16.  Default: the whole grid. */
int nlps_gpu_set_node_window(nlps_gpu *h, int layer_lo, int layer_hi);
/* Ghost bands of this rank: node layers <= band_lo and >= band_hi (slab axis) are shared with a neighbouring
 * rank (pass band_lo < 0 / band_hi >= n_layers for "none").  overlap: 0 = every exchange blocks in place; 1 =
 * explicit_step launches the tiles that touch a band and the others separately and every exchange runs behind the
 * interior tiles of the next stage (two-phase callback above, or the library's RCCL path); 2 = ONE launch per stage
 * with the boundary tiles first: the last of them releases the library's exchange stream through a device flag and
 * the exchange runs beside the interior tiles of the same launch (library RCCL path only; what nlps_gpu_rccl_attach
 * selects for world > 1). */
int nlps_gpu_set_ghost_bands(nlps_gpu *h, int band_lo, int band_hi, int overlap);
/* Range of node layers along the slab axis this rank's particles may touch (5^d stencil reach). */
int nlps_gpu_touched_layers(nlps_gpu *h, int *lo, int *hi);

/* ---- particle migration between slab ranks.  Ownership follows the closest node: a particle whose
 * I0 lies below node layer keep_lo moves to the rank below, above keep_hi to the rank above.  The caller moves the
 * packed rows between ranks (RCCL send/recv, see nl-partsol_amd/halo.py::SlabHalo.migrate) between the two calls.
 * Call it every few steps, before a particle can leave the node window (status flag 16). */
/* step 1: select and pack.  n_down / n_up rows of row_words 8-byte words each wait in two device buffers owned by
 * the handle (valid until the next select). */
int nlps_gpu_migration_select(nlps_gpu *h, int keep_lo, int keep_hi, int *n_down, int *n_up, int *row_words,
                              void **down_rows, void **up_rows);
/* step 2: the selected particles leave, n_a + n_b immigrants (packed rows received from the two neighbours, host
 * or device pointers, may be NULL/0) join; the arrays are re-sorted.  Capacity is fixed at create:
 * np + max(np/4, 1024) particles. */
int nlps_gpu_migration_commit(nlps_gpu *h, const void *rows_a, int n_a, const void *rows_b, int n_b);
/* Both steps with the transport in between done by the library over the communicator of nlps_gpu_rccl_attach (a C driver
 * needs nothing else): select and pack, the row counts and then the rows exchanged with rank - 1 / rank + 1 by
 * ncclSend / ncclRecv on the handle's stream, commit.  Collective over the communicator: every rank calls it at the
 * same step.  An edge rank's keep range is clamped to the grid on its outer side.  Any output may be NULL. */
int nlps_gpu_rccl_migrate(nlps_gpu *h, int keep_lo, int keep_hi, int *sent_down, int *sent_up, int *received);
/* world-size-1 self-test of that transport (one-GPU boxes): the rank is its own two neighbours, the particles that
 * leave the keep range come straight back as immigrants (no clamping). */
int nlps_gpu_rccl_selftest_migrate(nlps_gpu *h, int keep_lo, int keep_hi, int *sent_down, int *sent_up, int *received);
/* current number of particles of this handle */
int nlps_gpu_num_particles(nlps_gpu *h, int *np);
/* global particle ids (default: the index in the arrays given to nlps_gpu_create).  After the first migration
 * nlps_gpu_download_state / _lists / _ids return their rows in ascending id (arrays of nlps_gpu_num_particles rows). */
int nlps_gpu_set_particle_ids(nlps_gpu *h, const int *ids);
int nlps_gpu_download_ids(nlps_gpu *h, int *ids);

/* ------------------------------------------------------------------ host-only helpers (no GPU needed) */

/* Stencil-order tables the library derives for the canonical grid numbering (see csrc/nlps_tables.hpp):
 * rank1[27][27]  chain position of each 3^d offset of NodalLocality_0 per 1-ring boundary class,
 * order2[125][125] / count2[125]  walk order of NodalLocality per 2-ring boundary class,
 * h_avg1[27]     mean 1-ring distance per class for h = 1 (Read_GramsBox.c:460-507). */
int nlps_host_stencil_tables(int ndim, unsigned char *rank1, unsigned char *order2, unsigned char *count2,
                             double *h_avg1);

/* ---- input formats: what stands on the input side of the path in the reference.
 * GiD ASCII meshes exactly as Nodes/Read-GID-Mesh.c:225-430 reads them: line 0 "MESH dimension d ElemType T Nnode n",
 * a Coordinates ... End Coordinates block of 4-word lines "id x y z" (also in 2-D), an Elements ... End Elements
 * block of "id n1 .. nN" lines, 1-based.  All four return 0 or 1; nlps_host_io_last_error() holds the reason. */
typedef struct nlps_gid_info {
  int ndim, nnodes, nelem, nodes_per_elem;
  char elem_type[32]; /* Triangle | Quadrilateral | Tetrahedra | Hexahedra */
} nlps_gid_info;
const char *nlps_host_io_last_error(void);
/* Read_Mesh_Information, Read-GID-Mesh.c:225-300 (stricter: a malformed line inside a block is an error, where the
 * reference would count it and leave the node unread) */
int nlps_host_gid_mesh_info(const char *path, nlps_gid_info *info);
/* Fill_Coordinates :304-352 and Fill_Linear_Conectivity :356-408.  coords[nnodes][ndim]; conn[nelem][nodes_per_elem]
 * 0-based and in the order the reference's chains hold the nodes, which is the REVERSE of the file order
 * (push__SetLib__ prepends, ChainOp.c:163-182). */
int nlps_host_gid_mesh_read(const char *path, const nlps_gid_info *info, double *coords, int *conn);
/* The structured lattice behind a background mesh (the GramsBox of configs 1-5): spacing, nodes per axis, origin,
 * and canon[file node] = lattice id (x fastest), the numbering every node-indexed array of this library uses.
 * Replaces the O(N_nodes x N_elem) neighbour construction of Read_GramsBox.c:293-456 and the element search of
 * LME.c:63-115 by the closed-form tables of nlps_host_stencil_tables.  Fails if the nodes are not such a lattice. */
int nlps_host_lattice_from_nodes(int ndim, int nnodes, const double *coords, double *h, int n[3], double origin[3],
                                 int *canon);
/* Particles of a body mesh: initial_position__Particles__ (Particles-Tools.c:8-28; Q4.c:342-452 with 1, 4, 5 or 9,
 * H8.c:389-575 with 1, 8 or 27, T3.c:337-440 with 1, 3, 4 or 9 and T4.c:322-420 with 1, 4 or 10 particles per
 * element) and the volumes of initialise_particles
 * (Generate-One-Phase-Analysis.c:569-625: element volume by 2^d-point quadrature / particles per element; thickness
 * is Thickness_Plain_Stress of the 2-D build).  x[nelem * gp][ndim], vol0[nelem * gp], particle p = e * gp + j. */
int nlps_host_particles_from_mesh(const nlps_gid_info *info, const double *coords, const int *conn, int gp_per_elem,
                                  double thickness, double *x, double *vol0);

/* ---- command file (.nlp), the subset the path needs before its first step: NLPS-Solver (Read_GramsTime.c:44-378, with
 * its defaults and check_Solver), GramsShapeFun (Read_GramsShapeFun.c:20-200), the mesh of GramsBox
 * (Read_GramsBox.c:235-262) and the body mesh / particles per element of One-Phase-Analysis
 * (Generate-One-Phase-Analysis.c:386-445); file names come back joined to the directory of the command file
 * (generate_route).  Materials, initial values, boundary conditions and outputs are not read.  Where the reference
 * prints and exit()s, this returns 1 with the same wording in nlps_host_io_last_error(). */
typedef struct nlps_deck {
  char box_mesh[512], body_mesh[512];
  int gp_per_elem;
  char scheme[64]; /* NLPS-Solver Type */
  double CFL, Cel;
  int i0, N;
  double epsilon_mass_matrix, beta_newmark, gamma_newmark, tol_newmark, rb_generalized_alpha, tol_generalized_alpha;
  int max_iter, explicit_trial;
  char shape_fun[16]; /* GramsShapeFun Type */
  double gamma_lme, tol_zero_lme, tol_wrapper_lme;
  int max_iter_lme;
  char wrapper_lme[32];
} nlps_deck;
int nlps_host_read_deck(const char *path, nlps_deck *deck);
/* The Define-Material(idx=i,Model=m) { property = value ... } blocks of the same file for the four laws of this path
 * (Read_GramsMaterials2.c:51-175; property names, defaults and completeness checks of Material/Hyperelastic/
 * Neo-Hookean.c, Hencky.c, Material/Plasticity/Drucker-Prager.c incl. its default reference plastic strain, and
 * Von-Mises.c).  mats / rho / idx (may be NULL) have room for max_materials entries, *nmats comes back.  Any other
 * model, or Fbar = true, is an error: this path does not cover them. */
int nlps_host_read_materials(const char *path, int max_materials, nlps_material *mats, double *rho, int *idx,
                             int *nmats);
/* The Dirichlet boundaries of the same file, GramsBoundary (File=nodes.txt) { BcDirichlet V.x curve.txt | NULL ... }
 * (NLPS-Read-u-Dirichlet-Boundary-Conditions.c:46-300, File2Chain.c, ReadCurve.c with its six curve kinds), in the
 * layout of nlps_bcc: boundary b has nnodes[b] nodes (concatenated in nodes[], in the reference's reversed file
 * order and in FILE numbering: map them through canon[] of nlps_host_lattice_from_nodes), dir and value
 * [b][ndim][nsteps].  With nodes / dir / value NULL only the counts come back (*nbounds, and nnodes[] if given). */
int nlps_host_read_boundaries(const char *path, int ndim, int nsteps, int max_bounds, int node_cap, int *nbounds,
                              int *nnodes, int *nodes, int *dir, double *value);
/* The Neumann contours of the same file, Define-Neumann-Boundary(File=elements.txt) { T.x curve.txt | NULL ... }
 * (NLPS-Read-u-Neumann-Boundary-Conditions.c:150-352): as above, but the list names elements of the body mesh and every
 * element stands for its particles e * gp_per_elem + j; the result is what nlps_gpu_nodal_traction_forces takes. */
int nlps_host_read_neumann(const char *path, int ndim, int nsteps, int gp_per_elem, int max_bounds, int node_cap,
                           int *nbounds, int *nnodes, int *nodes, int *dir, double *value);
/* Assign-material-to-particles (MatIdx=i, Particles=elements.txt) (Generate-One-Phase-Analysis.c:458-566):
 * matidx[nparticles] is updated in place for the particles of the listed body elements. */
int nlps_host_read_material_assignment(const char *path, int gp_per_elem, int nmaterials, int nparticles, int *matidx);
/* The initial velocities of the same file, GramsInitials (Nodes=list.txt) { Value=[vx,vy,vz] }
 * (Read_GramsInitials.c:7-186): the list names ELEMENTS of the body mesh (0-based), all gp_per_elem particles of a
 * listed element get the value.  vel[nparticles][ndim] is updated in place. */
int nlps_host_read_initials(const char *path, int ndim, int gp_per_elem, int nparticles, double *vel);
/* The gravity field of the same file, generate-gravity-field-constant { g.x = .. } or generate-gravity-field-curve
 * { g = file.csv } (Read_Generate_Gravity_Field.c:170-371): g[nsteps][ndim], row t is the gravity argument of
 * nlps_gpu_explicit_step at step t; *found (may be NULL) tells whether the file holds such a block. */
int nlps_host_read_gravity(const char *path, int ndim, int nsteps, double *g, int *found);
/* The output block of the same file, GramsOutputs (i=int) { DIR=dir Particles-file=name Nodes-file=name Out-...=true|false }
 * (Outputs/Read_GramsOutputs.c:25-345): interval, directory (joined to the command file's; it has to exist), file
 * names, and the Out_* switches of the blocks nlps_host_write_particles_vtk writes; switches of other blocks are
 * accepted and counted in `unsupported` when on.  found = 0 if the file has no such block. */
typedef struct nlps_outputs {
  int found, results_time_step;
  char dir[512], particles_file[128], nodes_file[128];
  int global_coordinates, mass, density, nodal_idx, material_idx, velocity, acceleration, displacement, stress,
      volumetric_stress, deformation_gradient, energy, eps;
  int unsupported;
} nlps_outputs;
int nlps_host_read_outputs(const char *path, nlps_outputs *out);

/* ---- output format: the particle file of particle_results_vtk__InOutFun__ (InOutFun/Outputs/WriteVtk.c:95-266):
 * legacy ASCII VTK, one vertex cell per particle, numbers as %.20g, blocks in the reference's order.  Arrays are in
 * the layout of nlps_gpu_download_state ([np][ndim], tensors [np][5 | 9]); a NULL array leaves its block out, like
 * the reference's Out_* switches.  flags add the blocks that derive from shared arrays. */
typedef struct nlps_vtk_fields {
  const double *x;            /* POINTS (required); X_GC with NLPS_VTK_X_GC */
  const double *mass, *rho;   /* MASS, DENSITY */
  const int *I0, *matidx;     /* ELEM_i, MatIdx */
  const double *vel, *acc, *dis; /* VELOCITY, ACCELERATION, DISPLACEMENT */
  const double *stress;       /* STRESS (2-D: zz from slot 4); P with NLPS_VTK_P */
  const double *F_n;          /* DEFORMATION-GRADIENT */
  const double *W;            /* Energy-Potential + Energy-Kinetic with NLPS_VTK_ENERGY (needs vel, mass) */
  const double *eps;          /* EPS */
} nlps_vtk_fields;
enum { NLPS_VTK_X_GC = 1, NLPS_VTK_P = 2, NLPS_VTK_ENERGY = 4 };
int nlps_host_write_particles_vtk(const char *path, int results_time_step, int ndim, int np,
                                  const nlps_vtk_fields *fields, int flags);
/* The nodal file of nodal_results_vtk__InOutFun__ (WriteVtk.c:269-405): the background mesh in file numbering (info,
 * coords, conn as read by nlps_host_gid_mesh_read), the active-node mask and the reactions.  active[nnodes] and
 * reactions[nnodes][ndim] are the library's lattice-numbered arrays (nlps_gpu_download_active,
 * nlps_gpu_explicit_nodal); canon[file node] = lattice node, NULL = identity. */
int nlps_host_write_nodes_vtk(const char *path, const nlps_gid_info *info, const double *coords, const int *conn,
                              const int *canon, const unsigned char *active, const double *reactions);

/* ------------------------------------------------------------------ measurement */

/* Time (ms, HIP events on the handle's stream) of the kernels of the last explicit step:
 * [0] search+activate, [1] lists+Newton+P2G mass/momentum, [2] G2P grad+F+stress+P2G force,
 * [3] G2P kinematics+roll, [4] nodal/mask kernels, [5] a calibration bracket around a kernel of K3's grid that
 * does nothing (the part of a one-kernel bracket that is not kernel time), [7] the bracket around the contour-traction
 * kernel of nlps_gpu_set_explicit_loads (inside [4]; 0 without loads).  Enabled with nlps_gpu_set_timing(h,1). */
int nlps_gpu_set_timing(nlps_gpu *h, int on);
int nlps_gpu_get_timing(nlps_gpu *h, float ms[8]);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
