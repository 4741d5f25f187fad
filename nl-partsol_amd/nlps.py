"""ctypes binding of libnlps_gpu.so (include/nlps_gpu.h) and a thin host-side mirror of the
reference's stage interface.

Method names follow the reference's functions so that parity tests read like the reference driver
(nl-partsol/src/Formulations/Displacements/U-Newmark-beta.c:192-409):
    local_search__MeshTools__  -> Solver.local_search()
    get_active_nodes/dofs      -> Solver.active_masks()
    __compute_nodal_lumped_mass-> Solver.compute_nodal_lumped_mass() ...
The library is REQUIRED: a missing .so or a missing GPU raises, there is no CPU fallback here.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

MAXNB = 128
MAT_NEO_HOOKEAN, MAT_HENCKY, MAT_DRUCKER_PRAGER = 0, 1, 2

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


class Grid(C.Structure):
    _fields_ = [("ndim", C.c_int), ("n", C.c_int * 3), ("origin", C.c_double * 3), ("h", C.c_double),
                ("h_avg", _dp)]


class Params(C.Structure):
    _fields_ = [("gamma_lme", C.c_double), ("tol_zero_lme", C.c_double), ("tol_wrapper_lme", C.c_double),
                ("max_iter_lme", C.c_int), ("tol_radial_returning", C.c_double),
                ("max_iter_radial_returning", C.c_int), ("driver_eigenerosion", C.c_int),
                ("driver_eigensoftening", C.c_int)]


class Material(C.Structure):
    _fields_ = [("type", C.c_int), ("E", C.c_double), ("nu", C.c_double), ("phi_deg", C.c_double),
                ("psi_deg", C.c_double), ("kappa_0", C.c_double), ("exponent_ortiz", C.c_double),
                ("eps_0", C.c_double), ("p_ref", C.c_double), ("hardening_modulus", C.c_double),
                ("theta_voce", C.c_double), ("K0_voce", C.c_double), ("Kinf_voce", C.c_double),
                ("delta_voce", C.c_double), ("Ceps", C.c_double), ("Gf", C.c_double),
                ("cohesion", C.c_double), ("alpha_borja", C.c_double), ("a_borja", C.c_double * 3),
                ("ft", C.c_double), ("heps", C.c_double), ("wcrit", C.c_double),
                ("viscosity", C.c_double), ("compressibility", C.c_double), ("n_macdonald", C.c_double)]


_PD = ["x_GC", "dis", "vel", "acc", "F_n", "F_n1", "DF", "Stress", "b_e_n", "b_e_n1", "J_n", "J_n1", "rho",
       "mass", "Vol_0", "W", "Kappa_n", "Kappa_n1", "EPS_n", "EPS_n1"]


class Particles(C.Structure):
    _fields_ = ([("np", C.c_int)] + [(k, _dp) for k in _PD] +
                [("MatIdx", _ip), ("I0", _ip), ("lambda_", _dp), ("Beta", _dp), ("dt_F_n", _dp), ("dt_F_n1", _dp),
                 ("dt_DF", _dp), ("C_ep", _dp), ("Back_stress", _dp), ("Damage_n", _dp), ("Damage_n1", _dp),
                 ("Strain_f_n", _dp), ("Strain_f_n1", _dp)])


class Ksp(C.Structure):  # nlps_ksp (include/nlps_gpu.h): nlps_gpu_tangent_solve's settings and results
    _fields_ = [("pc", C.c_int), ("restart", C.c_int), ("max_it", C.c_int), ("x_is_guess", C.c_int),
                ("rtol", C.c_double), ("atol", C.c_double), ("dtol", C.c_double), ("history", _dp),
                ("reason", C.c_int), ("iterations", C.c_int), ("rnorm", C.c_double), ("bnorm", C.c_double),
                ("bytes", C.c_size_t)]


class Eig(C.Structure):  # nlps_eig: nlps_gpu_tangent_lambda_max's settings and results
    _fields_ = [("max_it", C.c_int), ("rtol", C.c_double), ("seed", C.c_ulonglong), ("history", _dp),
                ("reason", C.c_int), ("iterations", C.c_int), ("theta", C.c_double), ("resid", C.c_double),
                ("asymmetry", C.c_double), ("bytes", C.c_size_t)]


EIG_REASONS = {1: "converged", 2: "empty", -3: "diverged_its", -9: "diverged_nanorinf"}  # NLPS_EIG_*
PC_KINDS = {"none": 0, "jacobi": 1, "pbjacobi": 2}  # NLPS_PC_NONE / _JACOBI / _PBJACOBI
KSP_REASONS = {1: "converged_bzero", 2: "converged_rtol", 3: "converged_atol", -3: "diverged_its", -4: "diverged_dtol",
               -5: "diverged_breakdown", -8: "diverged_indefinite_pc", -9: "diverged_nanorinf"}
KSP_TYPES = {"gmres": 0, "minres": 1}  # NLPS_KSP_TYPE_GMRES / _MINRES


class Snes(C.Structure):  # nlps_snes: nlps_gpu_newton_solve's settings and results
    _fields_ = [("max_it", C.c_int), ("max_funcs", C.c_int), ("atol", C.c_double), ("rtol", C.c_double),
                ("stol", C.c_double), ("divtol", C.c_double), ("linesearch", C.c_int), ("ls_alpha", C.c_double),
                ("ls_steptol", C.c_double), ("ls_maxstep", C.c_double), ("ls_max_it", C.c_int),
                ("apply_dirichlet", C.c_int), ("ksp", Ksp), ("fnorm_history", _dp), ("lambda_history", _dp),
                ("ksp_iterations", _ip), ("reason", C.c_int), ("iterations", C.c_int),
                ("function_evaluations", C.c_int), ("linear_iterations", C.c_int), ("fnorm0", C.c_double),
                ("fnorm", C.c_double), ("snorm", C.c_double), ("xnorm", C.c_double)]


class Newmark(C.Structure):  # nlps_newmark
    _fields_ = [("beta", C.c_double), ("gamma", C.c_double), ("dt", C.c_double), ("alpha_blend", C.c_double),
                ("use_explicit_trial", C.c_int)]


LINE_SEARCHES = {"basic": 0, "bt": 1}  # NLPS_LS_BASIC / _BT
SNES_REASONS = {2: "converged_fnorm_abs", 3: "converged_fnorm_relative", 4: "converged_snorm_relative",
                -2: "diverged_function_count", -3: "diverged_linear_solve", -4: "diverged_fnorm_nan",
                -5: "diverged_max_it", -6: "diverged_line_search", -9: "diverged_dtol"}


class Bcc(C.Structure):
    _fields_ = [("nnodes", C.c_int), ("nodes", _ip), ("dim", C.c_int), ("dir", _ip), ("value", _dp)]


class FbarCfg(C.Structure):  # nlps_fbar_cfg
    _fields_ = [("block", C.c_int * 3), ("alpha", _dp), ("Fbar_n", _dp), ("Jbar_n", _dp)]


HALO_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int)

_LIB = None

# every symbol include/nlps_gpu.h declares
SYMBOLS = ["nlps_gpu_lagrangian_evaluation", "nlps_gpu_create", "nlps_gpu_destroy", "nlps_gpu_last_error", "nlps_gpu_synchronize",
           "nlps_gpu_download_state", "nlps_gpu_download_lists", "nlps_gpu_shape_functions", "nlps_gpu_download_active",
           "nlps_gpu_status_flags", "nlps_gpu_initialize_lme", "nlps_gpu_local_search", "nlps_gpu_active_masks",
           "nlps_gpu_set_node_numbering",
           "nlps_gpu_lumped_mass", "nlps_gpu_nodal_field_n", "nlps_gpu_compatibility", "nlps_gpu_constitutive",
           "nlps_gpu_internal_forces", "nlps_gpu_nodal_traction_forces", "nlps_gpu_roll_state", "nlps_gpu_update_kinetics",
           "nlps_gpu_explicit_step", "nlps_gpu_num_active", "nlps_gpu_explicit_nodal", "nlps_gpu_set_halo_exchange",
           "nlps_gpu_resort", "nlps_gpu_set_resort_interval", "nlps_gpu_set_adaptive_resort", "nlps_gpu_set_law_launch_mode", "nlps_gpu_set_deterministic", "nlps_gpu_set_explicit_damage",
           "nlps_gpu_set_explicit_fluid", "nlps_gpu_set_explicit_fbar", "nlps_gpu_download_fbar",
           "nlps_gpu_set_explicit_loads",
           "nlps_gpu_set_step_record", "nlps_gpu_step_record_layout", "nlps_gpu_record_now", "nlps_gpu_read_step_records",
           "nlps_host_courant_dt",
           "nlps_gpu_set_snapshots", "nlps_gpu_snapshot_begin", "nlps_gpu_snapshot_wait", "nlps_gpu_snapshot_release",
           "nlps_gpu_snapshot_bytes",
           "nlps_gpu_set_implicit_damage", "nlps_gpu_set_deterministic_damage",
           "nlps_gpu_rccl_unique_id", "nlps_gpu_rccl_attach", "nlps_gpu_rccl_attach_comm", "nlps_gpu_rccl_detach",
           "nlps_gpu_rccl_reduce", "nlps_gpu_rccl_info", "nlps_gpu_rccl_migrate", "nlps_gpu_rccl_selftest_migrate", "nlps_gpu_rccl_selftest_exchange", "nlps_gpu_touched_layers", "nlps_gpu_set_node_window", "nlps_gpu_set_ghost_bands",
           "nlps_gpu_form_initial_guess", "nlps_gpu_nodal_kinetic_increments", "nlps_gpu_nodal_inertial_forces",
           "nlps_gpu_tangent_assemble", "nlps_gpu_tangent_set_grouped", "nlps_gpu_set_tangent_alpha4", "nlps_gpu_tangent_coo",
           "nlps_gpu_sparsity_pattern", "nlps_gpu_tangent_operator", "nlps_gpu_tangent_apply",
           "nlps_gpu_tangent_block_diagonal", "nlps_gpu_tangent_solve", "nlps_gpu_set_linear_solver",
           "nlps_gpu_tangent_lambda_max",
           "nlps_host_critical_dt", "nlps_gpu_newton_solve", "nlps_gpu_newmark_step",
           "nlps_gpu_tangent_csr_pattern", "nlps_gpu_tangent_csr",
           "nlps_gpu_tangent_bsr_pattern", "nlps_gpu_tangent_bsr",
           "nlps_gpu_migration_select", "nlps_gpu_migration_commit", "nlps_gpu_num_particles",
           "nlps_gpu_set_particle_ids", "nlps_gpu_download_ids",
           "nlps_gpu_set_timing", "nlps_gpu_get_timing", "nlps_host_stencil_tables",
           "nlps_host_io_last_error", "nlps_host_gid_mesh_info", "nlps_host_gid_mesh_read",
           "nlps_host_lattice_from_nodes", "nlps_host_particles_from_mesh", "nlps_host_write_particles_vtk", "nlps_host_write_nodes_vtk", "nlps_host_read_deck", "nlps_host_read_materials", "nlps_host_read_boundaries", "nlps_host_read_initials", "nlps_host_read_gravity", "nlps_host_read_outputs", "nlps_host_read_neumann",
           "nlps_host_read_material_assignment"]


def lib():
    """Loads the HIP library; raises if it is missing (no fallback)."""
    global _LIB
    if _LIB is None:
        path = _build.LIB
        try:
            # torch bundles its own libamdhip64.so.7; loading it FIRST makes this library bind to that
            # same runtime (one HIP runtime per process), otherwise torch.cuda sees no device afterwards.
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(path):
            raise RuntimeError("libnlps_gpu.so is not built: run __graft_entry__.build() "
                               "(nl-partsol_amd has no CPU fallback)")
        L = C.CDLL(path)
        L.nlps_gpu_last_error.restype = C.c_char_p
        L.nlps_gpu_last_error.argtypes = [C.c_void_p]
        L.nlps_gpu_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(Grid), C.POINTER(Params),
                                      C.POINTER(Material), C.c_int, C.POINTER(Particles), C.c_int, C.c_void_p]
        L.nlps_gpu_set_resort_interval.argtypes = [C.c_void_p, C.c_int]
        L.nlps_gpu_set_law_launch_mode.argtypes = [C.c_void_p, C.c_int]
        L.nlps_gpu_set_deterministic.argtypes = [C.c_void_p, C.c_int]
        L.nlps_gpu_set_explicit_damage.argtypes = [C.c_void_p, C.c_int]
        if hasattr(L, "nlps_gpu_set_linear_solver"):  # (NLPS_GPU_LIB may name an older build)
            L.nlps_gpu_set_linear_solver.argtypes = [C.c_void_p, C.c_int]
        if hasattr(L, "nlps_gpu_set_explicit_fluid"):  # (NLPS_GPU_LIB may name an older build: tools/explicit_fluid_bench.py)
            L.nlps_gpu_set_explicit_fluid.argtypes = [C.c_void_p, C.c_int]
        if hasattr(L, "nlps_gpu_set_explicit_loads"):  # (NLPS_GPU_LIB may name an older build)
            L.nlps_gpu_set_explicit_loads.argtypes = [C.c_void_p, C.POINTER(Bcc), C.c_int, C.c_double, C.c_void_p]
        if hasattr(L, "nlps_gpu_set_deterministic_damage"):  # (NLPS_GPU_LIB may name an older build)
            L.nlps_gpu_set_deterministic_damage.argtypes = [C.c_void_p, C.c_int]
        if hasattr(L, "nlps_gpu_set_implicit_damage"):  # (NLPS_GPU_LIB may name an older build: tools/implicit_damage_bench.py)
            L.nlps_gpu_set_implicit_damage.argtypes = [C.c_void_p, C.c_int]
        L.nlps_gpu_rccl_unique_id.argtypes = [C.c_void_p]
        L.nlps_gpu_rccl_attach.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, _ip, _ip, C.c_int]
        L.nlps_gpu_rccl_attach_comm.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, _ip, _ip, C.c_int]
        L.nlps_gpu_rccl_detach.argtypes = [C.c_void_p]
        L.nlps_gpu_rccl_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.nlps_gpu_rccl_info.argtypes = [C.c_void_p, _ip, _ip, _ip]
        L.nlps_gpu_rccl_migrate.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, _ip, _ip]
        L.nlps_gpu_rccl_selftest_migrate.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, _ip, _ip]
        L.nlps_gpu_rccl_selftest_exchange.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.nlps_gpu_set_node_window.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.nlps_gpu_set_node_numbering.argtypes = [C.c_void_p, _ip]
        L.nlps_gpu_set_ghost_bands.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.nlps_gpu_form_initial_guess.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int,
                                                  C.POINTER(Bcc), C.c_int, C.c_int]
        L.nlps_gpu_nodal_kinetic_increments.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [_dp]
        L.nlps_gpu_nodal_inertial_forces.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [_dp, _dp]
        L.nlps_gpu_tangent_assemble.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        L.nlps_gpu_tangent_set_grouped.argtypes = [C.c_void_p, C.c_int]
        L.nlps_gpu_set_tangent_alpha4.argtypes = [C.c_void_p, C.c_double]
        L.nlps_gpu_tangent_coo.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_int, _ip, _ip, _dp]
        L.nlps_gpu_sparsity_pattern.argtypes = [C.c_void_p, _ip]
        L.nlps_gpu_tangent_operator.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]
        L.nlps_gpu_tangent_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.nlps_gpu_tangent_block_diagonal.argtypes = [C.c_void_p, C.c_void_p]
        L.nlps_gpu_tangent_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Ksp)]
        if hasattr(L, "nlps_gpu_tangent_lambda_max"):  # (NLPS_GPU_LIB may name an older build)
            L.nlps_gpu_tangent_lambda_max.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Eig), C.c_void_p]
            L.nlps_host_critical_dt.restype = C.c_double
            L.nlps_host_critical_dt.argtypes = [C.c_double, C.c_double, C.c_double]
        L.nlps_gpu_newton_solve.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [_dp, _dp, C.POINTER(Bcc), C.c_int, C.c_int,
                                            C.c_double, C.c_void_p, C.POINTER(Snes)]
        L.nlps_gpu_newmark_step.argtypes = [C.c_void_p, C.POINTER(Bcc), C.c_int, C.c_int, C.POINTER(Newmark), _dp,
                                            C.POINTER(Bcc), C.c_int, C.c_double, C.c_void_p, C.POINTER(Snes), _ip,
                                            C.c_void_p]
        if hasattr(L, "nlps_gpu_tangent_csr"):  # (NLPS_GPU_LIB may name an older build: tools/tangent_csr_bench.py)
            L.nlps_gpu_tangent_csr_pattern.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_size_t)]
            L.nlps_gpu_tangent_csr.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "nlps_gpu_tangent_bsr"):  # (the same hook: tools/tangent_bsr_bench.py)
            L.nlps_gpu_tangent_bsr_pattern.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_size_t)]
            L.nlps_gpu_tangent_bsr.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nlps_gpu_migration_select.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, _ip, _ip, C.POINTER(C.c_void_p),
                                                C.POINTER(C.c_void_p)]
        L.nlps_gpu_migration_commit.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.nlps_gpu_num_particles.argtypes = [C.c_void_p, _ip]
        L.nlps_gpu_set_particle_ids.argtypes = [C.c_void_p, _ip]
        L.nlps_gpu_download_ids.argtypes = [C.c_void_p, _ip]
        for name in ["nlps_gpu_destroy", "nlps_gpu_synchronize", "nlps_gpu_initialize_lme", "nlps_gpu_resort",
                     "nlps_gpu_local_search", "nlps_gpu_constitutive", "nlps_gpu_roll_state"]:
            getattr(L, name).argtypes = [C.c_void_p]
        L.nlps_gpu_download_state.argtypes = [C.c_void_p, C.POINTER(Particles)]
        L.nlps_gpu_download_lists.argtypes = [C.c_void_p, _ip, _ip]
        L.nlps_gpu_shape_functions.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.nlps_gpu_download_active.argtypes = [C.c_void_p, C.c_void_p]
        L.nlps_gpu_status_flags.argtypes = [C.c_void_p, _ip]
        L.nlps_gpu_active_masks.argtypes = [C.c_void_p, C.POINTER(Bcc), C.c_int, C.c_int, _ip, _ip, _ip, _ip]
        L.nlps_gpu_lumped_mass.argtypes = [C.c_void_p, C.c_void_p]
        L.nlps_gpu_nodal_field_n.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nlps_gpu_compatibility.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.nlps_gpu_internal_forces.argtypes = [C.c_void_p, C.c_void_p]
        L.nlps_gpu_update_kinetics.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p]
        L.nlps_gpu_explicit_step.argtypes = [C.c_void_p, C.POINTER(Bcc), C.c_int, C.c_int, C.c_double,
                                             C.c_double, _dp]
        L.nlps_gpu_explicit_nodal.argtypes = [C.c_void_p] + [C.c_void_p] * 5
        L.nlps_gpu_num_active.argtypes = [C.c_void_p, _ip]
        L.nlps_gpu_set_halo_exchange.argtypes = [C.c_void_p, HALO_FN, C.c_void_p]
        L.nlps_gpu_touched_layers.argtypes = [C.c_void_p, _ip, _ip]
        L.nlps_gpu_set_timing.argtypes = [C.c_void_p, C.c_int]
        L.nlps_gpu_get_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        _LIB = L
    return _LIB


def default_params():
    return Params(3.0, 1e-6, 1e-10, 10, 1e-14, 10, 0, 0)


def host_stencil_tables(ndim):
    """Host-only: the stencil order tables of csrc/nlps_tables.hpp (no GPU needed)."""
    rank1 = np.zeros((27, 27), dtype=np.uint8)
    order2 = np.zeros((125, 125), dtype=np.uint8)
    count2 = np.zeros(125, dtype=np.uint8)
    h1 = np.zeros(27)
    f = lib().nlps_host_stencil_tables
    f.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    st = f(int(ndim), rank1.ctypes.data_as(C.c_void_p), order2.ctypes.data_as(C.c_void_p),
           count2.ctypes.data_as(C.c_void_p), h1.ctypes.data_as(C.c_void_p))
    if st:
        raise NlpsError("nlps_host_stencil_tables failed")
    return rank1, order2, count2, h1


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _i(a):
    return None if a is None else a.ctypes.data_as(_ip)


def _vp(a):
    """numpy array (host) or torch tensor / int (device pointer) -> void*"""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    return C.c_void_p(int(a))


def _csr_arrays(nr, n, block, on_device):
    """(row pointer [nr] int32, indices [n] int32, values [n, *block] float64) for tangent_csr / tangent_bsr to fill: numpy
    arrays, or torch tensors on the GPU (an empty matrix still gets a valid device pointer: one entry, sliced to none)."""
    if on_device:
        import torch
        return (torch.empty(nr, dtype=torch.int32, device="cuda"),
                torch.empty(max(n, 1), dtype=torch.int32, device="cuda")[:n],
                torch.empty((max(n, 1),) + tuple(block), dtype=torch.float64, device="cuda")[:n])
    return np.zeros(nr, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros((n,) + tuple(block))


class BccSet:
    """FEM_Mesh.Bounds: list of dicts {nodes, dim, dir[dim][nsteps], value[dim][nsteps]}."""

    def __init__(self, bcs):
        self.keep = []
        self.n = len(bcs)
        self.arr = (Bcc * max(1, self.n))()
        for k, b in enumerate(bcs):
            nodes = np.ascontiguousarray(b["nodes"], dtype=np.int32)
            d = np.ascontiguousarray(b["dir"], dtype=np.int32)
            v = np.ascontiguousarray(b["value"], dtype=np.float64)
            self.keep += [nodes, d, v]
            self.arr[k] = Bcc(len(nodes), _i(nodes), int(b["dim"]), _i(d), _d(v))


class RecordCfg(C.Structure):  # nlps_record_cfg
    _fields_ = [("every", C.c_int), ("capacity", C.c_int), ("nsets", C.c_int), ("nprobes", C.c_int), ("probes", _ip),
                ("probe_fields", C.c_uint)]


# the global block of a row of the step record (NLPS_REC_*): name -> (offset, doubles)
REC_KIND_NOW, REC_KIND_EXPLICIT, REC_KIND_NEWMARK = 0, 1, 2
REC_NGLOBAL = 32
REC_COLUMNS = {"step": (0, 1), "kind": (1, 1), "dt": (2, 1), "time": (3, 1), "np": (4, 1), "mass": (5, 1), "momentum": (6, 3),
               "angular": (9, 3), "mass_x": (12, 3), "kinetic": (15, 1), "strain": (16, 1), "volume": (17, 1),
               "vmax_comp": (18, 1), "vmax_norm": (19, 1), "J_min": (20, 1), "J_max": (21, 1), "EPS_max": (22, 1),
               "Damage_max": (23, 1), "failed": (24, 1), "status": (25, 1)}
PROBE_X, PROBE_DIS, PROBE_VEL, PROBE_ACC, PROBE_F, PROBE_STRESS, PROBE_J, PROBE_EPS, PROBE_DAMAGE, PROBE_W = \
    1, 2, 4, 8, 16, 32, 64, 128, 256, 512
PROBE_ALL = 1023


class SnapshotCfg(C.Structure):  # nlps_snapshot_cfg
    _fields_ = [("fields", C.c_uint), ("slots", C.c_int)]


# the fields of a particle snapshot (NLPS_SNAP_*) in bit order: the names download_state() uses, the member of Particles
# and the columns of a row (d = ndim, T = 5 | 9)
SNAP_FIELDS = (("x_GC", "d"), ("dis", "d"), ("vel", "d"), ("acc", "d"), ("F_n", "T"), ("Stress", "T"), ("b_e_n", "T"),
               ("J_n", 1), ("rho", 1), ("mass", 1), ("Vol_0", 1), ("W", 1), ("Kappa_n", 1), ("EPS_n", 1), ("Back_stress", 3),
               ("Damage_n", 1), ("Strain_f_n", 1), ("lambda_", "d"), ("Beta", 1), ("I0", 1))
SNAP_BITS = {name: 1 << b for b, (name, _) in enumerate(SNAP_FIELDS)}
SNAP_ALL = (1 << len(SNAP_FIELDS)) - 1
SNAP_MAX_SLOTS = 4
# what gid.write_particles_vtk reads of a state
SNAP_VTK = sum(SNAP_BITS[k] for k in ("x_GC", "dis", "vel", "acc", "F_n", "Stress", "rho", "mass", "W", "EPS_n", "I0"))


def snapshot_mask(fields):
    """NLPS_SNAP_* bits from an int or from names as download_state() takes them (x, lambda, beta are aliases)"""
    if isinstance(fields, (int, np.integer)):
        return int(fields)
    alias = {"x": "x_GC", "lambda": "lambda_", "beta": "Beta"}
    return sum({SNAP_BITS[alias.get(k, k)] for k in fields})


def courant_dt(CFL, h, Cel, row=None):
    """CFL h / Cel, or with a row of the step record CFL h / (Cel + vmax_comp) (Courant.c, DynamicTimeStep); host only"""
    f = lib().nlps_host_courant_dt
    f.restype = C.c_double
    f.argtypes = [C.c_double, C.c_double, C.c_double, C.c_void_p]
    r = None if row is None else np.ascontiguousarray(row, dtype=np.float64)
    return f(float(CFL), float(h), float(Cel), None if r is None else r.ctypes.data_as(C.c_void_p))


def critical_dt(omega2, gamma=0.5, safety=0.9):
    """safety * sqrt(2 / gamma) / sqrt(omega2): the explicit scheme's stable step from omega_max^2 (pass theta + resid of
    Solver.tangent_lambda_max); +inf for omega2 <= 0, -1 for gamma < 0.5 (nlps_host_critical_dt); host only"""
    return lib().nlps_host_critical_dt(float(omega2), float(gamma), float(safety))


class NlpsError(RuntimeError):
    pass


class Solver:
    """Device-resident particle set + background grid; one method per reference stage function."""

    def __init__(self, ndim, grid_n, origin, h, cloud, materials, params=None, nsteps=1, stream=None,
                 h_avg=None):
        self.L = lib()
        self.ndim = int(ndim)
        self.T = 5 if ndim == 2 else 9
        self.np = int(cloud["x"].shape[0])
        n3 = list(grid_n) + [1] * (3 - len(grid_n))
        o3 = list(origin) + [0.0] * (3 - len(origin))
        self.grid_n = n3
        self.nnodes = n3[0] * n3[1] * n3[2]
        self._h_avg = None if h_avg is None else np.ascontiguousarray(h_avg, dtype=np.float64)
        g = Grid(self.ndim, (C.c_int * 3)(*n3), (C.c_double * 3)(*o3), float(h), _d(self._h_avg))
        self.params = params or default_params()
        self.nmats = len(materials)
        mats = (Material * len(materials))()
        for k, m in enumerate(materials):
            mats[k] = Material(int(m["type"]), float(m.get("E", 0.0)), float(m.get("nu", 0.0)), float(m.get("phi_deg", 0.0)),
                               float(m.get("psi_deg", 0.0)), float(m.get("kappa_0", 0.0)),
                               float(m.get("exponent_ortiz", 1.0)), float(m.get("eps_0", 1.0)),
                               float(m.get("p_ref", 0.0)), float(m.get("hardening_modulus", 0.0)),
                               float(m.get("theta_voce", 1.0)), float(m.get("K0_voce", 0.0)),
                               float(m.get("Kinf_voce", 0.0)), float(m.get("delta_voce", 0.0)),
                               float(m.get("Ceps", 0.0)), float(m.get("Gf", 0.0)), float(m.get("cohesion", 0.0)),
                               float(m.get("alpha_borja", 0.0)),
                               (C.c_double * 3)(*[float(v) for v in m.get("a_borja", (0.0, 0.0, 0.0))]),
                               float(m.get("ft", 0.0)), float(m.get("heps", 0.0)), float(m.get("wcrit", 1.0)),
                               float(m.get("viscosity", 0.0)), float(m.get("compressibility", 0.0)),
                               float(m.get("n_macdonald", 0.0)))
        self._host = {}
        hp = Particles()
        hp.np = self.np
        keymap = {"x_GC": "x", "dis": "dis", "vel": "vel", "acc": "acc", "F_n": "F_n", "b_e_n": "b_e_n",
                  "J_n": "J_n", "rho": "rho", "mass": "mass", "Vol_0": "vol0", "Kappa_n": "kappa_n",
                  "EPS_n": "eps_n", "lambda_": "lambda", "Beta": "beta", "dt_F_n": "dt_F_n",
                  "Back_stress": "back_stress", "Damage_n": "damage_n", "Strain_f_n": "strain_f_n",
                  # the n+1 state and the increments, for callers that enter at a per-particle stage (absent: NULL, and
                  # nlps_gpu_create starts them from the n state / the unit tensor)
                  "F_n1": "F_n1", "DF": "DF", "J_n1": "J_n1", "b_e_n1": "b_e_n1", "dt_F_n1": "dt_F_n1", "dt_DF": "dt_DF",
                  "Kappa_n1": "kappa_n1", "EPS_n1": "eps_n1"}
        for ck, k in keymap.items():
            if k in cloud and cloud[k] is not None:
                a = np.ascontiguousarray(cloud[k], dtype=np.float64)
                self._host[ck] = a
                setattr(hp, ck, _d(a))
        mi = np.ascontiguousarray(cloud["matidx"], dtype=np.int32)
        self._host["MatIdx"] = mi
        hp.MatIdx = _i(mi)
        if cloud.get("I0") is not None:
            i0 = np.ascontiguousarray(cloud["I0"], dtype=np.int32)
            self._host["I0"] = i0
            hp.I0 = _i(i0)
        self.nsteps = int(nsteps)
        self.h = C.c_void_p()
        st = self.L.nlps_gpu_create(C.byref(self.h), C.byref(g), C.byref(self.params), mats, len(materials),
                                    C.byref(hp), self.nsteps, C.c_void_p(stream) if stream else None)
        if st:
            raise NlpsError(self.L.nlps_gpu_last_error(self.h).decode())
        self.nactive = 0
        self.nfree = 0
        self._halo_cb = None

    # ------------------------------------------------------------------ helpers
    def _chk(self, st):
        if st:
            raise NlpsError(self.L.nlps_gpu_last_error(self.h).decode())

    def close(self):
        if self.h:
            self.L.nlps_gpu_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        self._chk(self.L.nlps_gpu_synchronize(self.h))

    # ------------------------------------------------------------------ reference stages
    def initialise_shapefun(self):          # initialise_shapefun__MeshTools__ -> initialize__LME__
        self._chk(self.L.nlps_gpu_initialize_lme(self.h))

    def local_search(self):                 # local_search__MeshTools__
        self._chk(self.L.nlps_gpu_local_search(self.h))

    def active_masks(self, bcs, step, download=True):   # get_active_nodes/_dofs__MeshTools__
        na, nf = C.c_int(0), C.c_int(0)
        n2m = np.zeros(self.nnodes, dtype=np.int32) if download else None
        d2m = np.zeros(self.nnodes * self.ndim, dtype=np.int32) if download else None
        self._chk(self.L.nlps_gpu_active_masks(self.h, bcs.arr, bcs.n, step, C.byref(na), C.byref(nf), _i(n2m),
                                               _i(d2m)))
        self.nactive, self.nfree = na.value, nf.value
        if download:
            return n2m, d2m[: self.nactive * self.ndim]
        return None, None

    def compute_nodal_lumped_mass(self, out=None):      # __compute_nodal_lumped_mass
        M = np.zeros(self.nactive * self.ndim) if out is None else out
        self._chk(self.L.nlps_gpu_lumped_mass(self.h, _vp(M)))
        return M

    def get_nodal_field_n(self, M, V=None, A=None):     # __get_nodal_field_n
        V = np.zeros(self.nactive * self.ndim) if V is None else V
        A = np.zeros(self.nactive * self.ndim) if A is None else A
        self._chk(self.L.nlps_gpu_nodal_field_n(self.h, _vp(V), _vp(A), _vp(M)))
        return V, A

    def local_compatibility_conditions(self, dU, dU_dt=None):   # __local_compatibility_conditions
        self._chk(self.L.nlps_gpu_compatibility(self.h, _vp(dU), _vp(dU_dt)))

    def constitutive_update(self):                      # __constitutive_update
        self._chk(self.L.nlps_gpu_constitutive(self.h))

    def nodal_internal_forces(self, R):                 # __nodal_internal_forces (accumulates into R)
        self._chk(self.L.nlps_gpu_internal_forces(self.h, _vp(R)))
        return R

    def nodal_traction_forces(self, R, loads, step, thickness=1.0, area0=None):   # __nodal_traction_forces
        self.L.nlps_gpu_nodal_traction_forces.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Bcc), C.c_int, C.c_int,
                                                          C.c_double, C.c_void_p]
        a0 = None if area0 is None else np.ascontiguousarray(area0, dtype=np.float64)
        self._chk(self.L.nlps_gpu_nodal_traction_forces(self.h, _vp(R), loads.arr, loads.n, int(step), float(thickness),
                                                        None if a0 is None else a0.ctypes.data))
        return R

    def update_particles_internal_variables(self):      # __update_particles_internal_variables
        self._chk(self.L.nlps_gpu_roll_state(self.h))

    def update_particles_kinetics_FLIP_PIC(self, alpha_blend, dU, Un_dt, dU_dt, dU_dt2):
        self._chk(self.L.nlps_gpu_update_kinetics(self.h, float(alpha_blend), _vp(dU), _vp(Un_dt), _vp(dU_dt),
                                                  _vp(dU_dt2)))

    def explicit_step(self, bcs, step, dt, gamma=0.5, gravity=None):
        g = None if gravity is None else np.ascontiguousarray(gravity, dtype=np.float64)
        self._chk(self.L.nlps_gpu_explicit_step(self.h, bcs.arr, bcs.n, int(step), float(dt), float(gamma), _d(g)))

    def explicit_nodal(self):
        """Nodal results of the last explicit step in masked numbering (host arrays)."""
        na = C.c_int(0)
        self._chk(self.L.nlps_gpu_num_active(self.h, C.byref(na)))
        self.nactive = na.value
        out = {k: np.zeros(self.nactive * self.ndim) for k in ("mass", "dU", "force", "accel", "reaction")}
        self._chk(self.L.nlps_gpu_explicit_nodal(self.h, *[_vp(out[k]) for k in
                                                           ("mass", "dU", "force", "accel", "reaction")]))
        return out

    # ------------------------------------------------------------------ downloads
    def download_state(self, fields=None):
        """All particle fields in the caller's order; `fields` (names as below) limits the download (large clouds)."""
        n, d, T = self.np, self.ndim, self.T
        o = {"x_GC": np.zeros((n, d)), "dis": np.zeros((n, d)), "vel": np.zeros((n, d)), "acc": np.zeros((n, d)),
             "F_n": np.zeros((n, T)), "F_n1": np.zeros((n, T)), "DF": np.zeros((n, T)), "Stress": np.zeros((n, T)),
             "b_e_n": np.zeros((n, T)), "b_e_n1": np.zeros((n, T)), "J_n": np.zeros(n), "J_n1": np.zeros(n),
             "rho": np.zeros(n), "mass": np.zeros(n), "Vol_0": np.zeros(n), "W": np.zeros(n),
             "Kappa_n": np.zeros(n), "Kappa_n1": np.zeros(n), "EPS_n": np.zeros(n), "EPS_n1": np.zeros(n),
             "lambda_": np.zeros((n, d)), "Beta": np.zeros(n), "dt_F_n": np.zeros((n, T)),
             "dt_F_n1": np.zeros((n, T)), "dt_DF": np.zeros((n, T)), "C_ep": np.zeros((n, d * d)),
             "Back_stress": np.zeros((n, 3)), "Damage_n": np.zeros(n), "Damage_n1": np.zeros(n),
             "Strain_f_n": np.zeros(n), "Strain_f_n1": np.zeros(n)}
        if fields is not None:
            alias = {"x": "x_GC", "lambda": "lambda_", "beta": "Beta"}
            want = {alias.get(k, k) for k in fields}
            o = {k: a for k, a in o.items() if k in want}
        i0 = np.zeros(n, dtype=np.int32) if fields is None or "I0" in fields else None
        hp = Particles()
        hp.np = n
        for k, a in o.items():
            setattr(hp, k, _d(a))
        hp.I0 = _i(i0)
        self._chk(self.L.nlps_gpu_download_state(self.h, C.byref(hp)))
        if i0 is not None:
            o["I0"] = i0
        for short, full in (("x", "x_GC"), ("lambda", "lambda_"), ("beta", "Beta")):
            if full in o:
                o[short] = o[full]
        return o

    def download_lists(self):
        nn = np.zeros(self.np, dtype=np.int32)
        lst = np.zeros((self.np, MAXNB), dtype=np.int32)
        self._chk(self.L.nlps_gpu_download_lists(self.h, _i(nn), _i(lst)))
        return nn, lst

    def shape_functions(self, first=0, count=None):
        """N[count][MAXNB] and dN[count][MAXNB][ndim] of particles first .. first + count - 1 in the order of their lists."""
        count = self.np - first if count is None else count
        N = np.zeros((count, MAXNB))
        dN = np.zeros((count, MAXNB, self.ndim))
        self._chk(self.L.nlps_gpu_shape_functions(self.h, int(first), int(count), _vp(N), _vp(dN)))
        return N, dN

    def download_active(self):
        a = np.zeros(self.nnodes, dtype=np.uint8)
        self._chk(self.L.nlps_gpu_download_active(self.h, a.ctypes.data_as(C.c_void_p)))
        return a

    def status_flags(self):
        f = C.c_int(0)
        self._chk(self.L.nlps_gpu_status_flags(self.h, C.byref(f)))
        return f.value

    # ------------------------------------------------------------------ multi-GPU / measurement
    def set_halo_exchange(self, pyfunc):
        """pyfunc(dptr:int, nfield:int, elem_bytes:int, kind:int[, phase:int]) -> int
        (phase 0 = exchange now, 1 = start, 2 = wait; a 4-argument function only ever sees blocking exchanges)"""
        if pyfunc is None:
            self._halo_cb = None
            self._chk(self.L.nlps_gpu_set_halo_exchange(self.h, C.cast(None, HALO_FN), None))
            return
        import inspect
        with_phase = len(inspect.signature(pyfunc).parameters) >= 5

        def _cb(ctx, dptr, nfield, elem, kind, phase):
            try:
                if with_phase:
                    return int(pyfunc(dptr, nfield, elem, kind, phase) or 0)
                if phase == 2:
                    return 0  # the matching start call already did the whole exchange in stream order
                return int(pyfunc(dptr, nfield, elem, kind) or 0)
            except Exception as e:  # never let an exception cross the C boundary
                print("halo exchange failed:", repr(e))
                return 1

        self._halo_cb = HALO_FN(_cb)
        self._chk(self.L.nlps_gpu_set_halo_exchange(self.h, self._halo_cb, None))

    def resort(self):
        self._chk(self.L.nlps_gpu_resort(self.h))

    def set_resort_interval(self, n):
        self._chk(self.L.nlps_gpu_set_resort_interval(self.h, int(n)))

    def set_adaptive_resort(self, budget, min_steps=4):
        self.L.nlps_gpu_set_adaptive_resort.argtypes = [C.c_void_p, C.c_double, C.c_int]
        self._chk(self.L.nlps_gpu_set_adaptive_resort(self.h, float(budget), int(min_steps)))

    def debug_option(self, name, value):
        """developer / test switch between equivalent launch forms (nlps_gpu_debug_option; the library reads no environment)"""
        self.L.nlps_gpu_debug_option.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
        self._chk(self.L.nlps_gpu_debug_option(self.h, name.encode(), float(value)))

    def debug_displaced(self):
        v, d = C.c_int(0), C.c_double(0)
        self.L.nlps_gpu_debug_displaced.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)]
        self._chk(self.L.nlps_gpu_debug_displaced(self.h, C.byref(v), C.byref(d)))
        return v.value, d.value

    def set_law_launch_mode(self, mode):
        self._chk(self.L.nlps_gpu_set_law_launch_mode(self.h, int(mode)))

    # ------------------------------------------------------------------ RCCL owned by the library
    @staticmethod
    def rccl_unique_id():
        """128-byte ncclUniqueId (made by rank 0, handed to the other ranks by the host driver)"""
        buf = (C.c_ubyte * 128)()
        if lib().nlps_gpu_rccl_unique_id(buf):
            raise NlpsError("nlps_gpu_rccl_unique_id failed (librccl.so.1 not loadable?)")
        return bytes(buf)

    def rccl_attach(self, uid, rank, world, layer_lo, layer_hi, mode=0):
        buf = (C.c_ubyte * 128).from_buffer_copy(uid)
        lo = np.ascontiguousarray(layer_lo, dtype=np.int32)
        hi = np.ascontiguousarray(layer_hi, dtype=np.int32)
        self._chk(self.L.nlps_gpu_rccl_attach(self.h, buf, int(rank), int(world), _i(lo), _i(hi), int(mode)))

    def rccl_detach(self):
        self._chk(self.L.nlps_gpu_rccl_detach(self.h))

    def rccl_reduce(self, dptr, n, root=-1):
        self._chk(self.L.nlps_gpu_rccl_reduce(self.h, _vp(dptr), int(n), int(root)))

    def rccl_info(self):
        """-> (nranks, rank) as RCCL reports them, overlap mode in force (0 blocking, 1 split launches, 2 one launch per stage)"""
        n, r, m = C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(self.L.nlps_gpu_rccl_info(self.h, C.byref(n), C.byref(r), C.byref(m)))
        return n.value, r.value, m.value

    def rccl_migrate(self, keep_lo, keep_hi, selftest=False):
        """Migration with the transport inside the library (ncclSend / ncclRecv): -> (sent_down, sent_up, received)"""
        d, u, g = C.c_int(0), C.c_int(0), C.c_int(0)
        fn = self.L.nlps_gpu_rccl_selftest_migrate if selftest else self.L.nlps_gpu_rccl_migrate
        self._chk(fn(self.h, int(keep_lo), int(keep_hi), C.byref(d), C.byref(u), C.byref(g)))
        self.num_particles()
        return d.value, u.value, g.value

    def rccl_selftest_exchange(self, dptr, nfield, elem_bytes, kind, overlap):
        self._chk(self.L.nlps_gpu_rccl_selftest_exchange(self.h, _vp(dptr), int(nfield), int(elem_bytes), int(kind),
                                                         1 if overlap else 0))

    def set_deterministic(self, on=True):
        self._chk(self.L.nlps_gpu_set_deterministic(self.h, 1 if on else 0))

    def set_explicit_damage(self, on=True):
        """The eigenerosion / eigensoftening hooks inside explicit_step (off by default: the step refuses a damage cloud);
        the definition of such a step is in include/nlps_gpu.h."""
        self._chk(self.L.nlps_gpu_set_explicit_damage(self.h, 1 if on else 0))

    def set_explicit_fluid(self, on=True):
        """explicit_step for a cloud that holds the compressible Newtonian fluid (off by default: the step refuses such a
        cloud); the rate of such a step, dt_F_n1 = (F_n1 - F_n) / dt, is defined in include/nlps_gpu.h."""
        self._chk(self.L.nlps_gpu_set_explicit_fluid(self.h, 1 if on else 0))

    def set_explicit_fbar(self, alpha, block=1, Fbar_n=None, Jbar_n=None):
        """F-bar on lattice-cell patches inside explicit_step.  alpha: one entry per material, alpha_Fbar in [0, 1] for a
        material whose law reads F-bar, < 0 for one that does not; alpha=None switches it off.  block: cells per patch, one
        number or one per axis.  Fbar_n [np][T] / Jbar_n [np] in the caller's order, None: F_n / J_n as they stand on the
        device.  The definition is in include/nlps_gpu.h."""
        self.L.nlps_gpu_set_explicit_fbar.argtypes = [C.c_void_p, C.POINTER(FbarCfg)]
        if alpha is None:
            self._chk(self.L.nlps_gpu_set_explicit_fbar(self.h, None))
            return
        b = [int(block)] * 3 if np.isscalar(block) else (list(int(v) for v in block) + [1, 1, 1])[:3]
        al = np.ascontiguousarray(alpha, dtype=np.float64)
        F = None if Fbar_n is None else np.ascontiguousarray(Fbar_n, dtype=np.float64)
        J = None if Jbar_n is None else np.ascontiguousarray(Jbar_n, dtype=np.float64)
        if al.size != self.nmats or (F is not None and F.shape != (self.np, self.T)) or (J is not None and J.shape != (self.np,)):
            raise NlpsError("set_explicit_fbar: alpha is [nmats], Fbar_n [np][T], Jbar_n [np]")
        cfg = FbarCfg((C.c_int * 3)(*b), _d(al), _d(F), _d(J))
        self._chk(self.L.nlps_gpu_set_explicit_fbar(self.h, C.byref(cfg)))

    def download_fbar(self):
        """-> (Fbar_n [np][T], Jbar_n [np]) in the caller's order"""
        F, J = np.zeros((self.np, self.T)), np.zeros(self.np)
        self.L.nlps_gpu_download_fbar.argtypes = [C.c_void_p, _dp, _dp]
        self._chk(self.L.nlps_gpu_download_fbar(self.h, _d(F), _d(J)))
        return F, J

    def set_explicit_loads(self, loads, thickness=1.0, area0=None):
        """The Neumann contours of explicit_step (compute_Nodal_Nominal_traction_Forces): a BccSet whose nodes are particle
        indices in the caller's order, or None to remove the loads.  Everything is copied to the device.  The contract is
        in include/nlps_gpu.h."""
        a0 = None if area0 is None else np.ascontiguousarray(area0, dtype=np.float64)
        self._chk(self.L.nlps_gpu_set_explicit_loads(self.h, None if loads is None else loads.arr, 0 if loads is None else loads.n,
                                                     float(thickness), None if a0 is None else a0.ctypes.data))

    def set_step_record(self, every=1, capacity=64, nsets=0, probes=None, probe_fields=0):
        """The step record: one row per recorded step, made on the device behind explicit_step / newmark_step and kept in a
        ring of `capacity` rows; every=None switches it off.  `probes`: particle indices in the caller's order,
        `probe_fields`: PROBE_* bits.  The contract is in include/nlps_gpu.h."""
        L = self.L
        L.nlps_gpu_set_step_record.argtypes = [C.c_void_p, C.POINTER(RecordCfg)]
        if every is None:
            self._chk(L.nlps_gpu_set_step_record(self.h, None))
            return
        ids = np.ascontiguousarray([] if probes is None else probes, dtype=np.int32)
        cfg = RecordCfg(int(every), int(capacity), int(nsets), int(ids.size), _i(ids) if ids.size else None,
                        int(probe_fields))
        self._chk(L.nlps_gpu_set_step_record(self.h, C.byref(cfg)))

    def step_record_layout(self):
        """-> (doubles per row, offset of the reaction block, offset of the probe block, doubles per probe)"""
        self.L.nlps_gpu_step_record_layout.argtypes = [C.c_void_p, _ip, _ip, _ip, _ip]
        v = [C.c_int(0) for _ in range(4)]
        self._chk(self.L.nlps_gpu_step_record_layout(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def record_now(self, tag=0):
        self.L.nlps_gpu_record_now.argtypes = [C.c_void_p, C.c_int]
        self._chk(self.L.nlps_gpu_record_now(self.h, int(tag)))

    def read_step_records(self, max_rows=None, counts_only=False):
        """The newest rows of the ring, oldest first: a dict with the named columns of the global block (REC_COLUMNS; the
        vectors as [rows][3]), `reactions` [rows][nsets][3], `probes` [rows][nprobes][doubles per probe] (`probe_slices`
        gives the slice of every selected field inside a probe's block), `rows` (the raw rows), `total` (rows written since
        the set) and `count`.  One synchronisation of the handle's stream."""
        L = self.L
        L.nlps_gpu_read_step_records.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), _ip, C.c_void_p, C.c_int]
        row, ro, po, pd = self.step_record_layout()
        total, count = C.c_longlong(0), C.c_int(0)
        self._chk(L.nlps_gpu_read_step_records(self.h, C.byref(total), C.byref(count), None,
                                               2 ** 31 - 1 if max_rows is None else int(max_rows)))
        out = {"total": total.value, "count": count.value}
        if counts_only:
            return out
        rows = np.zeros((count.value, row))
        self._chk(L.nlps_gpu_read_step_records(self.h, C.byref(total), C.byref(count), _vp(rows), count.value))
        out["rows"] = rows
        for name, (off, n) in REC_COLUMNS.items():
            out[name] = rows[:, off] if n == 1 else rows[:, off:off + n]
        nsets = (po - ro) // 3
        out["reactions"] = rows[:, ro:po].reshape(count.value, nsets, 3)
        out["probes"] = rows[:, po:].reshape(count.value, -1, pd) if pd else np.zeros((count.value, 0, 0))
        return out

    def probe_slices(self, probe_fields):
        """name -> slice inside a probe's block, for the fields selected in `probe_fields` (ascending bit order)"""
        d, T, off, out = self.ndim, self.T, 0, {}
        for b, (name, n) in enumerate((("x_GC", d), ("dis", d), ("vel", d), ("acc", d), ("F_n", T), ("Stress", T), ("J_n", 1),
                                       ("EPS_n", 1), ("Damage_n", 1), ("W", 1))):
            if (probe_fields >> b) & 1:
                out[name] = slice(off, off + n)
                off += n
        return out

    def set_snapshots(self, fields, slots=2):
        """The particle snapshot: `fields` is a mask of SNAP_BITS or a list of names as download_state() takes them, `slots`
        the number of snapshots that may be in flight or unreleased; fields=None switches it off (waits for the copies
        in flight, frees).  The contract is in include/nlps_gpu.h."""
        L = self.L
        L.nlps_gpu_set_snapshots.argtypes = [C.c_void_p, C.POINTER(SnapshotCfg)]
        if fields is None:
            self._chk(L.nlps_gpu_set_snapshots(self.h, None))
            return
        cfg = SnapshotCfg(snapshot_mask(fields) & 0xFFFFFFFF, int(slots))
        self._chk(L.nlps_gpu_set_snapshots(self.h, C.byref(cfg)))

    def snapshot_begin(self, tag=0):
        """Packs the selected fields of the state as it stands on the handle's stream and queues their copy to pinned
        memory on the snapshot stream; returns the slot at once (no synchronisation)."""
        self.L.nlps_gpu_snapshot_begin.argtypes = [C.c_void_p, C.c_int, _ip]
        slot = C.c_int(-1)
        self._chk(self.L.nlps_gpu_snapshot_begin(self.h, int(tag), C.byref(slot)))
        return slot.value

    def snapshot_wait(self, slot, copy=True):
        """Waits for that slot's copy alone; -> the dict download_state(fields) would have returned in place of
        snapshot_begin (same names, aliases included), with `tag`.  copy=False: the arrays are views of the slot's pinned
        block, valid until snapshot_release(slot) / set_snapshots / close()."""
        self.L.nlps_gpu_snapshot_wait.argtypes = [C.c_void_p, C.c_int, C.POINTER(Particles), _ip]
        hp, tag = Particles(), C.c_int(0)
        self._chk(self.L.nlps_gpu_snapshot_wait(self.h, int(slot), C.byref(hp), C.byref(tag)))
        n, o = hp.np, {}
        for name, w in SNAP_FIELDS:
            ptr = getattr(hp, name)
            if not ptr:
                continue
            w = {"d": self.ndim, "T": self.T}.get(w, w)
            shape = (n,) if w == 1 else (n, w)
            if n == 0:
                a = np.zeros(shape, dtype=np.int32 if name == "I0" else np.float64)
            else:
                a = np.ctypeslib.as_array(ptr, shape=shape)
            o[name] = a.copy() if copy else a
        for short, full in (("x", "x_GC"), ("lambda", "lambda_"), ("beta", "Beta")):
            if full in o:
                o[short] = o[full]
        o["tag"] = tag.value
        return o

    def snapshot_release(self, slot):
        self.L.nlps_gpu_snapshot_release.argtypes = [C.c_void_p, C.c_int]
        self._chk(self.L.nlps_gpu_snapshot_release(self.h, int(slot)))

    def snapshot_bytes(self):
        """-> (device bytes, pinned bytes) the snapshots hold"""
        self.L.nlps_gpu_snapshot_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        dev, pin = C.c_size_t(0), C.c_size_t(0)
        self._chk(self.L.nlps_gpu_snapshot_bytes(self.h, C.byref(dev), C.byref(pin)))
        return dev.value, pin.value

    def set_implicit_damage(self, on=True):
        """The eigenerosion / eigensoftening hooks inside the fused residual (off by default: lagrangian_evaluation runs the
        separate stages for a damage cloud); newton_solve and newmark_step take it too.  The definition is in
        include/nlps_gpu.h."""
        self._chk(self.L.nlps_gpu_set_implicit_damage(self.h, 1 if on else 0))

    def set_deterministic_damage(self, on=True):
        """Extends set_deterministic to a cloud with the damage hooks (off by default: the explicit step refuses such a
        cloud in the mode, the implicit path sums with atomics).  The contract is in include/nlps_gpu.h."""
        self._chk(self.L.nlps_gpu_set_deterministic_damage(self.h, 1 if on else 0))

    def debug_damage_runs(self, snapshot=False):
        """developer read-out: (key[np], first[nnodes], last[nnodes], sorted[np]) of the node runs the last step or
        residual evaluation left -- of the current closest nodes, or of the eigenerosion snapshot's"""
        key, srt = np.zeros(self.np, dtype=np.int32), np.zeros(self.np, dtype=np.int32)
        first, last = np.zeros(self.nnodes, dtype=np.int32), np.zeros(self.nnodes, dtype=np.int32)
        self.L.nlps_gpu_debug_damage_runs.argtypes = [C.c_void_p, C.c_int, _ip, _ip, _ip, _ip]
        self._chk(self.L.nlps_gpu_debug_damage_runs(self.h, 1 if snapshot else 0, _i(key), _i(first), _i(last), _i(srt)))
        return key, first, last, srt

    def debug_damage_counters(self):
        """developer read-out: (builds of the node runs of the current closest nodes, residual evaluations that took the fused
        damage form) since the handle was made"""
        b, e = C.c_int(0), C.c_int(0)
        self.L.nlps_gpu_debug_damage_counters.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        self._chk(self.L.nlps_gpu_debug_damage_counters(self.h, C.byref(b), C.byref(e)))
        return b.value, e.value

    def touched_layers(self):
        lo, hi = C.c_int(0), C.c_int(0)
        self._chk(self.L.nlps_gpu_touched_layers(self.h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def form_initial_guess(self, Un_dt, Un_dt2, dt, bcs, step, use_explicit_trial=True):  # __form_initial_guess
        dU = np.zeros(self.nactive * self.ndim)
        self._chk(self.L.nlps_gpu_form_initial_guess(self.h, _vp(dU), _vp(Un_dt), _vp(Un_dt2), float(dt),
                                                     1 if use_explicit_trial else 0, bcs.arr, bcs.n, int(step)))
        return dU

    def compute_nodal_kinetic_increments(self, dU, Un_dt, Un_dt2, alpha):  # __compute_nodal_kinetic_increments
        n = self.nactive * self.ndim
        dV, dA = np.zeros(n), np.zeros(n)
        al = np.ascontiguousarray(alpha, dtype=np.float64)
        self._chk(self.L.nlps_gpu_nodal_kinetic_increments(self.h, _vp(dV), _vp(dA), _vp(dU), _vp(Un_dt), _vp(Un_dt2),
                                                           _d(al)))
        return dV, dA

    def nodal_inertial_forces(self, R, M, dU, Un_dt, Un_dt2, alpha, gravity=None):  # __nodal_inertial_forces
        al = np.ascontiguousarray(alpha, dtype=np.float64)
        gv = None if gravity is None else np.ascontiguousarray(gravity, dtype=np.float64)
        self._chk(self.L.nlps_gpu_nodal_inertial_forces(self.h, _vp(R), _vp(M), _vp(dU), _vp(Un_dt), _vp(Un_dt2), _d(al),
                                                        _d(gv)))
        return R

    LAGR_RATES, LAGR_SEPARATE, LAGR_SAME_STEP = 1, 2, 4

    def lagrangian_evaluation(self, dU, Un_dt, Un_dt2, M, alpha, gravity=None, loads=None, step=0, thickness=1.0,
                              area0=None, flags=0, out=None):  # __lagrangian_evaluation
        """The residual of the implicit driver's SNES solve as one device call (nlps_gpu_lagrangian_evaluation).
        Vectors: numpy arrays (host) or torch tensors (device); out = the residual vector to overwrite (default: a new
        numpy array)."""
        self.L.nlps_gpu_lagrangian_evaluation.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [_dp, _dp, C.POINTER(Bcc), C.c_int,
                                                          C.c_int, C.c_double, C.c_void_p, C.c_int]
        R = np.zeros(self.nactive * self.ndim) if out is None else out
        al = np.ascontiguousarray(alpha, dtype=np.float64)
        gv = None if gravity is None else np.ascontiguousarray(gravity, dtype=np.float64)
        a0 = None if area0 is None else np.ascontiguousarray(area0, dtype=np.float64)
        self._chk(self.L.nlps_gpu_lagrangian_evaluation(
            self.h, _vp(R), _vp(dU), _vp(Un_dt), _vp(Un_dt2), _vp(M), _d(al), _d(gv), None if loads is None else loads.arr,
            0 if loads is None else loads.n, int(step), float(thickness), None if a0 is None else a0.ctypes.data, int(flags)))
        return R

    def set_tangent_alpha4(self, alpha_4):
        """alpha_4 of the Newmark scheme for the fluid law's tangent (0 = quasi-static, the default)."""
        self._chk(self.L.nlps_gpu_set_tangent_alpha4(self.h, float(alpha_4)))

    def jacobian_evaluation(self, alpha_1=0.0, lumped_mass=None, apply_dirichlet=False, on_device=False):  # __jacobian_evaluation
        """COO triplets (rows, cols, vals) of the tangent matrix in masked dof numbering.  on_device: torch tensors on
        the GPU, written by the emit kernel itself (what MatSetValuesCOO of a GPU matrix type takes; nothing crosses PCIe)."""
        nnz = C.c_longlong(0)
        self._chk(self.L.nlps_gpu_tangent_assemble(self.h, C.byref(nnz)))
        n = int(nnz.value)
        self.L.nlps_gpu_tangent_coo.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        if on_device:
            import torch
            rows = torch.empty(n, dtype=torch.int32, device="cuda")
            cols = torch.empty(n, dtype=torch.int32, device="cuda")
            vals = torch.empty(n, dtype=torch.float64, device="cuda")
        else:
            rows, cols, vals = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n)
        self._chk(self.L.nlps_gpu_tangent_coo(self.h, float(alpha_1), _vp(lumped_mass), 1 if apply_dirichlet else 0,
                                              _vp(rows), _vp(cols), _vp(vals)))
        return rows, cols, vals

    def tangent_operator(self, alpha_1=0.0, lumped_mass=None, apply_dirichlet=False):  # __jacobian_evaluation as a MatShell
        """Linearises at the current particle state without forming the matrix (nlps_gpu_tangent_operator): the operator of
        tangent_apply / tangent_block_diagonal, the same K as jacobian_evaluation(alpha_1, lumped_mass, apply_dirichlet).
        Returns the device bytes the operator holds."""
        nb = C.c_size_t(0)
        self._chk(self.L.nlps_gpu_tangent_operator(self.h, float(alpha_1), _vp(lumped_mass), 1 if apply_dirichlet else 0,
                                                   C.byref(nb)))
        return int(nb.value)

    def tangent_apply(self, x, out=None):
        """y = K x (MATOP_MULT).  x: numpy array (host) or torch tensor (device), masked [nactive*ndim]; y of the same kind
        (out = the vector to overwrite)."""
        if out is None:
            if isinstance(x, np.ndarray):
                out = np.empty(self.nactive * self.ndim)
            else:
                import torch
                out = torch.empty(self.nactive * self.ndim, dtype=torch.float64, device=x.device)
        self._chk(self.L.nlps_gpu_tangent_apply(self.h, _vp(x), _vp(out)))
        return out

    def tangent_block_diagonal(self, on_device=False):
        """The nactive d x d diagonal blocks of K, shape (nactive, ndim, ndim), masked node order (MATOP_GET_DIAGONAL)."""
        shape = (self.nactive, self.ndim, self.ndim)
        if on_device:
            import torch
            out = torch.empty(shape, dtype=torch.float64, device="cuda")
        else:
            out = np.empty(shape)
        self._chk(self.L.nlps_gpu_tangent_block_diagonal(self.h, _vp(out)))
        return out

    def tangent_csr_pattern(self):
        """The sparsity structure of the tangent of the last tangent_operator, for tangent_csr
        (nlps_gpu_tangent_csr_pattern).  Returns (nnz, bytes): the stored entries and the device bytes the CSR path keeps
        on the handle."""
        nnz, nb = C.c_longlong(0), C.c_size_t(0)
        self._chk(self.L.nlps_gpu_tangent_csr_pattern(self.h, C.byref(nnz), C.byref(nb)))
        self._csr_nnz = int(nnz.value)
        return self._csr_nnz, int(nb.value)

    def tangent_csr(self, on_device=False):
        """(row_ptr, cols, vals) of the tangent of the last tangent_operator in CSR, masked dof numbering, columns ascending
        in every row (nlps_gpu_tangent_csr; what MatCreateSeqAIJWithArrays takes).  Assembled row by row without float
        atomics: two calls return the same bits.  Needs tangent_csr_pattern() since the operator.  on_device: torch tensors
        on the GPU, written by the row kernel itself."""
        n = getattr(self, "_csr_nnz", 0)
        row_ptr, cols, vals = _csr_arrays(self.nactive * self.ndim + 1, n, (), on_device)
        self._chk(self.L.nlps_gpu_tangent_csr(self.h, _vp(row_ptr), _vp(cols), _vp(vals)))
        return row_ptr, cols, vals

    def tangent_bsr_pattern(self, kind="full"):
        """The block structure of the tangent of the last tangent_operator, for tangent_bsr
        (nlps_gpu_tangent_bsr_pattern).  kind: "full" (every d x d block, MATSEQBAIJ) or "upper" (the blocks B >= A of a
        Neo-Hookean cloud's symmetric tangent, MATSEQSBAIJ).  Returns (nblocks, bytes): the stored blocks and the device
        bytes the CSR / block-CSR path keeps on the handle."""
        kinds = {"full": 0, "upper": 1}
        nblk, nb = C.c_longlong(0), C.c_size_t(0)
        self._chk(self.L.nlps_gpu_tangent_bsr_pattern(self.h, kinds.get(kind, kind), C.byref(nblk), C.byref(nb)))
        self._bsr_nblocks = int(nblk.value)
        return self._bsr_nblocks, int(nb.value)

    def tangent_bsr(self, col_major=False, on_device=False):
        """(brow_ptr, bcols, vals) of the tangent of the last tangent_operator in block CSR, masked node numbering, bcols
        ascending in every block row, vals shaped (nblocks, ndim, ndim) (nlps_gpu_tangent_bsr; what
        MatCreateSeqBAIJWithArrays / MatCreateSeqSBAIJWithArrays take).  The values are the bits of tangent_csr's.
        col_major: vals[q] holds the transposed block (PETSc's Fortran-ordered blocks).  Needs tangent_bsr_pattern()
        since the operator.  on_device: torch tensors on the GPU, written by the row kernel itself."""
        n = getattr(self, "_bsr_nblocks", 0)
        brow_ptr, bcols, vals = _csr_arrays(self.nactive + 1, n, (self.ndim, self.ndim), on_device)
        self._chk(self.L.nlps_gpu_tangent_bsr(self.h, 1 if col_major else 0, _vp(brow_ptr), _vp(bcols), _vp(vals)))
        return brow_ptr, bcols, vals

    def set_linear_solver(self, kind):
        """The Krylov method of tangent_solve, newton_solve and newmark_step on this handle: "gmres" (the default) or
        "minres" (symmetric tangents: refused, naming the laws, unless every particle is Neo-Hookean)."""
        if kind not in KSP_TYPES:
            raise ValueError(f"kind must be one of {sorted(KSP_TYPES)}")
        self._chk(self.L.nlps_gpu_set_linear_solver(self.h, KSP_TYPES[kind]))

    def tangent_solve(self, b, x=None, pc="pbjacobi", restart=30, max_it=10000, rtol=1e-5, atol=0.0, dtol=1e5,
                      history=False, out=None):
        """K x = b on the device by GMRES(restart), right-preconditioned (nlps_gpu_tangent_solve; the driver's KSPSolve),
        or, after set_linear_solver("minres") on a Neo-Hookean cloud, by preconditioned MINRES (restart is then not read;
        reason may be -8, diverged_indefinite_pc).
        b: numpy array (host) or torch tensor (device), masked [nactive*ndim]; the result is of the same kind.  x: an
        initial guess (left as it is unless it is also out), None for x0 = 0.  out: the vector to write (default: a new
        one).  pc: "none", "jacobi" or "pbjacobi".  Returns (x, info), info = dict(iterations, reason (an NLPS_KSP_*
        value), reason_name, rnorm (the true residual of x), bnorm, bytes, history (iterations + 1 norms, or None))."""
        if pc not in PC_KINDS:
            raise ValueError(f"pc must be one of {sorted(PC_KINDS)}")
        n = self.nactive * self.ndim
        if out is None:
            if isinstance(b, np.ndarray):
                out = np.empty(n)
            else:
                import torch
                out = torch.empty(n, dtype=torch.float64, device=b.device)
        if x is not None and x is not out:
            if isinstance(out, np.ndarray):
                out[:] = x if isinstance(x, np.ndarray) else x.detach().cpu().numpy()
            else:
                import torch
                out.copy_(torch.as_tensor(x, dtype=torch.float64))
        hist = np.zeros(max_it + 1) if history else None
        k = Ksp(pc=PC_KINDS[pc], restart=int(restart), max_it=int(max_it), x_is_guess=1 if x is not None else 0,
                rtol=float(rtol), atol=float(atol), dtol=float(dtol), history=_d(hist) if hist is not None else None)
        self._chk(self.L.nlps_gpu_tangent_solve(self.h, _vp(b), _vp(out), C.byref(k)))
        info = dict(iterations=k.iterations, reason=k.reason, reason_name=KSP_REASONS.get(k.reason, str(k.reason)),
                    rnorm=k.rnorm, bnorm=k.bnorm, bytes=int(k.bytes),
                    history=hist[: k.iterations + 1].copy() if hist is not None else None)
        return out, info

    def tangent_lambda_max(self, mass, v0=None, max_it=64, rtol=1e-6, seed=0, mode=False, history=False):
        """The largest Ritz value of the pencil (K, M) on the free dofs of the last tangent_operator, by Lanczos on the
        device (nlps_gpu_tangent_lambda_max).  mass, v0: numpy arrays (host) or torch tensors (device), masked
        [nactive*ndim]; v0 None: the hash vector of seed.  mode: True for a new vector of mass's kind, or the vector to
        write.  Returns info = dict(theta, resid, asymmetry, iterations, reason (an NLPS_EIG_* value), reason_name, bytes,
        history (iterations values theta_j, or None), mode (or None))."""
        out = None
        if mode is True:
            if isinstance(mass, np.ndarray):
                out = np.empty(self.nactive * self.ndim)
            else:
                import torch
                out = torch.empty(self.nactive * self.ndim, dtype=torch.float64, device=mass.device)
        elif mode is not False and mode is not None:
            out = mode
        hist = np.zeros(max(int(max_it), 1)) if history else None
        e = Eig(max_it=int(max_it), rtol=float(rtol), seed=int(seed), history=_d(hist) if hist is not None else None)
        self._chk(self.L.nlps_gpu_tangent_lambda_max(self.h, _vp(mass), _vp(v0), C.byref(e), _vp(out)))
        return dict(theta=e.theta, resid=e.resid, asymmetry=e.asymmetry, iterations=e.iterations, reason=e.reason,
                    reason_name=EIG_REASONS.get(e.reason, str(e.reason)), bytes=int(e.bytes),
                    history=hist[: e.iterations].copy() if hist is not None else None, mode=out)

    @staticmethod
    def _snes(max_it, max_funcs, atol, rtol, stol, divtol, linesearch, ls_alpha, ls_steptol, ls_maxstep, ls_max_it,
              apply_dirichlet, ksp):
        """(nlps_snes, the host arrays it points to) from keyword settings; ksp: the keywords of tangent_solve"""
        if linesearch not in LINE_SEARCHES:
            raise ValueError(f"linesearch must be one of {sorted(LINE_SEARCHES)}")
        kw = dict(pc="jacobi", restart=30, max_it=10000, rtol=1e-5, atol=0.0, dtol=1e5)
        kw.update(ksp or {})
        if kw["pc"] not in PC_KINDS:
            raise ValueError(f"pc must be one of {sorted(PC_KINDS)}")
        m = max(int(max_it), 0)
        keep = dict(fnorm=np.zeros(m + 1), lam=np.zeros(max(m, 1)), kits=np.zeros(max(m, 1), dtype=np.int32))
        k = Ksp(pc=PC_KINDS[kw["pc"]], restart=int(kw["restart"]), max_it=int(kw["max_it"]), x_is_guess=0,
                rtol=float(kw["rtol"]), atol=float(kw["atol"]), dtol=float(kw["dtol"]), history=None)
        sn = Snes(max_it=int(max_it), max_funcs=int(max_funcs), atol=float(atol), rtol=float(rtol), stol=float(stol),
                  divtol=float(divtol), linesearch=LINE_SEARCHES[linesearch], ls_alpha=float(ls_alpha),
                  ls_steptol=float(ls_steptol), ls_maxstep=float(ls_maxstep), ls_max_it=int(ls_max_it),
                  apply_dirichlet=1 if apply_dirichlet else 0, ksp=k, fnorm_history=_d(keep["fnorm"]),
                  lambda_history=_d(keep["lam"]), ksp_iterations=_i(keep["kits"]))
        return sn, keep

    @staticmethod
    def _snes_info(sn, keep):
        it = sn.iterations
        failed = 1 if sn.reason == -3 else 0  # (the iterate whose linear solve failed still reports its Arnoldi steps)
        return dict(reason=sn.reason, reason_name=SNES_REASONS.get(sn.reason, str(sn.reason)), iterations=it,
                    function_evaluations=sn.function_evaluations, linear_iterations=sn.linear_iterations,
                    fnorm0=sn.fnorm0, fnorm=sn.fnorm, snorm=sn.snorm, xnorm=sn.xnorm,
                    fnorm_history=keep["fnorm"][: it + 1].copy(), lambda_history=keep["lam"][:it].copy(),
                    ksp_iterations=keep["kits"][: it + failed].copy(), ksp_reason=sn.ksp.reason, ksp_rnorm=sn.ksp.rnorm)

    def newton_solve(self, dU, Un_dt, Un_dt2, M, alpha, gravity=None, loads=None, step=0, thickness=1.0, area0=None,
                     max_it=50, max_funcs=10000, atol=1e-8, rtol=1e-10, stol=1e-8, divtol=1e4, linesearch="bt",
                     ls_alpha=1e-4, ls_steptol=1e-12, ls_maxstep=1e8, ls_max_it=40, apply_dirichlet=True, ksp=None,
                     out=None):
        """The driver's SNESSolve on the device (nlps_gpu_newton_solve): Newton with a "basic" or "bt" line search around
        lagrangian_evaluation, tangent_operator and tangent_solve.  dU: the initial guess (left as it is unless it is also
        out); vectors are numpy arrays (host) or torch tensors (device), the result is of dU's kind.  ksp: a dict of
        tangent_solve's settings (pc, restart, max_it, rtol, atol, dtol; the driver's PCJACOBI / GMRES(30) / 1e-5 by
        default).  Returns (dU, info): info = dict(reason (an NLPS_SNES_* value), reason_name, iterations,
        function_evaluations, linear_iterations, fnorm0, fnorm, snorm, xnorm, fnorm_history (iterations + 1),
        lambda_history and ksp_iterations (one per iterate), ksp_reason, ksp_rnorm (the last linear solve))."""
        if out is None:
            out = dU.copy() if isinstance(dU, np.ndarray) else dU.clone()
        elif out is not dU:
            if isinstance(out, np.ndarray):
                out[:] = dU if isinstance(dU, np.ndarray) else dU.detach().cpu().numpy()
            else:
                import torch
                out.copy_(torch.as_tensor(dU, dtype=torch.float64))
        sn, keep = self._snes(max_it, max_funcs, atol, rtol, stol, divtol, linesearch, ls_alpha, ls_steptol, ls_maxstep,
                              ls_max_it, apply_dirichlet, ksp)
        al = np.ascontiguousarray(alpha, dtype=np.float64)
        gv = None if gravity is None else np.ascontiguousarray(gravity, dtype=np.float64)
        a0 = None if area0 is None else np.ascontiguousarray(area0, dtype=np.float64)
        self._chk(self.L.nlps_gpu_newton_solve(
            self.h, _vp(out), _vp(Un_dt), _vp(Un_dt2), _vp(M), _d(al), _d(gv), None if loads is None else loads.arr,
            0 if loads is None else loads.n, int(step), float(thickness), None if a0 is None else a0.ctypes.data,
            C.byref(sn)))
        return out, self._snes_info(sn, keep)

    def newmark_step(self, bcs, step, dt, gravity=None, beta=0.25, gamma=0.5, alpha_blend=1.0, use_explicit_trial=True,
                     loads=None, thickness=1.0, area0=None, max_it=50, max_funcs=10000, atol=1e-8, rtol=1e-10,
                     stol=1e-8, divtol=1e4, linesearch="bt", ls_alpha=1e-4, ls_steptol=1e-12, ls_maxstep=1e8,
                     ls_max_it=40, ksp=None, dU_out=None):
        """One time step of the implicit driver on the device (nlps_gpu_newmark_step): search, masks, lumped mass, nodal
        field, initial guess, newton_solve, kinetic increments, roll and particle update.  The particles are updated only
        when info["reason"] > 0.  dU_out: a numpy array or torch tensor of at least nnodes*ndim doubles that receives the
        converged increments (its first nactive*ndim entries), or None.  Returns newton_solve's info with "nactive"."""
        sn, keep = self._snes(max_it, max_funcs, atol, rtol, stol, divtol, linesearch, ls_alpha, ls_steptol, ls_maxstep,
                              ls_max_it, True, ksp)
        nm = Newmark(float(beta), float(gamma), float(dt), float(alpha_blend), 1 if use_explicit_trial else 0)
        gv = None if gravity is None else np.ascontiguousarray(gravity, dtype=np.float64)
        a0 = None if area0 is None else np.ascontiguousarray(area0, dtype=np.float64)
        na = C.c_int(0)
        self._chk(self.L.nlps_gpu_newmark_step(
            self.h, bcs.arr, bcs.n, int(step), C.byref(nm), _d(gv), None if loads is None else loads.arr,
            0 if loads is None else loads.n, float(thickness), None if a0 is None else a0.ctypes.data, C.byref(sn),
            C.byref(na), _vp(dU_out)))
        self.nactive = na.value
        info = self._snes_info(sn, keep)
        info["nactive"] = na.value
        return info

    def create_sparsity_pattern(self):                  # __create_sparsity_pattern (after jacobian_evaluation)
        pat = np.zeros(self.nactive * self.ndim, dtype=np.int32)
        self._chk(self.L.nlps_gpu_sparsity_pattern(self.h, _i(pat)))
        return pat

    # ------------------------------------------------------------------ migration
    def num_particles(self):
        n = C.c_int(0)
        self._chk(self.L.nlps_gpu_num_particles(self.h, C.byref(n)))
        self.np = n.value
        return n.value

    def set_particle_ids(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        self._chk(self.L.nlps_gpu_set_particle_ids(self.h, _i(ids)))

    def download_ids(self):
        ids = np.zeros(self.num_particles(), dtype=np.int32)
        self._chk(self.L.nlps_gpu_download_ids(self.h, _i(ids)))
        return ids

    def migration_select(self, keep_lo, keep_hi):
        """-> (n_down, n_up, row_words, down_dptr, up_dptr): packed rows of the particles that leave"""
        nd, nu, rw = C.c_int(0), C.c_int(0), C.c_int(0)
        dp, up = C.c_void_p(), C.c_void_p()
        self._chk(self.L.nlps_gpu_migration_select(self.h, int(keep_lo), int(keep_hi), C.byref(nd), C.byref(nu),
                                                   C.byref(rw), C.byref(dp), C.byref(up)))
        return nd.value, nu.value, rw.value, dp.value, up.value

    def migration_commit(self, rows_a, n_a, rows_b, n_b):
        """rows_*: raw pointers (int) of packed rows, host or device"""
        self._chk(self.L.nlps_gpu_migration_commit(self.h, C.c_void_p(rows_a) if rows_a else None, int(n_a),
                                                   C.c_void_p(rows_b) if rows_b else None, int(n_b)))
        self.num_particles()

    def set_ghost_bands(self, band_lo, band_hi, overlap=True):
        """overlap: False / 0 blocking exchanges, True / 1 split launches, 2 one launch per stage (library RCCL only)"""
        self._chk(self.L.nlps_gpu_set_ghost_bands(self.h, int(band_lo), int(band_hi), int(overlap)))

    def set_node_numbering(self, lattice_of_file):
        """Masked numbering in the node order of a mesh file (None = lattice order): include/nlps_gpu.h"""
        a = None if lattice_of_file is None else np.ascontiguousarray(lattice_of_file, dtype=np.int32)
        self._chk(self.L.nlps_gpu_set_node_numbering(self.h, _i(a)))

    def set_node_window(self, layer_lo, layer_hi):
        self._chk(self.L.nlps_gpu_set_node_window(self.h, int(layer_lo), int(layer_hi)))

    def set_timing(self, on=True):
        self._chk(self.L.nlps_gpu_set_timing(self.h, 1 if on else 0))

    def get_timing(self):
        ms = (C.c_float * 8)()
        self._chk(self.L.nlps_gpu_get_timing(self.h, ms))
        return list(ms)
