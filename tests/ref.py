"""ctypes loader of oracle/_ref/libnlps_ref2d.so: the REFERENCE's own 2-D objects behind oracle/ref_bridge.c.

TEST INFRASTRUCTURE ONLY (CPU tests and tests/golden/make_ref_fixtures.py).  The reference exit()s on several failure
paths (the LME Newton, rcond, the tributary search), so no reference call runs in the test process: run() writes the
inputs to an .npz in a temporary directory, starts this file as a child Python process, and reads the outputs back.
A child that dies raises RefChildError: a test failure, never a skip.

    out = ref.run("matlib", A=A)                      # dict of arrays
    out = ref.run_cloud("init,shape", ref.cloud_inputs(case))
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STRIDE = 128   # slots per particle list (oracle.orc.MAXNB)
BEPS_STRIDE = 1024
MAT_TYPE_NAMES = ["Neo-Hookean-Wriggers", "Hencky", "Drucker-Prager", "Von-Mises", "Matsuoka-Nakai", "Lade-Duncan"]
_MAT_KEYS = ["E", "nu", "p_ref", "Ceps", "Gf", "ft", "heps", "wcrit", "kappa_0", "hardening_modulus", "eps_0",
             "cohesion", "phi_deg", "psi_deg", "exponent_ortiz", "K0_voce", "Kinf_voce", "delta_voce", "theta_voce"]
_MAT_DEFAULTS = {"exponent_ortiz": 1.0, "eps_0": 1.0, "theta_voce": 1.0, "wcrit": 1.0}


class RefChildError(RuntimeError):
    pass


def lib_path():
    """The library: rebuilt from the reference tree when that exists, else whatever oracle/_ref/ holds, else None."""
    from oracle import orc
    if os.path.isdir(orc.REF_ROOT):
        return orc.build_ref()
    return orc.REF_LIB if os.path.exists(orc.REF_LIB) else None


def available():
    from oracle import orc
    return os.path.isdir(orc.REF_ROOT) or os.path.exists(orc.REF_LIB)


def material_rows(materials):
    """materials: the dicts of tests/util.py and synth.py -> (type codes int32[nmat], parameters float64[nmat, 24])"""
    types = np.array([int(m["type"]) for m in materials], dtype=np.int32)
    rows = np.zeros((len(materials), 24))
    for i, m in enumerate(materials):
        rows[i, :19] = [float(m.get(k, _MAT_DEFAULTS.get(k, 0.0))) for k in _MAT_KEYS]
        rows[i, 19:22] = [float(v) for v in m.get("a_borja", (0.0, 0.0, 0.0))]
        rows[i, 22] = float(m.get("alpha_borja", 0.0))
        rows[i, 23] = float(m.get("p_atm", 0.0))
    return types, rows


def materials_from_rows(types, rows):
    """the inverse of material_rows(): dicts for oracle.orc.make_materials and nlps.Solver"""
    out = []
    for t, r in zip(types, rows):
        m = {k: float(v) for k, v in zip(_MAT_KEYS, r[:19])}
        m.update(type=int(t), a_borja=tuple(float(v) for v in r[19:22]), alpha_borja=float(r[22]))
        out.append(m)
    return out


def mesh_arrays(M):
    """The lattice tables the bridge fills the reference's Mesh with, from an oracle.orc.OracleMesh (2-D): node
    coordinates, Q4 connectivity in chain order (the mesh file lists a cell counter-clockwise from its low corner and
    push prepends), NodalLocality_0 / NodalLocality in chain order, h_avg, DeltaX.  The reference's mesh readers
    (InOutFun) are not part of the library: these tables are the project's and stay unpinned."""
    assert M.ndim == 2
    nx, ny = M.n[0], M.n[1]
    nn = M.nnodes
    elem = np.zeros(((nx - 1) * (ny - 1), 4), dtype=np.int32)
    for cj in range(ny - 1):
        for ci in range(nx - 1):
            a = ci + nx * cj
            elem[ci + (nx - 1) * cj] = [a + nx, a + nx + 1, a + 1, a]
    r1_ptr = np.array([M.m.r1_ptr[i] for i in range(nn + 1)], dtype=np.int32)
    r2_ptr = np.array([M.m.r2_ptr[i] for i in range(nn + 1)], dtype=np.int32)
    r1 = np.array([M.m.r1[i] for i in range(r1_ptr[-1])], dtype=np.int32)
    r2 = np.array([M.m.r2[i] for i in range(r2_ptr[-1])], dtype=np.int32)
    return {"coords": M.coords().copy(), "elem": elem, "r1_ptr": r1_ptr, "r1": r1, "r2_ptr": r2_ptr, "r2": r2,
            "h_avg": M.h_avg().copy(), "deltax": np.array(float(M.h))}


_CLOUD_KEYS = ["x", "dis", "vol0", "mass", "F_n", "b_e_n", "J_n", "kappa_n", "eps_n", "matidx"]


def cloud_inputs(case, prm=None):
    """What describes a tests/util.py case to run_cloud() and to a fixture: lattice parameters, particle arrays,
    materials as numbers and the globals.  Data only; the mesh tables are rebuilt from the lattice by with_mesh()."""
    from oracle import orc
    cl = case["cloud"]
    d = {"grid_n": np.array(case["grid_n"], dtype=np.int32), "origin": np.array(case["origin"], dtype=np.float64),
         "h": np.array(float(case["h"]))}
    for k in _CLOUD_KEYS:
        d[k] = np.ascontiguousarray(cl[k])
    for k in ("dt_F_n", "back_stress"):
        if cl.get(k) is not None:
            d[k] = np.ascontiguousarray(cl[k], dtype=np.float64)
    d["mat_types"], d["mat_params"] = material_rows(case["materials"])
    prm = prm or orc.default_params()
    gamma, tol0 = case.get("lme", (prm.gamma_lme, prm.tol_zero_lme))
    d["lme"] = np.array([gamma, tol0, prm.tol_wrapper_lme, prm.max_iter_lme], dtype=np.float64)
    d["rr"] = np.array([prm.tol_radial_returning, prm.max_iter_radial_returning], dtype=np.float64)
    return d


def fill_defaults(d):
    """The particle arrays a stored case may leave out, at the values synth.make_cloud gives a fresh 2-D cloud of
    4 particles per cell and one Neo-Hookean material: at rest, undeformed, density 1000."""
    from oracle import orc
    n, h = d["x"].shape[0], float(d["h"])
    ident = np.tile(np.array([1.0, 0.0, 0.0, 1.0, 1.0]), (n, 1))
    prm = orc.default_params()
    types, rows = material_rows([{"type": 0, "E": 1.0e7, "nu": 0.3}])
    defaults = {"dis": np.zeros((n, 2)), "vol0": np.full(n, h * h / 4), "mass": np.full(n, 1000.0 * h * h / 4),
                "F_n": ident, "b_e_n": ident, "J_n": np.ones(n), "kappa_n": np.zeros(n), "eps_n": np.zeros(n),
                "matidx": np.zeros(n, dtype=np.int32), "mat_types": types, "mat_params": rows,
                "rr": np.array([prm.tol_radial_returning, prm.max_iter_radial_returning], dtype=np.float64)}
    out = dict(d)
    for k, v in defaults.items():
        out.setdefault(k, v)
    return out


def strip_defaults(d):
    """drops what fill_defaults() would put back unchanged (keeps the fixtures small)"""
    full = fill_defaults({k: d[k] for k in ("x", "h")})
    return {k: v for k, v in d.items() if k in ("x", "h") or k not in full or not np.array_equal(full[k], v)}


def with_mesh(d):
    from oracle import orc
    d = fill_defaults(d)
    M = orc.OracleMesh(2, [int(v) for v in d["grid_n"]], [float(v) for v in d["origin"]], float(d["h"]))
    out = dict(d)
    out.update(mesh_arrays(M))
    return out


def run_cloud(stages, d, **extra):
    """run("cloud") on stored inputs `d` (cloud_inputs() plus whatever the stages read), mesh tables added here"""
    return run("cloud", stages=stages, **{**with_mesh(d), **extra})


def case_from_inputs(d):
    """The tests/util.py case a fixture's stored inputs describe (for oracle_setup / gpu_setup)."""
    d = fill_defaults(d)
    n = d["x"].shape[0]
    cloud = {k: np.array(d[k]) for k in _CLOUD_KEYS}
    cloud.update(ndim=2, vel=np.zeros((n, 2)), acc=np.zeros((n, 2)), rho=cloud["mass"] / cloud["vol0"])
    for k in ("dt_F_n", "back_stress", "damage_n", "strain_f_n"):
        if k in d:
            cloud[k] = np.array(d[k])
    gn = [int(v) for v in d["grid_n"]]
    return {"ndim": 2, "cells": [gn[0] - 1, gn[1] - 1], "grid_n": gn, "origin": [float(v) for v in d["origin"]],
            "h": float(d["h"]), "cloud": cloud, "materials": materials_from_rows(d["mat_types"], d["mat_params"]),
            "lme": (float(d["lme"][0]), float(d["lme"][1]))}


def run(fn_name, timeout=600, **kw):
    """Runs one of the child-side functions below in a fresh Python process; arrays in, dict of arrays out."""
    so = lib_path()
    if so is None:
        raise RefChildError("oracle/_ref/libnlps_ref2d.so is absent and there is no reference tree to build it from")
    arrays = {k: np.asarray(v) for k, v in kw.items() if not isinstance(v, str)}
    words = {k: v for k, v in kw.items() if isinstance(v, str)}
    with tempfile.TemporaryDirectory(prefix="nlps_ref_") as tmp:
        fin, fout = os.path.join(tmp, "in.npz"), os.path.join(tmp, "out.npz")
        np.savez(fin, **arrays)
        env = dict(os.environ, OMP_NUM_THREADS="1")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), so, fn_name, fin, fout, json.dumps(words)],
                           capture_output=True, text=True, timeout=timeout, env=env)
        if r.returncode != 0 or not os.path.exists(fout):
            raise RefChildError(f"reference child '{fn_name}' ended with status {r.returncode}\n"
                                f"{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        with np.load(fout) as z:
            return {k: z[k] for k in z.files}


# ----------------------------------------------------------------------------------------------------------------
# child side
# ----------------------------------------------------------------------------------------------------------------
def _load(so):
    import ctypes as C
    L = C.CDLL(so)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.ref_beta_lme.restype = C.c_double
    L.ref_beta_lme.argtypes = [C.c_double, C.c_double]
    L.ref_set_lme.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int]
    L.ref_set_radial_returning.argtypes = [C.c_double, C.c_int]
    L.ref_field.restype = dp
    L.ref_field.argtypes = [C.c_char_p, ip]
    L.ref_ifield.restype = ip
    L.ref_ifield.argtypes = [C.c_char_p]
    L.ref_p_lme.argtypes = [C.c_int, dp, dp, C.c_double, dp]
    L.ref_dp_lme.argtypes = [C.c_int, dp, dp, dp]
    L.ref_mesh_fill.argtypes = [dp, ip, C.c_int, ip, ip, ip, ip, dp, C.c_double]
    L.ref_set_material.argtypes = [C.c_int, C.c_char_p, dp]
    L.ref_particle_stiffness.argtypes = [C.c_int, C.c_double, dp, dp, dp]
    L.ref_eigenerosion.argtypes = [C.c_double]
    L.ref_softening_hook.argtypes = [C.c_double]
    return L


def _D(a):
    import ctypes as C
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _I(a):
    import ctypes as C
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _child_matlib(L, a, words):
    """sym_eigen_analysis__TensorLib__, compute_inverse__TensorLib__, Inverse__TensorLib__, rcond__TensorLib__ on
    A[n, 2, 2]; `invert` (bool[n]) selects the matrices handed to the inverses and to rcond."""
    A = _f64(a["A"]).reshape(-1, 4)
    n = A.shape[0]
    w, V = np.zeros((n, 2)), np.zeros((n, 4))
    st = L.ref_sym_eigen(n, _D(A), _D(w), _D(V))
    out = {"w": w, "V": V.reshape(n, 2, 2), "eig_status": np.array(st)}
    sel = np.asarray(a["invert"], dtype=bool) if "invert" in a else np.ones(n, dtype=bool)
    B = _f64(A[sel])
    m = B.shape[0]
    i1, i2, rc = np.zeros((m, 4)), np.zeros((m, 4)), np.zeros(m)
    st = L.ref_inverse(m, _D(B), _D(i1), _D(i2))
    L.ref_rcond(m, _D(B), _D(rc))
    out.update(inv_lapack=i1.reshape(m, 2, 2), inv_tensor=i2.reshape(m, 2, 2), rcond=rc, inv_status=np.array(st))
    return out


def _child_lme_pointwise(L, a, words):
    """beta__LME__(gamma, h), p__LME__(l, lambda, Beta), dp__LME__(l, p) for lists l[np, STRIDE, 2] of nn[np] rows"""
    l, nn, lam, beta = _f64(a["l"]), _i32(a["nn"]), _f64(a["lam"]), _f64(a["beta"])
    n = nn.shape[0]
    p, dp = np.zeros(l.shape[:2]), np.zeros(l.shape)
    for q in range(n):
        k = int(nn[q])
        lq, pq, dq = _f64(l[q, :k]), np.zeros(k), np.zeros((k, 2))
        L.ref_p_lme(k, _D(lq), _D(_f64(lam[q])), float(beta[q]), _D(pq))
        L.ref_dp_lme(k, _D(lq), _D(pq), _D(dq))
        p[q, :k], dp[q, :k] = pq, dq
    b = np.array([L.ref_beta_lme(float(g), float(h)) for g, h in zip(_f64(a["gamma"]), _f64(a["h_avg"]))])
    return {"p": p, "dp": dp, "beta_of": b}


def _child_cloud(L, a, words):
    """One cloud through the reference, stage by stage (words["stages"], comma separated, in order):
      init     initialise_shapefun__MeshTools__ (-> initialize__LME__)
      search   x <- x_moved, dis <- dis_moved, then local_search__MeshTools__ (-> local_search__LME__)
      shape    compute_N__MeshTools__ / compute_dN__MeshTools__ of every particle
      compat   the four functions of compute-Strains.c + I3 with dU (and dV) per mesh node
      stress   Stress_integration__Constitutive__ of every particle
      density  stiffness_density__Constitutive__ for every pair of list nodes of the particles sd_p, the gradients
               pushed to n+1 by push_forward_dN__MeshTools__ (after compat and stress)
      beps     compute_Beps__Constitutive__(Initialize = beps_init)
      erosion  Eigenerosion__Constitutive__ of every particle (drivers: erosion on)
      softening compute_damage__Constitutive__ with Driver_EigenSoftening and the driver's in-place stress scaling
    Outputs are named <field>@<k> with k the index of the stage in the list."""
    import ctypes as C
    x = _f64(a["x"])
    n = x.shape[0]
    coords = _f64(a["coords"])
    nnodes = coords.shape[0]
    elem = _i32(a["elem"])
    types, rows = _i32(a["mat_types"]), _f64(a["mat_params"])
    stages = [s for s in words["stages"].split(",") if s]
    fracture = any(s in ("beps", "erosion", "softening") for s in stages)
    L.ref_set_lme(float(a["lme"][0]), float(a["lme"][1]), float(a["lme"][2]), int(a["lme"][3]))
    L.ref_set_radial_returning(float(a["rr"][0]), int(a["rr"][1]))
    L.ref_set_drivers(1 if fracture and "softening" not in stages else 0, 1 if "softening" in stages else 0)
    L.ref_cloud_new(n, nnodes, elem.shape[0], types.shape[0])
    L.ref_mesh_fill(_D(coords), _I(elem), elem.shape[1], _I(_i32(a["r1_ptr"])), _I(_i32(a["r1"])),
                    _I(_i32(a["r2_ptr"])), _I(_i32(a["r2"])), _D(_f64(a["h_avg"])), float(a["deltax"]))
    for i in range(types.shape[0]):
        L.ref_set_material(i, MAT_TYPE_NAMES[int(types[i])].encode(), _D(_f64(rows[i])))

    def fld(name):
        cols = C.c_int(0)
        ptr = L.ref_field(name.encode(), C.byref(cols))
        assert ptr, name
        v = np.ctypeslib.as_array(ptr, shape=(n, cols.value))
        return v[:, 0] if cols.value == 1 else v

    def ifld(name):
        return np.ctypeslib.as_array(L.ref_ifield(name.encode()), shape=(n,))

    fld("x_GC")[:] = x
    fld("dis")[:] = a["dis"] if "dis" in a else 0.0
    fld("Vol_0")[:] = a["vol0"]
    fld("mass")[:] = a["mass"]
    for src, dst in (("F_n", "F_n"), ("F_n", "F_n1"), ("b_e_n", "b_e_n"), ("b_e_n", "b_e_n1")):
        fld(dst)[:] = a[src]
    fld("DF")[:] = [1.0, 0.0, 0.0, 1.0, 1.0]
    for src, dst in (("J_n", "J_n"), ("J_n", "J_n1"), ("kappa_n", "Kappa_n"), ("kappa_n", "Kappa_n1"),
                     ("eps_n", "EPS_n"), ("eps_n", "EPS_n1")):
        fld(dst)[:] = a[src]
    if "dt_F_n" in a:
        fld("dt_F_n")[:] = a["dt_F_n"]
    if "back_stress" in a:
        fld("Back_stress")[:, :3] = a["back_stress"]
    for src, dst in (("damage_n", "Damage_n"), ("damage_n", "Damage_n1"), ("strain_f_n", "Strain_f_n"),
                     ("strain_f_n", "Strain_f_n1")):
        if src in a:
            fld(dst)[:] = a[src]
    ifld("MatIdx")[:] = a["matidx"]

    out = {}

    def lme_state(k):
        lst = np.full((n, STRIDE), -1, dtype=np.int32)
        act = np.zeros(nnodes, dtype=np.int32)
        worst = L.ref_get_lists(_I(lst), STRIDE, _I(act))
        assert worst <= STRIDE
        out.update({f"I0@{k}": ifld("I0").copy(), f"nn@{k}": ifld("NumberNodes").copy(), f"list@{k}": lst,
                    f"active@{k}": act, f"beta@{k}": fld("Beta").copy(), f"lambda@{k}": fld("lambda").copy()})

    for k, s in enumerate(stages):
        if s == "init":
            L.ref_initialise_shapefun()
            lme_state(k)
        elif s == "search":
            fld("x_GC")[:] = a["x_moved"]
            fld("dis")[:] = a["dis_moved"]
            out[f"search_status@{k}"] = np.array(L.ref_local_search())
            lme_state(k)
        elif s == "shape":
            N, dN = np.zeros((n, STRIDE)), np.zeros((n, STRIDE, 2))
            L.ref_shape_functions(_D(N), _D(dN), STRIDE)
            out.update({f"N@{k}": N, f"dN@{k}": dN})
        elif s == "compat":
            dU = _f64(a["dU"])
            dV = _f64(a["dV"]) if "dV" in a else None
            L.ref_compatibility(_D(dU), _D(dV) if dV is not None else None)
            for f in ("DF", "F_n1", "J_n1", "dt_DF", "dt_F_n1"):
                out[f"{f}@{k}"] = fld(f).copy()
        elif s == "stress":
            status, failed = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
            L.ref_stress_integration(_I(status), _I(failed))
            out.update({f"status@{k}": status, f"failed@{k}": failed})
            for f in ("Stress", "b_e_n1", "Kappa_n1", "EPS_n1", "C_ep", "W", "Back_stress"):
                out[f"{f}@{k}"] = fld(f).copy()
        elif s == "density":
            sp = _i32(a["sd_p"])
            nnp = ifld("NumberNodes")
            mx = int(nnp[sp].max())
            res, g0, g1 = np.zeros((sp.shape[0], mx, mx, 4)), np.zeros((sp.shape[0], mx, 2)), np.zeros((sp.shape[0], mx, 2))
            st = np.zeros(sp.shape[0], dtype=np.int32)
            for q, p in enumerate(sp):
                m = int(nnp[p])
                Kd, a0, a1 = np.zeros((m, m, 4)), np.zeros((m, 2)), np.zeros((m, 2))
                st[q] = L.ref_particle_stiffness(int(p), 0.0, _D(Kd), _D(a0), _D(a1))
                res[q, :m, :m], g0[q, :m], g1[q, :m] = Kd, a0, a1
            out.update({f"sd@{k}": res, f"sd_dN_n@{k}": g0, f"sd_dN_n1@{k}": g1, f"sd_status@{k}": st})
        elif s == "beps":
            bn, b = np.zeros(n, dtype=np.int32), np.full((n, BEPS_STRIDE), -1, dtype=np.int32)
            worst = L.ref_compute_beps(int(a["beps_init"]) if "beps_init" in a else 1, _I(bn), _I(b), BEPS_STRIDE)
            assert worst <= BEPS_STRIDE
            out.update({f"beps_n@{k}": bn, f"beps@{k}": b})
        elif s == "erosion":
            out[f"status@{k}"] = np.array(L.ref_eigenerosion(float(a["deltax"])))
            out[f"Damage_n1@{k}"] = fld("Damage_n1").copy()
        elif s == "softening":
            out[f"status@{k}"] = np.array(L.ref_softening_hook(float(a["deltax"])))
            out[f"Damage_n1@{k}"] = fld("Damage_n1").copy()
            out[f"Strain_f_n1@{k}"] = fld("Strain_f_n1").copy()
            out[f"Stress@{k}"] = fld("Stress").copy()
        else:
            raise ValueError("unknown stage " + s)
    return out


_CHILD = {"matlib": _child_matlib, "lme_pointwise": _child_lme_pointwise, "cloud": _child_cloud}

if __name__ == "__main__":
    so, fn, fin, fout, words = sys.argv[1:6]
    with np.load(fin) as z:
        arrays = {k: z[k] for k in z.files}
    res = _CHILD[fn](_load(so), arrays, json.loads(words))
    sys.stdout.flush()
    np.savez(fout, **res)
