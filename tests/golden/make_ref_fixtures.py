"""Generates the reference-produced fixtures under tests/golden/ (run where the reference tree is present only):

    python tests/golden/make_ref_fixtures.py

ref_etm2d.npz   the REFERENCE's own Python check of its elastoplastic tangent
    (tests/Constitutive/Elastoplastic-Tangent-Matrix.py in the reference tree) re-derives with numpy, for one hard-coded
    2 x 2 case, the material part of the spectral stiffness density the C driver next to it evaluates.  That file is run
    unmodified (numpy only); its inputs and its A_ep are taken from the module namespace and stored.

ref2d_lme.npz, ref2d_strain_stress.npz, ref2d_fracture.npz, ref2d_tangent.npz
    what the reference's own 2-D objects (oracle/_ref/libnlps_ref2d.so, oracle/orc.py::build_ref) compute for the
    clouds built below: the inputs (lattice parameters, particle arrays, materials as numbers, nodal increments, the
    moved positions) and the arrays the reference produced from them, every reference call in a child process
    (tests/ref.py).  Keys are "<case>/in/<name>" and "<case>/out/<name>".  Data only, nothing of the reference's text.
    tests/test_reference_parity.py regenerates every output from the stored inputs with the live library (a stale or
    hand-edited fixture fails there) and holds the oracle to the same numbers; tests/test_gpu_reference_parity.py holds
    the HIP kernels to them on a machine that has neither the reference nor the library.

The case builders are imported by tests/test_reference_parity.py, which runs more cases live than are stored.
"""
import contextlib
import io
import os
import runpy
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import ref  # noqa: E402
import util  # noqa: E402
from util import synth  # noqa: E402

REF_ETM = "/root/reference/nl-partsol/tests/Constitutive/Elastoplastic-Tangent-Matrix.py"

ORIGIN = (-1.3, 2.7)
# (h, shifted origin?, gamma_LME, TOL_zero_LME): the points of tests/test_gpu_param_sweep.py
SWEEP = [(0.1, True, 3.0, 1e-6), (0.37, False, 1.8, 1e-6), (2.5, True, 4.0, 1e-8), (1.0, False, 6.0, 1e-6),
         (0.37, True, 1.8, 1e-8), (0.1, False, 6.0, 1e-8), (2.5, False, 3.0, 1e-6)]
BASE = (1.0, False, 3.0, 1e-6)
# stored: the base cloud with the tie particles, and h in {0.1, 0.37, 2.5} x shifted origin x gamma in {1.8, 4, 6} at 1e-8
LME_STORED = {"base": (BASE, True), "h2.5": (SWEEP[2], False), "h0.37": (SWEEP[4], False), "h0.1": (SWEEP[5], False)}
SAMPLE_EVERY = 13  # N and dN are stored for every 13th particle (test_shape_functions_level_a samples every 7th)

TOL_RR_FRICTIONAL = (1e-10, 20)  # upstream's Matsuoka-Nakai reader (InOutFun/Material/Plasticity/Matsuoka-Nakai.c:82-83)
SOFT_NH = {"type": 0, "E": 2.0e4, "nu": 0.3}
SOFT_HENCKY = {"type": 1, "E": 1.0e4, "nu": 0.25}


def etm_fixture():
    with contextlib.redirect_stdout(io.StringIO()):
        ns = runpy.run_path(REF_ETM)
    np.savez(os.path.join(HERE, "ref_etm2d.npz"),
             dN_alpha=np.asarray(ns["dN_alpha"], dtype=np.float64), dN_beta=np.asarray(ns["dN_beta"], dtype=np.float64),
             tau=np.asarray(ns["tau"], dtype=np.float64), D_phi=np.asarray(ns["D_phi"], dtype=np.float64),
             b_e=np.asarray(ns["b_e"], dtype=np.float64), a_ep=np.asarray(ns["a_ep"], dtype=np.float64),
             u=np.asarray(ns["u"], dtype=np.float64), v=np.asarray(ns["v"], dtype=np.float64),
             A_ep=np.asarray(ns["A_ep"], dtype=np.float64))
    print("ref_etm2d.npz: A_ep =\n", ns["A_ep"])


# ---------------------------------------------------------------------------------------------------------------- LME
def add_particles(cloud, xs):
    """appends particles at xs to a synth.make_cloud dict (every other field repeats particle 0)"""
    k = xs.shape[0]
    for key, v in list(cloud.items()):
        if isinstance(v, np.ndarray) and v.shape[:1] == (cloud["x"].shape[0],) and key != "x":
            cloud[key] = np.concatenate([v, np.repeat(v[:1], k, axis=0)])
    cloud["x"] = np.concatenate([cloud["x"], xs])


def lme_inputs(cfg, ties=False, seed=11):
    """make_case(2, [12, 11], [3, 3], [5, 4]) with jitter at one sweep point, then a motion of up to 0.37 h per axis
    (without ties: through nodal increments dU_move, as the kinetics update moves particles).
    ties: particles on the centres and on the faces of the block's cells in addition, equidistant from 4 or 2 nodes
    (get_closest_node__MeshTools__ keeps the first minimum with a strict '<'); they move by whole cells, so they are
    ties again after the motion.  Ties are exact only where the lattice is (h = 1, origin 0)."""
    h, shifted, gamma, tol = cfg
    origin = list(ORIGIN) if shifted else [0.0, 0.0]
    case = util.make_case(2, [12, 11], [3, 3], [5, 4], h=h, origin=origin, gamma=gamma, tol_zero=tol)
    n_jit = case["cloud"]["x"].shape[0]
    if ties:
        ij = np.array([(i, j) for j in range(3, 7) for i in range(3, 8)], dtype=np.float64)
        xs = np.concatenate([ij + [0.5, 0.5], ij + [0.5, 0.0], ij + [0.0, 0.5]]) * h + np.asarray(origin)
        add_particles(case["cloud"], xs)
    d = {k: v for k, v in ref.cloud_inputs(case).items() if k in ("grid_n", "origin", "h", "lme", "x")}  # the rest: defaults
    n = d["x"].shape[0]
    if ties:
        rng = np.random.default_rng(seed)
        dx = 0.37 * h * rng.uniform(-1, 1, size=(n, 2))
        steps = np.array([[1.0, 0.0], [0.0, -1.0], [1.0, 1.0], [-1.0, 0.0]])
        dx[n_jit:] = h * steps[np.arange(n - n_jit) % 4]
        d["dis_moved"] = dx  # the moved positions are x + dis_moved, to the bit (the ties must stay ties)
    else:
        # nodal increments of up to 0.6 h per axis (the wide kernels of gamma = 1.8 average them down), varying over the block; the particles move by their interpolation
        # (moved_by_kinetics), which is how update_particles_kinetics_FLIP_PIC moves them
        def field(X):
            return 0.6 * np.stack([np.sin(1.3 * X[:, 0] + 0.4 * X[:, 1]), np.cos(0.9 * X[:, 1] - 0.7 * X[:, 0])], axis=1)
        dU = nodal_field(d, field)
        I = np.arange(dU.shape[0])
        ij = np.stack([I % d["grid_n"][0], I // d["grid_n"][0]], axis=1)
        dU[np.any((ij < 1) | (ij > np.array([10, 9])), axis=1)] = 0.0  # nodes no particle of the block [3,8)x[3,7) lists
        d["dU_move"] = dU
    return d


def moved_by_kinetics(d):
    """dis = sum_A N_A dU_A over each particle's list in list order, with the REFERENCE's N after its initialisation
    (__update_particles_kinetics_FLIP_PIC, U-Newmark-beta.c:1993-2072, is a static of the PETSc driver: this sum is
    ours).  The moved positions are x + dis."""
    o = ref.run_cloud("init,shape", d)
    dis = np.zeros_like(d["x"])
    for p in range(dis.shape[0]):
        for a in range(int(o["nn@0"][p])):
            dis[p] += o["N@1"][p, a] * d["dU_move"][o["list@0"][p, a]]
    return dis


def lme_outputs(d):
    """initialise_shapefun, shape functions, the motion, local_search, shape functions: what the reference leaves"""
    dis = d["dis_moved"] if "dis_moved" in d else moved_by_kinetics(d)
    o = ref.run_cloud("init,shape,search,shape", d, x_moved=d["x"] + dis, dis_moved=dis)
    o["dis_moved"] = dis
    assert int(o["search_status@2"]) == 0
    mx = int(max(o["nn@0"].max(), o["nn@2"].max()))
    smp = np.arange(0, d["x"].shape[0], SAMPLE_EVERY)
    out = {"sample": smp.astype(np.int32)}
    for tag, k, ks in (("0", 0, 1), ("1", 2, 3)):
        out.update({"I0_" + tag: o[f"I0@{k}"], "nn_" + tag: o[f"nn@{k}"], "list_" + tag: o[f"list@{k}"][:, :mx],
                    "active_" + tag: o[f"active@{k}"].astype(np.uint8), "beta_" + tag: o[f"beta@{k}"],
                    "lambda_" + tag: o[f"lambda@{k}"], "N_" + tag: o[f"N@{ks}"][smp, :mx],
                    "dN_" + tag: o[f"dN@{ks}"][smp, :mx]})
    return out, o


# ------------------------------------------------------------------------------------------------- strains and stress
def nodal_field(d, fn):
    """a field per MESH node from its coordinates X[nnodes, 2] (relative to the lattice centre, in units of h)"""
    gn, h = d["grid_n"], float(d["h"])
    I = np.arange(int(gn[0]) * int(gn[1]))
    X = np.stack([I % gn[0], I // gn[0]], axis=1).astype(np.float64)
    return fn(X - 0.5 * (np.asarray(gn, dtype=np.float64) - 1.0)) * h


def stress_inputs(kind, block=(7, 6), lo=(3, 3), seed=7, rates=True):
    """One law ("nh", "hencky", "dp", "vm", "mn", "ld") or the cloud of three laws the dispatch kernel holds ("mixed":
    Neo-Hookean, Hencky, Drucker-Prager interleaved 1:1:4) on make_case(2, [14, 12], lo, block), with the nodal
    increments dU, dV that drive the cloud through the law's branches (rates=False: no dV, no dt_F_n).  Nodes further
    than two cells from the block, which no particle can list (the lists come from the two-ring of a cell corner), carry zero increments."""
    rng = np.random.default_rng(seed)
    mats = {"nh": [util.NH], "hencky": [util.HENCKY], "dp": [util.DP], "vm": [util.VM],
            "mn": [synth.matsuoka_nakai_material(False)], "ld": [synth.matsuoka_nakai_material(True)],
            "mixed": [SOFT_NH, SOFT_HENCKY, util.DP]}[kind]
    case = util.make_case(2, [14, 12], list(lo), list(block), material=mats[-1])
    cl = case["cloud"]
    n = cl["x"].shape[0]
    case["materials"] = mats
    if kind == "mixed":
        cl["matidx"] = np.array([0, 1, 2, 2, 2, 2], dtype=np.int32)[np.arange(n) % 6]
    dt_F_n = 0.1 * rng.normal(size=(n, 5))
    dt_F_n[:, 4] = 0.0
    if rates:
        cl["dt_F_n"] = dt_F_n
    prm = util.orc().default_params()
    if kind in ("mn", "ld"):
        cl["b_e_n"] = synth.frictional_states(2, mats[0], n, seed=5)
        cl["kappa_n"][:] = mats[0]["kappa_0"]  # Generate-One-Phase-Analysis.c:620-626
        cl["eps_n"][:] = mats[0]["eps_0"]
        prm.tol_radial_returning, prm.max_iter_radial_returning = TOL_RR_FRICTIONAL
    if kind == "vm":
        back0 = rng.normal(size=(n, 3))
        cl["back_stress"] = back0 - back0.mean(axis=1, keepdims=True)
    d = ref.cloud_inputs(case, prm)
    nn = int(d["grid_n"][0]) * int(d["grid_n"][1])
    amp = {"nh": 1e-3, "hencky": 1e-3, "vm": 1.5e-2, "mn": 1.5e-4, "ld": 1.5e-4}.get(kind)
    if amp is not None:
        d["dU"] = amp * rng.normal(size=(nn, 2))
    else:
        # Drucker-Prager: a volumetric stretch that grows along x, from nothing (over the low third of the block) to +6 % (elastic range, classical return,
        # apex: tests/test_gpu_parity.py::test_drucker_prager_return_branches), with a strip of 2 % compression at the
        # low end, a shear on top so that the principal axes are not the coordinate axes, and noise
        cx = 0.5 * (2 * lo[0] + block[0]) - 0.5 * (float(d["grid_n"][0]) - 1.0)
        cy = 0.5 * (2 * lo[1] + block[1]) - 0.5 * (float(d["grid_n"][1]) - 1.0)

        def field(X):
            r = X - [cx, cy]
            w = np.clip(2.0 * (r[:, 0] / block[0] + 0.5) - 0.7, 0.0, 1.0) ** 2
            s = 0.06 * w - 0.02 * (r[:, 0] / block[0] < -0.4)
            return s[:, None] * r + (0.015 * w)[:, None] * np.stack([r[:, 1], 0.3 * r[:, 0]], axis=1)
        d["dU"] = nodal_field(d, field) + 2e-4 * rng.normal(size=(nn, 2))
    dV = 1e-2 * rng.normal(size=(nn, 2))
    I = np.arange(nn)
    ij = np.stack([I % d["grid_n"][0], I // d["grid_n"][0]], axis=1)
    far = np.any((ij < np.asarray(lo) - 2) | (ij > np.asarray(lo) + np.asarray(block) + 2), axis=1)
    d["dU"][far] = 0.0
    if rates:
        dV[far] = 0.0
        d["dV"] = dV
    return ref.strip_defaults(d)


def stress_outputs(d):
    o = ref.run_cloud("init,compat,stress", d)
    out = {"I0": o["I0@0"], "nn": o["nn@0"]}
    for f in ("DF", "F_n1", "J_n1") + (("dt_DF", "dt_F_n1") if "dV" in d else ()):
        out[f] = o[f + "@1"]
    for f in ("Stress", "b_e_n1", "Kappa_n1", "EPS_n1", "W"):
        out[f] = o[f + "@2"]
    out["status"] = o["status@2"] + 2 * o["failed@2"]  # the function's return, and Status_particle in bit 1
    out["C_ep"] = o["C_ep@2"][:, :4]
    out["Back_stress"] = o["Back_stress@2"][:, :3]
    return out, o


def dp_branches(out, d):
    """Branch of every Drucker-Prager particle FROM THE REFERENCE'S OUTPUTS (Drucker-Prager.c:409-592): 0 elastic (the
    plastic strain is untouched and the stress has a deviator), 2 apex (the returned stress is hydrostatic: the apex
    return drops the deviator, :571), 1 classical return (plastic strain grew, deviator kept); -1 other laws."""
    d = ref.fill_defaults(d)
    S = out["Stress"]
    p = (S[:, 0] + S[:, 3] + S[:, 4]) / 3.0
    dev = np.sqrt((S[:, 0] - p) ** 2 + (S[:, 3] - p) ** 2 + (S[:, 4] - p) ** 2 + 2 * S[:, 1] ** 2)
    hydro = dev <= 1e-9 * np.maximum(np.abs(p), 1e-300)
    br = np.where(hydro, 2, np.where(out["EPS_n1"] != d["eps_n"], 1, 0))
    return np.where(d["mat_types"][d["matidx"]] == 2, br, -1)


# ------------------------------------------------------------------------------------------- tangent (per-pair density)
def density_particles(d, out):
    """the particles whose per-pair stiffness densities are compared: every 9th, and for Drucker-Prager the first three
    of every branch"""
    pick = set(range(0, d["x"].shape[0], 9))
    br = dp_branches(out, d)
    for b in range(3):
        pick.update(np.where(br == b)[0][:3].tolist())
    return np.array(sorted(pick), dtype=np.int32)


def density_outputs(d, sd_p):
    o = ref.run_cloud("init,compat,stress,density", d, sd_p=sd_p)
    assert not o["sd_status@3"].any()
    return {"sd": o["sd@3"], "dN_n": o["sd_dN_n@3"], "dN_n1": o["sd_dN_n1@3"]}, o


def tangent_inputs():
    """the 80-particle cloud (block 5 x 4) of Neo-Hookean, Hencky and Drucker-Prager particles, all three branches"""
    return stress_inputs("mixed", block=(5, 4), rates=False)


def tangent_outputs(d):
    """Dense K in masked numbering (the running index of the active nodes) from the REFERENCE's per-pair stiffness
    densities times the particle's reference volume, summed over particles, then list nodes A, then B, like
    __jacobian_evaluation (U-Newmark-beta.c:1646-1830) with alpha_1 = 0 and no Dirichlet rows.  That assembly loop
    lives in the PETSc driver: this one is ours, only the densities are the reference's."""
    n = d["x"].shape[0]
    o = ref.run_cloud("init,compat,stress,density", d, sd_p=np.arange(n, dtype=np.int32))
    assert not o["sd_status@3"].any() and not o["status@2"].any()
    vol0 = ref.fill_defaults(d)["vol0"]
    act = o["active@0"] != 0
    n2m = np.where(act, np.cumsum(act) - 1, -1)
    na = int(act.sum())
    K = np.zeros((2 * na, 2 * na))
    for p in range(n):
        k = int(o["nn@0"][p])
        rows = n2m[o["list@0"][p, :k]]
        Kd = o["sd@3"][p, :k, :k].reshape(k, k, 2, 2) * vol0[p]
        for A in range(k):
            for B in range(k):
                K[2 * rows[A]:2 * rows[A] + 2, 2 * rows[B]:2 * rows[B] + 2] += Kd[A, B]
    return {"I0": o["I0@0"], "active": act.astype(np.uint8), "K": K}, o


# ----------------------------------------------------------------------------------------------------------- fracture
def erosion_inputs(seed=21):
    """The 2-D cloud of tests/test_gpu_eigenerosion.py: a Neo-Hookean block stretched so that the principal stresses are
    positive, with Gf at the median of the particles' energy release rates G as the REFERENCE's W, J and lists give
    them (a first pass with Gf = 0), so that about half of the cloud fails."""
    rng = np.random.default_rng(seed)
    mat = {"type": 0, "E": 1.0e6, "nu": 0.25, "Ceps": 1.5, "Gf": 0.0}
    case = util.make_case(2, [14, 12], [3, 3], [7, 6], material=mat)
    d = ref.cloud_inputs(case)
    nn = int(d["grid_n"][0]) * int(d["grid_n"][1])
    amp = 1.0 + 0.5 * rng.uniform(size=(nn, 1))
    d["dU"] = nodal_field(d, lambda X: 0.02 * X) * amp
    o = ref.run_cloud("init,beps,compat,stress", d)
    d = ref.fill_defaults(d)
    V, W, bn, b = d["vol0"] * o["J_n1@2"], o["W@3"], o["beps_n@1"], o["beps@1"]
    G = np.array([mat["Ceps"] * float(d["h"]) / (V[p] + V[b[p, :bn[p]]].sum()) *
                  (V[p] * W[p] + (V[b[p, :bn[p]]] * W[b[p, :bn[p]]]).sum()) for p in range(V.shape[0])])
    Gf = float(np.median(G))
    assert np.count_nonzero(np.abs(G - Gf) < 1e-9 * Gf) == 0, "no particle may sit on the threshold"
    d["mat_params"][0, 4] = Gf
    return ref.strip_defaults(d)


def erosion_outputs(d):
    o = ref.run_cloud("init,beps,compat,stress,erosion", d)
    assert int(o["status@4"]) == 0
    mx = int(o["beps_n@1"].max())
    return {"I0": o["I0@0"], "beps_n": o["beps_n@1"], "beps": o["beps@1"][:, :mx], "J_n1": o["J_n1@2"],
            "Stress": o["Stress@3"], "W": o["W@3"], "Damage_n1": o["Damage_n1@4"]}, o


def softening_inputs(seed=33):
    """The 2-D cloud of tests/test_gpu_eigensoftening.py: half of the particles have moved before (compute_Beps with
    Initialize_Beps = false rebuilds their lists, the others keep an empty one), a tenth starts failed, a tenth partly
    damaged, some with a fracture strain on record; ft at the median of the smallest principal Kirchhoff stress of the
    undamaged candidates as the REFERENCE computes the stresses (a first pass), so that about half of them start to
    fracture, and with no particle on the threshold."""
    rng = np.random.default_rng(seed)
    mat = {"type": 0, "E": 1.0e6, "nu": 0.25, "Ceps": 1.5, "ft": 0.0, "heps": 2.0, "wcrit": 0.05}
    case = util.make_case(2, [14, 12], [3, 3], [7, 6], material=mat)
    n = case["cloud"]["x"].shape[0]
    dis = np.zeros((n, 2))
    dis[rng.uniform(size=n) < 0.5] = 1e-3
    case["cloud"]["dis"] = dis
    d = ref.cloud_inputs(case)
    pick = rng.permutation(n)
    d["damage_n"], d["strain_f_n"] = np.zeros(n), np.zeros(n)
    d["damage_n"][pick[:n // 10]] = 1.0
    d["damage_n"][pick[n // 10: n // 5]] = 0.3
    d["strain_f_n"][pick[n // 10: n // 4]] = 1e-3
    nn = int(d["grid_n"][0]) * int(d["grid_n"][1])
    d["dU"] = nodal_field(d, lambda X: 0.02 * X) * (1.0 + 0.5 * rng.uniform(size=(nn, 1)))
    o = ref.run_cloud("init,compat,stress", d)
    tau = o["Stress@2"][:, :4].reshape(n, 2, 2)
    T0 = np.linalg.eigvalsh(0.5 * (tau + np.transpose(tau, (0, 2, 1))))[:, 0]
    cand = (d["damage_n"] == 0.0) & (T0 > 0.0)
    assert cand.sum() > n // 4
    # ft halfway between the two middle candidates: a particle without neighbours compares its own T0 with ft, so the
    # median itself would put one particle on the threshold.  No particle may sit within 1e-9 of it: the reference gives
    # the same set of starters with ft a little lower and a little higher
    srt = np.sort(T0[cand])
    ft = float(0.5 * (srt[srt.size // 2 - 1] + srt[srt.size // 2]))
    started = []
    for f in (ft * (1 - 1e-9), ft * (1 + 1e-9), ft):
        d["mat_params"][0, 5] = f
        started.append(softening_outputs(d)[0]["Strain_f_n1"] > 0)
    assert np.array_equal(started[0], started[1]) and np.array_equal(started[0], started[2]), "a particle sits on the threshold"
    return ref.strip_defaults(d)


def softening_outputs(d):
    o = ref.run_cloud("init,beps,compat,stress,softening", d, beps_init=np.array(0))
    assert int(o["status@4"]) == 0
    mx = max(1, int(o["beps_n@1"].max()))
    return {"I0": o["I0@0"], "beps_n": o["beps_n@1"], "beps": o["beps@1"][:, :mx], "J_n1": o["J_n1@2"],
            "Stress": o["Stress@4"], "Damage_n1": o["Damage_n1@4"], "Strain_f_n1": o["Strain_f_n1@4"]}, o


# ------------------------------------------------------------------------------------------------------------- output
def pack(cases):
    flat = {}
    for name, (d, out) in cases.items():
        flat.update({f"{name}/in/{k}": v for k, v in d.items()})
        flat.update({f"{name}/out/{k}": v for k, v in out.items()})
    return flat


def unpack(path):
    cases = {}
    with np.load(path) as z:
        for key in z.files:
            name, io_, k = key.split("/")
            cases.setdefault(name, ({}, {}))[0 if io_ == "in" else 1][k] = z[key]
    return cases


def write(name, cases):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **pack(cases))
    print("%s: %d bytes, cases %s" % (name, os.path.getsize(path), ", ".join(cases)))


def build_lme():
    cases = {}
    for name, (cfg, ties) in LME_STORED.items():
        d = lme_inputs(cfg, ties)
        cases[name] = (d, lme_outputs(d)[0])
    return cases


STRESS_STORED = {"mixed": dict(block=(6, 6)), "vm": dict(block=(3, 3), rates=False), "mn": dict(block=(3, 3), rates=False),
                 "ld": dict(block=(3, 3), rates=False)}


def build_strain_stress():
    cases = {}
    for kind, kw in STRESS_STORED.items():
        d = stress_inputs(kind, **kw)
        out = stress_outputs(d)[0]
        if kind == "mixed":
            print("mixed cloud, Drucker-Prager branches (elastic, classical, apex):",
                  [int((dp_branches(out, d) == b).sum()) for b in range(3)])
        cases[kind] = (d, out)
    return cases


def build_fracture():
    d = erosion_inputs()
    out = erosion_outputs(d)[0]
    print("eigenerosion: %d of %d particles fail" % (int(out["Damage_n1"].sum()), out["Damage_n1"].shape[0]))
    ds = softening_inputs()
    outs = softening_outputs(ds)[0]
    print("eigensoftening: %d particles start to fracture, damage grows on %d" % (
        int(((outs["Strain_f_n1"] > 0) & (ds["strain_f_n"] == 0)).sum()), int((outs["Damage_n1"] > ds["damage_n"]).sum())))
    return {"erosion": (d, out), "softening": (ds, outs)}


def build_tangent():
    d = tangent_inputs()
    out = tangent_outputs(d)[0]
    print("tangent: K %s, %d particles" % (out["K"].shape, d["x"].shape[0]))
    return {"mixed80": (d, out)}


BUILDERS = {"ref2d_lme.npz": build_lme, "ref2d_strain_stress.npz": build_strain_stress,
            "ref2d_fracture.npz": build_fracture, "ref2d_tangent.npz": build_tangent}
OUTPUTS = {"ref2d_tangent.npz": tangent_outputs, "ref2d_lme.npz": lme_outputs, "ref2d_strain_stress.npz": stress_outputs, "ref2d_fracture.npz": lambda d: softening_outputs(d) if "strain_f_n" in d else erosion_outputs(d)}


def main():
    etm_fixture()
    for name, fn in BUILDERS.items():
        write(name, fn())


if __name__ == "__main__":
    main()
