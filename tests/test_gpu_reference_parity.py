"""The HIP kernels against numbers the REFERENCE ITSELF produced, with no oracle in between (2-D).

tests/golden/ref2d_*.npz hold clouds and what the reference's own objects computed for them
(tests/golden/make_ref_fixtures.py; tests/test_reference_parity.py keeps them equal to the live reference where that
exists).  This module reads those files only: neither the reference tree nor the library built from it is needed here.
Every launch goes through the existing Solver calls.  Tolerances are those of tests/test_reference_parity.py: integers
exact, N 1e-11, grad N 1e-9, lambda 1e-9 of max|lambda|, Beta equal, 1e-10 for DF, F_n1, J, stresses and internal
variables (1e-8 for Matsuoka-Nakai and Lade-Duncan, as in test_gpu_frictional.py)."""
import os

import numpy as np
import pytest

import ref
from util import assert_close, gpu_setup, nlps, relerr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL_STAGE = 1e-10
TOL_FRICTIONAL = 1e-8


def load(name):
    cases = {}
    with np.load(os.path.join(GOLDEN, name)) as z:
        for key in z.files:
            case, io_, k = key.split("/")
            cases.setdefault(case, ({}, {}))[0 if io_ == "in" else 1][k] = z[key]
    return {c: (ref.fill_defaults(d), out) for c, (d, out) in cases.items()}


LME = load("ref2d_lme.npz")
STRESS = load("ref2d_strain_stress.npz")
FRACTURE = load("ref2d_fracture.npz")
TANGENT = load("ref2d_tangent.npz")


def compare_lme(S, out, tag, what):
    st = S.download_state()
    assert np.array_equal(st["I0"], out["I0_" + tag]), f"{what}: I0"
    nn, lst = S.download_lists()
    assert np.array_equal(nn, out["nn_" + tag]), f"{what}: NumberNodes"
    ref_list = out["list_" + tag]
    valid = np.arange(ref_list.shape[1])[None, :] < nn[:, None]
    assert np.array_equal(np.where(valid, lst[:, : ref_list.shape[1]], -1), np.where(valid, ref_list, -1)), \
        f"{what}: ListNodes (order included)"
    assert np.array_equal(S.download_active() != 0, out["active_" + tag] != 0), f"{what}: ActiveNode"
    assert np.array_equal(st["beta"], out["beta_" + tag]), f"{what}: Beta"
    assert_close(st["lambda"], out["lambda_" + tag], 1e-9, f"{what}: lambda")
    N, dN = S.shape_functions()
    wn = wd = 0.0
    for row, p in enumerate(out["sample"]):
        k = int(nn[p])
        wn = max(wn, float(np.abs(N[p, :k] - out["N_" + tag][row, :k]).max()))
        wd = max(wd, float(np.abs(dN[p, :k] - out["dN_" + tag][row, :k]).max() / np.abs(out["dN_" + tag][row, :k]).max()))
        assert not N[p, k:].any() and not dN[p, k:].any()
    print("%s: lambda %.1e, N %.1e, dN %.1e" % (what, relerr(st["lambda"], out["lambda_" + tag]), wn, wd))
    assert wn < 1e-11, f"{what}: N differs by {wn:.2e}"
    assert wd < 1e-9, f"{what}: dN differs by {wd:.2e} of its magnitude"


@pytest.mark.parametrize("name", sorted(LME))
def test_initialise_shapefun_against_the_reference(name):
    """initialise_shapefun(): I0, NumberNodes, ListNodes with order, ActiveNode, Beta, lambda, N and grad N as
    initialize__LME__ / compute_N / compute_dN of the reference left them ('base' includes particles on cell centres and
    cell faces, the ties of get_closest_node)."""
    d, out = LME[name]
    S = gpu_setup(ref.case_from_inputs(d))
    compare_lme(S, out, "0", name + " after initialise_shapefun")
    S.close()


def masked(S, d, key):
    """the fixture's increments per mesh node in the Solver's masked numbering"""
    n = nlps()
    n2m, _ = S.active_masks(n.BccSet([]), 0)
    act = n2m >= 0
    v = np.zeros((S.nactive, 2))
    v[n2m[act]] = d[key][act]
    return v.ravel()


@pytest.mark.parametrize("name", sorted(LME))
def test_local_search_against_the_reference(name):
    """local_search() after the fixture's motion: the same index maps and shape functions as local_search__LME__.
    The jittered clouds move through update_particles_kinetics_FLIP_PIC with the fixture's nodal increments (the
    reference side interpolated the same increments with its own N).  'base' holds particles exactly on cell faces and
    centres, which must stay ties to the bit: there the moved positions and the reference's I0, lambda and Beta after
    its initialisation are uploaded instead, since an interpolated increment differs in the last place."""
    d, out = LME[name]
    case = ref.case_from_inputs(d)
    if "dU_move" in d:
        S = gpu_setup(case)
        dU = masked(S, d, "dU_move")
        zero = np.zeros_like(dU)
        S.update_particles_kinetics_FLIP_PIC(1.0, dU, zero, zero, zero)
    else:
        cloud = dict(case["cloud"])
        cloud.update(x=d["x"] + d["dis_moved"], dis=d["dis_moved"].copy(), I0=out["I0_0"].copy(),
                     beta=out["beta_0"].copy(), **{"lambda": out["lambda_0"].copy()})
        case["cloud"] = cloud
        S = gpu_setup(case, init=False)
    S.local_search()
    assert np.count_nonzero(out["I0_0"] != out["I0_1"]) >= 10
    compare_lme(S, out, "1", name + " after local_search")
    S.close()


STRESS_RUNS = [("mixed", None), ("mixed", 1), ("mixed", 2), ("vm", None), ("mn", None), ("ld", None)]


@pytest.mark.parametrize("name,mode", STRESS_RUNS, ids=["%s-mode%s" % r for r in STRESS_RUNS])
def test_strains_and_stress_against_the_reference(name, mode):
    """local_compatibility_conditions(dU, dV) and constitutive_update() against compute-Strains.c and
    Stress_integration__Constitutive__ of the reference: the cloud of Neo-Hookean, Hencky and Drucker-Prager particles
    (all three return branches; in the default and in both law launch modes), Von-Mises with a back stress,
    Matsuoka-Nakai and Lade-Duncan."""
    n = nlps()
    d, out = STRESS[name]
    case = ref.case_from_inputs(d)
    params = n.default_params()
    params.gamma_lme, params.tol_zero_lme = case["lme"]
    params.tol_radial_returning, params.max_iter_radial_returning = float(d["rr"][0]), int(d["rr"][1])
    S = gpu_setup(case, params=params)
    if mode is not None:
        S.set_law_launch_mode(mode)
    assert np.array_equal(S.download_state(["I0"])["I0"], out["I0"])
    dU = masked(S, d, "dU")
    dV = masked(S, d, "dV") if "dV" in d else None
    S.local_compatibility_conditions(dU, dV)
    S.constitutive_update()
    assert S.status_flags() == 0 and not out["status"].any()
    st = S.download_state()
    worst = {}
    for k in ("DF", "F_n1", "J_n1") + (("dt_DF", "dt_F_n1") if dV is not None else ()):
        assert_close(st[k], out[k], TOL_STAGE, f"{name}: {k}")
        worst[k] = relerr(st[k], out[k])
    tol = TOL_FRICTIONAL if name in ("mn", "ld") else TOL_STAGE
    E = max(m["E"] for m in case["materials"])
    for k in ("Stress", "b_e_n1", "Kappa_n1", "EPS_n1", "W", "C_ep", "Back_stress"):
        scale = {"W": E * 1e-4, "C_ep": E}.get(k)
        assert_close(st[k], out[k], tol, f"{name}: {k}", scale=scale)
        worst[k] = relerr(st[k], out[k], scale)
    print("%s mode %s: " % (name, mode) + ", ".join("%s %.1e" % kv for kv in worst.items()))
    S.close()


def test_eigenerosion_against_the_reference():
    """The eigenerosion hook of the force stage against Eigenerosion__Constitutive__ over the reference's own
    compute_Beps lists: the damage field is exact, the Kirchhoff stress is the reference's scaled by (1 - damage)."""
    n = nlps()
    d, out = FRACTURE["erosion"]
    case = ref.case_from_inputs(d)
    params = n.default_params()
    params.driver_eigenerosion = 1
    S = gpu_setup(case, nsteps=2, params=params)
    assert np.array_equal(S.download_state(["I0"])["I0"], out["I0"])
    dU = masked(S, d, "dU")
    S.local_compatibility_conditions(dU)
    S.constitutive_update()
    S.nodal_internal_forces(np.zeros(S.nactive * 2))
    st = S.download_state()
    assert np.array_equal(st["Damage_n1"], out["Damage_n1"]), "damage field"
    assert 0 < out["Damage_n1"].sum() < S.np
    assert_close(st["J_n1"], out["J_n1"], TOL_STAGE, "J_n1")
    assert_close(st["W"], out["W"], TOL_STAGE, "W", scale=case["materials"][0]["E"] * 1e-4)
    assert_close(st["Stress"], out["Stress"] * (1.0 - out["Damage_n1"])[:, None], TOL_STAGE, "scaled Kirchhoff stress")
    print("eigenerosion: %d of %d particles fail; stress %.1e" % (
        int(out["Damage_n1"].sum()), S.np, relerr(st["Stress"], out["Stress"] * (1.0 - out["Damage_n1"])[:, None])))
    S.close()


def test_eigensoftening_against_the_reference():
    """The eigensoftening hook of the force stage against compute_damage__Constitutive__ /
    Eigensoftening__Constitutive__ over the reference's own compute_Beps lists (Initialize_Beps = false: a particle that
    has not moved has none), with the driver's in-place stress scaling: which particles start to fracture is exact;
    fracture strain, damage and scaled Kirchhoff stress at 1e-10."""
    n = nlps()
    d, out = FRACTURE["softening"]
    case = ref.case_from_inputs(d)
    params = n.default_params()
    params.driver_eigensoftening = 1
    S = gpu_setup(case, nsteps=2, params=params)
    assert np.array_equal(S.download_state(["I0"])["I0"], out["I0"])
    dU = masked(S, d, "dU")
    S.local_compatibility_conditions(dU)
    S.constitutive_update()
    S.nodal_internal_forces(np.zeros(S.nactive * 2))
    st = S.download_state()
    started = (out["Strain_f_n1"] > 0) & (d["strain_f_n"] == 0)
    assert started.sum() >= 10 and (out["Damage_n1"] > d["damage_n"]).sum() >= 10
    assert np.array_equal(st["Strain_f_n1"] > 0, out["Strain_f_n1"] > 0), "which particles start to fracture"
    assert_close(st["Strain_f_n1"], out["Strain_f_n1"], TOL_STAGE, "fracture strain")
    assert_close(st["Damage_n1"], out["Damage_n1"], TOL_STAGE, "damage field")
    assert_close(st["Stress"], out["Stress"], TOL_STAGE, "scaled Kirchhoff stress")
    print("eigensoftening: fracture strain %.1e, damage %.1e, stress %.1e" % (
        relerr(st["Strain_f_n1"], out["Strain_f_n1"]), relerr(st["Damage_n1"], out["Damage_n1"]),
        relerr(st["Stress"], out["Stress"])))
    S.close()


def test_assembled_tangent_against_the_reference():
    """jacobian_evaluation(0.0, None, False) on the 80-particle Neo-Hookean / Hencky / Drucker-Prager cloud against the
    dense K stored in ref2d_tangent.npz.  That K was assembled in numpy (tests/golden/make_ref_fixtures.py::
    tangent_outputs) from the reference's per-pair stiffness densities times volume in the order of
    U-Newmark-beta.c:1646-1830: the assembly loop is ours, since the reference's lives inside the PETSc driver; the
    densities are the reference's own.  Bound: the 1e-8 of the spectral tangent (test_gpu_tangent_operator.py)."""
    n = nlps()
    d, out = TANGENT["mixed80"]
    case = ref.case_from_inputs(d)
    params = n.default_params()
    params.tol_radial_returning, params.max_iter_radial_returning = float(d["rr"][0]), int(d["rr"][1])
    S = gpu_setup(case, params=params)
    assert S.np == 80 and np.array_equal(S.download_state(["I0"])["I0"], out["I0"])
    dU = masked(S, d, "dU")
    assert np.array_equal(S.download_active() != 0, out["active"] != 0)
    S.local_compatibility_conditions(dU)
    S.constitutive_update()
    rows, cols, vals = S.jacobian_evaluation(0.0, None, False)
    K = np.zeros_like(out["K"])
    np.add.at(K, (rows, cols), vals)
    print("assembled tangent: %.1e of max|K|, %d dofs" % (relerr(K, out["K"]), K.shape[0]))
    assert_close(K, out["K"], 1e-8, "assembled tangent")
    S.close()
