"""The checker of the explicit step with F-bar (tests/explicit_fbar_ref.py) on the CPU: what tests/test_gpu_explicit_fbar.py
rests on, established on the checker alone, each with its margin printed.

(a) with every alpha < 0 the insertion swaps nothing: the checker is orc.ExplicitStepper to 1e-12;
(b) alpha = 0: det(c DF) is J_patch for every particle and sum_patch Vol_0 J_n det(c DF) = Vn1, to 1e-13;
(c) a homogeneous step (affine dU on a uniformly pre-stretched cloud): F-bar on equals off to 1e-12;
(d) the GPU cases: the barred stress differs from the plain step's by more than 1e-3, no particle lies within 1e-9 h of a
    cell face, every J stays positive;
(e) four steps straight equal two steps, a restart from (state, Fbar_n, Jbar_n), two more, to 1e-12."""
import numpy as np
import pytest

import explicit_fbar_ref as xb
import explicit_fluid_ref as xf
from util import assert_close, oracle_setup, orc, relerr

# (ndim, materials, alpha, block, layout) of every reference the GPU tests compare against
GPU_CASES = [(nd, (0,), (a,), b, None) for nd in (2, 3) for a in (0.0, 0.5, 1.0) for b in (1, 3)] + \
            [(nd, (1,), (0.0,), 1, None) for nd in (2, 3)] + \
            [(3, (1, 2), (0.0, -1.0), 1, "interleaved"), (3, (1, 2), (0.0, -1.0), 1, "tiles"),
             (3, (0, 3), (0.5, -1.0), 3, "interleaved"), (3, (0, 4), (0.5, -1.0), 3, "interleaved")]


@pytest.mark.parametrize("ndim", [2, 3])
def test_with_nothing_swapped_the_checker_is_the_oracle_step(ndim):
    """(a)"""
    o = orc()
    nsteps = 3
    case = xb.fbar_case(ndim)
    bcs, g = xb.dirichlet(case, nsteps), xb.gravity(ndim)
    M, P, prm, mats = oracle_setup(case)
    stepper = o.ExplicitStepper(P, M, mats, prm, o.BccSet(bcs), nsteps, gravity=g)
    R = xb.FbarStepRef(case, [-1.0], 3, bcs, (), nsteps, g)
    worst = 0.0
    for t in range(nsteps):
        assert stepper.step(t, xb.DT) == 0
        R.step(t, xb.DT)
        assert stepper.out.nactive == R.na
        for k in ("mass", "dU", "force", "accel", "reaction"):
            worst = max(worst, relerr(R.nodal[k], stepper.nodal(k)))
            assert_close(R.nodal[k], stepper.nodal(k), 1e-12, f"step {t} nodal {k}")
        for k in xf.FluidStepRef.FIELDS + ("F_n1", "J_n1", "DF"):
            worst = max(worst, relerr(R.P[k], P[k]))
            assert_close(R.P[k], P[k], 1e-12, f"step {t} {k}")
        # W at the project's 1e-12 unless the two F_n1 already differ by more than its conditioning lets through: W is
        # quadratic in the strain e = max |F - I| where the stress is linear, so a relative difference d_F of F moves W by
        # up to 2 d_F / e of max |W| (2000 d_F at e = 1e-3).  Both are measured here and printed.
        nd2 = ndim * ndim
        d_F = max(relerr(R.P["F_n1"][:, :nd2], P["F_n1"][:, :nd2]), relerr(R.P["J_n1"], P["J_n1"]))
        strain = float(np.abs(P["F_n1"][:, :nd2] - np.eye(ndim).ravel()).max())
        bound = max(1e-12, 2.0 * d_F / strain)
        print(f"(a) {ndim}-D step {t}: W {relerr(R.P['W'], P['W']):.2e} of max |W| (bound {bound:.1e}: project 1e-12, F agrees to "
              f"{d_F:.1e}, strain {strain:.1e})")
        assert_close(R.P["W"], P["W"], bound, f"step {t} W")
        assert relerr(R.Fbar_n, R.P["F_n"]) > 1e-6, "the barred values are formed all the same"
    print(f"(a) {ndim}-D: largest relative difference against orc.ExplicitStepper {worst:.2e} (bound 1e-12)")


@pytest.mark.parametrize("ndim,block", [(2, 1), (2, 3), (3, 1), (3, 3)])
def test_alpha_zero_gives_every_particle_the_volume_ratio_of_its_patch(ndim, block):
    """(b)"""
    snaps = xb.reference(ndim, (0,), (0.0,), block)
    worst_det = worst_sum = 0.0
    for s in snaps:
        L = s["last"]
        cDF = L["c"][:, None] * L["DF"][:, : ndim * ndim]
        d = xf.det_block(cDF, ndim)
        worst_det = max(worst_det, float(np.abs(d / L["Jp"] - 1.0).max()))
        total = np.bincount(L["pid"], weights=L["vol0"] * L["J_n"] * d, minlength=L["Vn1"].size)
        used = L["Vn"] > 0.0
        assert used.sum() > 1, "more than one patch"
        worst_sum = max(worst_sum, float(np.abs(total[used] / L["Vn1"][used] - 1.0).max()))
    print(f"(b) {ndim}-D block {block}: det(c DF) / J_patch - 1 {worst_det:.2e}, patch volume {worst_sum:.2e} (bound 1e-13)")
    assert worst_det <= 1e-13 and worst_sum <= 1e-13


@pytest.mark.parametrize("ndim", [2, 3])
def test_a_homogeneous_step_is_left_alone(ndim):
    """(c) every particle pre-stretched by the same F, an affine dU: DF, J_n and J_n1 are uniform, so J_patch = det DF,
    c = 1 and Fbar_n1 = F_n1 whatever alpha"""
    o = orc()
    rng = np.random.default_rng(11)
    F0 = np.eye(ndim) + 0.05 * rng.normal(size=(ndim, ndim))
    A = 1e-3 * rng.normal(size=(ndim, ndim))
    stress, real = {}, {}
    for alpha in (None, 0.0, 0.5):
        case = xb.fbar_case(ndim)
        cloud = case["cloud"]
        n = cloud["x"].shape[0]
        T = cloud["F_n"].shape[1]
        Fn = np.zeros((n, T))
        Fn[:, : ndim * ndim] = F0.ravel()
        if ndim == 2:
            Fn[:, 4] = 1.0
        cloud["F_n"] = Fn
        cloud["J_n"] = np.full(n, np.linalg.det(F0))
        R = xb.FbarStepRef(case, [-1.0 if alpha is None else alpha], 3)
        P = R.P
        assert o.local_search(P, R.M, R.prm) == 0
        n2m, na = o.active_nodes(R.M)
        node_x = np.array([[case["origin"][k] + case["h"] * ((A_ // int(np.prod(case["grid_n"][:k]))) % case["grid_n"][k])
                            for k in range(ndim)] for A_ in np.nonzero(n2m >= 0)[0]])
        dU = np.zeros((na, ndim))
        dU[n2m[np.nonzero(n2m >= 0)[0]]] = node_x @ A.T
        P["dt_F_n"][:] = 0.0
        assert o.compatibility(dU.ravel(), dU.ravel() / xb.DT, P, R.M, n2m) == 0
        DFx = np.tile((np.eye(ndim) + A).ravel(), (n, 1))
        spread = relerr(P["DF"][:, : ndim * ndim], DFx)
        assert spread < 1e-12, "LME reproduces affine fields"
        # First the step as the oracle's compatibility leaves it.  Its DF is uniform only as far as the Newton tolerance of the
        # LME multipliers lets it be (`spread`, measured 1e-13), and a patch ratio that differs from det DF by d * spread
        # moves the volumetric stress by lambda d spread: the bound of this part is the issue's 1e-12 or that, whichever is
        # larger, with everything in it measured here.
        R.F.stress()
        real[alpha] = (P["stress"].copy(), spread)
        # Then the premise itself, a HOMOGENEOUS step, made exactly: DF = I + A, F_n1 = DF F_0, J_n1.
        P["DF"][:, : ndim * ndim] = DFx
        P["F_n1"][:, : ndim * ndim] = ((np.eye(ndim) + A) @ F0).ravel()
        P["J_n1"][:] = np.linalg.det((np.eye(ndim) + A) @ F0)
        R.F.stress()
        stress[alpha] = P["stress"].copy()
        if alpha is not None:
            assert np.abs(R.last["c"] - 1.0).max() < 1e-13
    for alpha in (0.0, 0.5):
        e = relerr(stress[alpha], stress[None])
        print(f"(c) {ndim}-D alpha {alpha}: F-bar on against off {e:.2e} (bound 1e-12)")
        assert e <= 1e-12
        lam = xb.NH49["E"] * xb.NH49["nu"] / ((1.0 + xb.NH49["nu"]) * (1.0 - 2.0 * xb.NH49["nu"]))
        spread = max(real[alpha][1], real[None][1])
        bound = max(1e-12, lam * ndim * spread / np.abs(real[None][0]).max())
        e = relerr(real[alpha][0], real[None][0])
        print(f"(c) {ndim}-D alpha {alpha}, the step as the oracle makes it: F-bar on against off {e:.2e} (bound {bound:.1e}: "
              f"DF uniform to {spread:.1e})")
        assert e <= bound
    assert np.abs(stress[None]).max() > 0.0


@pytest.mark.parametrize("ndim,materials,alpha,block,layout", GPU_CASES)
def test_the_gpu_cases_show_fbar_and_stay_clear_of_cell_faces(ndim, materials, alpha, block, layout):
    """(d)"""
    snaps = xb.reference(ndim, materials, alpha, block, layout)
    plain = xb.reference(ndim, materials, None, 1, layout)
    case = xb.fbar_case(ndim, materials, layout)
    rows = np.asarray(alpha)[case["cloud"]["matidx"]] >= 0.0
    diff = relerr(snaps[-1]["stress"][rows], plain[-1]["stress"][rows])
    clear, Jmin = np.inf, np.inf
    for s in snaps:
        L = s["last"]
        u = (L["x"] - np.asarray(case["origin"])) / case["h"]
        clear = min(clear, float(np.abs(u - np.round(u)).min()))
        Jmin = min(Jmin, float(L["J_n1"].min()), float(s["Jbar_n"].min()), float(L["Jp"].min()))
        assert np.unique(L["pid"]).size > 1
    print(f"(d) {ndim}-D {materials} alpha {alpha} block {block} {layout}: barred against plain stress {diff:.2e} (> 1e-3), "
          f"closest particle to a cell face {clear:.2e} h (> 1e-9), smallest J {Jmin:.6f}")
    assert diff > 1e-3 and clear > 1e-9 and Jmin > 0.0


@pytest.mark.parametrize("ndim", [2, 3])
def test_a_restart_from_state_and_barred_state_continues_the_run(ndim):
    """(e)"""
    straight = xb.reference(ndim, (0,), (0.5,), 3)
    case = xb.fbar_case(ndim)
    s = straight[1]
    cloud = case["cloud"]
    for ck, k in (("x", "x"), ("dis", "dis"), ("vel", "vel"), ("acc", "acc"), ("F_n", "F_n"), ("J_n", "J_n"), ("rho", "rho")):
        cloud[ck] = s[k].copy()
    R = xb.FbarStepRef(case, [0.5], 3, xb.dirichlet(case), (), xb.NSTEPS, xb.gravity(ndim), Fbar_n=s["Fbar_n"], Jbar_n=s["Jbar_n"])
    for k in ("lambda", "beta", "I0"):  # the search continues from the multipliers and closest nodes of the run
        R.P[k][...] = s[k]
    worst = 0.0
    for t in (2, 3):
        R.step(t, xb.DT)
        snap = R.snapshot()
        for k in xf.FluidStepRef.FIELDS + ("Fbar_n", "Jbar_n"):
            worst = max(worst, relerr(snap[k], straight[t][k]))
            assert_close(snap[k], straight[t][k], 1e-12, f"restarted, step {t}: {k}")
    print(f"(e) {ndim}-D: restarted against straight {worst:.2e} (bound 1e-12)")
