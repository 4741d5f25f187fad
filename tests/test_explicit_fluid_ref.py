"""The checker of the explicit step with the fluid law (tests/explicit_fluid_ref.py) on the CPU: its numpy restatement of
the nodal algebra is orc.ExplicitStepper's on a cloud without the fluid, and the rate it hands to the law is the one
include/nlps_gpu.h defines for nlps_gpu_set_explicit_fluid."""
import numpy as np
import pytest

import explicit_fluid_ref as xf
import fluid_ref
from util import assert_close, oracle_setup, orc, relerr


@pytest.mark.parametrize("ndim", [2, 3])
def test_composition_on_a_neo_hookean_cloud_is_the_oracle_step(ndim):
    """(a) gravity, one Dirichlet set, three steps: every particle field and the nodal arrays against orc_explicit_step"""
    o = orc()
    nsteps = 3
    case = xf.fluid_case(ndim, [xf.SOFT_NH])
    bcs, g = xf.dirichlet(case, nsteps), xf.gravity(ndim)
    M, P, prm, mats = oracle_setup(case)
    stepper = o.ExplicitStepper(P, M, mats, prm, o.BccSet(bcs), nsteps, gravity=g)
    R = xf.FluidStepRef(case, bcs, (), nsteps, g)
    for t in range(nsteps):
        assert stepper.step(t, xf.DT) == 0
        R.step(t, xf.DT)
        assert stepper.out.nactive == R.na
        for k in ("mass", "dU", "force", "accel", "reaction"):
            assert_close(R.nodal[k], stepper.nodal(k), 1e-12, f"step {t} nodal {k}")
        assert np.abs(stepper.nodal("reaction")).max() > 0.0, "the plane has to hold something"
        for k in xf.FluidStepRef.FIELDS + ("W", "F_n1", "J_n1", "DF", "b_e_n"):
            assert_close(R.P[k], P[k], 1e-12, f"step {t} {k}")


@pytest.mark.parametrize("ndim", [2, 3])
def test_the_rate_is_the_mean_rate_of_the_step(ndim):
    """(b) dt_F_n1 == (F_n1 - F_n) / dt and L == (I - DF^-1) / dt per particle; the roll hands the rate on"""
    s = xf.reference(ndim)[0]
    nd, n = ndim, s["F_n"].shape[0]
    B = lambda a: a[:, : nd * nd].reshape(n, nd, nd)  # noqa: E731
    F1, F0, DF, rate = B(s["F_n"]), B(s["F_before"]), B(s["DF"]), B(s["dt_F_n1"])
    assert np.abs(rate).max() > 1.0, "velocity gradients of 10 - 15 1/s"
    worst_r = worst_L = 0.0
    for p in range(n):
        worst_r = max(worst_r, relerr(rate[p], (F1[p] - F0[p]) / xf.DT))
        L = fluid_ref.velocity_gradient(F1[p], rate[p])
        worst_L = max(worst_L, relerr(L, (np.eye(nd) - np.linalg.inv(DF[p])) / xf.DT))
    print(f"{ndim}-D: dt_F_n1 against (F_n1 - F_n) / dt {worst_r:.2e}, L against (I - DF^-1) / dt {worst_L:.2e}")
    assert worst_r <= 1e-10 and worst_L <= 1e-10
    assert_close(B(s["dt_DF"]), (DF - np.eye(nd)) / xf.DT, 1e-10, "dt_DF")
    assert np.array_equal(s["dt_F_n"], s["dt_F_n1"])


@pytest.mark.parametrize("ndim", [2, 3])
def test_without_viscosity_the_stress_is_the_pressure_whatever_dt(ndim):
    """(c) viscosity = 0: stress = -pressure(J) I, the same at another dt for the same dU"""
    o = orc()
    stress = {}
    for mu in (0.0, xf.FLUID["viscosity"]):
        mat = dict(xf.FLUID, viscosity=mu)
        R = xf.FluidStepRef(xf.fluid_case(ndim, [mat]))
        P = R.P
        assert o.local_search(P, R.M, R.prm) == 0
        n2m, na = o.active_nodes(R.M)
        dU = 1e-3 * np.random.default_rng(3).normal(size=na * ndim)
        for dt in (1e-4, 3e-4):
            P["dt_F_n"][:] = 0.0
            assert o.compatibility(dU, dU / dt, P, R.M, n2m) == 0
            R.F.stress()
            stress[(mu, dt)] = P["stress"].copy()
        if mu == 0.0:
            want = np.zeros_like(P["stress"])
            p = fluid_ref.pressure(mat, P["J_n1"])
            for q in ([0, 3, 4] if ndim == 2 else [0, 4, 8]):
                want[:, q] = -p
            assert np.abs(p).max() > 0.0
            assert_close(stress[(0.0, 1e-4)], want, 1e-13, "stress against -pressure(J) I")
    assert_close(stress[(0.0, 3e-4)], stress[(0.0, 1e-4)], 1e-13, "another dt, no viscosity")
    mu = xf.FLUID["viscosity"]
    assert relerr(stress[(mu, 3e-4)], stress[(mu, 1e-4)]) > 1e-2, "with viscosity the rate, and so dt, is in the stress"


@pytest.mark.parametrize("ndim", [2, 3])
def test_a_steady_flow_keeps_its_viscous_stress(ndim):
    """(d) two steps under a steady velocity field: the viscous part of the stress over J repeats to within the change of J
    and of L over a step, both O(|L| dt); ten times the measured change of J is the bound.  With the carried term
    DF dt_F_n of the Newmark path kept in, it doubles."""
    def viscous(carried):
        case = xf.fluid_case(ndim)
        R = xf.FluidStepRef(case, carried=carried)
        out = []
        for t in range(2):
            R.step(t, xf.DT)
            P = R.P  # (after the roll: F_n, dt_F_n, J_n are the step's F_n1, dt_F_n1, J_n1)
            out.append((np.array([fluid_ref.stress_terms(xf.FLUID, P["F_n"][p], P["dt_F_n"][p], P["J_n"][p], ndim)[2] / P["J_n"][p]
                                  for p in range(P.np)]), P["J_n"].copy()))
        return out
    (v1, J1), (v2, J2) = viscous(False)
    dJ = float(np.abs(J2 / J1 - 1.0).max())
    e = relerr(v2, v1)
    print(f"{ndim}-D: viscous stress / J, step 2 against step 1: {e:.2e}; largest change of J {dJ:.2e}")
    assert 0.0 < dJ < 1e-2 and e <= 10.0 * dJ
    (c1, _), (c2, _) = viscous(True)
    assert_close(c1, v1, 1e-12, "the first step carries nothing")
    ratio = np.linalg.norm(c2) / np.linalg.norm(c1)
    print(f"{ndim}-D: with the carried term the viscous stress grows by {ratio:.3f}")
    assert ratio > 1.9
