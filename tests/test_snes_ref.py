"""tests/snes_ref.py (the numpy statement of nlps_gpu_newton_solve's algorithm) over the CPU oracle's stage functions,
with the residual composed as tests/newmark.py composes it: the case that backtracks, which makes the GPU test on the same
case non-vacuous, and the mild case as its control.  No GPU."""
import numpy as np

import snes_ref
from newmark import newmark_parameters
from test_gpu_parity import _OracleStages
from util import dirichlet_plane, make_case

SOFT = {"type": 0, "E": 2.0e5, "nu": 0.3}


def oracle_problem(velocity, dt, nsteps=2):
    """Step 0 of the 2-D block over a fixed floor: (residual, tangent, number of dofs) over the oracle."""
    case = make_case(2, [12, 11], [3, 3], [5, 4], material=SOFT, velocity=velocity)
    bcs = [dirichlet_plane(case, 1, 3, nsteps)]
    gravity = [0.0, -9.81]
    a = newmark_parameters(0.25, 0.5, dt)
    st = _OracleStages(case, nsteps)
    st.local_search()
    _, d2m, na = st.masks(bcs, 0)
    free = d2m != -1
    M = st.lumped_mass()
    V, A = st.nodal_field_n(M)
    bvec = np.tile(np.asarray(gravity), na)

    def residual(dU):
        dU_dt = a["a4"] * dU + (a["a5"] - 1) * V + a["a6"] * A
        st.compatibility(dU, dU_dt)
        st.constitutive()
        R = st.internal_forces()
        R[free] += (M * (a["a1"] * dU - a["a2"] * V - a["a3"] * A - bvec))[free]
        R[~free] = 0.0
        return R

    return residual, (lambda: st.tangent(a["a1"], M)), na * 2


def test_the_violent_case_backtracks_once_then_takes_full_steps():
    residual, tangent, n = oracle_problem([5.0, -40.0], 5.0e-2)
    x, info = snes_ref.newton(residual, tangent, np.zeros(n), linesearch="bt", rtol=1e-8, atol=0.0, stol=0.0,
                              linear="dense")
    print("fnorm", info["fnorm_history"], "lambda", info["lambda_history"])
    lam = info["lambda_history"]
    assert info["reason"] == snes_ref.CONVERGED_FNORM_RELATIVE, info
    assert lam[0] < 1.0, lam
    assert lam[0] == 0.1, "the clamped quadratic step"
    assert np.all(lam[1:] == 1.0) and len(lam) >= 2, lam
    assert info["fnorm"] <= 1e-8 * info["fnorm0"]
    # one evaluation at the guess, two for the iterate that backtracks, one for every other
    assert info["function_evaluations"] == info["iterations"] + 2
    # the basic line search takes the rejected full step: another path
    _, basic = snes_ref.newton(residual, tangent, np.zeros(n), linesearch="basic", rtol=1e-8, atol=0.0, stol=0.0,
                               linear="dense", max_it=1)
    assert basic["fnorm"] > info["fnorm0"], "the full first step does not decrease the residual"
    # no backtracking allowed: the search fails, x is the guess, the state is evaluated at the guess again
    x0, fail = snes_ref.newton(residual, tangent, np.zeros(n), linesearch="bt", rtol=1e-8, atol=0.0, stol=0.0,
                               linear="dense", ls_max_it=0)
    assert fail["reason"] == snes_ref.DIVERGED_LINE_SEARCH and fail["iterations"] == 0 and not x0.any()
    assert fail["function_evaluations"] == 3 and fail["fnorm"] == info["fnorm0"]


def test_the_mild_case_takes_full_steps():
    residual, tangent, n = oracle_problem([0.5, -1.0], 2.0e-2)
    x, info = snes_ref.newton(residual, tangent, np.zeros(n), linesearch="bt", rtol=1e-8, atol=0.0, stol=0.0,
                              linear="dense")
    print("fnorm", info["fnorm_history"], "lambda", info["lambda_history"])
    assert info["reason"] == snes_ref.CONVERGED_FNORM_RELATIVE and info["iterations"] == 2, info
    assert np.all(info["lambda_history"] == 1.0)
    assert info["function_evaluations"] == 3
    xg, ig = snes_ref.newton(residual, tangent, np.zeros(n), linesearch="bt", rtol=1e-8, atol=0.0, stol=0.0,
                             linear="gmres", ksp=dict(pc="pbjacobi", restart=200, rtol=1e-12), ndim=2)
    assert ig["iterations"] == 2 and ig["reason"] == info["reason"] and ig["linear_iterations"] > 0
    assert np.abs(xg - x).max() <= 1e-8 * np.abs(x).max()


def test_stopping_tests_of_the_reference():
    """A scalar-free check of the reference's own bookkeeping on a small algebraic system (no oracle)."""
    Adiag = np.array([1.0, 2.0, 4.0])
    state = {}

    def residual(x):
        state["x"] = x.copy()
        return Adiag * x + x ** 3 - 1.0

    def tangent():
        return np.diag(Adiag + 3.0 * state["x"] ** 2)

    x, info = snes_ref.newton(residual, tangent, np.zeros(3), rtol=1e-12, atol=0.0, stol=0.0)
    assert info["reason"] == snes_ref.CONVERGED_FNORM_RELATIVE and np.abs(residual(x)).max() < 1e-11
    assert len(info["fnorm_history"]) == info["iterations"] + 1 == len(info["lambda_history"]) + 1
    _, i1 = snes_ref.newton(residual, tangent, np.zeros(3), rtol=1e-12, atol=0.0, stol=0.0, max_it=1)
    assert i1["reason"] == snes_ref.DIVERGED_MAX_IT and i1["iterations"] == 1
    _, i2 = snes_ref.newton(residual, tangent, np.zeros(3), atol=10.0)
    assert i2["reason"] == snes_ref.CONVERGED_FNORM_ABS and i2["iterations"] == 0 and i2["function_evaluations"] == 1
    _, i3 = snes_ref.newton(residual, tangent, np.zeros(3), rtol=0.0, atol=0.0, stol=1e-3)
    assert i3["reason"] == snes_ref.CONVERGED_SNORM_RELATIVE
    _, i4 = snes_ref.newton(residual, tangent, np.zeros(3), rtol=1e-12, atol=0.0, stol=0.0, linear="gmres",
                            ksp=dict(pc="none", max_it=1, rtol=1e-14), ndim=1)
    assert i4["reason"] == snes_ref.DIVERGED_LINEAR_SOLVE and i4["iterations"] == 0
