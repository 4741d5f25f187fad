"""The device Newton solve (nlps_gpu_newton_solve) and the one-call implicit time step (nlps_gpu_newmark_step) against
tests/snes_ref.py, the numpy statement of the same algorithm, run over a SECOND handle's lagrangian_evaluation and
assembled tangent (dense solve or tests/krylov_ref.py's GMRES): reasons, iteration and evaluation counts, step lengths,
residual histories, the returned dU, the particle state the call leaves, and the call contract."""
import numpy as np
import pytest

import snes_ref
from newmark import newmark_parameters
from test_gpu_tangent_operator import _coo_dense
from util import DP, NH, assert_close, dirichlet_plane, gpu_setup, make_case, nlps

pytestmark = pytest.mark.gpu

SOFT = {"type": 0, "E": 2.0e5, "nu": 0.3}
TIGHT = dict(pc="pbjacobi", restart=200, max_it=2000, rtol=1e-12)  # a linear solve as good as the dense one
DRIVER = dict(pc="jacobi", restart=30, max_it=10000, rtol=1e-5)    # PCJACOBI, GMRES(30), KSP's default rtol
# fnorm_history against the reference, entries at or above 1e-7 fnorm0: ten times the largest relative difference
# measured on the MI355X over the three cases of test_against_the_dense_newton, 4.19e-8 (Drucker-Prager, second time
# step; Neo-Hookean 3.4e-9 in 2-D and 8.0e-9 in 3-D)
HISTORY_TOL = 4.2e-7
STATE = ("DF", "F_n1", "J_n1", "Stress", "b_e_n1")


def _problem(ndim, law="neo-hookean", violent=False, case=None, plane=None):
    """case: another cloud than the two below; plane: the layer of grid nodes that is fixed, if not theirs."""
    mat = SOFT if law == "neo-hookean" else DP
    if case is None and ndim == 2:
        case = make_case(2, [12, 11], [3, 3], [5, 4], material=mat, velocity=[5.0, -40.0] if violent else [0.5, -1.0])
    elif case is None:
        case = make_case(3, [8, 8, 7], [3, 3, 2], [2, 2, 2], material=mat, velocity=[0.5, 0.2, -1.0])
    nsteps = 3
    if plane is None:
        plane = 3 if ndim == 2 else 2
    bcs = nlps().BccSet([dirichlet_plane(case, ndim - 1, plane, nsteps)])
    return case, bcs, [0.0] * (ndim - 1) + [-9.81], nsteps


def _alpha(dt):
    a = newmark_parameters(0.25, 0.5, dt)
    return [a["a1"], a["a2"], a["a3"], a["a4"], a["a5"], a["a6"]]


class _Step:
    """One handle at the start of a time step: masks, M, Un_dt, Un_dt2, and the callables snes_ref wants."""

    def __init__(self, S, bcs, step, alpha, gravity):
        self.S, self.alpha, self.gravity = S, alpha, gravity
        S.local_search()
        S.active_masks(bcs, step)
        self.M = S.compute_nodal_lumped_mass()
        self.V, self.A = S.get_nodal_field_n(self.M)
        self.n = S.nactive * S.ndim

    def residual(self, x):
        return self.S.lagrangian_evaluation(np.ascontiguousarray(x), self.V, self.A, self.M, self.alpha, self.gravity)

    def tangent(self):
        return _coo_dense(self.S, self.n, self.alpha[0], self.M, True)

    def solve(self, dU, **kw):
        return self.S.newton_solve(dU, self.V, self.A, self.M, self.alpha, self.gravity, **kw)

    def advance(self, dU):
        dV, dA = self.S.compute_nodal_kinetic_increments(dU, self.V, self.A, self.alpha)
        self.S.update_particles_internal_variables()
        self.S.update_particles_kinetics_FLIP_PIC(1.0, dU, self.V, dV, dA)


def _same_counts(info, ref, what):
    for k in ("reason", "iterations", "function_evaluations"):
        assert info[k] == ref[k], f"{what}: {k} {info[k]} vs the reference's {ref[k]}\n{info}\n{ref}"


def _check_state(S, twin, dU, law, what):
    """The state the solve left on S against a separate evaluation at the returned dU on the twin handle."""
    twin.residual(dU)
    a, b = S.download_state(), twin.S.download_state()
    for k in STATE + (("Kappa_n1", "EPS_n1") if law == "drucker-prager" else ()):
        assert_close(a[k], b[k], 1e-10, f"{what}: state {k}")


@pytest.mark.parametrize("ndim,law", [(2, "neo-hookean"), (3, "neo-hookean"), (3, "drucker-prager")])
def test_against_the_dense_newton(ndim, law):
    """Three time steps, basic line search, a linear solve at 1e-12: the same Newton as snes_ref with a dense solve."""
    case, bcs, gravity, nsteps = _problem(ndim, law)
    alpha = _alpha(1.0e-2)
    S, S2 = gpu_setup(case, nsteps=nsteps), gpu_setup(case, nsteps=nsteps)
    kw = dict(max_it=12, rtol=1e-10, atol=0.0, stol=0.0)
    worst = 0.0
    for step in range(nsteps):
        what = f"{law} {ndim}-D step {step}"
        dev, ref = _Step(S, bcs, step, alpha, gravity), _Step(S2, bcs, step, alpha, gravity)
        dU, info = dev.solve(np.zeros(dev.n), linesearch="basic", ksp=TIGHT, **kw)
        xr, ir = snes_ref.newton(ref.residual, ref.tangent, np.zeros(ref.n), linesearch="basic", linear="dense", **kw)
        print(what, "device", info["fnorm_history"], "reference", ir["fnorm_history"])
        assert info["reason"] == snes_ref.CONVERGED_FNORM_RELATIVE and info["iterations"] >= 2, info
        _same_counts(info, ir, what)
        assert np.all(info["lambda_history"] == 1.0) and len(info["ksp_iterations"]) == info["iterations"]
        assert info["linear_iterations"] == info["ksp_iterations"].sum() > 0
        assert_close(dU, xr, 1e-8, f"{what}: dU", scale=np.abs(xr).max())
        rn = np.linalg.norm(ref.residual(dU))
        assert abs(info["fnorm"] - rn) <= 1e-2 * info["fnorm"] + 1e-13 * info["fnorm0"], \
            f"{what}: fnorm {info['fnorm']:.6e} vs a separate evaluation {rn:.6e}"
        hd, hr = info["fnorm_history"], ir["fnorm_history"]
        big = hr >= 1e-7 * hr[0]  # (below that the entries are summation noise of the residual's atomics)
        assert big[:2].all(), f"{what}: the first two entries are above 1e-7 fnorm0: {hr}"
        err = float((np.abs(hd - hr)[big] / hr[big]).max())
        worst = max(worst, err)
        print(what, "fnorm_history: largest relative difference %.3e" % err)
        assert err <= HISTORY_TOL, f"{what}: fnorm_history, relative {err:.3e}\n{hd}\n{hr}"
        _check_state(S, ref, dU, law, what)  # (the twin is at dU now: both advance from the same state)
        dev.advance(dU)
        ref.advance(dU)
    print(f"{law} {ndim}-D: fnorm_history worst relative difference {worst:.3e}")
    S.close()
    S2.close()


def test_backtracking_and_a_failed_line_search():
    """The case tests/test_snes_ref.py pins down on the CPU: the first full step is rejected, the clamped quadratic step
    0.1 is accepted, full steps follow.  With ls_max_it = 0 the rejected trial fails the search: dU and the state are
    those of the guess."""
    case, bcs, gravity, nsteps = _problem(2, violent=True)
    alpha = _alpha(5.0e-2)
    S, S2 = gpu_setup(case, nsteps=nsteps), gpu_setup(case, nsteps=nsteps)
    dev, ref = _Step(S, bcs, 0, alpha, gravity), _Step(S2, bcs, 0, alpha, gravity)
    kw = dict(max_it=50, rtol=1e-8, atol=0.0, stol=0.0, linesearch="bt")
    dU, info = dev.solve(np.zeros(dev.n), ksp=TIGHT, **kw)
    xr, ir = snes_ref.newton(ref.residual, ref.tangent, np.zeros(ref.n), linear="dense", **kw)
    print("device", info["fnorm_history"], info["lambda_history"], "reference", ir["fnorm_history"], ir["lambda_history"])
    ld, lr = info["lambda_history"], ir["lambda_history"]
    assert lr[0] < 1.0 and np.all(lr[1:] == 1.0), lr
    _same_counts(info, ir, "bt")
    assert info["reason"] == snes_ref.CONVERGED_FNORM_RELATIVE
    assert len(ld) == len(lr) and np.all(np.abs(ld - lr) <= 1e-6 * lr), (ld, lr)
    assert ld[0] == 0.1 == lr[0], "the clamped quadratic step"
    assert_close(dU, xr, 1e-8, "bt: dU", scale=np.abs(xr).max())
    _check_state(S, ref, dU, "neo-hookean", "bt")
    guess = np.zeros(dev.n)
    d0, i0 = dev.solve(guess, ksp=TIGHT, ls_max_it=0, **kw)
    x0, r0 = snes_ref.newton(ref.residual, ref.tangent, np.zeros(ref.n), linear="dense", ls_max_it=0, **kw)
    assert i0["reason"] == snes_ref.DIVERGED_LINE_SEARCH == r0["reason"] and i0["iterations"] == 0, i0
    assert i0["function_evaluations"] == r0["function_evaluations"] == 3
    assert np.array_equal(d0, guess), "dU comes back as the guess"
    _check_state(S, ref, guess, "neo-hookean", "failed line search")  # (not the state of the rejected trial)
    st = S.download_state()
    ref.residual(guess - np.linalg.solve(ref.tangent(), ref.residual(guess)))
    rejected = S2.download_state()
    assert np.abs(st["Stress"] - rejected["Stress"]).max() > 1e-3 * np.abs(st["Stress"]).max(), "the trial's state differs"
    S.close()
    S2.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_the_drivers_settings_against_the_reference_gmres(ndim):
    """PCJACOBI, GMRES(30) at 1e-5, the driver's SNES tolerances, bt: the reference with krylov_ref.gmres."""
    case, bcs, gravity, nsteps = _problem(ndim)
    alpha = _alpha(1.0e-2)
    S, S2 = gpu_setup(case, nsteps=nsteps), gpu_setup(case, nsteps=nsteps)
    dev, ref = _Step(S, bcs, 0, alpha, gravity), _Step(S2, bcs, 0, alpha, gravity)
    kw = dict(max_it=50, atol=1e-8, rtol=1e-10, stol=1e-8, linesearch="bt")
    dU, info = dev.solve(np.zeros(dev.n), ksp=DRIVER, **kw)
    xr, ir = snes_ref.newton(ref.residual, ref.tangent, np.zeros(ref.n), linear="gmres", ksp=DRIVER, ndim=ndim, **kw)
    print("device", info["fnorm_history"], info["ksp_iterations"], "reference", ir["fnorm_history"], ir["ksp_iterations"])
    assert info["reason"] > 0 and info["reason"] == ir["reason"] and info["iterations"] == ir["iterations"], (info, ir)
    assert np.all(np.abs(info["ksp_iterations"] - ir["ksp_iterations"]) <= 1), (info["ksp_iterations"], ir["ksp_iterations"])
    assert info["linear_iterations"] == info["ksp_iterations"].sum()
    S.close()
    S2.close()


def test_call_contract():
    import torch
    n = nlps()
    case, bcs, gravity, nsteps = _problem(2)
    alpha = _alpha(2.0e-2)
    S = gpu_setup(case, nsteps=nsteps)
    with pytest.raises(n.NlpsError, match="nlps_gpu_newton_solve: call nlps_gpu_(active_masks|local_search)"):
        S.newton_solve(np.zeros(4), np.zeros(4), np.zeros(4), np.zeros(4), alpha, gravity)
    dev = _Step(S, bcs, 0, alpha, gravity)
    kw = dict(rtol=1e-8, atol=0.0, stol=0.0, linesearch="bt", ksp=TIGHT)
    guess = np.zeros(dev.n)
    dU, info = dev.solve(guess, **kw)
    assert isinstance(dU, np.ndarray) and info["reason"] == snes_ref.CONVERGED_FNORM_RELATIVE and info["iterations"] == 2
    assert not guess.any(), "the guess is left as it is"
    # torch device vectors: the same solve, the result on the device
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    dT, iT = S.newton_solve(t(guess), t(dev.V), t(dev.A), t(dev.M), alpha, gravity, **kw)
    assert isinstance(dT, torch.Tensor) and dT.is_cuda and iT["iterations"] == info["iterations"]
    assert_close(dT.cpu().numpy(), dU, 1e-8, "device vs host vectors", scale=np.abs(dU).max())
    out = np.full(dev.n, 7.0)
    r, _ = dev.solve(guess, out=out, **kw)
    assert r is out
    assert_close(out, dU, 1e-8, "out", scale=np.abs(dU).max())
    # max_it = 1: one iterate, not converged
    d1, i1 = dev.solve(guess, max_it=1, **kw)
    assert i1["reason"] == snes_ref.DIVERGED_MAX_IT and i1["iterations"] == 1 and len(i1["fnorm_history"]) == 2
    assert d1.any() and i1["function_evaluations"] == 2
    # a linear solve that fails: dU unchanged
    start = 1e-4 * np.random.default_rng(5).normal(size=dev.n)
    d2, i2 = dev.solve(start, rtol=1e-8, atol=0.0, stol=0.0, ksp=dict(pc="pbjacobi", restart=30, max_it=1, rtol=1e-12))
    assert i2["reason"] == snes_ref.DIVERGED_LINEAR_SOLVE and i2["iterations"] == 0 and i2["ksp_reason"] == -3, i2
    assert np.array_equal(d2, start) and list(i2["ksp_iterations"]) == [1]
    # atol above the first norm: converged before any iterate
    d3, i3 = dev.solve(guess, rtol=1e-8, atol=10.0 * info["fnorm0"], stol=0.0, ksp=TIGHT)
    assert i3["reason"] == snes_ref.CONVERGED_FNORM_ABS and i3["iterations"] == 0 and i3["function_evaluations"] == 1
    assert np.array_equal(d3, guess) and i3["fnorm"] == i3["fnorm0"] == pytest.approx(info["fnorm0"], rel=1e-12)
    # misuse
    with pytest.raises(n.NlpsError, match="nlps_gpu_newton_solve: .*>= 0"):
        dev.solve(guess, rtol=-1.0)
    with pytest.raises(n.NlpsError, match="nlps_gpu_newton_solve: .*>= 0"):
        dev.solve(guess, max_it=-1)
    with pytest.raises(n.NlpsError, match="ls_max_it"):
        dev.solve(guess, ls_max_it=-1)
    with pytest.raises(ValueError):
        dev.solve(guess, linesearch="cp")
    S.set_halo_exchange(lambda dptr, nfield, elem, kind: 0)
    with pytest.raises(n.NlpsError, match="nlps_gpu_newton_solve: single rank only"):
        dev.solve(guess, **kw)
    S.set_halo_exchange(None)
    dev.solve(guess, **kw)
    S.close()


def test_a_step_longer_than_maxstep_is_scaled():
    """ls_maxstep far below the Newton step: every iterate is the scaled full step, accepted at lambda = 1, and the full
    step evaluated before its length was known counts (include/nlps_gpu.h)."""
    case, bcs, gravity, nsteps = _problem(2)
    alpha = _alpha(2.0e-2)
    S, S2 = gpu_setup(case, nsteps=nsteps), gpu_setup(case, nsteps=nsteps)
    dev, ref = _Step(S, bcs, 0, alpha, gravity), _Step(S2, bcs, 0, alpha, gravity)
    kw = dict(max_it=3, rtol=1e-8, atol=0.0, stol=0.0, linesearch="bt", ls_maxstep=1e-3)
    dU, info = dev.solve(np.zeros(dev.n), ksp=TIGHT, **kw)
    xr, ir = snes_ref.newton(ref.residual, ref.tangent, np.zeros(ref.n), linear="dense", **kw)
    print("device", info["fnorm_history"], info["lambda_history"], "reference", ir["fnorm_history"], ir["lambda_history"])
    _same_counts(info, ir, "maxstep")
    assert info["reason"] == snes_ref.DIVERGED_MAX_IT and info["function_evaluations"] == 7
    assert np.array_equal(info["lambda_history"], ir["lambda_history"]) and np.all(info["lambda_history"] == 1.0)
    assert abs(info["snorm"] - 1e-3) <= 1e-12 and abs(ir["snorm"] - 1e-3) <= 1e-12
    assert abs(np.linalg.norm(dU) - info["xnorm"]) <= 1e-12 * info["xnorm"]
    assert_close(dU, xr, 1e-8, "maxstep: dU", scale=np.abs(xr).max())
    assert_close(info["fnorm_history"], ir["fnorm_history"], HISTORY_TOL, "maxstep: fnorm_history")
    _check_state(S, ref, dU, "neo-hookean", "maxstep")
    S.close()
    S2.close()


def test_quasi_static():
    """Zeros in alpha (U-Static.c): no inertia, the load against the stiffness alone, the floor fixed.  Without alpha_1 M
    the nodes at the rim of the cloud carry almost no stiffness (cond ~1e11, test_quasi_static_against_a_dense_solve), and
    under the whole of gravity in one step they move by many cells.  The static driver ramps its loads, so the test takes
    one increment of a thousandth of gravity: the step is then nearly linear, the linear solve runs at KSP's default 1e-5
    (with a long restart: GMRES(30) stalls at 2.5e-4 on this right-hand side) and Newton at rtol 1e-4."""
    case = make_case(3, [8, 8, 7], [3, 3, 2], [2, 2, 2], material=NH)
    nsteps = 2
    bcs = nlps().BccSet([dirichlet_plane(case, 2, 2, nsteps)])
    S = gpu_setup(case, nsteps=nsteps)
    dev = _Step(S, bcs, 0, [0.0] * 6, [0.0, 0.0, -9.81e-3])
    dU, info = dev.solve(np.zeros(dev.n), rtol=1e-4, atol=0.0, stol=0.0, linesearch="bt",
                         ksp=dict(pc="pbjacobi", restart=200, max_it=6000, rtol=1e-5))
    print("quasi-static", info)
    assert info["reason"] == snes_ref.CONVERGED_FNORM_RELATIVE and info["iterations"] >= 1, info
    rn = np.linalg.norm(dev.residual(dU))
    assert rn <= 1.01e-4 * info["fnorm0"] and dU.min() < 0.0
    S.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_newmark_step(ndim):
    """Three steps in one call each against the same steps made of the separate calls and newton_solve."""
    case, bcs, gravity, nsteps = _problem(ndim)
    dt = 2.0e-2
    alpha = _alpha(dt)
    S, S2 = gpu_setup(case, nsteps=nsteps), gpu_setup(case, nsteps=nsteps)
    kw = dict(max_it=50, atol=1e-8, rtol=1e-10, stol=1e-8, linesearch="bt", ksp=DRIVER)
    dU_out = np.zeros(S.nnodes * ndim)
    for step in range(nsteps):
        info = S.newmark_step(bcs, step, dt, gravity, dU_out=dU_out, **kw)
        sep = _Step(S2, bcs, step, alpha, gravity)
        guess = S2.form_initial_guess(sep.V, sep.A, dt, bcs, step)
        dU, ir = sep.solve(guess, **kw)
        sep.advance(dU)
        print(f"step {step}", info["fnorm_history"], info["ksp_iterations"], ir["fnorm_history"], ir["ksp_iterations"])
        assert info["nactive"] == S2.nactive and info["reason"] > 0
        for k in ("reason", "iterations", "function_evaluations", "linear_iterations"):
            assert info[k] == ir[k], f"step {step}: {k} {info[k]} vs {ir[k]}"
        assert np.array_equal(info["lambda_history"], ir["lambda_history"])
        assert_close(dU_out[: sep.n], dU, 1e-8, f"step {step}: dU", scale=np.abs(dU).max())
    a, b = S.download_state(), S2.download_state()
    for k in ("x", "vel", "acc", "F_n", "Stress", "J_n"):
        assert_close(a[k], b[k], 1e-8, f"after three steps: {k}")
    assert np.abs(a["Stress"]).max() > 10.0
    # a step whose solve does not converge leaves the particles where they are, not rolled
    S.close()
    S2.close()
    S = gpu_setup(case, nsteps=nsteps)
    before = S.download_state()
    x0, f0 = before["x"].copy(), before["F_n"].copy()
    bad = S.newmark_step(bcs, 0, dt, gravity, **dict(kw, max_it=1))
    assert bad["reason"] == snes_ref.DIVERGED_MAX_IT and bad["iterations"] == 1
    st = S.download_state()
    assert np.array_equal(st["x"], x0) and np.array_equal(st["F_n"], f0)
    assert np.abs(st["F_n1"] - f0).max() > 0.0, "the last evaluated state is there"
    S.close()
