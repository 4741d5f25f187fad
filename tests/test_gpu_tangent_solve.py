"""Device GMRES on the matrix-free tangent (nlps_gpu_tangent_solve): x against a dense solve of the assembled COO, the
iteration history against the numpy reference of the same algorithm (tests/krylov_ref.py), the call contract, Newton
steps with the device solve, and the bench cube at 1 M particles."""
import numpy as np
import pytest

import krylov_ref
from newmark import newmark_parameters
from test_gpu_tangent_operator import _coo_dense, _linearised
from util import DP, assert_close, dirichlet_plane, gpu_setup, make_case, nlps

pytestmark = pytest.mark.gpu

ALPHA_1 = 4.0e4


def _dyn(s, alpha_1=ALPHA_1, dirichlet=True):
    """The dynamic operator (alpha_1 M, Dirichlet on) on the device and as a dense matrix."""
    S, na = s["S"], s["na"]
    ndim = S.ndim
    K = _coo_dense(S, na * ndim, alpha_1, s["Mv"], dirichlet)
    S.tangent_operator(alpha_1, s["Mv"], dirichlet)
    return K


def _check_solution(K, b, x, info, rtol, what):
    ref = np.linalg.solve(K, b)
    assert info["reason"] > 0, f"{what}: not converged: {info}"
    assert info["rnorm"] <= rtol * info["bnorm"], f"{what}: rnorm {info['rnorm']:.3e} > rtol ||b||"
    assert abs(info["bnorm"] - np.linalg.norm(b)) <= 1e-12 * np.linalg.norm(b)
    r_dense = np.linalg.norm(b - K @ x)
    assert abs(info["rnorm"] - r_dense) <= 1e-2 * r_dense + 1e-13 * np.linalg.norm(b), \
        f"{what}: rnorm {info['rnorm']:.6e} vs the dense ||b - K x|| {r_dense:.6e}"
    assert_close(x, ref, 1e-6, f"{what}: x vs np.linalg.solve", scale=np.abs(ref).max())


def _check_against_reference(K, b, x, info, pc, restart, rtol, ndim, what, max_it=2000):
    xr, ir = krylov_ref.gmres(K, b, krylov_ref.preconditioner(K, pc, ndim), restart=restart, max_it=max_it, rtol=rtol)
    assert info["reason"] == ir["reason"], f"{what}: reason {info['reason']} vs reference {ir['reason']}"
    assert abs(info["iterations"] - ir["iterations"]) <= 1, f"{what}: iterations {info['iterations']} vs reference {ir['iterations']}"
    nh = min(10, len(ir["history"]), len(info["history"]))
    hd, hr = info["history"][:nh], ir["history"][:nh]
    err = np.abs(hd - hr) / np.maximum(hr, 1e-12 * hr[0])
    assert err.max() <= 1e-6, f"{what}: history vs reference, relative {err.max():.3e}:\n{hd}\n{hr}"
    if ir["reason"] > 0:
        assert_close(x, xr, 1e-5, f"{what}: x vs reference GMRES", scale=np.abs(xr).max())
    return ir


@pytest.mark.parametrize("ndim,law", [(2, "neo-hookean"), (3, "neo-hookean"), (3, "hencky"), (3, "drucker-prager"),
                                      (3, "matsuoka-nakai")])
def test_against_a_dense_solve(ndim, law):
    s = _linearised(ndim, law, with_oracle=False)
    S, na = s["S"], s["na"]
    K = _dyn(s)
    b = s["rng"].normal(size=na * ndim)
    x, info = S.tangent_solve(b, pc="pbjacobi", rtol=1e-10, max_it=2000)
    assert isinstance(x, np.ndarray) and info["iterations"] > 0
    _check_solution(K, b, x, info, 1e-10, f"{law} {ndim}-D")
    S.close()


def test_quasi_static_against_a_dense_solve():
    """No mass term (U-Static.c): K alone, Dirichlet on.  Without alpha_1 M the nodes at the rim of the cloud, which
    carry little of any particle's support, make K ill-conditioned (cond ~1e11 here): b is a consistent right-hand side
    K x_true, the tolerance the driver's KSP default (GMRES(30) stagnates near 1e-6 here), and the check is on the
    residual, against the dense K and the reference GMRES."""
    s = _linearised(3, "neo-hookean", with_oracle=False)
    S, na = s["S"], s["na"]
    K = _coo_dense(S, na * 3, 0.0, None, True)
    S.tangent_operator(0.0, None, True)
    b = K @ s["rng"].normal(size=na * 3)
    x, info = S.tangent_solve(b, pc="pbjacobi", restart=30, rtol=1e-5, max_it=3000, history=True)
    assert info["reason"] > 0, info
    r_dense = np.linalg.norm(b - K @ x)
    assert r_dense <= 1.01e-5 * np.linalg.norm(b)
    assert abs(info["rnorm"] - r_dense) <= 1e-2 * r_dense + 1e-13 * np.linalg.norm(b)
    xr, ir = krylov_ref.gmres(K, b, krylov_ref.preconditioner(K, "pbjacobi", 3), restart=30, max_it=3000, rtol=1e-5)
    assert ir["reason"] > 0 and abs(info["iterations"] - ir["iterations"]) <= 1, (info["iterations"], ir["iterations"])
    S.close()


@pytest.mark.parametrize("restart", [30, 5])
@pytest.mark.parametrize("pc", ["none", "jacobi", "pbjacobi"])
def test_against_the_reference_gmres(pc, restart):
    """Iteration counts within one and the first 10 residual norms to 1e-6: a wrong or stale preconditioner changes them
    (it would still converge).  Drucker-Prager 3-D with a small alpha_1 (12 steps to 1e-8 with either Jacobi).  Without
    a preconditioner the identity rows of the Dirichlet dofs against the stiffness make GMRES crawl: both stop at
    max_it = 60, same reason."""
    s = _linearised(3, "drucker-prager", with_oracle=False)
    S, na = s["S"], s["na"]
    K = _dyn(s, alpha_1=10.0)
    b = s["rng"].normal(size=na * 3)
    rtol, max_it = 1e-8, (60 if pc == "none" else 2000)
    x, info = S.tangent_solve(b, pc=pc, restart=restart, rtol=rtol, max_it=max_it, history=True)
    assert len(info["history"]) == info["iterations"] + 1
    ir = _check_against_reference(K, b, x, info, pc, restart, rtol, 3, f"pc={pc} restart={restart}", max_it=max_it)
    if restart == 5:
        assert ir["iterations"] > 5, "the case must need more than one cycle"
    S.close()


def test_host_and_device_vectors_guess_zero_rhs_max_it_and_two_rhs():
    import torch
    s = _linearised(3, "hencky", with_oracle=False)
    S, na = s["S"], s["na"]
    n = na * 3
    K = _dyn(s)
    rng = s["rng"]
    b = rng.normal(size=n)
    b0 = b.copy()
    x_h, info_h = S.tangent_solve(b, rtol=1e-10, history=True)
    assert np.array_equal(b, b0), "b is not touched"
    _check_solution(K, b, x_h, info_h, 1e-10, "host vectors")
    bd = torch.from_numpy(b).cuda()
    x_d, info_d = S.tangent_solve(bd, rtol=1e-10, history=True)
    assert isinstance(x_d, torch.Tensor) and x_d.is_cuda
    assert info_d["iterations"] == info_h["iterations"]
    assert_close(x_d.cpu().numpy(), x_h, 1e-9, "device vs host x", scale=np.abs(x_h).max())
    assert_close(info_d["history"], info_h["history"], 1e-8, "device vs host history", scale=info_h["history"][0])
    out = torch.full((n,), 3.0, dtype=torch.float64, device="cuda")
    r, _ = S.tangent_solve(bd, rtol=1e-10, out=out)
    assert r is out
    # the exact solution as the guess: no Arnoldi step
    x_exact = np.linalg.solve(K, b)
    xg, ig = S.tangent_solve(b, x=x_exact, rtol=1e-8)
    assert ig["iterations"] == 0 and ig["reason"] > 0, ig
    assert_close(xg, x_exact, 1e-12, "guess returned as it is", scale=np.abs(x_exact).max())
    # b = 0: x = 0, even over a guess
    xz, iz = S.tangent_solve(np.zeros(n), x=x_exact)
    assert iz["reason"] == 1 and iz["iterations"] == 0 and not xz.any()
    # max_it too small: the call succeeds, the reason says it did not converge
    xm, im = S.tangent_solve(b, rtol=1e-12, max_it=2, history=True)
    assert im["reason"] == -3 and im["iterations"] == 2 and len(im["history"]) == 3, im
    assert im["rnorm"] > 1e-12 * im["bnorm"] and np.isfinite(xm).all()
    # two right-hand sides on one linearisation (the preconditioner is reused)
    for _ in range(2):
        b2 = rng.normal(size=n)
        x2, i2 = S.tangent_solve(b2, rtol=1e-10)
        _check_solution(K, b2, x2, i2, 1e-10, "second right-hand side")
    S.close()


def test_relinearised_operator_rebuilds_the_preconditioner():
    """A new dU on the same particles (no search: the operator's generation does not move) and a new operator: the
    solve must follow the reference GMRES of the NEW matrix, preconditioner included."""
    s = _linearised(3, "neo-hookean", with_oracle=False)
    S, na = s["S"], s["na"]
    n = na * 3
    K1 = _dyn(s)
    b = s["rng"].normal(size=n)
    x1, i1 = S.tangent_solve(b, pc="pbjacobi", restart=5, rtol=1e-8, history=True)
    _check_against_reference(K1, b, x1, i1, "pbjacobi", 5, 1e-8, 3, "first linearisation")
    S.local_compatibility_conditions(0.1 * s["rng"].normal(size=n))  # (a large step: other blocks)
    S.constitutive_update()
    K2 = _dyn(s, alpha_1=1.0e3)
    assert np.abs(K2 - K1).max() > 1e-3 * np.abs(K1).max()
    for pc in ("pbjacobi", "jacobi"):
        x2, i2 = S.tangent_solve(b, pc=pc, restart=5, rtol=1e-8, history=True)
        _check_against_reference(K2, b, x2, i2, pc, 5, 1e-8, 3, f"second linearisation, {pc}")
    S.close()


def test_stale_operator_and_halo_handles_are_refused():
    n = nlps()
    s = _linearised(2, "neo-hookean", with_oracle=False)
    S, na, Mv = s["S"], s["na"], s["Mv"]
    b = s["rng"].normal(size=na * 2)
    with pytest.raises(n.NlpsError, match="nlps_gpu_tangent_solve: call nlps_gpu_tangent_operator\\(\\) first"):
        S.tangent_solve(b)
    S.tangent_operator(ALPHA_1, Mv, True)
    S.tangent_solve(b)
    with pytest.raises(ValueError):
        S.tangent_solve(b, pc="ilu")
    with pytest.raises(n.NlpsError, match="restart"):
        S.tangent_solve(b, restart=0)
    S.local_search()
    with pytest.raises(n.NlpsError, match="stale: .*nlps_gpu_local_search"):
        S.tangent_solve(b)
    bcs = n.BccSet([dirichlet_plane(make_case(2, [12, 11], [3, 3], [5, 4]), 1, 3, 2)])
    S.active_masks(bcs, 1)
    S.tangent_operator(ALPHA_1, S.compute_nodal_lumped_mass(), True)
    S.set_halo_exchange(lambda dptr, nfield, elem, kind: 0)
    with pytest.raises(n.NlpsError, match="single rank only"):
        S.tangent_solve(np.ones(S.nactive * 2))
    S.set_halo_exchange(None)
    S.tangent_solve(np.ones(S.nactive * 2))
    S.close()


@pytest.mark.parametrize("ndim,law", [(2, "neo-hookean"), (3, "neo-hookean"), (3, "drucker-prager")])
def test_newton_with_the_device_solve(ndim, law):
    """test_newton_krylov_steps with nlps_gpu_tangent_solve on torch device vectors in place of scipy GMRES: the same
    Newton iteration counts as the dense solve and dU within 1e-8."""
    import torch
    n = nlps()
    mat = {"type": 0, "E": 2.0e5, "nu": 0.3} if law == "neo-hookean" else DP
    if ndim == 2:
        case = make_case(2, [12, 11], [3, 3], [5, 4], material=mat, velocity=[0.5, -1.0])
    else:
        case = make_case(3, [8, 8, 7], [3, 3, 2], [2, 2, 2], material=mat, velocity=[0.5, 0.2, -1.0])
    nsteps = 3
    bcs = n.BccSet([dirichlet_plane(case, ndim - 1, 3 if ndim == 2 else 2, nsteps)])
    gravity = [0.0] * (ndim - 1) + [-9.81]
    dt = 1.0e-2
    a = newmark_parameters(0.25, 0.5, dt)
    alpha = [a["a1"], a["a2"], a["a3"], a["a4"], a["a5"], a["a6"]]
    runs = []
    for device in (False, True):
        S = gpu_setup(case, nsteps=nsteps)
        its_all, dU_all = [], []
        for step in range(nsteps):
            S.local_search()
            S.active_masks(bcs, step)
            Mv = S.compute_nodal_lumped_mass()
            V, A = S.get_nodal_field_n(Mv)
            ntot = S.nactive * ndim
            dU = np.zeros(ntot)
            R = S.lagrangian_evaluation(dU, V, A, Mv, alpha, gravity)
            r0 = np.linalg.norm(R)
            its = 0
            while np.linalg.norm(R) > 1e-10 * max(r0, 1e-30) and its < 12:
                if device:
                    S.tangent_operator(a["a1"], Mv, True)
                    rhs = torch.from_numpy(-R).cuda()
                    dd, info = S.tangent_solve(rhs, pc="pbjacobi", restart=200, max_it=2000, rtol=1e-12)
                    assert info["reason"] > 0, info
                    d = dd.cpu().numpy()
                else:
                    K = _coo_dense(S, ntot, a["a1"], Mv, True)
                    d = np.linalg.solve(K, -R)
                dU = dU + d
                R = S.lagrangian_evaluation(dU, V, A, Mv, alpha, gravity)
                its += 1
            assert np.linalg.norm(R) <= 1e-10 * max(r0, 1e-30), f"step {step}: Newton did not converge"
            its_all.append(its)
            dU_all.append(dU.copy())
            dV = a["a4"] * dU + (a["a5"] - 1) * V + a["a6"] * A
            dA = a["a1"] * dU - a["a2"] * V - (a["a3"] + 1) * A
            S.update_particles_internal_variables()
            S.update_particles_kinetics_FLIP_PIC(1.0, dU, V, dV, dA)
        runs.append((its_all, dU_all))
        S.close()
    assert runs[0][0] == runs[1][0], f"Newton iterations: dense {runs[0][0]} vs device GMRES {runs[1][0]}"
    for s_ in range(nsteps):
        assert_close(runs[1][1][s_], runs[0][1][s_], 1e-8, f"step {s_}: converged dU", scale=np.abs(runs[0][1][s_]).max())


@pytest.mark.parametrize("law", ["neo-hookean", "drucker-prager"])
def test_full_size(law):
    """The bench cube at 1 M particles after one fused residual, rtol 1e-8, PBJACOBI: the true residual recomputed
    with tangent_apply, and the workspace bytes of the header's formula."""
    import os
    import sys
    import torch
    from util import ROOT, synth
    sys.path.insert(0, ROOT)
    import bench
    n = nlps()
    case = bench.build_case(0, 1, 50)
    if law == "drucker-prager":
        case["materials"] = [synth.drucker_prager_material()]
    nsteps = 2
    bcs = n.BccSet([dirichlet_plane(case, 2, case["block_lo"][2], nsteps)])
    S = gpu_setup(case, nsteps=nsteps)
    S.local_search()
    S.active_masks(bcs, 0)
    Mv = S.compute_nodal_lumped_mass()
    V, A = S.get_nodal_field_n(Mv)
    na = S.nactive
    ntot = na * 3
    a = newmark_parameters(0.25, 0.5, 1.0e-3)
    alpha = [a["a1"], a["a2"], a["a3"], a["a4"], a["a5"], a["a6"]]
    rng = np.random.default_rng(11)
    S.lagrangian_evaluation(1e-4 * rng.normal(size=ntot), V, A, Mv, alpha, [0.0, 0.0, -9.81])
    S.tangent_operator(a["a1"], Mv, True)
    b = torch.from_numpy(rng.normal(size=ntot)).cuda()
    restart = 30
    x, info = S.tangent_solve(b, pc="pbjacobi", restart=restart, rtol=1e-8, max_it=3000)
    assert info["reason"] > 0, info
    r = b - S.tangent_apply(x)
    rn = float(torch.linalg.norm(r))
    assert rn <= 1.01e-8 * info["bnorm"], f"true residual {rn:.3e} vs bnorm {info['bnorm']:.3e}"
    assert abs(rn - info["rnorm"]) <= 1e-6 * info["bnorm"] * 1e-8 + 1e-3 * rn
    nb = (ntot + 511) // 512
    m = restart
    expect = 8 * ((m + 3) * ntot + (m + 2) * nb + 6 * (m + 2) + 8 + m * (m + 1) + na * 9)
    assert info["bytes"] == expect, f"bytes {info['bytes']} vs the header's formula {expect}"
    S.close()
