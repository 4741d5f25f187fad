"""Device Lanczos on the matrix-free tangent (nlps_gpu_tangent_lambda_max) and nlps_host_critical_dt: the iteration against
the numpy reference of the same algorithm (tests/lanczos_ref.py) on the device-assembled K, theta against dense
eigenvalues, the mode, the call contract, and the bench cube at 1 M particles."""
import numpy as np
import pytest

import lanczos_ref
from test_gpu_tangent_operator import _coo_dense, _linearised
from util import assert_close, dirichlet_plane, gpu_setup, make_case, nlps

pytestmark = pytest.mark.gpu

CASES = [(2, "neo-hookean"), (3, "neo-hookean"), (3, "hencky"), (3, "drucker-prager")]
# history (theta_j) against the reference, entry by entry, relative: ten times the largest difference measured on the
# MI355X over every run of test_against_the_reference and test_several_blocks_and_waves (HIST_MEASURED, printed by
# them), and never above the 1e-6 of tests/test_gpu_tangent_solve.py:44
HIST_MEASURED = 9.7e-16
HIST_TOL = min(10 * HIST_MEASURED, 1e-6)
EPS = 2.220446049250313e-16  # the dense eigenvalue itself is good to n eps ||A||: the lower side of the bracket allows that


def _operator(s, alpha_1=0.0, dirichlet=True):
    """The operator on the device, its dense K, and the fixed mask the call projects with."""
    S, na = s["S"], s["na"]
    n = na * S.ndim
    mass = s["Mv"] if alpha_1 != 0.0 else None
    K = _coo_dense(S, n, alpha_1, mass, dirichlet)
    S.tangent_operator(alpha_1, mass, dirichlet)
    fixed = (s["d2m"] == -1) if dirichlet else np.zeros(n, dtype=bool)
    return K, fixed


def _hist_err(info, ref):
    k = min(len(info["history"]), len(ref["history"]))
    return float((np.abs(info["history"][:k] - ref["history"][:k]) / np.abs(ref["history"][:k])).max())


def _check_reference(info, ref, what):
    assert info["reason"] == ref["reason"], f"{what}: reason {info['reason']} vs reference {ref['reason']}"
    assert abs(info["iterations"] - ref["iterations"]) <= 1, f"{what}: iterations {info['iterations']} vs {ref['iterations']}"
    assert len(info["history"]) == info["iterations"]
    err = _hist_err(info, ref)
    print(f"{what}: {info['iterations']} steps, history vs reference {err:.3e}, theta {info['theta']:.9e}, "
          f"resid {info['resid']:.3e}, asymmetry {info['asymmetry']:.3e} (reference {ref['asymmetry']:.3e})")
    assert err <= HIST_TOL, f"{what}: history vs reference, relative {err:.3e}"


def _free_block(K, Mv, fixed):
    A, _ = lanczos_ref.scaled_operator(K, Mv, fixed)
    return A[np.ix_(~fixed, ~fixed)]


def _dense_resid(K, Mv, fixed, mode, theta):
    A, ps = lanczos_ref.scaled_operator(K, Mv, fixed)
    y = np.where(ps != 0.0, mode * np.sqrt(Mv), 0.0)
    return float(np.linalg.norm(A @ y - theta * y))


@pytest.mark.parametrize("ndim,law", CASES)
def test_against_the_reference(ndim, law):
    """Hash start and a caller's v0, host and device pointers: reason, iterations within one, the history entry by entry."""
    import torch
    s = _linearised(ndim, law, with_oracle=False)
    S, Mv = s["S"], s["Mv"]
    K, fixed = _operator(s)
    n = K.shape[0]
    v0 = s["rng"].normal(size=n)
    Md = torch.from_numpy(np.ascontiguousarray(Mv)).cuda()
    for start, v in (("hash", None), ("v0", v0)):
        ref = lanczos_ref.lanczos(K, Mv, fixed, v0=v, seed=5, max_it=60, rtol=1e-8)
        assert ref["reason"] == lanczos_ref.CONVERGED
        for where in ("host", "device"):
            what = f"{law} {ndim}-D {start} {where}"
            if where == "host":
                v_in = None if v is None else v.copy()
                info = S.tangent_lambda_max(Mv, v0=v_in, seed=5, max_it=60, rtol=1e-8, mode=True, history=True)
                assert isinstance(info["mode"], np.ndarray)
                assert v is None or np.array_equal(v_in, v), "v0 is not touched"
                mode = info["mode"]
            else:
                vd = None if v is None else torch.from_numpy(v).cuda()
                info = S.tangent_lambda_max(Md, v0=vd, seed=5, max_it=60, rtol=1e-8, mode=True, history=True)
                assert isinstance(info["mode"], torch.Tensor) and info["mode"].is_cuda
                mode = info["mode"].cpu().numpy()
            _check_reference(info, ref, what)
            if info["iterations"] == ref["iterations"]:
                sign = 1.0 if mode @ (Mv * ref["mode"]) > 0 else -1.0
                assert_close(sign * mode, ref["mode"], 1e-6, f"{what}: mode vs reference", scale=np.abs(ref["mode"]).max())
    S.close()


@pytest.mark.parametrize("ndim,law", CASES)
def test_against_dense_eigenvalues(ndim, law):
    s = _linearised(ndim, law, with_oracle=False)
    S, Mv = s["S"], s["Mv"]
    K, fixed = _operator(s)
    Aff = _free_block(K, Mv, fixed)
    ref = lanczos_ref.lanczos(K, Mv, fixed, seed=0, max_it=60, rtol=1e-8)
    info = S.tangent_lambda_max(Mv, seed=0, max_it=60, rtol=1e-8, mode=True)
    theta, mode = info["theta"], info["mode"]
    assert info["reason"] == 1 and info["reason_name"] == "converged"
    # the mode: 0 on the fixed dofs, M-normalised and, for a symmetric tangent, its Rayleigh quotient through an independent
    # product (the symmetric recurrence of an unsymmetric A does not keep y . A y = theta)
    assert fixed.any() and not mode[fixed].any(), "exactly 0 on the fixed dofs"
    assert abs(mode @ (Mv * mode) - 1.0) <= 1e-12
    rd = _dense_resid(K, Mv, fixed, mode, theta)
    if law == "neo-hookean":
        rq = (mode @ S.tangent_apply(mode)) / (mode @ (Mv * mode))
        assert abs(rq - theta) <= 1e-10 * abs(theta), f"Rayleigh quotient {rq:.15e} vs theta {theta:.15e}"
        lam = np.linalg.eigvalsh(0.5 * (Aff + Aff.T))[-1]
        print(f"{law} {ndim}-D: lambda_max {lam:.12e}, lambda_max - theta {lam - theta:.3e}, resid {info['resid']:.3e} "
              f"(dense {rd:.3e}), asymmetry {info['asymmetry']:.3e} (reference {ref['asymmetry']:.3e}), "
              f"critical dt {nlps().critical_dt(theta + info['resid'], safety=1.0):.4e}")
        assert -EPS * len(Aff) * lam <= lam - theta <= info["resid"] + 1e-12 * lam
        assert abs(info["resid"] - rd) <= 1e-2 * rd + 1e-13 * lam
        assert info["asymmetry"] <= min(100 * ref["asymmetry"], 1e-8)
    else:
        lam = np.linalg.eigvals(Aff).real.max()
        print(f"{law} {ndim}-D: max Re eig {lam:.12e}, theta - . {theta - lam:.3e} (reference {ref['theta'] - lam:.3e}), "
              f"asymmetry {info['asymmetry']:.3e} (reference {ref['asymmetry']:.3e})")
        assert abs(theta - lam) <= 10 * abs(ref["theta"] - lam)
        assert ref["asymmetry"] / 10 <= info["asymmetry"] <= 10 * ref["asymmetry"] and info["asymmetry"] > 1e-6
    S.close()


def test_several_blocks_and_waves():
    """More than three blocks of 512 dofs (and not a multiple of 512) and a T of 80 rows, more than the 64 lanes of the
    Ritz kernel: every history entry, theta, resid and the mode against the reference."""
    case = make_case(2, [40, 30], [3, 3], [32, 20])  # (a block of 30 x 20 cells activates 759 nodes: 1518 dofs, short of 1536)
    n = nlps()
    nsteps = 2
    S = gpu_setup(case, nsteps=nsteps)
    S.local_search()
    _, d2m = S.active_masks(n.BccSet([dirichlet_plane(case, 1, 3, nsteps)]), 1)
    ntot = S.nactive * 2
    assert ntot > 1536 and ntot % 512 != 0
    S.local_compatibility_conditions(2e-2 * np.random.default_rng(3).normal(size=ntot))
    S.constitutive_update()
    Mv = S.compute_nodal_lumped_mass()
    K = _coo_dense(S, ntot, 0.0, None, True)
    S.tangent_operator(0.0, None, True)
    fixed = d2m == -1
    ref = lanczos_ref.lanczos(K, Mv, fixed, seed=1, max_it=80, rtol=0.0)
    info = S.tangent_lambda_max(Mv, seed=1, max_it=80, rtol=0.0, mode=True, history=True)
    assert info["iterations"] == 80 and info["reason"] == -3 and ref["iterations"] == 80
    _check_reference(info, ref, f"2-D, {ntot} dofs, 80 steps")
    lam = np.linalg.eigvalsh(_free_block(K, Mv, fixed))
    assert abs(info["theta"] - ref["theta"]) <= HIST_TOL * ref["theta"]
    assert -EPS * len(lam) * lam[-1] <= lam[-1] - info["theta"] <= info["resid"] + 1e-12 * lam[-1]
    assert abs(info["resid"] - ref["resid"]) <= 1e-2 * ref["resid"] + 1e-12 * lam[-1]
    # the Ritz vector moves with rounding over the relative gap to the next eigenvalue
    gap = (lam[-1] - lam[-2]) / lam[-1]
    tol = min(80 * 1e-15 / gap + 2 * ref["resid"] / (gap * lam[-1]), 1e-6)
    mode = info["mode"]
    sign = 1.0 if mode @ (Mv * ref["mode"]) > 0 else -1.0
    print(f"relative gap {gap:.3e}, mode tolerance {tol:.3e}, difference {np.abs(sign * mode - ref['mode']).max() / np.abs(ref['mode']).max():.3e}")
    assert_close(sign * mode, ref["mode"], tol, "mode vs reference", scale=np.abs(ref["mode"]).max())
    assert not mode[fixed].any()
    S.close()


def test_alpha_1_shift_and_dirichlet_off():
    s = _linearised(3, "neo-hookean", with_oracle=False)
    S, Mv = s["S"], s["Mv"]
    Ka, _ = _operator(s, alpha_1=4.0e4)
    a = S.tangent_lambda_max(Mv, max_it=60, rtol=1e-8)
    # the workspace is the solve's: a solve between two calls disturbs neither
    rhs = s["rng"].normal(size=len(Ka))
    x, ik = S.tangent_solve(rhs, pc="pbjacobi", rtol=1e-10, max_it=2000)
    assert ik["reason"] > 0
    assert_close(x, np.linalg.solve(Ka, rhs), 1e-6, "a solve after the Lanczos call", scale=np.abs(x).max())
    a2 = S.tangent_lambda_max(Mv, max_it=60, rtol=1e-8)
    assert a2["iterations"] == a["iterations"] and abs(a2["theta"] - a["theta"]) <= 1e-13 * a["theta"]
    _operator(s)
    b = S.tangent_lambda_max(Mv, max_it=60, rtol=1e-8)
    assert a["reason"] == 1 and b["reason"] == 1
    assert abs(a["theta"] - b["theta"] - 4.0e4) <= a["resid"] + b["resid"] + 1e-12 * a["theta"], (a, b)
    # apply_dirichlet = 0: P = I, the full pencil
    K, fixed = _operator(s, dirichlet=False)
    assert not fixed.any()
    c = S.tangent_lambda_max(Mv, max_it=60, rtol=1e-8, mode=True)
    lam = np.linalg.eigvalsh(_free_block(K, Mv, fixed))[-1]
    assert c["reason"] == 1 and -EPS * len(K) * lam <= lam - c["theta"] <= c["resid"] + 1e-12 * lam
    floor = s["d2m"] == -1
    assert np.abs(c["mode"][floor]).max() > 0.0, "the mode lives on the floor too"
    assert abs(c["mode"] @ (Mv * c["mode"]) - 1.0) <= 1e-12
    S.close()


def test_deterministic_mode_repeats_bit_for_bit():
    runs = []
    for _ in range(2):
        n = nlps()
        case = make_case(3, [8, 8, 7], [3, 3, 2], [2, 2, 2], velocity=[1.0, -2.0, 0.5])
        S = gpu_setup(case, nsteps=2)
        S.set_deterministic(True)
        S.local_search()
        S.active_masks(n.BccSet([dirichlet_plane(case, 2, 3, 2)]), 1)
        ntot = S.nactive * 3
        S.local_compatibility_conditions(2e-2 * np.random.default_rng(13).normal(size=ntot))
        S.constitutive_update()
        Mv = S.compute_nodal_lumped_mass()
        S.tangent_operator(0.0, None, True)
        for _ in range(2):
            runs.append(S.tangent_lambda_max(Mv, seed=2, max_it=40, rtol=1e-8, mode=True, history=True))
        S.close()
    for r in runs[1:]:
        assert r["theta"] == runs[0]["theta"] and r["resid"] == runs[0]["resid"] and r["iterations"] == runs[0]["iterations"]
        assert np.array_equal(r["history"], runs[0]["history"]) and np.array_equal(r["mode"], runs[0]["mode"])
    assert runs[0]["reason"] == 1


def test_refusals_empty_and_workspace():
    n = nlps()
    s = _linearised(2, "neo-hookean", with_oracle=False)
    S, Mv, na = s["S"], s["Mv"], s["na"]
    ntot = na * 2

    def good(what):
        K, fixed = _operator(s)
        ref = lanczos_ref.lanczos(K, Mv, fixed, seed=9, max_it=60, rtol=1e-8)
        _check_reference(S.tangent_lambda_max(Mv, seed=9, max_it=60, rtol=1e-8, history=True), ref, "after " + what)
        return K, fixed

    with pytest.raises(n.NlpsError, match="nlps_gpu_tangent_lambda_max: call nlps_gpu_tangent_operator\\(\\) first"):
        S.tangent_lambda_max(Mv)
    K, fixed = good("no operator")
    with pytest.raises(n.NlpsError, match="lumped_mass is required"):
        S.tangent_lambda_max(None)
    for max_it in (0, 257):
        with pytest.raises(n.NlpsError, match="max_it must be 1"):
            S.tangent_lambda_max(Mv, max_it=max_it)
    with pytest.raises(n.NlpsError, match="rtol must be >= 0"):
        S.tangent_lambda_max(Mv, rtol=-1.0)
    S.L.nlps_gpu_tangent_lambda_max.restype = int
    assert S.L.nlps_gpu_tangent_lambda_max(S.h, n._vp(Mv), None, None, None) == 1
    assert b"eig is required" in S.L.nlps_gpu_last_error(S.h)
    good("the argument refusals")
    free_node = int(np.flatnonzero(~fixed)[0]) // 2
    for value in (0.0, -1.0, np.nan, np.inf):
        bad = Mv.copy()
        bad[free_node * 2 + 1] = value
        with pytest.raises(n.NlpsError, match=f"lumped mass of masked node {free_node} "):
            S.tangent_lambda_max(bad)
    bad = Mv.copy()
    bad[fixed] = -1.0  # (the mass of a fixed dof is not read)
    assert S.tangent_lambda_max(bad, seed=9, max_it=60, rtol=1e-8)["reason"] == 1
    good("a bad mass")
    S.local_search()
    with pytest.raises(n.NlpsError, match="stale: .*nlps_gpu_local_search"):
        S.tangent_lambda_max(Mv)
    bcs = n.BccSet([dirichlet_plane(make_case(2, [12, 11], [3, 3], [5, 4]), 1, 3, 2)])
    S.active_masks(bcs, 1)
    S.tangent_operator(0.0, None, True)
    S.set_halo_exchange(lambda dptr, nfield, elem, kind: 0)
    with pytest.raises(n.NlpsError, match="single rank only"):
        S.tangent_lambda_max(Mv)
    S.set_halo_exchange(None)
    K, fixed = good("the stale operator and the halo handle")
    # max_it = 1: theta = alpha_1 = q_1 . A q_1, not converged
    one = S.tangent_lambda_max(Mv, seed=9, max_it=1, rtol=1e-8, history=True, mode=True)
    ref = lanczos_ref.lanczos(K, Mv, fixed, seed=9, max_it=1, rtol=1e-8)
    assert one["reason"] == -3 and one["iterations"] == 1 and abs(one["theta"] - ref["theta"]) <= 1e-12 * ref["theta"]
    assert abs(one["resid"] - ref["resid"]) <= 1e-10 * ref["resid"]
    # the workspace only grows: a smaller call after a larger one reports its own bytes, by the formula
    for max_it in (200, 3):
        r = S.tangent_lambda_max(Mv, max_it=max_it, rtol=0.0)
        assert r["iterations"] == max_it
        nb, nbg = (ntot + 511) // 512, (S.nnodes + 255) // 256
        assert r["bytes"] == 8 * ((max_it + 4) * ntot + (max_it + 2) * nb + nbg + 5 * (max_it + 2) + 8)
    good("a larger workspace")
    # P v0 == 0 and a cloud whose every active dof is fixed: EMPTY, no iteration
    v0 = np.zeros(ntot)
    v0[fixed] = 1.0
    e = S.tangent_lambda_max(Mv, v0=v0, mode=True)
    assert e["reason"] == 2 and e["reason_name"] == "empty" and e["iterations"] == 0 and not e["mode"].any()
    # a non-finite start vector: the call succeeds and says so, nothing is iterated
    v0 = np.ones(ntot)
    v0[np.flatnonzero(~fixed)[3]] = np.nan
    e = S.tangent_lambda_max(Mv, v0=v0, mode=True)
    r = lanczos_ref.lanczos(K, Mv, fixed, v0=v0)
    assert e["reason"] == r["reason"] == -9 and e["reason_name"] == "diverged_nanorinf" and e["iterations"] == 0
    assert np.isnan(e["resid"]) and not e["mode"].any()
    good("a non-finite start vector")
    case = make_case(2, [12, 11], [3, 3], [5, 4])
    all_nodes = {"nodes": np.arange(int(np.prod(case["grid_n"])), dtype=np.int32), "dim": 2,
                 "dir": np.ones((2, 2), dtype=np.int32), "value": np.zeros((2, 2))}
    S.active_masks(n.BccSet([all_nodes]), 1)
    assert S.nfree == 0
    S.tangent_operator(0.0, None, True)
    e = S.tangent_lambda_max(S.compute_nodal_lumped_mass())
    assert e["reason"] == 2 and e["iterations"] == 0 and e["theta"] == 0.0
    S.close()


def test_host_critical_dt():
    n = nlps()
    assert n.critical_dt(4.0, gamma=0.5, safety=1.0) == 1.0  # 2 / omega
    assert n.critical_dt(3.01e4, gamma=0.5, safety=1.0) == pytest.approx(2.0 / np.sqrt(3.01e4), rel=1e-15)
    assert n.critical_dt(4.0) == pytest.approx(0.9, rel=1e-15)
    assert n.critical_dt(4.0, gamma=0.75, safety=1.0) == pytest.approx(np.sqrt(2.0 / 0.75) / 2.0, rel=1e-15)
    assert n.critical_dt(0.0) == np.inf and n.critical_dt(-3.0) == np.inf
    assert n.critical_dt(4.0, gamma=0.49) == -1.0 and n.critical_dt(-1.0, gamma=0.0) == -1.0


def test_full_size():
    """The bench cube at 1 M particles, Neo-Hookean, floor fixed, 12 steps."""
    import sys
    import torch
    from util import ROOT
    sys.path.insert(0, ROOT)
    import bench
    n = nlps()
    case = bench.build_case(0, 1, 50)
    nsteps = 2
    S = gpu_setup(case, nsteps=nsteps)
    S.local_search()
    S.active_masks(n.BccSet([dirichlet_plane(case, 2, case["block_lo"][2], nsteps)]), 0)
    Mv = torch.from_numpy(S.compute_nodal_lumped_mass()).cuda()
    ntot = S.nactive * 3
    S.local_compatibility_conditions(np.zeros(ntot))
    S.constitutive_update()
    S.tangent_operator(0.0, None, True)
    assert S.num_particles() == 1000000
    info = S.tangent_lambda_max(Mv, max_it=12, rtol=0.0, mode=True, history=True)
    assert info["iterations"] == 12 and info["reason"] == -3
    theta, mode = info["theta"], info["mode"]
    assert np.all(np.diff(info["history"]) >= -1e-13 * theta), info["history"]
    rq = float((mode @ S.tangent_apply(mode)) / (mode @ (Mv * mode)))
    assert abs(rq - theta) <= 1e-10 * theta, f"Rayleigh quotient {rq:.15e} vs theta {theta:.15e}"
    nnodes = int(np.prod(case["grid_n"]))
    nb, nbg = (ntot + 511) // 512, (nnodes + 255) // 256
    assert info["bytes"] == 8 * ((12 + 4) * ntot + (12 + 2) * nb + nbg + 5 * (12 + 2) + 8), "bytes vs the header's formula"
    mat = case["materials"][0]
    lame = mat["E"] * mat["nu"] / ((1 + mat["nu"]) * (1 - 2 * mat["nu"]))
    G = mat["E"] / (2 * (1 + mat["nu"]))
    rho = float(np.asarray(case["cloud"]["rho"]).ravel()[0]) if "rho" in case["cloud"] else float("nan")
    print(f"1 M particles: theta {theta:.6e}, resid {info['resid']:.3e}, asymmetry {info['asymmetry']:.3e}, "
          f"critical_dt(theta + resid) {n.critical_dt(theta + info['resid']):.4e}, "
          f"courant_dt(1, h, sqrt((lambda + 2 G) / rho)) {n.courant_dt(1.0, case['h'], np.sqrt((lame + 2 * G) / rho)):.4e}")
    S.close()
