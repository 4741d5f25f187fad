"""Device MINRES on the matrix-free tangent (nlps_gpu_set_linear_solver + nlps_gpu_tangent_solve) against the numpy
statement of the same algorithm (tests/minres_ref.py) on the dense matrix of the device's own COO, and against a dense
solve.  tests/minres_cases.py describes the cases; tests/test_minres_ref.py holds, on the CPU oracle's matrices, the
conditions these comparisons rest on (the iteration-count margins, the GMRES gap, the indefinite tangent)."""
import numpy as np
import pytest

import krylov_ref
import minres_cases as mc
import minres_ref
import snes_ref
import solver_exit_cases as sx
from test_gpu_newton_solve import TIGHT, _alpha, _check_state, _problem, _same_counts, _Step
from test_gpu_tangent_operator import LAWS, _case, _coo_dense, _linearised
from util import assert_close, dirichlet_plane, gpu_setup, make_case, nlps

pytestmark = pytest.mark.gpu

NHK = "neo-hookean"


def _operator(s, alpha_1, ndim):
    """The operator (alpha_1 M, Dirichlet on) on the device and as the dense matrix of the device's COO."""
    S, na = s["S"], s["na"]
    mass = s["Mv"] if alpha_1 != 0.0 else None
    K = _coo_dense(S, na * ndim, alpha_1, mass, True)
    S.tangent_operator(alpha_1, mass, True)
    return K


def _reference(K, b, pc, ndim, **kw):
    return minres_ref.minres(K, b, krylov_ref.preconditioner(K, pc, ndim), **kw)


def _check_rnorm(K, b, x, info, what):
    r_dense = np.linalg.norm(b - K @ x)
    assert abs(info["bnorm"] - np.linalg.norm(b)) <= 1e-12 * np.linalg.norm(b)
    assert abs(info["rnorm"] - r_dense) <= 1e-2 * r_dense + 1e-13 * np.linalg.norm(b), \
        f"{what}: rnorm {info['rnorm']:.6e} vs the dense ||b - K x|| {r_dense:.6e}"


def _check_history(info, ref, what):
    assert len(info["history"]) == info["iterations"] + 1
    err = mc.history_error(info["history"], ref["history"])
    assert err <= 1e-6, f"{what}: history vs reference, relative {err:.3e}:\n{info['history'][:10]}\n{ref['history'][:10]}"


# ------------------------------------------------------------------------------------------------ 1. dense solve
@pytest.mark.parametrize("ndim", [2, 3])
def test_against_a_dense_solve_and_the_reference(ndim):
    c = mc.DENSE
    s = _linearised(ndim, NHK, with_oracle=False)
    S, na = s["S"], s["na"]
    S.set_linear_solver("minres")
    K = _operator(s, c["alpha_1"], ndim)
    b = mc.rhs(na * ndim, c["seed"])
    xs = np.linalg.solve(K, b)
    for pc in mc.PCS:
        what = f"{ndim}-D pc={pc}"
        kw = dict(rtol=c["rtol"], max_it=c["max_it"][pc])
        x, info = S.tangent_solve(b, pc=pc, history=True, **kw)
        xr, ir = _reference(K, b, pc, ndim, **kw)
        print(what, info["iterations"], info["reason_name"], info["rnorm"] / info["bnorm"], "reference", ir["iterations"])
        assert_close(x, xs, 1e-6, f"{what}: x vs np.linalg.solve", scale=np.abs(xs).max())
        _check_rnorm(K, b, x, info, what)
        assert info["reason"] == ir["reason"], f"{what}: reason {info['reason_name']} vs reference {ir['reason']}"
        assert abs(info["iterations"] - ir["iterations"]) <= 1, f"{what}: {info['iterations']} vs {ir['iterations']}"
        _check_history(info, ir, what)
        if pc != "none":
            assert info["reason"] == minres_ref.CONVERGED_RTOL and info["rnorm"] <= c["rtol"] * info["bnorm"]
    S.close()


# ------------------------------------------------------------------------------------------------ 2. the GMRES gap
@pytest.mark.parametrize("pc", mc.GAP["pcs"])
def test_converges_where_gmres30_does_not(pc):
    c = mc.GAP
    s = _linearised(3, NHK, with_oracle=False)
    S, na = s["S"], s["na"]
    K = _operator(s, c["alpha_1"], 3)
    b = mc.rhs(na * 3, c["seed"])
    S.set_linear_solver("minres")
    x, info = S.tangent_solve(b, pc=pc, rtol=c["rtol"], max_it=2000, history=True)
    xr, ir = _reference(K, b, pc, 3, rtol=c["rtol"], max_it=2000)
    print(f"gap {pc}: device {info['iterations']} reference {ir['iterations']} confirmations {ir['confirmations']}")
    assert info["reason"] == minres_ref.CONVERGED_RTOL == ir["reason"], info
    assert info["iterations"] <= ir["iterations"] + c["margin"], (info["iterations"], ir["iterations"])
    _check_rnorm(K, b, x, info, f"gap {pc}")
    assert np.linalg.norm(b - K @ x) <= 1.01 * c["rtol"] * np.linalg.norm(b)
    _check_history(info, ir, f"gap {pc}")
    S.set_linear_solver("gmres")
    xg, ig = S.tangent_solve(b, pc=pc, restart=30, rtol=c["rtol"], max_it=2 * info["iterations"])
    assert ig["reason"] == krylov_ref.DIVERGED_ITS and ig["iterations"] == 2 * info["iterations"], ig
    S.close()


# ------------------------------------------------------------------------------------------------ 3. indefinite K
@pytest.mark.parametrize("pc", mc.INDEFINITE["pcs"])
def test_indefinite_quasi_static_tangent(pc):
    c = mc.INDEFINITE
    s = _linearised(3, NHK, with_oracle=False)
    S, na = s["S"], s["na"]
    K = _operator(s, c["alpha_1"], 3)
    assert np.linalg.eigvalsh(0.5 * (K + K.T))[0] < -1e-3, "the device's matrix is indefinite too"
    b = K @ mc.rhs(na * 3, c["seed"])
    S.set_linear_solver("minres")
    x, info = S.tangent_solve(b, pc=pc, rtol=c["rtol"], max_it=3000, history=True)
    xr, ir = _reference(K, b, pc, 3, rtol=c["rtol"], max_it=3000)
    print(f"indefinite {pc}: device {info['iterations']} reference {ir['iterations']}")
    assert info["reason"] == minres_ref.CONVERGED_RTOL == ir["reason"], info
    assert abs(info["iterations"] - ir["iterations"]) <= c["margin"], (info["iterations"], ir["iterations"])
    r_dense = np.linalg.norm(b - K @ x)
    assert r_dense <= 1.01e-5 * np.linalg.norm(b)
    _check_rnorm(K, b, x, info, f"indefinite {pc}")
    S.close()


# ------------------------------------------------------------------------------------------------ 4. several tiles
def test_several_tiles_with_a_ragged_tail():
    c = mc.WIDE
    s = sx.wide_device()
    S, na = s["S"], s["na"]
    n = na * 2
    assert n == 1610 == 3 * 512 + 74
    K = _operator(s, c["alpha_1"], 2)
    b = mc.rhs(n, c["seed"])
    xs = np.linalg.solve(K, b)
    S.set_linear_solver("minres")
    for pc in c["pcs"]:
        x, info = S.tangent_solve(b, pc=pc, rtol=c["rtol"], max_it=3000, history=True)
        xr, ir = _reference(K, b, pc, 2, rtol=c["rtol"], max_it=3000)
        print(f"wide {pc}: device {info['iterations']} reference {ir['iterations']}")
        assert info["reason"] == minres_ref.CONVERGED_RTOL == ir["reason"], info
        assert abs(info["iterations"] - ir["iterations"]) <= c["margin"], (info["iterations"], ir["iterations"])
        assert abs(ir["iterations"] - c["counts"][pc]) <= c["margin"], ir["iterations"]
        assert_close(x, xs, 1e-6, f"wide {pc}: x vs np.linalg.solve", scale=np.abs(xs).max())
        _check_rnorm(K, b, x, info, f"wide {pc}")
        _check_history(info, ir, f"wide {pc}")
    S.close()


# ------------------------------------------------------------------------------------------------ 5. the contract
def test_contract():
    import torch
    s = _linearised(3, NHK, with_oracle=False)
    S, na = s["S"], s["na"]
    n = na * 3
    S.set_linear_solver("minres")
    K = _operator(s, mc.ALPHA_DYNAMIC, 3)
    rng = np.random.default_rng(77)
    b = rng.normal(size=n)
    b0 = b.copy()
    xs = np.linalg.solve(K, b)
    x_h, info_h = S.tangent_solve(b, rtol=1e-10, history=True)
    assert np.array_equal(b, b0), "b is not touched"
    assert info_h["reason"] == minres_ref.CONVERGED_RTOL and info_h["iterations"] > 0
    assert_close(x_h, xs, 1e-6, "host vectors", scale=np.abs(xs).max())
    bd = torch.from_numpy(b).cuda()
    x_d, info_d = S.tangent_solve(bd, rtol=1e-10, history=True)
    assert isinstance(x_d, torch.Tensor) and x_d.is_cuda
    assert info_d["iterations"] == info_h["iterations"]
    assert_close(x_d.cpu().numpy(), x_h, 1e-9, "device vs host x", scale=np.abs(x_h).max())
    out = torch.full((n,), 3.0, dtype=torch.float64, device="cuda")
    r, _ = S.tangent_solve(bd, rtol=1e-10, out=out)
    assert r is out
    # restart is not read
    x_r, info_r = S.tangent_solve(b, rtol=1e-10, restart=0)
    assert info_r["iterations"] == info_h["iterations"]
    # the exact solution as the guess: no step
    xg, ig = S.tangent_solve(b, x=xs, rtol=1e-8)
    assert ig["iterations"] == 0 and ig["reason"] == minres_ref.CONVERGED_RTOL, ig
    assert_close(xg, xs, 1e-12, "guess returned as it is", scale=np.abs(xs).max())
    # a rough guess: the reference from the same guess
    x0 = xs * (1.0 + 1e-3 * rng.normal(size=n))
    xq, iq = S.tangent_solve(b, x=x0, pc="jacobi", rtol=1e-10, history=True)
    xr, ir = _reference(K, b, "jacobi", 3, rtol=1e-10, x0=x0)
    assert iq["reason"] == ir["reason"] and abs(iq["iterations"] - ir["iterations"]) <= 1
    assert_close(xq, xs, 1e-6, "from a guess", scale=np.abs(xs).max())
    # b = 0: x = 0, even over a guess
    xz, iz = S.tangent_solve(np.zeros(n), x=xs)
    assert iz["reason"] == minres_ref.CONVERGED_BZERO and iz["iterations"] == 0 and not xz.any()
    # max_it too small: the call succeeds, the reason says it did not converge
    xm, im = S.tangent_solve(b, rtol=1e-12, max_it=2, history=True)
    assert im["reason"] == minres_ref.DIVERGED_ITS and im["iterations"] == 2 and len(im["history"]) == 3, im
    assert im["rnorm"] > 1e-12 * im["bnorm"] and np.isfinite(xm).all()
    _check_rnorm(K, b, xm, im, "max_it = 2")
    # two right-hand sides on one linearisation (the preconditioner is reused)
    for _ in range(2):
        b2 = rng.normal(size=n)
        x2, i2 = S.tangent_solve(b2, rtol=1e-10)
        assert i2["reason"] > 0
        x2s = np.linalg.solve(K, b2)
        assert_close(x2, x2s, 1e-6, "second right-hand side", scale=np.abs(x2s).max())
    # bytes: the header's formula, below GMRES(30)'s
    nb, nbn = (n + 511) // 512, (na + 255) // 256
    for pc, npc in (("none", 0), ("jacobi", na * 9), ("pbjacobi", na * 9)):
        _, i3 = S.tangent_solve(b, pc=pc, rtol=1e-3, max_it=5)
        expect = 8 * (7 * n + nb + nbn + 16 + npc)
        assert i3["bytes"] == expect, f"bytes {i3['bytes']} vs the header's formula {expect}"
    S.set_linear_solver("gmres")
    _, i4 = S.tangent_solve(b, pc="pbjacobi", restart=30, rtol=1e-3)
    assert i3["bytes"] < i4["bytes"] == 8 * (33 * n + 32 * nb + 6 * 32 + 8 + 30 * 31 + na * 9)
    S.close()


def test_relinearised_operator_follows_the_new_matrix():
    s = _linearised(3, NHK, with_oracle=False)
    S, na = s["S"], s["na"]
    n = na * 3
    S.set_linear_solver("minres")
    K1 = _operator(s, mc.ALPHA_DYNAMIC, 3)
    b = mc.rhs(n, 19)
    x1, i1 = S.tangent_solve(b, pc="pbjacobi", rtol=1e-8, history=True)
    _, r1 = _reference(K1, b, "pbjacobi", 3, rtol=1e-8)
    assert i1["reason"] == r1["reason"] and abs(i1["iterations"] - r1["iterations"]) <= 1
    _check_history(i1, r1, "first linearisation")
    S.local_compatibility_conditions(0.1 * s["rng"].normal(size=n))  # (a large step: other blocks)
    S.constitutive_update()
    K2 = _operator(s, 1.0e3, 3)
    assert np.abs(K2 - K1).max() > 1e-3 * np.abs(K1).max()
    for pc in ("pbjacobi", "jacobi"):
        x2, i2 = S.tangent_solve(b, pc=pc, rtol=1e-8, history=True)
        _, r2 = _reference(K2, b, pc, 3, rtol=1e-8)
        assert i2["reason"] == r2["reason"] > 0 and abs(i2["iterations"] - r2["iterations"]) <= 1, (i2, r2["iterations"])
        _check_history(i2, r2, f"second linearisation, {pc}")
        x2s = np.linalg.solve(K2, b)
        assert_close(x2, x2s, 1e-5, f"second linearisation, {pc}: x", scale=np.abs(x2s).max())
    S.close()


# ------------------------------------------------------------------------------------------------ 6. the exits
def test_exits_and_the_handle_after_them():
    s = _linearised(3, NHK, with_oracle=False)
    S, na, d2m = s["S"], s["na"], s["d2m"]
    n = na * 3
    S.set_linear_solver("minres")
    K = _operator(s, mc.ALPHA_DYNAMIC, 3)
    b = mc.rhs(n, 3)
    xs = np.linalg.solve(K, b)

    def good(after):
        x, i = S.tangent_solve(b, pc="jacobi", rtol=1e-10)
        assert i["reason"] == minres_ref.CONVERGED_RTOL, f"after {after}: {i}"
        assert_close(x, xs, 1e-6, f"a good system after {after}", scale=np.abs(xs).max())

    x, i = S.tangent_solve(b, pc="jacobi", rtol=1e-12, atol=2.0 * np.linalg.norm(b), history=True)
    assert i["reason"] == minres_ref.CONVERGED_ATOL and i["iterations"] == 0 and not x.any() and len(i["history"]) == 1
    good("atol")
    x, i = S.tangent_solve(b, pc="jacobi", rtol=1e-12, dtol=0.5)
    assert i["reason"] == minres_ref.DIVERGED_DTOL and i["iterations"] == 0 and i["rnorm"] == i["bnorm"]
    good("dtol")
    for bad in (np.nan, np.inf):
        bb = b.copy()
        bb[n // 2] = bad
        x, i = S.tangent_solve(bb, pc="jacobi")
        assert i["reason"] == minres_ref.DIVERGED_NANORINF and i["iterations"] == 0 and np.isfinite(x).all(), i
        good(f"b with {bad}")
    # a Jacobi preconditioner that is negative on every free dof (nlps_gpu_tangent_operator takes a negative alpha_1)
    Kn = _operator(s, mc.NEGATIVE_ALPHA, 3)
    free = d2m != -1
    assert np.all(np.diag(Kn)[free] < 0.0) and np.all(np.diag(Kn)[~free] == 1.0)
    bf = mc.free_dof_rhs(d2m, mc.SEED_INDEFINITE_PC)
    x, i = S.tangent_solve(bf, pc="jacobi", history=True)
    _, ir = _reference(Kn, bf, "jacobi", 3)
    assert ir["reason"] == minres_ref.DIVERGED_INDEFINITE_PC and ir["iterations"] == 0
    assert i["reason"] == minres_ref.DIVERGED_INDEFINITE_PC and i["reason_name"] == "diverged_indefinite_pc", i
    assert i["iterations"] == 0 and not x.any() and i["rnorm"] == i["bnorm"] and len(i["history"]) == 1
    _operator(s, mc.ALPHA_DYNAMIC, 3)
    good("an indefinite preconditioner")
    S.close()


# ------------------------------------------------------------------------------------------------ 7. refusals
@pytest.mark.parametrize("law,names", [("hencky", "Hencky"), ("drucker-prager", "Drucker-Prager")])
def test_setter_refuses_a_tangent_that_is_not_symmetric(law, names):
    n = nlps()
    s = _linearised(3, law, with_oracle=False)
    S, na = s["S"], s["na"]
    with pytest.raises(n.NlpsError, match=f"nlps_gpu_set_linear_solver: .*this cloud holds {names} "):
        S.set_linear_solver("minres")
    # still on GMRES: restart is read, and the solve is the GMRES one
    K = _operator(s, mc.ALPHA_DYNAMIC, 3)
    b = mc.rhs(na * 3, 3)
    with pytest.raises(n.NlpsError, match="restart"):
        S.tangent_solve(b, restart=0)
    x, info = S.tangent_solve(b, pc="pbjacobi", restart=30, rtol=1e-10, history=True)
    xr, ir = krylov_ref.gmres(K, b, krylov_ref.preconditioner(K, "pbjacobi", 3), restart=30, rtol=1e-10)
    assert info["reason"] == ir["reason"] > 0 and abs(info["iterations"] - ir["iterations"]) <= 1
    assert mc.history_error(info["history"], ir["history"]) <= 1e-6
    S.close()


def test_setter_refuses_a_mixed_cloud_and_an_unknown_type():
    n = nlps()
    case = _case(2, LAWS["drucker-prager"])  # (test_gpu_tangent_bsr.py::test_upper_refused_for_a_mixed_cloud's cloud)
    npart = case["cloud"]["x"].shape[0]
    case["materials"] = [{"type": 0, "E": 2.0e4, "nu": 0.3}, {"type": 1, "E": 1.0e4, "nu": 0.25}, LAWS["drucker-prager"]]
    case["cloud"]["matidx"] = (np.arange(npart) % 3).astype(np.int32)
    S = gpu_setup(case, nsteps=2)
    with pytest.raises(n.NlpsError, match="nlps_gpu_set_linear_solver: .*this cloud holds Neo-Hookean, Hencky, Drucker-Prager "):
        S.set_linear_solver("minres")
    S.local_search()
    S.active_masks(n.BccSet([dirichlet_plane(case, 1, 3, 2)]), 1)
    S.local_compatibility_conditions(8e-3 * np.random.default_rng(5).normal(size=S.nactive * 2))
    S.constitutive_update()
    Mv = S.compute_nodal_lumped_mass()
    Km = _coo_dense(S, S.nactive * 2, mc.ALPHA_DYNAMIC, Mv, True)
    S.tangent_operator(mc.ALPHA_DYNAMIC, Mv, True)
    bm = mc.rhs(S.nactive * 2, 3)
    with pytest.raises(n.NlpsError, match="restart"):
        S.tangent_solve(bm, restart=0)  # (GMRES reads it)
    xm, im = S.tangent_solve(bm, pc="pbjacobi", rtol=1e-10)
    xms = np.linalg.solve(Km, bm)
    assert im["reason"] > 0
    assert_close(xm, xms, 1e-6, "the mixed cloud by GMRES", scale=np.abs(xms).max())
    S.close()
    s = _linearised(2, NHK, with_oracle=False)
    S = s["S"]
    with pytest.raises(ValueError):
        S.set_linear_solver("cg")
    assert S.L.nlps_gpu_set_linear_solver(S.h, 7) == 1
    assert "nlps_gpu_set_linear_solver: type 7 is neither" in S.L.nlps_gpu_last_error(S.h).decode()
    S.set_linear_solver("minres")
    assert S.L.nlps_gpu_set_linear_solver(S.h, -1) == 1
    # the handle is still on MINRES and usable: restart = 0 passes
    K = _operator(s, mc.ALPHA_DYNAMIC, 2)
    b = mc.rhs(s["na"] * 2, 3)
    x, i = S.tangent_solve(b, restart=0, rtol=1e-10)
    xs = np.linalg.solve(K, b)
    assert i["reason"] > 0
    assert_close(x, xs, 1e-6, "after the refusals", scale=np.abs(xs).max())
    S.close()


def test_stale_operator_and_halo_handles_are_refused():
    n = nlps()
    s = _linearised(2, NHK, with_oracle=False)
    S, na, Mv = s["S"], s["na"], s["Mv"]
    S.set_linear_solver("minres")
    b = mc.rhs(na * 2, 3)
    with pytest.raises(n.NlpsError, match="nlps_gpu_tangent_solve: call nlps_gpu_tangent_operator\\(\\) first"):
        S.tangent_solve(b)
    S.tangent_operator(mc.ALPHA_DYNAMIC, Mv, True)
    S.tangent_solve(b)
    with pytest.raises(ValueError):
        S.tangent_solve(b, pc="ilu")
    with pytest.raises(n.NlpsError, match="max_it >= 0"):
        S.tangent_solve(b, max_it=-1)
    with pytest.raises(n.NlpsError, match="rtol and atol must be >= 0"):
        S.tangent_solve(b, rtol=-1.0)
    S.local_search()
    with pytest.raises(n.NlpsError, match="stale: .*nlps_gpu_local_search"):
        S.tangent_solve(b)
    bcs = n.BccSet([dirichlet_plane(make_case(2, [12, 11], [3, 3], [5, 4]), 1, 3, 2)])
    S.active_masks(bcs, 1)
    S.tangent_operator(mc.ALPHA_DYNAMIC, S.compute_nodal_lumped_mass(), True)
    S.set_halo_exchange(lambda dptr, nfield, elem, kind: 0)
    with pytest.raises(n.NlpsError, match="nlps_gpu_tangent_solve: single rank only"):
        S.tangent_solve(np.ones(S.nactive * 2))
    S.set_halo_exchange(None)
    x, i = S.tangent_solve(np.ones(S.nactive * 2))
    assert i["reason"] > 0
    S.close()


# ------------------------------------------------------------------------------------------------ 8. Newton and Newmark
@pytest.mark.parametrize("ndim", [2, 3])
def test_newton_solve_follows_the_selection(ndim):
    """test_gpu_newton_solve.py::test_against_the_dense_newton's first step with MINRES selected: the linear solve at
    1e-12 is as good as the dense one, so the Newton iteration is snes_ref's with a dense solve."""
    case, bcs, gravity, nsteps = _problem(ndim)
    alpha = _alpha(1.0e-2)
    S, S2 = gpu_setup(case, nsteps=nsteps), gpu_setup(case, nsteps=nsteps)
    S.set_linear_solver("minres")
    kw = dict(max_it=12, rtol=1e-10, atol=0.0, stol=0.0)
    dev, ref = _Step(S, bcs, 0, alpha, gravity), _Step(S2, bcs, 0, alpha, gravity)
    dU, info = dev.solve(np.zeros(dev.n), linesearch="basic", ksp=dict(TIGHT, restart=0), **kw)
    xr, ir = snes_ref.newton(ref.residual, ref.tangent, np.zeros(ref.n), linesearch="basic", linear="dense", **kw)
    print("device", info["fnorm_history"], info["ksp_iterations"], "reference", ir["fnorm_history"])
    assert info["reason"] == snes_ref.CONVERGED_FNORM_RELATIVE and info["iterations"] >= 2, info
    _same_counts(info, ir, f"{ndim}-D")
    assert len(info["ksp_iterations"]) == info["iterations"] and np.all(info["ksp_iterations"] > 0)
    assert info["linear_iterations"] == info["ksp_iterations"].sum()
    assert_close(dU, xr, 1e-8, f"{ndim}-D: dU", scale=np.abs(xr).max())
    _check_state(S, ref, dU, NHK, f"{ndim}-D")
    S.close()
    S2.close()


def test_newmark_steps_follow_the_selection():
    """Three steps on a MINRES handle against the same steps on a GMRES handle, both linear solves at rtol 1e-12 and Newton
    at rtol 1e-10.  Each linear solve leaves ||F - K y|| <= 1e-12 ||F||, so a Newton update differs between the handles by
    at most cond(K) 1e-12 of its own length (cond about 1e4 in this dynamic regime: 1e-8), and the update of the last
    iteration is itself below 1e-5 of dU: the converged dU, and the particle state it moves, agree far below 1e-8, the
    tolerance test_gpu_newton_solve.py::test_newmark_step holds two routes through the same solver to."""
    case, bcs, gravity, nsteps = _problem(3)
    dt = 2.0e-2
    S, S2 = gpu_setup(case, nsteps=nsteps), gpu_setup(case, nsteps=nsteps)
    S.set_linear_solver("minres")
    kw = dict(max_it=50, atol=0.0, rtol=1e-10, stol=0.0, linesearch="bt")
    for step in range(nsteps):
        im = S.newmark_step(bcs, step, dt, gravity, ksp=dict(TIGHT, restart=0), **kw)
        ig = S2.newmark_step(bcs, step, dt, gravity, ksp=TIGHT, **kw)
        print(f"step {step}", im["fnorm_history"], im["ksp_iterations"], ig["fnorm_history"], ig["ksp_iterations"])
        assert im["reason"] > 0 and im["reason"] == ig["reason"] and im["iterations"] == ig["iterations"], (im, ig)
        assert len(im["ksp_iterations"]) == im["iterations"] and np.all(im["ksp_iterations"] > 0)
        assert im["linear_iterations"] == im["ksp_iterations"].sum()
    a, b = S.download_state(), S2.download_state()
    for k in ("x", "vel", "acc", "F_n", "Stress", "J_n"):
        assert_close(a[k], b[k], 1e-8, f"after three steps: {k}")
    assert np.abs(a["Stress"]).max() > 10.0
    S.close()
    S2.close()


# ------------------------------------------------------------------------------------------------ 9. and 10. bits
def _bits(S, b, **kw):
    x, info = S.tangent_solve(b, history=True, **kw)
    return x, info["history"], info


@pytest.mark.parametrize("ndim", [2, 3])
def test_deterministic_mode_repeats_bit_for_bit(ndim):
    runs = []
    for _ in range(2):
        s = sx.linearised_device(ndim, NHK, deterministic=True)
        S = s["S"]
        S.set_linear_solver("minres")
        S.tangent_operator(10.0, s["Mv"], True)
        b = mc.rhs(s["na"] * ndim, 29)
        x, h, info = _bits(S, b, pc="pbjacobi", rtol=1e-8, max_it=2000)
        assert info["reason"] == minres_ref.CONVERGED_RTOL and info["iterations"] > 20
        x2, h2, _ = _bits(S, b, pc="pbjacobi", rtol=1e-8, max_it=2000)
        assert np.array_equal(x, x2) and np.array_equal(h, h2), "two solves on one handle"
        runs.append((x, h))
        S.close()
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), "two runs"


def test_gmres_is_what_it_was():
    """Deterministic mode on, so bits can be compared: a handle that never calls the setter, and a handle set to MINRES
    and back, return the same bits from the GMRES solve, which are also those of a solve made before the switch."""
    kw = dict(pc="pbjacobi", restart=5, rtol=1e-8, max_it=400)
    out = []
    for switch in (False, True):
        s = sx.linearised_device(3, NHK, deterministic=True)
        S = s["S"]
        S.tangent_operator(10.0, s["Mv"], True)
        b = mc.rhs(s["na"] * 3, 29)
        x0, h0, i0 = _bits(S, b, **kw)
        assert i0["iterations"] > 10, "several cycles"
        if switch:
            S.set_linear_solver("minres")
            xm, hm, im = _bits(S, b, **kw)
            assert im["reason"] > 0 and not np.array_equal(hm[: len(h0)], h0[: len(hm)]), "MINRES ran in between"
            S.set_linear_solver("gmres")
        x1, h1, i1 = _bits(S, b, **kw)
        assert np.array_equal(x0, x1) and np.array_equal(h0, h1), f"switch={switch}: before vs after"
        assert i1["bytes"] == i0["bytes"]
        out.append((x1, h1))
        S.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), "never set vs set and back"
