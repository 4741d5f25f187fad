#!/usr/bin/env python3
"""Developer tool: the device GMRES on the matrix-free tangent (nlps_gpu_tangent_solve) on the bench cube, linearised
after one fused residual evaluation, in one process.  Prints one JSON line:
  per case (Neo-Hookean 1 M, Drucker-Prager 1 M, Neo-Hookean 8 M): the point-block Jacobi build ms, iterations and solve
  ms at rtol 1e-5 (the driver's KSP default) and 1e-8, ms per Arnoldi step (over a full 30-step cycle and between the
  two tolerances), tangent_apply ms measured alongside, workspace bytes;
  host_driven (1 M NH): the same solve by scipy GMRES through host tangent_apply products (the MatShell path);
  implicit_step (1 M NH): one whole implicit Newmark step -- search, masks, mass, nodal field, initial guess, Newton with
  the fused residual, the operator and the device solve (PCJACOBI, KSP rtol 1e-5; SNES's tests at the driver's
  tolerances), kinetic increments, update, roll -- total ms and the split.
    python tools/tangent_solve_bench.py [cells=50] [big_cells=100]     (big_cells=0 skips the 8 M case)"""
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

nlps = importlib.import_module("nl-partsol_amd.nlps")
synth = importlib.import_module("nl-partsol_amd.synth")
cells = int(sys.argv[1]) if len(sys.argv) > 1 else 50
big = int(sys.argv[2]) if len(sys.argv) > 2 else 100
BETA, GAMMA, DT = 0.25, 0.5, 1.0e-3
A = [1 / (BETA * DT * DT), 1 / (BETA * DT), (1 - 2 * BETA) / (2 * BETA), GAMMA / (BETA * DT), 1 - GAMMA / BETA,
     (1 - GAMMA / (2 * BETA)) * DT]
GRAV = [0.0, 0.0, -9.81]


def ms(S, fn, reps=1):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        S.synchronize()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), r


def setup(law, c):
    case = bench.build_case(0, 1, c)
    if law == "drucker-prager":
        case["materials"] = [synth.drucker_prager_material()]
    nst = 4
    S = nlps.Solver(3, case["grid_n"], case["origin"], case["h"], case["cloud"], case["materials"], nsteps=nst)
    S.initialise_shapefun()
    nodes = synth.plane_nodes(case["grid_n"], 2, 0)
    gb = nlps.BccSet([{"nodes": nodes, "dim": 3, "dir": np.ones((3, nst), dtype=np.int32), "value": np.zeros((3, nst))}])
    return case, S, gb


def run(law, c, host_driven):
    case, S, gb = setup(law, c)
    S.local_search()
    S.active_masks(gb, 1, download=False)
    n = S.nactive * 3
    dev = lambda: torch.zeros(n, dtype=torch.float64, device="cuda")  # noqa: E731
    M, V, Ac, R = dev(), dev(), dev(), dev()
    S.compute_nodal_lumped_mass(out=M)
    S.get_nodal_field_n(M, V, Ac)
    g = torch.Generator(device="cuda").manual_seed(3)
    dU = 1e-4 * torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    S.lagrangian_evaluation(dU, V, Ac, M, A, GRAV, None, 1, 1.0, None, out=R)
    out = {"particles": int(case["cloud"]["x"].shape[0]), "nactive": int(S.nactive), "dofs": n}
    b = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    x = dev()
    y = dev()
    S.tangent_operator(A[0], M, True)
    S.tangent_apply(b, out=y)
    out["apply_ms"] = round(ms(S, lambda: S.tangent_apply(b, out=y), 50)[0], 3)
    # the preconditioner: a solve with max_it = 0 right after the operator builds it, the same solve again reuses it
    S.tangent_solve(b, pc="pbjacobi", max_it=0, out=x)
    t_build = []
    for _ in range(5):
        S.tangent_operator(A[0], M, True)
        t_first = ms(S, lambda: S.tangent_solve(b, pc="pbjacobi", max_it=0, out=x))[0]
        t_again = ms(S, lambda: S.tangent_solve(b, pc="pbjacobi", max_it=0, out=x))[0]
        t_build.append(t_first - t_again)
    out["pc_build_ms"] = round(float(np.median(t_build)), 3)
    for rtol in (1e-5, 1e-8):
        key = "rtol_%.0e" % rtol
        S.tangent_solve(b, pc="pbjacobi", rtol=rtol, out=x)  # (warm: workspace allocated, PC cached)
        t, (_, info) = ms(S, lambda: S.tangent_solve(b, pc="pbjacobi", rtol=rtol, out=x), 3)
        out[key] = {"iterations": info["iterations"], "reason": info["reason"], "solve_ms": round(t, 3),
                    "ms_per_step": round(t / max(info["iterations"], 1), 4),
                    "rnorm_over_bnorm": info["rnorm"] / info["bnorm"], "bytes": info["bytes"]}
    # one whole cycle of restart 30 (rtol 0, max_it 30: exactly 30 Arnoldi steps, orthogonalisation against up to 30
    # vectors), less the fixed part of a solve (a max_it = 0 solve: ||b||, r0, the true residual)
    S.tangent_solve(b, pc="pbjacobi", rtol=0.0, max_it=30, out=x)
    t30, (_, i30) = ms(S, lambda: S.tangent_solve(b, pc="pbjacobi", rtol=0.0, max_it=30, out=x), 3)
    t0 = ms(S, lambda: S.tangent_solve(b, pc="pbjacobi", max_it=0, out=x), 5)[0]
    out["cycle_30"] = {"iterations": i30["iterations"], "reason": i30["reason"], "solve_ms": round(t30, 3),
                       "fixed_ms": round(t0, 3), "ms_per_step": round((t30 - t0) / max(i30["iterations"], 1), 4)}
    out["cycle_30"]["ms_per_step_over_apply"] = round(out["cycle_30"]["ms_per_step"] / out["apply_ms"], 3)
    # the marginal cost of a step: the fixed part of a solve (||b||, r0, the update, the true residual) cancels
    lo, hi = out["rtol_1e-05"], out["rtol_1e-08"]
    if hi["iterations"] > lo["iterations"]:
        out["ms_per_step_marginal"] = round((hi["solve_ms"] - lo["solve_ms"]) / (hi["iterations"] - lo["iterations"]), 4)
        out["ms_per_step_marginal_over_apply"] = round(out["ms_per_step_marginal"] / out["apply_ms"], 3)
    out["ms_per_step_over_apply"] = round(hi["ms_per_step"] / out["apply_ms"], 3)
    if host_driven:
        from scipy.sparse.linalg import LinearOperator, gmres
        bh = b.cpu().numpy()
        yh = np.empty(n)

        def host_solve():
            Bl = S.tangent_block_diagonal()
            Binv = np.linalg.inv(Bl)
            Kop = LinearOperator((n, n), matvec=lambda v: S.tangent_apply(np.ascontiguousarray(v), out=yh).copy())
            Pre = LinearOperator((n, n), matvec=lambda v: np.einsum("aij,aj->ai", Binv, v.reshape(-1, 3)).ravel())
            cnt = [0]
            try:
                xh, info = gmres(Kop, bh, rtol=1e-5, atol=0.0, M=Pre, restart=30, maxiter=100,
                                 callback=lambda pr: cnt.__setitem__(0, cnt[0] + 1), callback_type="pr_norm")
            except TypeError:  # older scipy
                xh, info = gmres(Kop, bh, tol=1e-5, atol=0.0, M=Pre, restart=30, maxiter=100,
                                 callback=lambda pr: cnt.__setitem__(0, cnt[0] + 1), callback_type="pr_norm")
            return xh, info, cnt[0]

        t, (xh, info, its) = ms(S, host_solve, 1)
        rh = float(np.linalg.norm(bh - S.tangent_apply(xh)) / np.linalg.norm(bh))
        out["host_driven_rtol_1e-05"] = {"solve_ms": round(t, 3), "iterations": its, "info": int(info),
                                         "true_rnorm_over_bnorm": rh,
                                         "speedup_of_device_solve": round(t / out["rtol_1e-05"]["solve_ms"], 2)}
    S.close()
    return out


def implicit_step(c):
    """One implicit Newmark step with the device solve as the linear solver (U-Newmark-beta.c:192-409)."""
    case, S, gb = setup("neo-hookean", c)
    T = {}

    def timed(name, fn):
        t, r = ms(S, fn)
        T[name] = T.get(name, 0.0) + t
        return r

    res = None
    for step in range(1, 3):  # (step 1 warms the workspace; step 2 is reported)
        T.clear()
        timed("local_search", S.local_search)
        timed("active_masks", lambda: S.active_masks(gb, step, download=False))
        n = S.nactive * 3
        dev = lambda: torch.zeros(n, dtype=torch.float64, device="cuda")  # noqa: E731
        M, V, Ac, R, d = dev(), dev(), dev(), dev(), dev()
        timed("lumped_mass", lambda: S.compute_nodal_lumped_mass(out=M))
        timed("nodal_field_n", lambda: S.get_nodal_field_n(M, V, Ac))
        dU = torch.from_numpy(timed("form_initial_guess", lambda: S.form_initial_guess(V, Ac, DT, gb, step))).cuda()
        timed("residual", lambda: S.lagrangian_evaluation(dU, V, Ac, M, A, GRAV, None, step, 1.0, None, out=R))
        r0 = float(torch.linalg.norm(R))
        # SNES's tests with the driver's tolerances (TOL_Newmark_beta 1e-10, atol 100 x that, stol 1e-8, 50 iterates)
        newton, kits, norms, why = 0, [], [r0], "max_it"
        while newton < 50:
            if norms[-1] < 1e-8:
                why = "fnorm_abs"
                break
            if norms[-1] <= 1e-10 * r0:
                why = "fnorm_relative"
                break
            timed("tangent_operator", lambda: S.tangent_operator(A[0], M, True))
            _, info = timed("tangent_solve", lambda: S.tangent_solve(-R, pc="jacobi", rtol=1e-5, out=d))
            kits.append(info["iterations"])
            dU = dU + d
            timed("residual", lambda: S.lagrangian_evaluation(dU, V, Ac, M, A, GRAV, None, step, 1.0, None, out=R))
            norms.append(float(torch.linalg.norm(R)))
            newton += 1
            if float(torch.linalg.norm(d)) <= 1e-8 * float(torch.linalg.norm(dU)):
                why = "snorm_relative"
                break
        dVn, dAn = timed("kinetic_increments", lambda: S.compute_nodal_kinetic_increments(dU, V, Ac, A))
        dV, dA = torch.from_numpy(dVn).cuda(), torch.from_numpy(dAn).cuda()
        timed("update_kinetics", lambda: S.update_particles_kinetics_FLIP_PIC(1.0, dU, V, dV, dA))
        timed("roll_state", S.update_particles_internal_variables)
        res = {"particles": int(case["cloud"]["x"].shape[0]), "newton_iterations": newton, "newton_stop": why,
               "krylov_iterations": kits,
               "residual_norms": norms, "total_ms": round(sum(T.values()), 3),
               "split_ms": {k: round(v, 3) for k, v in sorted(T.items(), key=lambda kv: -kv[1])}}
    S.close()
    return res


result = {"tool": "tangent_solve_bench", "restart": 30, "pc": "pbjacobi",
          "nh_1m": run("neo-hookean", cells, True), "dp_1m": run("drucker-prager", cells, False)}
if big > 0:
    result["nh_8m"] = run("neo-hookean", big, False)
result["implicit_step_1m"] = implicit_step(cells)
print(json.dumps(result))
