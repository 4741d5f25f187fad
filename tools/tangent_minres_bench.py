#!/usr/bin/env python3
"""Developer tool: the device MINRES beside the device GMRES(30) (nlps_gpu_set_linear_solver, nlps_gpu_tangent_solve) on the
bench cube, Neo-Hookean, linearised after one fused residual evaluation; both solvers on ONE handle in one process, point-
block Jacobi.  Prints one JSON line:
  small_alpha: the first alpha_1 of 4e6 x (1e-4, 1e-5, 1e-6, 1e-7, 0) at which GMRES(30) needs more than 100 steps to
    rtol 1e-5 (a large dt; the dynamic 4e6 of dt = 1e-3 takes a handful), and there, per solver: steps, reason, solve ms,
    the true residual over ||b||, workspace bytes;
  per_step, at that alpha_1 (so that every step still has a residual to reduce: with rtol = 0 on the dynamic operator
    MINRES's |eta| underflows long before 200 steps): ms per step over 30 and over 200 steps, (solve ms - the ms of a
    max_it = 0 solve) / steps, and tangent_apply ms measured alongside.
    python tools/tangent_minres_bench.py [cells=50]
--profile: after the warm-up one 30-step solve per solver only, for `rocprofv3 --kernel-trace --stats -- python ...`."""
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
args = [a for a in sys.argv[1:] if not a.startswith("--")]
profile = "--profile" in sys.argv[1:]
cells = int(args[0]) if args else 50
BETA, GAMMA, DT = 0.25, 0.5, 1.0e-3
A = [1 / (BETA * DT * DT), 1 / (BETA * DT), (1 - 2 * BETA) / (2 * BETA), GAMMA / (BETA * DT), 1 - GAMMA / BETA,
     (1 - GAMMA / (2 * BETA)) * DT]
GRAV = [0.0, 0.0, -9.81]
SOLVERS = ("gmres", "minres")


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


case = bench.build_case(0, 1, cells)
nst = 4
S = nlps.Solver(3, case["grid_n"], case["origin"], case["h"], case["cloud"], case["materials"], nsteps=nst)
S.initialise_shapefun()
nodes = synth.plane_nodes(case["grid_n"], 2, 0)
gb = nlps.BccSet([{"nodes": nodes, "dim": 3, "dir": np.ones((3, nst), dtype=np.int32), "value": np.zeros((3, nst))}])
S.local_search()
S.active_masks(gb, 1, download=False)
n = S.nactive * 3
dev = lambda: torch.zeros(n, dtype=torch.float64, device="cuda")  # noqa: E731
M, V, Ac, R, x, y = dev(), dev(), dev(), dev(), dev(), dev()
S.compute_nodal_lumped_mass(out=M)
S.get_nodal_field_n(M, V, Ac)
g = torch.Generator(device="cuda").manual_seed(3)
dU = 1e-4 * torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
S.lagrangian_evaluation(dU, V, Ac, M, A, GRAV, None, 1, 1.0, None, out=R)
b = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
KW = dict(pc="pbjacobi", restart=30, out=x)
out = {"tool": "tangent_minres_bench", "particles": int(case["cloud"]["x"].shape[0]), "nactive": int(S.nactive), "dofs": n,
       "pc": "pbjacobi", "restart": 30}


def solve(kind, **kw):
    S.set_linear_solver(kind)
    return S.tangent_solve(b, **dict(KW, **kw))


# the small alpha_1: GMRES(30) above 100 steps at rtol 1e-5
alpha = None
for f in (1e-4, 1e-5, 1e-6, 1e-7, 0.0):
    S.tangent_operator(A[0] * f, M if f else None, True)
    solve("gmres", rtol=1e-5, max_it=1000)  # (warm: workspace, preconditioner)
    t, (_, info) = ms(S, lambda: solve("gmres", rtol=1e-5, max_it=1000))
    alpha = A[0] * f
    if info["iterations"] > 100 or profile:
        break
if profile:
    for kind in SOLVERS:
        solve(kind, rtol=0.0, max_it=30)
        solve(kind, rtol=0.0, max_it=30)
    S.close()
    sys.exit(0)
small = {"alpha_1": alpha}
for kind in SOLVERS:
    solve(kind, rtol=1e-5, max_it=1000)
    t, (_, info) = ms(S, lambda: solve(kind, rtol=1e-5, max_it=1000), 3)
    S.tangent_apply(x, out=y)
    small[kind] = {"steps": info["iterations"], "reason": info["reason_name"], "solve_ms": round(t, 3),
                   "ms_per_step": round(t / max(info["iterations"], 1), 4), "bytes": info["bytes"],
                   "rnorm_over_bnorm": info["rnorm"] / info["bnorm"],
                   "true_rnorm_over_bnorm": float(torch.linalg.norm(b - y) / torch.linalg.norm(b))}
small["steps_gmres_over_minres"] = round(small["gmres"]["steps"] / max(small["minres"]["steps"], 1), 3)
small["ms_gmres_over_minres"] = round(small["gmres"]["solve_ms"] / small["minres"]["solve_ms"], 3)
small["bytes_gmres_over_minres"] = round(small["gmres"]["bytes"] / small["minres"]["bytes"], 3)
out["small_alpha"] = small
# ms per step
S.tangent_apply(b, out=y)
per = {"alpha_1": alpha, "apply_ms": round(ms(S, lambda: S.tangent_apply(b, out=y), 50)[0], 3)}
for kind in SOLVERS:
    t0 = ms(S, lambda: solve(kind, max_it=0), 5)[0]
    per[kind] = {"fixed_ms": round(t0, 3)}
    for steps in (30, 200):
        solve(kind, rtol=0.0, max_it=steps)
        t, (_, info) = ms(S, lambda: solve(kind, rtol=0.0, max_it=steps), 3)
        per[kind]["steps_%d" % steps] = {"iterations": info["iterations"], "reason": info["reason_name"], "solve_ms": round(t, 3),
                                         "ms_per_step": round((t - t0) / max(info["iterations"], 1), 4)}
for steps in ("steps_30", "steps_200"):
    per["minres_over_gmres_" + steps] = round(per["minres"][steps]["ms_per_step"] / per["gmres"][steps]["ms_per_step"], 3)
per["minres_200_over_gmres_cycle_30"] = round(per["minres"]["steps_200"]["ms_per_step"] / per["gmres"]["steps_30"]["ms_per_step"], 3)
out["per_step"] = per
S.close()
print(json.dumps(out))
