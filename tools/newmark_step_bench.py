#!/usr/bin/env python3
"""Developer tool: one implicit Newmark time step on the bench cube (1 M Neo-Hookean particles, dt = 1e-3) in two forms,
in one process, on two handles that start from the same cloud:
  (a) composed -- the step of tools/tangent_solve_bench.py::implicit_step: the stage calls, the Newton loop and its
      norms in Python, torch device vectors, a synchronise after every stage;
  (b) one call -- nlps_gpu_newmark_step with the same settings (explicit trial, full Newton steps, SNES atol 1e-8 / rtol
      1e-10 / stol 1e-8, PCJACOBI, GMRES(30) at 1e-5).
After one warm-up step each, `pairs` alternating pairs of steps are timed with the host clock around work that ends in a
synchronise.  Prints one JSON line (per-pair times, Newton / Krylov counts and stopping reasons of both forms, whether
they agree, and whether (b) was slower than (a) in any pair) and writes it to the file given as third argument.
    python tools/newmark_step_bench.py [cells=50] [pairs=5] [out.json]
    python tools/newmark_step_bench.py cells steps --trace     (only form (b), `steps` steps: for a kernel trace)"""
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
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
BETA, GAMMA, DT = 0.25, 0.5, 1.0e-3
A = [1 / (BETA * DT * DT), 1 / (BETA * DT), (1 - 2 * BETA) / (2 * BETA), GAMMA / (BETA * DT), 1 - GAMMA / BETA,
     (1 - GAMMA / (2 * BETA)) * DT]
GRAV = [0.0, 0.0, -9.81]
SNES = dict(max_it=50, atol=1e-8, rtol=1e-10, stol=1e-8, linesearch="basic", ksp=dict(pc="jacobi", restart=30, rtol=1e-5))
REASON = {"fnorm_abs": 2, "fnorm_relative": 3, "snorm_relative": 4, "max_it": -5}


def setup(nst):
    case = bench.build_case(0, 1, cells)
    S = nlps.Solver(3, case["grid_n"], case["origin"], case["h"], case["cloud"], case["materials"], nsteps=nst)
    S.initialise_shapefun()
    nodes = synth.plane_nodes(case["grid_n"], 2, 0)
    gb = nlps.BccSet([{"nodes": nodes, "dim": 3, "dir": np.ones((3, nst), dtype=np.int32), "value": np.zeros((3, nst))}])
    return case, S, gb


def wall(S, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    S.synchronize()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


def composed(S, gb, step):
    """tools/tangent_solve_bench.py::implicit_step, one step: -> (sum of the stage times, info)"""
    T = [0.0]

    def timed(fn):
        t, r = wall(S, fn)
        T[0] += t
        return r

    timed(S.local_search)
    timed(lambda: S.active_masks(gb, step, download=False))
    n = S.nactive * 3
    dev = lambda: torch.zeros(n, dtype=torch.float64, device="cuda")  # noqa: E731
    M, V, Ac, R, d = dev(), dev(), dev(), dev(), dev()
    timed(lambda: S.compute_nodal_lumped_mass(out=M))
    timed(lambda: S.get_nodal_field_n(M, V, Ac))
    dU = torch.from_numpy(timed(lambda: S.form_initial_guess(V, Ac, DT, gb, step))).cuda()
    timed(lambda: S.lagrangian_evaluation(dU, V, Ac, M, A, GRAV, None, step, 1.0, None, out=R))
    r0 = float(torch.linalg.norm(R))
    newton, kits, norms, why = 0, [], [r0], "max_it"
    while newton < 50:
        if norms[-1] < 1e-8:
            why = "fnorm_abs"
            break
        if norms[-1] <= 1e-10 * r0:
            why = "fnorm_relative"
            break
        timed(lambda: S.tangent_operator(A[0], M, True))
        _, info = timed(lambda: S.tangent_solve(-R, pc="jacobi", rtol=1e-5, out=d))
        kits.append(info["iterations"])
        dU = dU + d
        timed(lambda: S.lagrangian_evaluation(dU, V, Ac, M, A, GRAV, None, step, 1.0, None, out=R))
        norms.append(float(torch.linalg.norm(R)))
        newton += 1
        if float(torch.linalg.norm(d)) <= 1e-8 * float(torch.linalg.norm(dU)):
            why = "snorm_relative"
            break
    dVn, dAn = timed(lambda: S.compute_nodal_kinetic_increments(dU, V, Ac, A))
    dV, dA = torch.from_numpy(dVn).cuda(), torch.from_numpy(dAn).cuda()
    timed(lambda: S.update_particles_kinetics_FLIP_PIC(1.0, dU, V, dV, dA))
    timed(S.update_particles_internal_variables)
    return T[0], dict(reason=REASON[why], iterations=newton, ksp_iterations=kits, fnorm_history=norms)


def one_call(S, gb, step):
    return S.newmark_step(gb, step, DT, GRAV, beta=BETA, gamma=GAMMA, **SNES)


if "--trace" in sys.argv:
    _, S, gb = setup(pairs + 1)
    for step in range(1, pairs + 1):
        info = one_call(S, gb, step)
        S.synchronize()
        print(step, info["reason_name"], info["iterations"], list(info["ksp_iterations"]), info["function_evaluations"])
    S.close()
    sys.exit(0)

nst = pairs + 2
case, Sa, gba = setup(nst)
_, Sb, gbb = setup(nst)
out = {"tool": "newmark_step_bench", "particles": int(case["cloud"]["x"].shape[0]), "dt": DT, "pairs": []}
for step in range(1, pairs + 2):  # (step 1 warms the workspaces of both forms)
    ta_wall, (ta, ia) = wall(Sa, lambda: composed(Sa, gba, step))
    tb, ib = wall(Sb, lambda: one_call(Sb, gbb, step))
    if step == 1:
        continue
    out["pairs"].append({
        "step": step, "composed_ms": round(ta, 3), "composed_wall_ms": round(ta_wall, 3), "one_call_ms": round(tb, 3),
        "composed": {"reason": ia["reason"], "newton": ia["iterations"], "krylov": ia["ksp_iterations"],
                     "fnorm": ia["fnorm_history"]},
        "one_call": {"reason": ib["reason"], "newton": ib["iterations"], "krylov": [int(k) for k in ib["ksp_iterations"]],
                     "fnorm": [float(f) for f in ib["fnorm_history"]], "function_evaluations": ib["function_evaluations"]},
        "agree": ia["reason"] == ib["reason"] and ia["iterations"] == ib["iterations"] and
                 ia["ksp_iterations"] == [int(k) for k in ib["ksp_iterations"]]})
out["nactive"] = int(Sb.nactive)
out["forms_agree"] = all(p["agree"] for p in out["pairs"])
out["one_call_slower_in_a_pair"] = any(p["one_call_ms"] > p["composed_ms"] for p in out["pairs"])
out["median_composed_ms"] = round(float(np.median([p["composed_ms"] for p in out["pairs"]])), 3)
out["median_one_call_ms"] = round(float(np.median([p["one_call_ms"] for p in out["pairs"]])), 3)
Sa.close()
Sb.close()
line = json.dumps(out)
print(line)
if len(sys.argv) > 3:
    with open(sys.argv[3], "w") as f:
        f.write(line + "\n")
