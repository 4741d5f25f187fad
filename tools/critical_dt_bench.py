#!/usr/bin/env python3
"""Developer tool: the device Lanczos bound on the explicit step's stable dt (nlps_gpu_tangent_lambda_max) on the bench cube,
Neo-Hookean, floor fixed, linearised at the undeformed state (dU = 0) with no mass term, in one process.  Writes one JSON
object (default profiles/r19_critical_dt_bench.json) and prints it:
  lanczos_30: ms per Lanczos step over a 30-step run (rtol = 0), less the fixed part of a call (a 1-step run minus its one
    step, see fixed_ms), next to apply_ms (one tangent_apply) and gmres_cycle_30 (the per-step cost of tangent_solve over
    a 30-step cycle, PBJACOBI, with the mass term of a dt = 1e-3 Newmark step so that it has something to solve);
  rtol_1e-03 / rtol_1e-06: the steps taken, theta, resid, asymmetry, the call's ms;
  critical_dt (safety 0.9 and 1.0, from theta + resid of the rtol 1e-6 run) next to courant_dt(1, h, sqrt((lambda + 2 G) / rho)).
  mpm_probe: how the bound relates to the limit the particle / grid step itself has, in the linear regime only: the cube at
    rest, the particle velocities moved by the nodal field 1e-9 * mode (through the FLIP update), then up to 20 explicit
    steps at 0.9 and at 1.1 of critical_dt (safety 1.0) on twin handles, a run stopped at the first record row whose
    kinetic energy exceeds 1e6 times the first row's or whose status is not 0; the kinetic-energy ratio last / first row.
    python tools/critical_dt_bench.py [cells=50] [out=profiles/r19_critical_dt_bench.json]"""
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

nlps = importlib.import_module("nl-partsol_amd.nlps")
synth = importlib.import_module("nl-partsol_amd.synth")
cells = int(sys.argv[1]) if len(sys.argv) > 1 else 50
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r19_critical_dt_bench.json")


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
nst = 2
S = nlps.Solver(3, case["grid_n"], case["origin"], case["h"], case["cloud"], case["materials"], nsteps=nst)
S.initialise_shapefun()
nodes = synth.plane_nodes(case["grid_n"], 2, case["block_lo"][2])
gb = nlps.BccSet([{"nodes": nodes, "dim": 3, "dir": np.ones((3, nst), dtype=np.int32), "value": np.zeros((3, nst))}])
S.local_search()
S.active_masks(gb, 0, download=False)
n = S.nactive * 3
dev = lambda: torch.zeros(n, dtype=torch.float64, device="cuda")  # noqa: E731
M, x, y = dev(), dev(), dev()
S.compute_nodal_lumped_mass(out=M)
S.local_compatibility_conditions(dev())
S.constitutive_update()
res = {"tool": "critical_dt_bench", "particles": int(case["cloud"]["x"].shape[0]), "nactive": int(S.nactive), "dofs": n,
       "h": case["h"]}

# the GMRES yardstick first (its operator carries the mass term), then the operator the bound is taken on
g = torch.Generator(device="cuda").manual_seed(3)
b = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
S.tangent_operator(1.0 / (0.25 * 1e-3 * 1e-3), M, True)
S.tangent_solve(b, pc="pbjacobi", rtol=0.0, max_it=30, out=x)
t30, (_, i30) = ms(S, lambda: S.tangent_solve(b, pc="pbjacobi", rtol=0.0, max_it=30, out=x), 3)
t0 = ms(S, lambda: S.tangent_solve(b, pc="pbjacobi", max_it=0, out=x), 5)[0]
res["gmres_cycle_30"] = {"iterations": i30["iterations"], "solve_ms": round(t30, 3), "fixed_ms": round(t0, 3),
                         "ms_per_step": round((t30 - t0) / max(i30["iterations"], 1), 4)}

S.tangent_operator(0.0, None, True)
S.tangent_apply(b, out=y)
res["apply_ms"] = round(ms(S, lambda: S.tangent_apply(b, out=y), 50)[0], 4)
mode = dev()
S.tangent_lambda_max(M, max_it=30, rtol=0.0, mode=mode)  # (warm: the workspace is sized)
t30, i30 = ms(S, lambda: S.tangent_lambda_max(M, max_it=30, rtol=0.0, mode=mode), 3)
t1, _ = ms(S, lambda: S.tangent_lambda_max(M, max_it=1, rtol=0.0, mode=mode), 5)
per = (t30 - t1) / 29.0
res["lanczos_30"] = {"iterations": i30["iterations"], "call_ms": round(t30, 3), "one_step_call_ms": round(t1, 3),
                     "fixed_ms": round(t1 - per, 3), "ms_per_step": round(per, 4),
                     "ms_per_step_over_apply": round(per / res["apply_ms"], 3),
                     "ms_per_step_over_gmres_step": round(per / res["gmres_cycle_30"]["ms_per_step"], 3),
                     "theta": i30["theta"], "resid": i30["resid"], "bytes": i30["bytes"]}
last = None
for rtol in (1e-3, 1e-6):
    t, info = ms(S, lambda: S.tangent_lambda_max(M, max_it=256, rtol=rtol, mode=mode, history=True), 1)
    res["rtol_%.0e" % rtol] = {"iterations": info["iterations"], "reason": info["reason_name"], "call_ms": round(t, 3),
                               "theta": info["theta"], "resid": info["resid"], "asymmetry": info["asymmetry"],
                               "bytes": info["bytes"]}
    last = info
mat = case["materials"][0]
lame = mat["E"] * mat["nu"] / ((1 + mat["nu"]) * (1 - 2 * mat["nu"]))
G = mat["E"] / (2 * (1 + mat["nu"]))
rho = float(np.asarray(case["cloud"]["rho"]).ravel()[0])
cel = float(np.sqrt((lame + 2 * G) / rho))
Mh = M.cpu().numpy()
res["mass_min"], res["mass_max"] = float(Mh.min()), float(Mh.max())
res["celerity"] = cel
res["courant_dt_cfl_1"] = nlps.courant_dt(1.0, case["h"], cel)
res["critical_dt_safety_0.9"] = nlps.critical_dt(last["theta"] + last["resid"])
res["critical_dt_safety_1.0"] = nlps.critical_dt(last["theta"] + last["resid"], safety=1.0)
res["critical_over_courant"] = res["critical_dt_safety_1.0"] / res["courant_dt_cfl_1"]
S.close()


def probe(factor):
    """The cube at rest with 1e-9 * mode on the velocities, up to 20 explicit steps at factor * critical_dt."""
    cloud = dict(case["cloud"])
    cloud["vel"] = np.zeros_like(np.asarray(cloud["vel"], dtype=np.float64))
    T = nlps.Solver(3, case["grid_n"], case["origin"], case["h"], cloud, case["materials"], nsteps=32)
    T.initialise_shapefun()
    tb = nlps.BccSet([{"nodes": nodes, "dim": 3, "dir": np.ones((3, 32), dtype=np.int32), "value": np.zeros((3, 32))}])
    T.local_search()
    T.active_masks(tb, 0, download=False)
    assert T.nactive * 3 == n
    z = dev()
    T.update_particles_kinetics_FLIP_PIC(1.0, z, z, 1e-9 * mode, z)
    T.set_step_record(every=1, capacity=64)
    dt = factor * res["critical_dt_safety_1.0"]
    kin, status, stopped, err = [], 0, None, None
    for t in range(20):
        try:
            T.explicit_step(tb, t, dt)
            rec = T.read_step_records()
        except nlps.NlpsError as e:
            err, stopped = str(e)[:200], t
            break
        kin = [float(v) for v in np.asarray(rec["kinetic"]).ravel()]
        status = int(np.asarray(rec["status"]).ravel()[-1])
        if status != 0 or kin[-1] > 1e6 * kin[0]:
            stopped = t
            break
    T.close()
    return {"dt": dt, "steps": len(kin), "stopped_at": stopped, "status": status, "error": err, "kinetic_first": kin[0] if kin else None,
            "kinetic_last": kin[-1] if kin else None, "kinetic_ratio": (kin[-1] / kin[0]) if kin and kin[0] > 0 else None}


res["mpm_probe"] = {"0.9": probe(0.9), "1.1": probe(1.1)}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
