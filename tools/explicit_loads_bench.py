#!/usr/bin/env python3
"""Developer tool: the Neumann contours inside the explicit step (nlps_gpu_set_explicit_loads) on the bench
cube (1 M Neo-Hookean particles, the rigid floor and the time step of bench.py), with the whole +z face of the cube as one
contour (100 x 100 particles at 50 cells).  ONE handle; `rounds` alternating rounds of `steps` steps each are timed with
the host clock around work that ends in a synchronise, in three states of that handle:
  plain        no loads set (set_explicit_loads(None))
  loaded       the contour set, the shipped mapping of the kernel (one wave per contour particle)
  loaded_lane  the contour set, one lane per contour particle (developer switch "loads_lane_map")
then, with the brackets of nlps_gpu_set_timing on, the kernel's own bracket (slot 7) and the calibration bracket of an
empty kernel (slot 5) for both mappings.  Medians over the rounds.  Prints one JSON line and writes it to the file given
as fourth argument.
    python tools/explicit_loads_bench.py [cells=50] [rounds=7] [steps=20] [out.json]
With NLPS_GPU_LIB naming a build of the library without the entry point (the parent commit's), only `plain` is measured:
the yardstick of the same session."""
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

nlps = importlib.import_module("nl-partsol_amd.nlps")
synth = importlib.import_module("nl-partsol_amd.synth")
args = [a for a in sys.argv[1:] if not a.startswith("--")]
cells = int(args[0]) if len(args) > 0 else 50
rounds = int(args[1]) if len(args) > 1 else 7
steps = int(args[2]) if len(args) > 2 else 20
WARM = 5

case = bench.build_case(0, 1, cells)
dt = 0.1 * case["h"] / 100.0  # bench.py: CFL 0.1, celerity sqrt(E / rho) = 100
nodes = synth.plane_nodes(case["grid_n"], 2, 0)
bcs = nlps.BccSet([{"nodes": nodes, "dim": 3, "dir": np.ones((3, 1), dtype=np.int32), "value": np.zeros((3, 1))}])
x = case["cloud"]["x"]
face = np.where(x[:, 2] > x[:, 2].max() - 0.25)[0].astype(np.int32)
loads = nlps.BccSet([{"nodes": face, "dim": 3, "dir": np.ones((3, 1), dtype=np.int32),
                      "value": np.array([[0.0], [0.0], [-1.0e4]])}])
area0 = np.full(x.shape[0], 0.25)

S = nlps.Solver(3, case["grid_n"], case["origin"], case["h"], case["cloud"], case["materials"], nsteps=1)
S.initialise_shapefun()
S.set_adaptive_resort(0.0)
S.set_resort_interval(0)  # (no re-sort inside a round: the rounds compare the same work)
have = hasattr(S.L, "nlps_gpu_set_explicit_loads")


def state(name):
    if not have:
        return
    if name == "plain":
        S.set_explicit_loads(None)
    else:
        S.set_explicit_loads(loads, 1.0, area0)
        S.debug_option("loads_lane_map", 1 if name == "loaded_lane" else 0)


def run(n):
    S.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        S.explicit_step(bcs, 0, dt)
    S.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


names = ["plain", "loaded", "loaded_lane"] if have else ["plain"]
for k in names:
    state(k)
    run(WARM)
times = {k: [] for k in names}
for _ in range(rounds):
    for k in names:
        state(k)
        run(2)  # (the first step behind a change of state rebuilds its lists in front of K2)
        times[k].append(run(steps))
out = {"tool": "explicit_loads_bench", "library": "this commit" if have else "without nlps_gpu_set_explicit_loads (parent)",
       "particles": int(x.shape[0]), "contour_particles": int(face.size), "dt": dt, "rounds": rounds, "steps_per_round": steps,
       "ms_per_step": {k: [round(t, 4) for t in v] for k, v in times.items()},
       "median_ms_per_step": {k: round(float(np.median(v)), 4) for k, v in times.items()}}
if have:
    med = out["median_ms_per_step"]
    out["extra_ms_per_step"] = {k: round(med[k] - med["plain"], 4) for k in names[1:]}
    S.set_timing(True)
    kern = {}
    for k in names[1:]:
        state(k)
        run(2)
        own, cal = [], []
        for _ in range(steps):
            S.explicit_step(bcs, 0, dt)
            ms = S.get_timing()
            own.append(ms[7])
            cal.append(ms[5])
        kern[k] = {"bracket_ms": round(float(np.median(own)), 4), "empty_kernel_bracket_ms": round(float(np.median(cal)), 4)}
    S.set_timing(False)
    out["kernel"] = kern
S.close()
line = json.dumps(out)
print(line)
if len(args) > 3:
    with open(args[3], "w") as f:
        f.write(line + "\n")
