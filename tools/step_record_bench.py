#!/usr/bin/env python3
"""Developer tool: the step record (nlps_gpu_set_step_record) on the bench cube (1 M Neo-Hookean particles,
the rigid floor and the time step of bench.py).  ONE handle; `rounds` alternating rounds of `steps` steps each are timed
with the host clock around work that ends in a synchronise, in four states of that handle:
  plain      no record set (set_step_record(every=None))
  every1     a row every step, particle sums only
  probes     a row every step with 64 probes (every field) and the reaction totals of the floor
  every10    a row every 10 steps, particle sums only
The step argument runs 0, 1, 2 .. inside a round, so `every10` records two steps of twenty.  Then the copy of
tools/hbm_calib.hip (2^27 doubles read, 2^27 written, 8 B per lane) is timed in the same process, and the bytes
k_rec_particles reads per particle (counted from the kernel: mass, vel, x, J_n, Vol_0, EPS_n, Damage_n and -- after a folded
step of a hyperelastic law -- the material index and F_n, else W) are priced at that rate.  Medians over the rounds.  Prints
one JSON line and writes it to the file given as fourth argument.
    python tools/step_record_bench.py [cells=50] [rounds=7] [steps=20] [out.json]
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
NSTEPS = steps + 2

case = bench.build_case(0, 1, cells)
dt = 0.1 * case["h"] / 100.0  # bench.py: CFL 0.1, celerity sqrt(E / rho) = 100
nodes = synth.plane_nodes(case["grid_n"], 2, 0)
bcs = nlps.BccSet([{"nodes": nodes, "dim": 3, "dir": np.ones((3, NSTEPS), dtype=np.int32), "value": np.zeros((3, NSTEPS))}])
npart = int(case["cloud"]["x"].shape[0])
probes = np.random.default_rng(1).choice(npart, size=64, replace=False).astype(np.int32)

S = nlps.Solver(3, case["grid_n"], case["origin"], case["h"], case["cloud"], case["materials"], nsteps=NSTEPS)
S.initialise_shapefun()
S.set_adaptive_resort(0.0)
S.set_resort_interval(0)  # (no re-sort inside a round: the rounds compare the same work)
have = hasattr(S.L, "nlps_gpu_set_step_record")


def state(name):
    if not have:
        return
    if name == "plain":
        S.set_step_record(every=None)
    elif name == "every1":
        S.set_step_record(every=1, capacity=64)
    elif name == "probes":
        S.set_step_record(every=1, capacity=64, nsets=1, probes=probes, probe_fields=nlps.PROBE_ALL)
    else:
        S.set_step_record(every=10, capacity=64)


def run(n):
    S.synchronize()
    t0 = time.perf_counter()
    for t in range(n):
        S.explicit_step(bcs, t, dt)
    S.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


names = ["plain", "every1", "probes", "every10"] if have else ["plain"]
for k in names:
    state(k)
    run(WARM)
times = {k: [] for k in names}
for _ in range(rounds):
    for k in names:
        state(k)
        run(2)  # (the first step behind a change of state rebuilds its lists in front of K2)
        times[k].append(run(steps))
out = {"tool": "step_record_bench", "library": "this commit" if have else "without nlps_gpu_set_step_record (parent)",
       "particles": npart, "dt": dt, "rounds": rounds, "steps_per_round": steps,
       "ms_per_step": {k: [round(t, 4) for t in v] for k, v in times.items()},
       "median_ms_per_step": {k: round(float(np.median(v)), 4) for k, v in times.items()}}
if have:
    med = out["median_ms_per_step"]
    out["extra_ms_per_step"] = {k: round(med[k] - med["plain"], 4) for k in names[1:]}
    rec = S.read_step_records()
    out["rows_in_the_last_state"] = {"total": rec["total"], "kinetic": float(rec["kinetic"][-1]), "strain": float(rec["strain"][-1]),
                                     "J_min": float(rec["J_min"][-1]), "vmax_comp": float(rec["vmax_comp"][-1])}
    # the copy of tools/hbm_calib.hip, timed: 2^27 doubles in, 2^27 out, 8 B per lane
    import torch
    n = 1 << 27
    a = torch.zeros(n, dtype=torch.float64, device="cuda")
    b = torch.empty_like(a)
    for _ in range(2):
        torch.add(a, 1.0, out=b)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rates = []
    for _ in range(5):
        ev[0].record()
        torch.add(a, 1.0, out=b)
        ev[1].record()
        ev[1].synchronize()
        rates.append(16.0 * n / (1e-3 * ev[0].elapsed_time(ev[1])) / 1e9)
    rate = float(np.median(rates))
    # bytes k_rec_particles reads per particle in 3-D: mass, J_n, Damage_n, EPS_n, Vol_0 (8 each), x and vel (24 each); after
    # a folded Neo-Hookean / Hencky step the material index (4) and F_n (72) to re-form W, in every other state W (8)
    lazy_bytes, stored_bytes = 5 * 8 + 2 * 24 + 4 + 72, 5 * 8 + 2 * 24 + 8
    out["copy_rate_GB_s"] = round(rate, 1)
    out["bytes_read_per_particle"] = {"re-formed W (folded step, hyperelastic law)": lazy_bytes, "stored W": stored_bytes}
    out["ms_for_those_bytes_at_the_copy_rate"] = {"re-formed W": round(1e3 * lazy_bytes * npart / (rate * 1e9), 4),
                                                  "stored W": round(1e3 * stored_bytes * npart / (rate * 1e9), 4)}
S.close()
line = json.dumps(out)
print(line)
if len(args) > 3:
    with open(args[3], "w") as f:
        f.write(line + "\n")
