#!/usr/bin/env python3
"""Developer tool: what an output costs a run (the particle snapshot, nlps_gpu_set_snapshots) on the bench
cube of bench.py (1 M Neo-Hookean particles, its rigid floor and time step).  Every run is a fresh handle on one
caller-owned stream -- the cube falls, so only runs over the same steps compare the same work -- with `warm` warm-up
steps and `steps` timed steps (host clock around work that ends in a synchronise of the handle's stream); `repeats`
repeats of the three runs, in an order that rotates from repeat to repeat:
  a  no output
  b  download_state of the VTK field set every `every` steps (the parent's way: the entry is untouched)
  c  snapshot_begin every `every` steps, with snapshot_wait + snapshot_release of the previous one just before it
The last snapshot of run c is waited for behind the clock.  Recorded besides: the host time of every begin, the pack
kernel's time by an event bracket on the handle's stream around begin (the copy is on another stream), the time spent
in every wait, snapshot_bytes, and the device-to-host rate from one begin + wait on the idle handle with the pack time
taken off.  Stall per output = (ms per step of the run - ms per step of a) x every.
Prints one JSON line and writes it to the file given as sixth argument.
    python tools/snapshot_bench.py [cells=50] [repeats=5] [steps=200] [every=20] [warm=10] [out.json]"""
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
args = sys.argv[1:]
cells = int(args[0]) if len(args) > 0 else 50
repeats = int(args[1]) if len(args) > 1 else 5
steps = int(args[2]) if len(args) > 2 else 200
every = int(args[3]) if len(args) > 3 else 20
warm = int(args[4]) if len(args) > 4 else 10
NSTEPS = 4  # (the floor is held at every step: the tables repeat)
VTK = ["x", "dis", "vel", "acc", "F_n", "Stress", "rho", "mass", "W", "EPS_n", "I0"]  # what gid.write_particles_vtk reads
RUNS = "abc"

case = bench.build_case(0, 1, cells)
dt = 0.1 * case["h"] / 100.0  # bench.py: CFL 0.1, celerity sqrt(E / rho) = 100
nodes = synth.plane_nodes(case["grid_n"], 2, 0)
bcs = nlps.BccSet([{"nodes": nodes, "dim": 3, "dir": np.ones((3, NSTEPS), dtype=np.int32), "value": np.zeros((3, NSTEPS))}])
npart = int(case["cloud"]["x"].shape[0])
ts = torch.cuda.Stream()
torch.cuda.set_stream(ts)
log = {"wait_ms": [], "wait_behind_the_clock_ms": [], "begin_host_ms": [], "pack_ms": []}
idle, nbytes, mapping = [], None, {"by_slot": [], "by_caller": []}


def bracketed_begin(S, tag):
    """-> slot, the two events around the pack on the handle's stream, host ms of begin"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record(ts)
    h0 = time.perf_counter()
    slot = S.snapshot_begin(tag)
    host = 1e3 * (time.perf_counter() - h0)
    ev[1].record(ts)
    return slot, ev, host


def run(kind):
    """-> ms per step of `steps` steps with the outputs of `kind`, on a handle of its own"""
    global nbytes
    S = nlps.Solver(3, case["grid_n"], case["origin"], case["h"], case["cloud"], case["materials"], nsteps=NSTEPS,
                    stream=ts.cuda_stream)
    S.initialise_shapefun()
    S.set_adaptive_resort(0.0)
    S.set_resort_interval(0)  # (no re-sort inside a run: the runs compare the same work)
    S.set_snapshots(VTK, 2)
    nbytes = S.snapshot_bytes()
    t = 0
    for _ in range(warm):
        S.explicit_step(bcs, t % NSTEPS, dt)
        t += 1
    S.download_state(fields=VTK)  # (first use of either path: the staging vector, the pinned pages)
    for _ in range(2):
        S.snapshot_release(S.snapshot_begin(0))
    prev, brackets = None, []
    S.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        S.explicit_step(bcs, t % NSTEPS, dt)
        t += 1
        if (i + 1) % every:
            continue
        if kind == "b":
            S.download_state(fields=VTK)
        elif kind == "c":
            if prev is not None:
                h0 = time.perf_counter()
                S.snapshot_wait(prev, copy=False)
                log["wait_ms"].append(1e3 * (time.perf_counter() - h0))
                S.snapshot_release(prev)
            prev, ev, host = bracketed_begin(S, t)
            log["begin_host_ms"].append(host)
            brackets.append(ev)
    S.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    if prev is not None:
        h0 = time.perf_counter()
        S.snapshot_wait(prev, copy=False)
        log["wait_behind_the_clock_ms"].append(1e3 * (time.perf_counter() - h0))
        S.snapshot_release(prev)
        log["pack_ms"] += [float(a.elapsed_time(b)) for a, b in brackets]
        # one snapshot on the idle handle: begin -> wait is the pack and the copy, nothing else
        S.synchronize()
        h0 = time.perf_counter()
        slot, ev, _ = bracketed_begin(S, 0)
        S.snapshot_wait(slot, copy=False)
        total = 1e3 * (time.perf_counter() - h0)
        S.snapshot_release(slot)
        idle.append((total, float(ev[0].elapsed_time(ev[1]))))
        # the two mappings of the pack kernel on this state: one thread per memory slot / per caller's index
        for name, on in (("by_slot", 0), ("by_caller", 1)):
            S.debug_option("snapshot_by_caller", on)
            S.snapshot_release(S.snapshot_begin(0))  # (by_caller: makes the inverse permutation)
            for _ in range(3):
                slot, ev, _ = bracketed_begin(S, 0)
                S.snapshot_wait(slot, copy=False)
                S.snapshot_release(slot)
                mapping[name].append(float(ev[0].elapsed_time(ev[1])))
    S.close()
    return ms


times = {k: [] for k in RUNS}
orders = []
for r in range(repeats):
    order = RUNS[r % len(RUNS):] + RUNS[:r % len(RUNS)]
    orders.append(order)
    for k in order:
        times[k].append(run(k))
    print("repeat %d (%s): %s ms per step" % (r, order, " ".join("%s %.4f" % (k, times[k][-1]) for k in RUNS)), file=sys.stderr,
          flush=True)


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4), "n": int(v.size)}


med = {k: float(np.median(v)) for k, v in times.items()}
spread_a = float(np.max(times["a"]) - np.min(times["a"]))
slot_bytes = nbytes[1] // 2
copy_ms = float(np.median([a - b for a, b in idle]))
out = {"tool": "snapshot_bench", "particles": npart, "dt": dt, "repeats": repeats, "steps_per_run": steps, "output_every": every,
       "warmup_steps": warm, "run_order_per_repeat": orders, "fields": VTK,
       "ms_per_step": {k: [round(t, 4) for t in v] for k, v in times.items()},
       "ms_per_step_stats": {k: stats(v) for k, v in times.items()},
       "spread_of_a_ms_per_step": round(spread_a, 4),
       "stall_per_output_ms": {"download_state": round((med["b"] - med["a"]) * every, 4),
                               "snapshot": round((med["c"] - med["a"]) * every, 4),
                               "spread_of_a_x_every": round(spread_a * every, 4)},
       "stall_ratio_download_over_snapshot": round((med["b"] - med["a"]) / (med["c"] - med["a"]), 2) if med["c"] > med["a"] else None,
       "steps_one_download_costs": round((med["b"] - med["a"]) * every / med["a"], 1),
       "pack_kernel_ms": stats(log["pack_ms"]), "begin_host_ms": stats(log["begin_host_ms"]),
       "wait_ms": stats(log["wait_ms"]), "wait_behind_the_clock_ms": stats(log["wait_behind_the_clock_ms"]),
       "snapshot_bytes": {"device": nbytes[0], "pinned": nbytes[1], "per_slot": slot_bytes},
       "idle_begin_to_wait_ms": stats([a for a, _ in idle]), "idle_pack_ms": stats([b for _, b in idle]),
       "d2h_GB_s": round(slot_bytes / (copy_ms * 1e-3) / 1e9, 2),
       "pack_mapping_ab_ms": {k: stats(v) for k, v in mapping.items()}}
line = json.dumps(out)
print(line)
if len(args) > 5:
    with open(args[5], "w") as f:
        f.write(line + "\n")
