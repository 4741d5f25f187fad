#!/usr/bin/env python3
"""Developer tool: the explicit step with F-bar on lattice-cell patches (nlps_gpu_set_explicit_fbar) on the
bench cube (1 M particles, Neo-Hookean at nu = 0.49, gravity, dt = 1e-4).  Three handles that start from the same
geometry, in one process, each on a stream of its own:
  (a) plain_non_folded -- the step without F-bar in the form a step with F-bar runs (debug option lazy_nodal = 0): the
      fused K3 (MODE 1).  This is the yardstick;
  (b) fbar_block1 -- F-bar with alpha = 0 on patches of one cell: the kinematic half of K3 (MODE 8), the stress kernel,
      the force half;
  (c) fbar_block2 -- the same on patches of 2 x 2 x 2 cells.
Two warm-up runs, then `rounds` alternating runs of `steps` steps, each between two events on the handle's stream; medians
over the rounds; then the K3 bracket of nlps_gpu_set_timing (everything between the nodal dU and the nodal forces) over
ten more steps of every form.  Prints one JSON line and writes it to the file given as fourth argument.
    python tools/explicit_fbar_bench.py [cells=50] [rounds=5] [steps=10] [out.json]
Under `rocprofv3 --kernel-trace --stats -- python tools/explicit_fbar_bench.py ...` the per-kernel times of the three
kernels of (b) and (c) are k3_kin_tile, k_fbar_stress and k3f_tile."""
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

nlps = importlib.import_module("nl-partsol_amd.nlps")
args = [a for a in sys.argv[1:] if not a.startswith("--")]
cells = int(args[0]) if len(args) > 0 else 50
rounds = int(args[1]) if len(args) > 1 else 5
steps = int(args[2]) if len(args) > 2 else 10
DT, WARM = 1.0e-4, 2
NH49 = {"type": 0, "E": 1.0e7, "nu": 0.49}
GRAVITY = [0.0, -9.81, 0.0]


class Form:
    def __init__(self, block):
        case = bench.build_case(0, 1, cells)
        case["materials"] = [NH49]
        self.stream = torch.cuda.Stream()
        self.S = nlps.Solver(3, case["grid_n"], case["origin"], case["h"], case["cloud"], case["materials"], nsteps=1,
                             stream=self.stream.cuda_stream)
        self.S.initialise_shapefun()
        self.S.debug_option("lazy_nodal", 0)
        if block:
            self.S.set_explicit_fbar([0.0], block)
        self.none = nlps.BccSet([])

    def run(self, n):
        """ms per step, between two events on the handle's stream"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(self.stream)
        for _ in range(n):
            self.S.explicit_step(self.none, 0, DT, gravity=GRAVITY)
        b.record(self.stream)
        b.synchronize()
        return a.elapsed_time(b) / n


forms = {"plain_non_folded": Form(0), "fbar_block1": Form(1), "fbar_block2": Form(2)}
for _ in range(WARM):
    for f in forms.values():
        f.run(steps)
times = {k: [] for k in forms}
for _ in range(rounds):
    for k, f in forms.items():
        times[k].append(f.run(steps))
out = {"tool": "explicit_fbar_bench", "particles": int(forms["plain_non_folded"].S.np), "material": NH49, "dt": DT,
       "warm_up_runs": WARM, "rounds": rounds, "steps_per_run": steps,
       "ms_per_step": {k: [round(t, 4) for t in v] for k, v in times.items()},
       "median_ms_per_step": {k: round(float(np.median(v)), 4) for k, v in times.items()}}
k3 = {}
for k, f in forms.items():
    f.S.set_timing(True)
    v = []
    for _ in range(10):
        f.S.explicit_step(f.none, 0, DT, gravity=GRAVITY)
        ms = f.S.get_timing()
        v.append(ms[2] - ms[5])
    f.S.set_timing(False)
    k3[k] = round(float(np.median(v)), 4)
out["median_k3_bracket_ms"] = k3
med = out["median_ms_per_step"]
out["fbar_over_plain"] = {k: round(med[k] / med["plain_non_folded"], 3) for k in ("fbar_block1", "fbar_block2")}
out["k3_bracket_fbar_over_plain"] = {k: round(k3[k] / k3["plain_non_folded"], 3) for k in ("fbar_block1", "fbar_block2")}
for k, f in forms.items():
    st = f.S.download_state(["J_n"])
    out.setdefault("status_flags", {})[k] = f.S.status_flags()
    out.setdefault("J_range", {})[k] = [float(st["J_n"].min()), float(st["J_n"].max())]
    if k != "plain_non_folded":
        Jb = f.S.download_fbar()[1]
        out.setdefault("Jbar_range", {})[k] = [float(Jb.min()), float(Jb.max())]
for f in forms.values():
    f.S.close()
line = json.dumps(out)
print(line)
if len(args) > 3:
    with open(args[3], "w") as f:
        f.write(line + "\n")
