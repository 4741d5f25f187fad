#!/usr/bin/env python3
"""Developer tool: the explicit step of a fluid cloud (nlps_gpu_set_explicit_fluid) on the bench cube
(1 M particles, the FLUID of tests/test_gpu_fluid.py, gravity, dt = 1e-4).  Three handles that start from the same
geometry, in one process, each on a stream of its own:
  (a) fluid_explicit -- the fluid cloud, the switch on: the non-folded form of the step on one stream, K3 in MODE 7;
  (b) solid_non_folded -- a Neo-Hookean cloud in the form a fluid cloud runs (debug options lazy_nodal = 0), K3 in MODE 1;
  (c) fluid_newmark -- nlps_gpu_newmark_step on the fluid cloud, the only way to advance such a cloud without the switch.
Two warm-up runs, then `rounds` alternating runs of `steps` steps, each between two events on the handle's stream;
medians over the rounds.  Prints one JSON line and writes it to the file given as fourth argument.
    python tools/explicit_fluid_bench.py [cells=50] [rounds=5] [steps=10] [out.json]
    NLPS_GPU_LIB=<the parent commit's libnlps_gpu.so> python tools/explicit_fluid_bench.py cells rounds steps parent.json --solid-only
        (b) alone on another build of the library: shows that the solids' step did not move
    python tools/explicit_fluid_bench.py cells rounds steps out.json --parent parent.json
        the same run with the --solid-only result of the parent build copied into its line"""
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
flags = [a for a in sys.argv[1:] if a.startswith("--")]
cells = int(args[0]) if len(args) > 0 else 50
rounds = int(args[1]) if len(args) > 1 else 5
steps = int(args[2]) if len(args) > 2 else 10
DT, WARM = 1.0e-4, 2
FLUID = {"type": 6, "E": 0.0, "nu": 0.0, "p_ref": 1.0e3, "viscosity": 40.0, "compressibility": 2.0e5, "n_macdonald": 7.0}
GRAVITY = [0.0, -9.81, 0.0]
NEWMARK = dict(max_it=50, atol=1e-8, rtol=1e-10, stol=1e-8, linesearch="bt", ksp=dict(pc="jacobi", restart=30, max_it=10000, rtol=1e-5))


class Form:
    def __init__(self, fluid, newmark=False):
        case = bench.build_case(0, 1, cells)
        if fluid:
            case["materials"] = [FLUID]
        self.stream = torch.cuda.Stream()
        self.S = nlps.Solver(3, case["grid_n"], case["origin"], case["h"], case["cloud"], case["materials"], nsteps=1,
                             stream=self.stream.cuda_stream)
        self.S.initialise_shapefun()
        self.newmark = newmark
        if fluid and not newmark:
            self.S.set_explicit_fluid(True)
        if not fluid:
            self.S.debug_option("lazy_nodal", 0)
        self.none = nlps.BccSet([])

    def run(self, n):
        """ms per step, between two events on the handle's stream"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(self.stream)
        for _ in range(n):
            if self.newmark:
                self.S.newmark_step(self.none, 0, DT, GRAVITY, **NEWMARK)
            else:
                self.S.explicit_step(self.none, 0, DT, gravity=GRAVITY)
        b.record(self.stream)
        b.synchronize()
        return a.elapsed_time(b) / n


if "--solid-only" in flags:
    forms = {"solid_non_folded": Form(False)}
else:
    forms = {"fluid_explicit": Form(True), "solid_non_folded": Form(False), "fluid_newmark": Form(True, newmark=True)}
per_run = {k: (max(1, steps // 5) if f.newmark else steps) for k, f in forms.items()}  # (a Newmark step costs several explicit ones)
errors = {}
for _ in range(WARM):
    for k, f in list(forms.items()):
        try:
            f.run(per_run[k])
        except nlps.NlpsError as e:  # (a Newmark step that does not converge: reported, not timed)
            errors[k] = str(e)
            f.S.close()
            del forms[k]
times = {k: [] for k in forms}
for _ in range(rounds):
    for k, f in forms.items():
        times[k].append(f.run(per_run[k]))
out = {"tool": "explicit_fluid_bench", "library": "another build (NLPS_GPU_LIB)" if os.environ.get("NLPS_GPU_LIB") else "this tree", "particles": int(forms["solid_non_folded"].S.np),
       "dt": DT, "warm_up_runs": WARM, "rounds": rounds, "steps_per_run": per_run,
       "ms_per_step": {k: [round(t, 4) for t in v] for k, v in times.items()},
       "median_ms_per_step": {k: round(float(np.median(v)), 4) for k, v in times.items()}}
# the K3 bracket of nlps_gpu_set_timing (ms[2], less the calibration bracket ms[5]) over ten more steps of the two explicit
# forms: MODE 7 against MODE 1, outside the timed rounds (the brackets synchronise every step)
k3 = {}
for k, f in forms.items():
    if not f.newmark:
        f.S.set_timing(True)
        v = []
        for _ in range(10):
            f.S.explicit_step(f.none, 0, DT, gravity=GRAVITY)
            ms = f.S.get_timing()
            v.append(ms[2] - ms[5])
        f.S.set_timing(False)
        k3[k] = round(float(np.median(v)), 4)
out["median_k3_bracket_ms"] = k3
if "fluid_explicit" in forms:
    st = forms["fluid_explicit"].S.download_state(["J_n"])
    out["fluid_status_flags"] = forms["fluid_explicit"].S.status_flags()
    out["fluid_J_range"] = [float(st["J_n"].min()), float(st["J_n"].max())]
    med = out["median_ms_per_step"]
    out["fluid_over_solid"] = round(med["fluid_explicit"] / med["solid_non_folded"], 3)
    if "fluid_newmark" in med:
        out["newmark_over_fluid_explicit"] = round(med["fluid_newmark"] / med["fluid_explicit"], 2)
if errors:
    out["errors"] = errors
if "--parent" in flags:
    with open(sys.argv[sys.argv.index("--parent") + 1]) as f:
        parent = json.loads(f.readline())
    out["parent_library"] = {k: parent[k] for k in ("median_ms_per_step", "ms_per_step", "median_k3_bracket_ms")}
    out["solid_this_over_parent"] = round(out["median_ms_per_step"]["solid_non_folded"] /
                                          parent["median_ms_per_step"]["solid_non_folded"], 3)
for f in forms.values():
    f.S.close()
line = json.dumps(out)
print(line)
if len(args) > 3:
    with open(args[3], "w") as f:
        f.write(line + "\n")
