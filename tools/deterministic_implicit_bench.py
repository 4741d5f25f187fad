#!/usr/bin/env python3
"""Developer tool: what nlps_gpu_set_deterministic costs on the implicit path.  The bench cube (1 M Neo-Hookean particles,
dt = 1e-3), two handles from the same cloud -- one with the mode off, one with it on --, torch device vectors.  After a
warm-up, `rounds` alternating rounds time on each handle, with the host clock around work that ends in a synchronise:
  one fused residual (nlps_gpu_lagrangian_evaluation), one K x (nlps_gpu_tangent_apply), one block diagonal, the lumped
  mass plus the nodal field, and -- on a second pair of handles, since it moves the particles -- one nlps_gpu_newmark_step.
Prints one JSON line (medians per mode, their ratios, whether the deterministic figures repeated bit for bit over the
rounds, and the bytes of window slabs the mode holds) and writes it to the file given as third argument.
    python tools/deterministic_implicit_bench.py [cells=50] [rounds=7] [out.json]"""
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
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
BETA, GAMMA, DT = 0.25, 0.5, 1.0e-3
A = [1 / (BETA * DT * DT), 1 / (BETA * DT), (1 - 2 * BETA) / (2 * BETA), GAMMA / (BETA * DT), 1 - GAMMA / BETA,
     (1 - GAMMA / (2 * BETA)) * DT]
GRAV = [0.0, 0.0, -9.81]
SNES = dict(max_it=50, atol=1e-8, rtol=1e-10, stol=1e-8, linesearch="basic", ksp=dict(pc="jacobi", restart=30, rtol=1e-5))
MODES = ("atomic", "deterministic")


def setup(nst, deterministic):
    case = bench.build_case(0, 1, cells)
    S = nlps.Solver(3, case["grid_n"], case["origin"], case["h"], case["cloud"], case["materials"], nsteps=nst)
    S.initialise_shapefun()
    S.set_deterministic(deterministic)
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


class Stage:
    """A handle at the start of step 1 with device vectors; every timed call leaves the particles where they are."""

    def __init__(self, deterministic):
        self.case, self.S, self.gb = setup(2, deterministic)
        S = self.S
        S.local_search()
        S.active_masks(self.gb, 1, download=False)
        n = S.nactive * 3
        dev = lambda: torch.zeros(n, dtype=torch.float64, device="cuda")  # noqa: E731
        self.M, self.V, self.Ac, self.R, self.y = dev(), dev(), dev(), dev(), dev()
        self.mass_and_field()
        self.dU = torch.from_numpy(S.form_initial_guess(self.V, self.Ac, DT, self.gb, 1)).cuda()
        self.x = torch.from_numpy(np.random.default_rng(1).normal(size=n)).cuda()
        self.residual()
        S.tangent_operator(A[0], self.M, True)

    def mass_and_field(self):
        self.S.compute_nodal_lumped_mass(out=self.M)
        self.S.get_nodal_field_n(self.M, self.V, self.Ac)

    def residual(self):
        self.S.lagrangian_evaluation(self.dU, self.V, self.Ac, self.M, A, GRAV, None, 1, 1.0, None, out=self.R)

    def product(self):
        self.S.tangent_apply(self.x, out=self.y)

    def blocks(self):
        self.B = self.S.tangent_block_diagonal(on_device=True)


stages = {m: Stage(m == "deterministic") for m in MODES}
case = stages["atomic"].case
what = ("residual", "tangent_apply", "block_diagonal", "mass_and_field")
times = {m: {w: [] for w in what} for m in MODES}
repeat = {w: True for w in what}
first = {}
for r in range(rounds + 1):  # (round 0 warms both handles)
    for m in MODES:
        st = stages[m]
        for w, fn, res in (("mass_and_field", st.mass_and_field, lambda s: torch.cat([s.M, s.V, s.Ac])),
                           ("residual", st.residual, lambda s: s.R), ("tangent_apply", st.product, lambda s: s.y),
                           ("block_diagonal", st.blocks, lambda s: s.B.reshape(-1))):
            t, _ = wall(st.S, fn)
            if r > 0:
                times[m][w].append(t)
            if m == "deterministic":
                v = res(st).clone()
                if w in first:
                    repeat[w] = repeat[w] and bool(torch.equal(v, first[w]))
                else:
                    first[w] = v
nactive = int(stages["atomic"].S.nactive)
for st in stages.values():
    st.S.close()
del stages, first

# the one-call step moves the particles: its own pair of handles, one step per round
steps = {}
handles = {m: setup(rounds + 2, m == "deterministic") for m in MODES}
infos = {m: [] for m in MODES}
for step in range(1, rounds + 2):
    for m in MODES:
        _, S, gb = handles[m]
        t, info = wall(S, lambda: S.newmark_step(gb, step, DT, GRAV, beta=BETA, gamma=GAMMA, **SNES))
        if step > 1:
            steps.setdefault(m, []).append(t)
            infos[m].append({"reason": info["reason"], "newton": info["iterations"],
                             "krylov": [int(k) for k in info["ksp_iterations"]]})
for _, S, _ in handles.values():
    S.close()

med = lambda v: round(float(np.median(v)), 4)  # noqa: E731
grid_n = case["grid_n"]
ntiles = int(np.prod([(int(n) + 3) // 4 for n in grid_n]))
# fields per window of the largest user (12: the explicit step's four force slabs of d fields; the block diagonal needs
# d^2 = 9) x 800 slots of a 3-D accumulator window x 8 bytes, per tile of 4^3 closest nodes
slab_bytes = ntiles * 12 * 800 * 8
out = {"tool": "deterministic_implicit_bench", "particles": int(case["cloud"]["x"].shape[0]), "nactive": nactive, "dt": DT,
       "rounds": rounds, "tiles": ntiles, "slab_bytes": slab_bytes,
       "median_ms": {m: dict({w: med(times[m][w]) for w in what}, newmark_step=med(steps[m])) for m in MODES},
       "deterministic_repeats_bit_for_bit": repeat, "newmark": infos}
out["ratio"] = {w: round(out["median_ms"]["deterministic"][w] / out["median_ms"]["atomic"][w], 3)
                for w in what + ("newmark_step",)}
line = json.dumps(out)
print(line)
if len(sys.argv) > 3:
    with open(sys.argv[3], "w") as f:
        f.write(line + "\n")
