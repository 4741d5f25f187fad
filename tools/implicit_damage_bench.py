#!/usr/bin/env python3
"""Developer tool: the residual and the one-call Newmark step of a damage cloud with the fused damage residual
(nlps_gpu_set_implicit_damage) off and on, on the bench cube (1 M Neo-Hookean particles, dt = 1e-3), which is
given an expanding velocity field so that every principal stress is positive; driver_eigenerosion, no Dirichlet set, no
gravity, device-resident vectors.  Handles that start from the same cloud, in one process:
  residual   -- one nlps_gpu_lagrangian_evaluation at the explicit trial dU, Gf = the 75 % quantile of an estimate of G
                at that evaluation, so that about a quarter of the cloud fails (the share is reported): `reps`
                evaluations per round;
  newmark    -- one nlps_gpu_newmark_step per round (explicit trial, bt line search, SNES atol 1e-8 / rtol 1e-10 / stol
                1e-8, PCJACOBI, GMRES(30) at 1e-5): first for a Gf nobody reaches (1e300), then for the 75 % quantile
                of the estimate of G at the END of that dry series -- the field keeps stretching the cloud, so G grows
                from step to step and the failures spread over the timed steps towards a quarter of the cloud (the
                failed share after every timed step is reported).
The estimate of G_p = Ceps h sum(V W) / sum(V) over the epsilon-neighbourhood: the sums over the 3 x 3 x 3 block of grid
cells around the particle's cell (edge 3 h for a ball of radius Ceps h = 1.5 h), from a download of x, W, J and Vol_0.
After a warm-up each, `rounds` alternating rounds are timed with the host clock around work that ends in a synchronise;
medians over the rounds, and the spread (max - min) of every series.  Against a library without the switch (a build of
the parent commit, through NLPS_GPU_LIB) only the form that exists there is timed, on two alternating handles as the
two forms are, under the names "parent" and "parent_twin".  Prints one
JSON line and writes it to the file given as fourth argument.
    python tools/implicit_damage_bench.py [cells=50] [rounds=5] [reps=5] [out.json]
    python tools/implicit_damage_bench.py [cells] [rounds] [reps] [out.json] --deterministic
        the switch-on handle beside a twin with nlps_gpu_set_deterministic and nlps_gpu_set_deterministic_damage on
        (DESIGN.md 6b), under the names "on" and "on_deterministic": the same series and the ratios of the medians
    python tools/implicit_damage_bench.py cells steps --trace     (switch on, `steps` steps: for a kernel trace)"""
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
args = [a for a in sys.argv[1:] if not a.startswith("--")]
cells = int(args[0]) if len(args) > 0 else 50
rounds = int(args[1]) if len(args) > 1 else 5
reps = int(args[2]) if len(args) > 2 else 5
BETA, GAMMA, DT, CEPS, RATE = 0.25, 0.5, 1.0e-3, 1.5, 2.0
A = [1 / (BETA * DT * DT), 1 / (BETA * DT), (1 - 2 * BETA) / (2 * BETA), GAMMA / (BETA * DT), 1 - GAMMA / BETA,
     (1 - GAMMA / (2 * BETA)) * DT]
SNES = dict(max_it=50, atol=1e-8, rtol=1e-10, stol=1e-8, linesearch="bt", ksp=dict(pc="jacobi", restart=30, rtol=1e-5))
HAS_SWITCH = hasattr(nlps.lib(), "nlps_gpu_set_implicit_damage")
# (without the switch two handles of the one form alternate, as "off" and "on" do: two clouds of 1 M particles share the caches)
FORMS = ("off", "on") if HAS_SWITCH else ("parent", "parent_twin")
DET = "--deterministic" in sys.argv
if DET:
    FORMS = ("on", "on_deterministic")
none = nlps.BccSet([])


def solver(Gf, form, nst):
    case = bench.build_case(0, 1, cells)
    x = case["cloud"]["x"]
    u = np.random.default_rng(7).uniform(size=(x.shape[0], 1))
    case["cloud"]["vel"] = RATE * (x - x.mean(axis=0)) * (1.0 + 0.5 * u)
    case["materials"] = [dict(case["materials"][0], Ceps=CEPS, Gf=Gf)]
    prm = nlps.default_params()
    prm.driver_eigenerosion = 1
    S = nlps.Solver(3, case["grid_n"], case["origin"], case["h"], case["cloud"], case["materials"], params=prm, nsteps=nst)
    S.initialise_shapefun()
    if form in ("on", "on_deterministic"):
        S.set_implicit_damage(True)
    if form == "on_deterministic":
        S.set_deterministic(True)
        S.set_deterministic_damage(True)
    return case, S


class Residual:
    """a handle at the start of its first step, every vector on the device"""

    def __init__(self, Gf, form):
        self.case, self.S = solver(Gf, form, 1)
        S = self.S
        S.local_search()
        S.active_masks(none, 0, download=False)
        n = S.nactive * 3
        dev = lambda: torch.zeros(n, dtype=torch.float64, device="cuda")  # noqa: E731
        self.M, self.V, self.Ac, self.R = dev(), dev(), dev(), dev()
        S.compute_nodal_lumped_mass(out=self.M)
        S.get_nodal_field_n(self.M, self.V, self.Ac)
        self.dU = torch.from_numpy(S.form_initial_guess(self.V, self.Ac, DT, none, 0)).cuda()

    def run(self, n):
        S = self.S
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            S.lagrangian_evaluation(self.dU, self.V, self.Ac, self.M, A, None, None, 0, 1.0, None, out=self.R)
        S.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n


def step(S, t):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    info = S.newmark_step(none, t, DT, None, beta=BETA, gamma=GAMMA, **SNES)
    S.synchronize()
    return 1e3 * (time.perf_counter() - t0), info


def estimate_G(S, case, slot):
    """Ceps h sum(V W) / sum(V) over the 3 x 3 x 3 cells around every particle's cell (V = Vol_0 J of `slot`)"""
    st = S.download_state(["x_GC", "W", slot, "Vol_0"])
    h = case["h"]
    c = np.floor((st["x_GC"] - np.asarray(case["origin"])) / h).astype(np.int64)
    c -= c.min(axis=0) - 1  # (one empty rim cell on every side)
    dims = c.max(axis=0) + 2
    V = (st["Vol_0"] * st[slot]).ravel()
    sums = []
    for w in (V * st["W"].ravel(), V):
        g = np.zeros(dims)
        np.add.at(g, (c[:, 0], c[:, 1], c[:, 2]), w)
        for ax in range(3):
            g = g + np.roll(g, 1, axis=ax) + np.roll(g, -1, axis=ax)  # (the rim cells are empty: nothing wraps)
        sums.append(g[c[:, 0], c[:, 1], c[:, 2]])
    return CEPS * h * sums[0] / sums[1]


def quantile_Gf():
    r = Residual(1e300, FORMS[0])
    r.run(1)
    G = estimate_G(r.S, r.case, "J_n1")
    r.S.close()
    return float(np.quantile(G, 0.75))


def series(v):
    return {"ms": [round(t, 4) for t in v], "median_ms": round(float(np.median(v)), 4), "spread_ms": round(float(max(v) - min(v)), 4)}


if "--trace" in sys.argv:
    _, S = solver(quantile_Gf(), FORMS[-1], rounds + 1)
    for t in range(rounds):
        ms, info = step(S, t)
        print(t, info["reason_name"], info["iterations"], list(info["ksp_iterations"]), info["function_evaluations"])
    S.close()
    sys.exit(0)

Gf = quantile_Gf()
out = {"tool": "implicit_damage_bench", "library_has_the_switch": HAS_SWITCH, "dt": DT, "rounds": rounds,
       "evaluations_per_round": reps, "Gf": Gf}
# ---- one residual evaluation
res = {f: Residual(Gf, f) for f in FORMS}
for r in res.values():
    r.run(2)
times = {f: [] for f in FORMS}
for _ in range(rounds):
    for f, r in res.items():
        times[f].append(r.run(reps))
dmg = res[FORMS[-1]].S.download_state(["Damage_n1"])["Damage_n1"]
out["particles"] = int(dmg.size)
out["nactive"] = int(res[FORMS[-1]].S.nactive)
out["residual"] = {"failed_share": round(float(dmg.mean()), 4), "ms_per_evaluation": {f: series(v) for f, v in times.items()}}
for r in res.values():
    r.S.close()
del res
# ---- one Newmark step
out["newmark_step"] = {}
Gf_steps = 1e300
for label in ("Gf_nobody_reaches", "Gf_q75_of_G_at_the_end_of_the_dry_series"):
    made = {f: solver(Gf_steps, f, rounds + 2) for f in FORMS}
    hs = {f: m[1] for f, m in made.items()}
    times = {f: [] for f in FORMS}
    infos = {f: [] for f in FORMS}
    shares = {f: [] for f in FORMS}
    for t in range(rounds + 1):  # (step 0 warms the workspaces)
        for f, S in hs.items():
            ms, info = step(S, t)
            if t > 0:
                times[f].append(ms)
                infos[f].append({"reason": info["reason"], "newton": info["iterations"],
                                 "function_evaluations": info["function_evaluations"],
                                 "krylov": [int(k) for k in info["ksp_iterations"]]})
                shares[f].append(round(float(S.download_state(["Damage_n"])["Damage_n"].mean()), 4))
    failed = {f: round(float(S.download_state(["Damage_n"])["Damage_n"].mean()), 4) for f, S in hs.items()}
    out["newmark_step"][label] = {"Gf": Gf_steps, "failed_share_at_the_end": failed, "failed_share_after_each_step": shares,
                                  "ms_per_step": {f: series(v) for f, v in times.items()},
                                  "solves": infos}
    if Gf_steps == 1e300:
        Gf_steps = float(np.quantile(estimate_G(hs[FORMS[0]], made[FORMS[0]][0], "J_n"), 0.75))
    for S in hs.values():
        S.close()
if DET:
    ratio = lambda d: round(d["on_deterministic"]["median_ms"] / d["on"]["median_ms"], 3)  # noqa: E731
    out["deterministic_over_atomic"] = {"residual": ratio(out["residual"]["ms_per_evaluation"]),
                                        **{k: ratio(v["ms_per_step"]) for k, v in out["newmark_step"].items()}}
line = json.dumps(out)
print(line)
if len(args) > 3:
    with open(args[3], "w") as f:
        f.write(line + "\n")
