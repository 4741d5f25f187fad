#!/usr/bin/env python3
"""Developer tool: the explicit step with the damage hooks (nlps_gpu_set_explicit_damage) on the bench cube
(1 M Neo-Hookean particles, dt = 1e-3), which is given an expanding velocity field so that every principal stress is
positive.  Three handles that start from the same cloud, in one process:
  (a) plain -- a handle without the driver, the non-folded form of the explicit step (debug option lazy_nodal = 0);
  (b) damage, nobody fails -- driver_eigenerosion, the switch on, Gf = 1e300;
  (c) damage, about a quarter fails -- Gf = the 75 % quantile of Ceps h W of a first step (G_p is a volume-weighted mean
      of W over the epsilon-neighbourhood times Ceps h); the failed share that results is reported.
After `warm` steps each, `rounds` alternating rounds of `steps` steps are timed with the host clock around work that ends
in a synchronise; medians over the rounds.  Prints one JSON line and writes it to the file given as fourth argument.
    python tools/explicit_damage_bench.py [cells=50] [rounds=5] [steps=10] [out.json]
    python tools/explicit_damage_bench.py [cells] [rounds] [steps] [out.json] --deterministic
        handle (c) beside a twin with nlps_gpu_set_deterministic and nlps_gpu_set_deterministic_damage on:
        the same rounds, the ratio of the medians, and whether the two damage fields are equal at the end
    python tools/explicit_damage_bench.py cells steps --trace
        for a kernel trace of its own: `steps` level-B force evaluations of the driver cloud (search, masks,
        compatibility, constitutive update, internal forces with the hook: two sorts, k_node_ranges, k_damage,
        kb_fint_tile) and then `steps` damage steps (k_run_*, k_damage, k3f_tile)"""
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
steps = int(args[2]) if len(args) > 2 else 10
DT, CEPS, RATE, WARM = 1.0e-3, 1.5, 2.0, 3


def make_case(Gf):
    case = bench.build_case(0, 1, cells)
    x = case["cloud"]["x"]
    u = np.random.default_rng(7).uniform(size=(x.shape[0], 1))
    case["cloud"]["vel"] = RATE * (x - x.mean(axis=0)) * (1.0 + 0.5 * u)
    case["materials"] = [dict(case["materials"][0], Ceps=CEPS, Gf=Gf)]
    return case


def solver(Gf, driver, nst, deterministic=False):
    case = make_case(Gf)
    prm = nlps.default_params()
    if driver:
        prm.driver_eigenerosion = 1
    S = nlps.Solver(3, case["grid_n"], case["origin"], case["h"], case["cloud"], case["materials"], params=prm, nsteps=nst)
    S.initialise_shapefun()
    if driver:
        S.set_explicit_damage(True)
        if deterministic:
            S.set_deterministic(True)
            S.set_deterministic_damage(True)
    else:
        S.debug_option("lazy_nodal", 0)
    return case, S


def run(S, none, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        S.explicit_step(none, 0, DT)
    S.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


def quantile_Gf(none):
    case, S = solver(1e300, True, 1)
    S.explicit_step(none, 0, DT)
    W = S.download_state(["W"])["W"]
    S.close()
    return float(np.quantile(CEPS * case["h"] * W, 0.75))


none = nlps.BccSet([])
if "--trace" in sys.argv:
    n = rounds
    Gf = quantile_Gf(none)
    _, L = solver(Gf, True, 1)
    dU = None
    for _ in range(n):
        L.local_search()
        L.active_masks(none, 0, download=False)
        if dU is None:
            dU = torch.zeros(L.nactive * 3, dtype=torch.float64, device="cuda")
        L.local_compatibility_conditions(dU)
        L.constitutive_update()
        L.nodal_internal_forces(torch.zeros_like(dU))
    L.synchronize()
    L.close()
    _, S = solver(Gf, True, 1)
    run(S, none, n)
    S.close()
    sys.exit(0)

Gf = quantile_Gf(none)
DET = "--deterministic" in sys.argv
if DET:
    forms = {"damage_quarter_fails": solver(Gf, True, 1)[1], "damage_quarter_fails_deterministic": solver(Gf, True, 1, True)[1]}
else:
    forms = {"plain": solver(1e300, False, 1)[1], "damage_none_fails": solver(1e300, True, 1)[1],
             "damage_quarter_fails": solver(Gf, True, 1)[1]}
for S in forms.values():
    run(S, none, WARM)
times = {k: [] for k in forms}
for _ in range(rounds):
    for k, S in forms.items():
        times[k].append(run(S, none, steps))
dmg = forms["damage_quarter_fails"].download_state(["Damage_n"])["Damage_n"]
out = {"tool": "explicit_damage_bench", "particles": int(dmg.size), "dt": DT, "rounds": rounds, "steps_per_round": steps,
       "Gf": Gf, "failed_share_at_the_end": round(float(dmg.mean()), 4),
       "ms_per_step": {k: [round(t, 4) for t in v] for k, v in times.items()},
       "median_ms_per_step": {k: round(float(np.median(v)), 4) for k, v in times.items()}}
if DET:
    med = out["median_ms_per_step"]
    twin = forms["damage_quarter_fails_deterministic"].download_state(["Damage_n"])["Damage_n"]
    out["deterministic_over_atomic"] = round(med["damage_quarter_fails_deterministic"] / med["damage_quarter_fails"], 3)
    out["damage_fields_equal"] = bool(np.array_equal(dmg, twin))
for S in forms.values():
    S.close()
line = json.dumps(out)
print(line)
if len(args) > 3:
    with open(args[3], "w") as f:
        f.write(line + "\n")
