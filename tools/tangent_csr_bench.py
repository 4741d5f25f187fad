#!/usr/bin/env python3
"""Developer tool: the tangent in CSR (nlps_gpu_tangent_csr_pattern + nlps_gpu_tangent_csr into device arrays) against
the atomic path (nlps_gpu_tangent_assemble + nlps_gpu_tangent_coo into device arrays) on the bench cube, linearised
after one fused residual evaluation, Neo-Hookean and Drucker-Prager.  The two paths are timed alternately, median of
`reps` rounds after one warm-up round.  Prints one JSON line and, with out=, writes it to a file.

    python tools/tangent_csr_bench.py [cells=50] [reps=5] [out=profiles/r20_tangent_csr_bench.json] [parent=<libnlps_gpu.so>]

cells=50: 1 M particles.  parent= names a build of the PARENT commit's library: the atomic path is then also timed on it, in
a fresh child process of this tool (NLPS_GPU_LIB), inside the same run, and the ratio is taken against that figure.
--profile: one warm-up round and one round of each path only (for rocprofv3 --kernel-trace --stats, or counters)."""
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

nlps = importlib.import_module("nl-partsol_amd.nlps")
synth = importlib.import_module("nl-partsol_amd.synth")
opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
cells, reps = int(opts.get("cells", 50)), int(opts.get("reps", 5))
profile = "--profile" in sys.argv
have_csr = hasattr(nlps.lib(), "nlps_gpu_tangent_csr")


def timed(S, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    S.synchronize()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def run(law):
    case = bench.build_case(0, 1, cells)
    if law == "drucker-prager":
        case["materials"] = [synth.drucker_prager_material()]
    nst = 4
    S = nlps.Solver(3, case["grid_n"], case["origin"], case["h"], case["cloud"], case["materials"], nsteps=nst)
    S.initialise_shapefun()
    nodes = synth.plane_nodes(case["grid_n"], 2, 0)
    gb = nlps.BccSet([{"nodes": nodes, "dim": 3, "dir": np.ones((3, nst), dtype=np.int32), "value": np.zeros((3, nst))}])
    beta, gamma, dt = 0.25, 0.5, 1.0e-3
    a = [1 / (beta * dt * dt), 1 / (beta * dt), (1 - 2 * beta) / (2 * beta), gamma / (beta * dt), 1 - gamma / beta,
         (1 - gamma / (2 * beta)) * dt]
    S.local_search()
    S.active_masks(gb, 1, download=False)
    n = S.nactive * 3
    dev = lambda: torch.zeros(n, dtype=torch.float64, device="cuda")  # noqa: E731
    M, V, A, R = dev(), dev(), dev(), dev()
    S.compute_nodal_lumped_mass(out=M)
    S.get_nodal_field_n(M, V, A)
    g = torch.Generator(device="cuda").manual_seed(3)
    dU = 1e-4 * torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    S.lagrangian_evaluation(dU, V, A, M, a, [0.0, 0.0, -9.81], None, 1, 1.0, None, out=R)
    nnodes = int(np.prod(case["grid_n"]))
    out = {"particles": int(case["cloud"]["x"].shape[0]), "nactive": int(S.nactive), "nnodes": nnodes}
    keep = {}

    def atomic():
        keep.pop("coo", None)  # (the last round's triplets go before the next ones are allocated)
        keep["coo"] = S.jacobian_evaluation(a[0], M, True, on_device=True)

    def csr():
        keep.pop("csr", None)
        keep["nnz"], keep["bytes"] = S.tangent_csr_pattern()
        keep["csr"] = S.tangent_csr(on_device=True)

    if have_csr:
        out["operator_ms"] = round(timed(S, lambda: S.tangent_operator(a[0], M, True)), 3)
    t_atomic, t_csr = [], []
    for r in range(2 if profile else reps + 1):
        ta = timed(S, atomic)
        tc = timed(S, csr) if have_csr else 0.0
        if r > 0:  # (round 0 warms both paths up: first allocations, code objects)
            t_atomic.append(ta)
            t_csr.append(tc)
    nnz = int(keep["coo"][0].numel())
    out["nnz"] = nnz
    out["atomic_assemble_coo_ms"] = round(float(np.median(t_atomic)), 3)
    out["atomic_ms_rounds"] = [round(t, 3) for t in t_atomic]
    out["atomic_path_bytes"] = 8 * 9 * (729 * nnodes + nnz // 9)  # 8 d^2 (9^d nnodes + blocks)
    if have_csr:
        assert keep["nnz"] == nnz
        out["csr_pattern_plus_csr_ms"] = round(float(np.median(t_csr)), 3)
        out["csr_ms_rounds"] = [round(t, 3) for t in t_csr]
        out["csr_bytes"] = int(keep["bytes"])
        out["csr_output_bytes"] = 4 * (n + 1) + 12 * nnz
        # the same matrix: y = K x through both forms
        rows, cols, vals = keep["coo"]
        rp, cc, vv = keep["csr"]
        x = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
        y_coo = torch.zeros(n, dtype=torch.float64, device="cuda").index_add_(0, rows.long(), vals * x[cols.long()])
        crow = torch.repeat_interleave(torch.arange(n, device="cuda"), (rp[1:] - rp[:-1]).long())
        y_csr = torch.zeros(n, dtype=torch.float64, device="cuda").index_add_(0, crow, vv * x[cc.long()])
        out["Kx_csr_vs_coo"] = float((y_csr - y_coo).abs().max() / y_coo.abs().max())
    keep.clear()
    torch.cuda.empty_cache()
    S.close()
    return out


res = {"tool": "tangent_csr_bench", "cells": cells, "reps": reps,
       "library": "another build (NLPS_GPU_LIB)" if os.environ.get("NLPS_GPU_LIB") else "this tree",
       "nh": run("neo-hookean"), "dp": run("drucker-prager")}
if "parent" in opts and not os.environ.get("NLPS_GPU_LIB"):
    env = dict(os.environ, NLPS_GPU_LIB=os.path.abspath(opts["parent"]))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "cells=%d" % cells, "reps=%d" % reps], env=env,
                       capture_output=True, text=True, check=True)
    parent = json.loads(p.stdout.strip().splitlines()[-1])
    for law in ("nh", "dp"):
        res[law]["parent_atomic_assemble_coo_ms"] = parent[law]["atomic_assemble_coo_ms"]
        res[law]["parent_atomic_ms_rounds"] = parent[law]["atomic_ms_rounds"]
        assert parent[law]["nnz"] == res[law]["nnz"]
        res[law]["csr_over_parent_atomic"] = round(res[law]["csr_pattern_plus_csr_ms"] / parent[law]["atomic_assemble_coo_ms"], 3)
line = json.dumps(res)
print(line)
if "out" in opts:
    with open(opts["out"], "w") as f:
        f.write(line + "\n")
