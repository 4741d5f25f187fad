#!/usr/bin/env python3
"""Developer tool: the tangent in block CSR (nlps_gpu_tangent_bsr_pattern + nlps_gpu_tangent_bsr into device arrays),
every block and the upper blocks, against the CSR path (nlps_gpu_tangent_csr_pattern + nlps_gpu_tangent_csr) and the
atomic path (nlps_gpu_tangent_assemble + nlps_gpu_tangent_coo) on the bench cube, linearised after one fused residual
evaluation, Neo-Hookean and Drucker-Prager (the upper form: Neo-Hookean only).  The paths are timed alternately, each
on a linearisation of its own (an untimed nlps_gpu_tangent_operator before every timed path: the forms share their
per-particle records on one linearisation, and every figure here includes building them), median of `reps` rounds
after one warm-up round.  Prints one JSON line and, with out=, writes it to a file.

    python tools/tangent_bsr_bench.py [cells=50] [reps=5] [out=profiles/r21_tangent_bsr_bench.json] [parent=<libnlps_gpu.so>]

cells=50: 1 M particles.  parent= names a build of the PARENT commit's library: every path it has is then
timed in a fresh child process of this tool (NLPS_GPU_LIB), inside the same run, and the ratios are taken against those.
--profile [only=full|upper]: one warm-up round and one round only (for rocprofv3 --kernel-trace --stats, or counters)."""
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
only = opts.get("only")
have_bsr = hasattr(nlps.lib(), "nlps_gpu_tangent_bsr")


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
    out = {"particles": int(case["cloud"]["x"].shape[0]), "nactive": int(S.nactive), "nnodes": int(np.prod(case["grid_n"]))}
    keep = {}

    def atomic():
        keep["out"] = S.jacobian_evaluation(a[0], M, True, on_device=True)

    def csr():
        keep["nnz"], _ = S.tangent_csr_pattern()
        keep["out"] = S.tangent_csr(on_device=True)

    def bsr(kind):
        def go():
            keep["nblocks_" + kind], keep["bytes"] = S.tangent_bsr_pattern(kind)
            keep["out"] = S.tangent_bsr(col_major=True, on_device=True)
        return go

    paths = {"atomic": atomic, "csr": csr}
    if have_bsr:
        paths["bsr_full"] = bsr("full")
        if law == "neo-hookean":
            paths["bsr_upper"] = bsr("upper")
    if profile and only:
        paths = {"bsr_" + only: paths["bsr_" + only]}
    times = {k: [] for k in paths}
    for r in range(2 if profile else reps + 1):
        for k, fn in paths.items():
            keep.pop("out", None)  # (the last path's arrays go before the next ones are allocated)
            S.tangent_operator(a[0], M, True)  # (a linearisation of its own: nothing of another form to reuse)
            t = timed(S, fn)
            if r > 0:  # (round 0 warms every path up: first allocations, code objects)
                times[k].append(t)
            if k == "atomic":
                out["nnz"] = int(keep["out"][0].numel())
    for k, ts in times.items():
        out[k + "_ms"] = round(float(np.median(ts)), 3)
        out[k + "_ms_rounds"] = [round(t, 3) for t in ts]
    nnz = out.get("nnz", keep.get("nnz"))
    if have_bsr and not (profile and only):
        nb, nu = keep["nblocks_full"], keep.get("nblocks_upper")
        assert keep["nnz"] == nnz == 9 * nb
        out["kept_bytes"] = int(keep["bytes"])
        # bytes written per assembly, from the array lengths
        out["csr_output_bytes"] = 4 * (n + 1) + 12 * nnz
        out["bsr_full_output_bytes"] = 4 * (S.nactive + 1) + (4 + 72) * nb
        out["nblocks_full"] = int(nb)
        if nu is not None:
            assert nb == 2 * nu - S.nactive, "FULL = 2 UPPER - diagonal blocks (every active node holds its own)"
            out["nblocks_upper"] = int(nu)
            out["bsr_upper_output_bytes"] = 4 * (S.nactive + 1) + (4 + 72) * nu
            out["upper_over_full"] = round(out["bsr_upper_ms"] / out["bsr_full_ms"], 3)
    keep.clear()
    torch.cuda.empty_cache()
    S.close()
    return out


res = {"tool": "tangent_bsr_bench", "cells": cells, "reps": reps,
       "library": "another build (NLPS_GPU_LIB)" if os.environ.get("NLPS_GPU_LIB") else "this tree",
       "nh": run("neo-hookean")}
if not (profile and only):
    res["dp"] = run("drucker-prager")
if "parent" in opts and not os.environ.get("NLPS_GPU_LIB"):
    env = dict(os.environ, NLPS_GPU_LIB=os.path.abspath(opts["parent"]))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "cells=%d" % cells, "reps=%d" % reps], env=env,
                       capture_output=True, text=True, check=True)
    parent = json.loads(p.stdout.strip().splitlines()[-1])
    for law in ("nh", "dp"):
        r = res[law]
        assert parent[law]["nnz"] == r["nnz"]
        for k in ("csr", "atomic", "bsr_full", "bsr_upper"):
            if k + "_ms" not in parent[law]:  # (a parent without the block forms; the upper form: Neo-Hookean only)
                continue
            r["parent_%s_ms" % k] = parent[law][k + "_ms"]
            r["parent_%s_ms_rounds" % k] = parent[law][k + "_ms_rounds"]
            if k != "atomic":  # the same path on both sides
                r["%s_over_parent" % k] = round(r[k + "_ms"] / r["parent_%s_ms" % k], 3)
        r["full_over_parent_csr"] = round(r["bsr_full_ms"] / r["parent_csr_ms"], 3)
        if "bsr_upper_ms" in r:
            r["upper_over_parent_csr"] = round(r["bsr_upper_ms"] / r["parent_csr_ms"], 3)
            r["upper_over_parent_atomic"] = round(r["bsr_upper_ms"] / r["parent_atomic_ms"], 3)
line = json.dumps(res)
print(line)
if "out" in opts:
    with open(opts["out"], "w") as f:
        f.write(line + "\n")
