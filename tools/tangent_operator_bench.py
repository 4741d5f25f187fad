#!/usr/bin/env python3
"""Developer tool: the matrix-free tangent (nlps_gpu_tangent_operator / _apply / _block_diagonal) against the assembled
path (nlps_gpu_tangent_assemble + the COO triplets written on the device) on the bench cube, linearised after one fused
residual evaluation.  Prints one JSON line: per case setup ms, apply ms (median of 50), block-diagonal ms, assembled ms,
operator bytes against stencil + triplet bytes.
    python tools/tangent_operator_bench.py [cells=50] [big_cells=100]     (50: 1 M particles, 100: 8 M, Neo-Hookean only;
                                                                           big_cells=0 skips it)"""
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
big = int(sys.argv[2]) if len(sys.argv) > 2 else 100


def timed(S, fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        S.synchronize()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


def run(law, c, assembled):
    case = bench.build_case(0, 1, c)
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
    out = {"particles": int(case["cloud"]["x"].shape[0]), "nactive": int(S.nactive)}
    nb = S.tangent_operator(a[0], M, True)
    out["setup_ms"] = round(timed(S, lambda: S.tangent_operator(a[0], M, True), 5), 3)
    x = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    y = dev()
    S.tangent_apply(x, out=y)
    out["apply_ms"] = round(timed(S, lambda: S.tangent_apply(x, out=y), 50), 3)
    blocks = torch.empty((S.nactive, 3, 3), dtype=torch.float64, device="cuda")
    S.L.nlps_gpu_tangent_block_diagonal(S.h, nlps._vp(blocks))
    out["block_diagonal_ms"] = round(timed(S, lambda: S._chk(S.L.nlps_gpu_tangent_block_diagonal(S.h, nlps._vp(blocks))), 10), 3)
    out["operator_bytes"] = int(nb)
    nnodes = int(np.prod(case["grid_n"]))
    stencil = nnodes * 729 * (9 * 8 + 1)  # [nnodes][9^3][3x3] doubles + the visit bytes
    out["stencil_bytes"] = int(stencil)
    if assembled:
        holder = {}

        def assemble():
            holder["coo"] = S.jacobian_evaluation(a[0], M, True, on_device=True)

        out["assembled_ms"] = round(timed(S, assemble, 3), 3)
        nnz = int(holder["coo"][0].numel())
        out["triplet_bytes"] = nnz * 16
        del holder
        torch.cuda.empty_cache()
    S.close()
    return out


res = {"tool": "tangent_operator_bench", "nh_1m": run("neo-hookean", cells, True), "dp_1m": run("drucker-prager", cells, True)}
if big > 0:
    res["nh_8m"] = run("neo-hookean", big, False)  # (the assembled path would need ~170 GB here: not run)
print(json.dumps(res))
