"""Worker of tests/test_gpu_step_record_multirank.py (launched by torch.distributed.run).

Every rank drives the HIP library on the SAME card for its slab of a z-stacked Neo-Hookean cloud (3-D), with the
ghost-node exchange of nl-partsol_amd/halo.py behind the C-ABI halo callback (gloo + host staging) and the node window of
its slab, as tests/mr_gpu_tangent_worker.py does.  Each rank takes three explicit steps with a step record of the particle
sums alone; rank 0 also runs the whole cloud in one solver.  Every particle lives on exactly one rank, so the ranks' sums
added must equal the whole cloud's row to 1e-12 of sum|term| (the whole cloud's terms, from a download), the counts
exactly, and the minima / maxima taken across the ranks to 1e-12 relative: a rank's particle state differs from the whole
cloud's by the order of the nodal sums only.  A record with a reaction set is refused on the rank handles."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ND, CELLS, MARGIN, NSTEPS = 3, 8, 5, 3
DT = 0.4 / 100.0


def rank_cloud(synth, rank, world):
    gc = [CELLS + 2 * MARGIN] * (ND - 1) + [CELLS * world + 2 * MARGIN]
    lo = [MARGIN] * (ND - 1) + [MARGIN + CELLS * rank]
    return gc, synth.make_cloud(ND, gc, lo, [CELLS] * ND, h=1.0, jitter=0.05, seed=777 + rank, velocity=[1.0, 0.5, -10.0])


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    import torch
    import torch.distributed as dist
    import step_record_ref as rr
    import util
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    nlps = util.nlps()
    synth = util.synth
    halo_mod = importlib.import_module("nl-partsol_amd.halo")
    gc, cloud = rank_cloud(synth, rank, world)
    gn = synth.grid_nodes(gc)
    nnodes = int(np.prod(gn))
    mats = [util.NH]
    bc = {"nodes": synth.plane_nodes(gn, ND - 1, MARGIN + 1), "dim": ND, "dir": np.ones((ND, NSTEPS), dtype=np.int32),
          "value": np.zeros((ND, NSTEPS))}
    gb = nlps.BccSet([bc])
    work_stream = torch.cuda.Stream()  # library kernels and callback ops share one real stream
    torch.cuda.set_stream(work_stream)
    S = nlps.Solver(ND, gn, [0.0] * ND, 1.0, cloud, mats, nsteps=NSTEPS, stream=work_stream.cuda_stream)
    lo, hi = halo_mod.SlabHalo.layer_ranges(world, CELLS, MARGIN, gn[ND - 1], reach=3)
    halo = halo_mod.SlabHalo(torch, dist, rank, world, nnodes // gn[ND - 1], gn[ND - 1], lo, hi)
    band_lo, band_hi = halo.ghost_bands(rank)
    S.set_halo_exchange(lambda dptr, nfield, elem, kind, phase: halo.exchange_ptr(dptr, nnodes * nfield, nfield, elem,
                                                                                 kind, phase))
    S.set_node_window(lo[rank], hi[rank])
    S.set_ghost_bands(band_lo, band_hi, True)
    S.initialise_shapefun()
    refused = False
    try:
        S.set_step_record(every=1, capacity=NSTEPS, nsets=1)
    except nlps.NlpsError as e:
        refused = "built for one rank" in str(e)
    assert refused, "a record with a reaction set on a slab rank"
    S.set_step_record(every=1, capacity=NSTEPS)
    for t in range(NSTEPS):
        S.explicit_step(gb, t, DT)
    assert S.status_flags() == 0
    mine = S.read_step_records()
    assert mine["total"] == NSTEPS and mine["count"] == NSTEPS
    parts = [None] * world
    dist.gather_object(mine, parts if rank == 0 else None, dst=0)
    if rank == 0:
        clouds = [rank_cloud(synth, r, world)[1] for r in range(world)]
        whole = {}
        for k, v in clouds[0].items():
            whole[k] = np.concatenate([c[k] for c in clouds]) if isinstance(v, np.ndarray) else v
        G = nlps.Solver(ND, gn, [0.0] * ND, 1.0, whole, mats, nsteps=NSTEPS)
        G.initialise_shapefun()
        G.set_step_record(every=1, capacity=NSTEPS)
        worst = 0.0
        for t in range(NSTEPS):
            G.explicit_step(gb, t, DT)
            st = G.download_state()
            row = {k: v[-1] for k, v in G.read_step_records().items() if isinstance(v, np.ndarray)}
            for name, terms in rr.sums(st, ND).items():
                got, scale = sum(p[name][t] for p in parts), np.abs(terms).sum(axis=0)
                err = np.abs(got - row[name])
                worst = max(worst, float(np.max(err / np.maximum(scale, 1e-300))))
                assert np.all(err <= 1e-12 * scale), "step %d %s: ranks %r, whole %r, sum|term| %r" % (t, name, got, row[name], scale)
            for name in ("np", "failed"):
                assert sum(p[name][t] for p in parts) == row[name], name
            for name, pick in (("vmax_comp", max), ("vmax_norm", max), ("J_min", min), ("J_max", max), ("EPS_max", max),
                               ("Damage_max", max)):
                got = pick(p[name][t] for p in parts)
                assert abs(got - row[name]) <= 1e-12 * abs(row[name]), "step %d %s: ranks %r, whole %r" % (t, name, got, row[name])
            for name in ("step", "kind", "dt", "time"):
                assert all(p[name][t] == row[name] for p in parts), name
        assert G.status_flags() == 0
        print("MULTIRANK_RECORD_OK world=%d particles=%d worst=%.2e" % (world, whole["x"].shape[0], worst))
    dist.barrier()
    dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
