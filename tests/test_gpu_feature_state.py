"""The feature state of the handle across set, replace, drop and re-sort: the explicit loads, the probes of the step record
and the snapshot pack share ONE caller's-index -> slot map, which a re-sort voids for all of them, and the node runs of the
damage hooks are dropped by the mode switches.  Nothing here is held to a tolerance: every handle runs in deterministic
mode, where equal inputs give equal bits, so a feature that left something behind on another one, or read a stale map,
shows as a difference.

Every run takes NSTEPS steps with a re-sort interval of 2 and one explicit resort() in front of step MID.  The contour
and Dirichlet tables of explicit_loads_ref.py hold four steps, the first of them ten times longer than the others: the
runs go through the table once and then repeat its short steps (TABLE_STEP).

A download re-makes rho (see test_gpu_step_record.py, "the record leaves the lazy state alone"), so handles that are
compared download at the same steps."""
import numpy as np
import pytest

import explicit_damage_ref as xr
import explicit_loads_ref as lr
from test_gpu_explicit_damage import damage_solver
from test_gpu_explicit_loads import NODAL, loaded_solver, results, step
from test_gpu_snapshot import per_particle_bytes
from test_gpu_step_record import ALL, probe_ids
from util import nlps

pytestmark = pytest.mark.gpu

NSTEPS, MID = 8, 4
TABLE_STEP = (0, 1, 2, 3, 1, 2, 3, 1)  # the step of the four-step tables that run step t takes
assert len(TABLE_STEP) == NSTEPS and max(TABLE_STEP) < lr.NSTEPS


TILE_EDGE = {2: 16, 3: 4}  # nodes per tile edge (TileCfg<ND>::TB)


def sort_key(case, x, i0):
    """The key resort() sorts the slots by, restated from k_sort_keys: (tile of the closest node, corner type, closest
    node inside the tile), all three with the first axis fastest.  Corner type: bit a is set when the closest node lies
    above the particle's cell along axis a."""
    nd, n, tb = case["ndim"], np.asarray(case["grid_n"])[: case["ndim"]], TILE_EDGE[case["ndim"]]
    ijk = np.stack([i0 % n[0], (i0 // n[0]) % n[1]] + ([i0 // (n[0] * n[1])] if nd == 3 else []), axis=1).astype(np.int64)
    cell = np.clip(np.floor((x - np.asarray(case["origin"])) / case["h"]).astype(np.int64), 0, n - 2)
    nt = (n + tb - 1) // tb
    kt = kn = kc = 0
    mt = mn = mc = 1
    for a in range(nd):
        kt, mt = kt + mt * (ijk[:, a] // tb), mt * nt[a]
        kn, mn = kn + mn * (ijk[:, a] % tb), mn * tb
        kc, mc = kc + mc * (ijk[:, a] > cell[:, a]), mc * 2
    return (kt * mc + kc) * mn + kn


def assert_slots_permuted(S, case, what):
    """resort() has just put the slots in non-decreasing order of sort_key (a stable sort of the keys, nothing else).  Along
    the caller's order the key is NOT non-decreasing, so the slot order is not the caller's order, and an identity map in
    place of the inverse permutation would address other particles.  (download_ids cannot show this: on a handle that
    has not migrated it returns the caller's own numbering whatever the slots are.)"""
    st = S.download_state(["x_GC", "I0"])
    key = sort_key(case, st["x_GC"], st["I0"])
    descents = int(np.count_nonzero(np.diff(key) < 0))
    assert descents > 0, f"{what}: the caller's order is already the sorted one"


def prepare(case):
    """-> what every handle of these tests does before its first step"""
    def go(S):
        S.set_deterministic(True)
        S.resort()
        S.set_resort_interval(2)
        assert_slots_permuted(S, case, "behind the first re-sort")
    return go


def run(S, bset, each=None):
    for t in range(NSTEPS):
        if t == MID:
            S.resort()
        step(S, bset, TABLE_STEP[t])
        if each:
            each(t)


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), f"{what}: {int(np.sum(a != b))} of {a.size} entries differ"


def same_results(A, B, what):
    (na, sa), (nb, sb) = results(A), results(B)
    for k in NODAL:
        same(na[k], nb[k], f"{what}: nodal {k}")
    for k, v in sa.items():
        if isinstance(v, np.ndarray):
            same(v, sb[k], f"{what}: {k}")


def record(S, probes):
    S.set_step_record(every=1, capacity=NSTEPS, nsets=1, probes=probes, probe_fields=ALL)


# The handles of the scenarios (tools/solver_digest.py digests the same ones).  Each -> (handle, its Dirichlet sets).
def had_loads(case, probes):
    """a record; loads were set and removed again"""
    n = nlps()
    S, bset = loaded_solver(case, None, prepare(case))
    record(S, probes)
    S.set_explicit_loads(n.BccSet(lr.contours(case)), lr.THICKNESS, lr.area0(case))
    S.set_explicit_loads(None)
    return S, bset


def had_record(case, probes):
    """loads; a record was set and dropped again"""
    S, bset = loaded_solver(case, prepare=prepare(case))
    record(S, probes)
    S.set_step_record(every=None)
    return S, bset


def carrying(case, probes, users, by_caller=1):
    """loads, and of "record" and "snapshots" those named in `users`.  The loads are physics, so every handle of a
    comparison carries them; what a handle lacks is the other users of the map."""
    S, bset = loaded_solver(case, prepare=prepare(case))
    if "record" in users:
        record(S, probes)
    if "snapshots" in users:
        S.debug_option("snapshot_by_caller", by_caller)
        S.set_snapshots(nlps().SNAP_ALL, 2)
    return S, bset


def run_with_downloads(S, bset, snapshots, what):
    """run() with a download behind every step (every handle of a comparison: see the header) and, with `snapshots`, a
    snapshot in front of it, which is checked against that download; -> the snapshots"""
    snaps = []

    def each(t):
        slot = S.snapshot_begin(t) if snapshots else None
        ref = S.download_state()
        if slot is None:
            return
        snap = S.snapshot_wait(slot)
        assert snap.pop("tag") == t
        for f in snap:
            same(snap[f], ref[f], f"{what}: snapshot of step {t} against the download, {f}")
        snaps.append(snap)
        S.snapshot_release(slot)
    run(S, bset, each)
    return snaps


# 1. the map outlives whichever of its users goes first
@pytest.mark.parametrize("ndim", [2, 3])
def test_record_and_loads_come_and_go(ndim):
    n = nlps()
    case = lr.loaded_case(ndim)
    probes = probe_ids(case["cloud"]["x"].shape[0])
    # record, then loads set and removed, against a record alone
    (A, ba), (B, bb) = had_loads(case, probes), loaded_solver(case, None, prepare(case))
    record(B, probes)
    run(A, ba)
    run(B, bb)
    ra, rb = A.read_step_records(), B.read_step_records()
    assert ra["total"] == rb["total"] == NSTEPS and ra["count"] == NSTEPS
    same(ra["rows"], rb["rows"], "rows of the handle that had loads for a while")
    assert np.abs(rb["probes"]).max() > 0.0 and not np.array_equal(rb["probes"][0], rb["probes"][-1])
    same_results(A, B, "state of the handle that had loads for a while")
    # loads, then a record set and dropped, against loads alone
    (C, bc), (D, bd) = had_record(case, probes), loaded_solver(case, prepare=prepare(case))
    run(C, bc)
    run(D, bd)
    same_results(C, D, "state of the handle that had a record for a while")
    with pytest.raises(n.NlpsError, match="no step record is set"):
        C.read_step_records()
    for S in (A, B, C, D):
        S.close()


# 2. and 4. the three users of the map on one handle, both mappings of the snapshot pack
def together(ndim, by_caller):
    case = lr.loaded_case(ndim)
    probes = probe_ids(case["cloud"]["x"].shape[0])
    users = {"all": ("record", "snapshots"), "loads": (), "record": ("record",), "snapshots": ("snapshots",)}
    handles = {k: carrying(case, probes, u, by_caller) for k, u in users.items()}
    snaps = {k: run_with_downloads(S, bset, "snapshots" in users[k], k) for k, (S, bset) in handles.items()}
    assert len(snaps["all"]) == len(snaps["snapshots"]) == NSTEPS
    for t, (a, b) in enumerate(zip(snaps["all"], snaps["snapshots"])):
        for f in a:
            same(a[f], b[f], f"snapshot of step {t} with and without the other users, {f}")
    ra, rb = handles["all"][0].read_step_records(), handles["record"][0].read_step_records()
    assert ra["total"] == rb["total"] == NSTEPS
    same(ra["rows"], rb["rows"], "rows with and without the other users")
    for k in ("loads", "record", "snapshots"):
        same_results(handles["all"][0], handles[k][0], f"final state against the handle with {k} alone")
    for S, _ in handles.values():
        S.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_loads_probes_and_snapshots_together(ndim):
    together(ndim, 1)


@pytest.mark.parametrize("ndim", [2, 3])
def test_the_same_with_the_pack_by_slot(ndim):
    together(ndim, 0)


# 3. snapshots dropped with a slot begun, then set again
def test_snapshots_dropped_in_flight_and_set_again():
    n = nlps()
    case = lr.loaded_case(3)
    S, bset = loaded_solver(case, prepare=prepare(case))

    def bytes_of(mask, slots):
        per = per_particle_bytes(mask, 3)
        return slots * S.np * per + 4 * S.np, slots * S.np * per  # (the header's formula; + the inverse permutation)

    S.set_snapshots(n.SNAP_ALL, 2)
    assert S.snapshot_bytes() == bytes_of(n.SNAP_ALL, 2)
    for t in range(3):
        step(S, bset, t)
    S.snapshot_begin(1)
    S.set_snapshots(None)  # with the copy in flight
    for call in (lambda: S.snapshot_begin(0), S.snapshot_bytes):
        with pytest.raises(n.NlpsError, match="no snapshots are set"):
            call()
    step(S, bset, 3)  # (the step behind the interval re-sorts)
    mask = n.snapshot_mask(["x", "vel", "Stress", "I0"])
    S.set_snapshots(mask, 3)
    assert S.snapshot_bytes() == bytes_of(mask, 3)
    step(S, bset, 0)
    slot = S.snapshot_begin(5)
    ref = S.download_state()
    snap = S.snapshot_wait(slot)
    assert snap["tag"] == 5 and sorted(snap) == ["I0", "Stress", "tag", "vel", "x", "x_GC"]
    for f in snap:
        if f != "tag":
            same(snap[f], ref[f], f"behind the second set: {f}")
    S.snapshot_release(slot)
    S.close()


# 5. the node runs of the damage hooks under re-sorts and mode switches
def damage_handle(case):
    S = damage_solver(case)
    S.set_deterministic_damage(True)
    prepare(case)(S)
    return S


def damage_steps(S, switches):
    """NSTEPS steps; with `switches`, out of a mode and back between two steps: every cached run table is dropped"""
    none = nlps().BccSet([])
    for t in range(NSTEPS):
        if t == MID:
            S.resort()
        if switches and t in (1, 2, 5):
            S.set_deterministic(False)
            S.set_deterministic(True)
        if switches and t == 3:
            S.set_deterministic_damage(False)
            S.set_deterministic_damage(True)
        S.explicit_step(none, TABLE_STEP[t], xr.DT[TABLE_STEP[t]], xr.GAMMA)


def test_damage_runs_across_resorts_and_mode_switches():
    case = xr.erosion_case(3, 0, Gf=xr.erosion_Gf(3, 0))
    A, B = damage_handle(case), damage_handle(case)
    damage_steps(A, True)
    damage_steps(B, False)
    na, nb = A.explicit_nodal(), B.explicit_nodal()
    for k in ("mass", "dU", "force", "accel"):
        same(na[k], nb[k], f"nodal {k}")
    sa, sb = A.download_state(), B.download_state()
    for k, v in sa.items():
        if isinstance(v, np.ndarray):
            same(v, sb[k], k)
    failed = int(sa["Damage_n1"].sum())
    print(f"{failed} of {A.np} particles failed")
    assert 0 < failed < A.np
    A.close()
    B.close()
