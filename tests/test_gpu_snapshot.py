"""The particle snapshot (nlps_gpu_set_snapshots): what snapshot_begin packs on the device and copies out on
its own stream is, bit for bit, what download_state() returns when it is called right behind it -- the download comes
second, so the pack has read the pending state (a deferred move, tau / W a folded step did not store, rho J, renamed
slots, a permutation of the slots), not a materialised one.  Every one-rank form of the step, the level-B stages,
newmark_step, slots in flight across later steps, the contract of the five entries, and the VTK writer."""
import functools

import numpy as np
import pytest

import explicit_loads_ref as lr
from test_gpu_async_lists import DT, the_case
from test_gpu_newton_solve import DRIVER, _problem
from test_gpu_parity import _random_cloud_case
from util import DP, HENCKY, NH, dirichlet_plane, gpu_setup, nlps

pytestmark = pytest.mark.gpu

LAWS = {"neo-hookean": NH, "hencky": HENCKY, "drucker-prager": DP}
FORMS = ("non_folded", "folded", "async_lists", "deferred_move", "deterministic", "damage", "loads")
NSTEPS = lr.NSTEPS  # the step count the contour tables are made for; three steps run


def assert_same(snap, ref, what, keys=None):
    """every field of the snapshot against the download, bit for bit; the aliases too"""
    keys = [k for k in snap if k != "tag"] if keys is None else keys
    assert keys
    for k in keys:
        a, b = snap[k], ref[k]
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {k} {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
        assert np.array_equal(a, b), f"{what}: {k} differs in {int(np.sum(a != b))} of {a.size} entries"


@functools.lru_cache(maxsize=None)
def form_case(ndim, law, form):
    """the cloud of test_gpu_async_lists.py with that law; the damage form pre-damaged, with strains at the onset"""
    case = the_case(ndim)
    mat = dict(LAWS[law])
    cloud = dict(case["cloud"])
    if law == "drucker-prager":
        cloud["kappa_n"] = np.full_like(cloud["kappa_n"], mat["kappa_0"])
    if form == "damage":
        mat.update(Ceps=1.5, ft=1.0e3, heps=2.0, wcrit=0.05)
        rng = np.random.default_rng(33)
        npart = cloud["x"].shape[0]
        pick = rng.permutation(npart)
        damage0, strain_f0 = np.zeros(npart), np.zeros(npart)
        damage0[pick[:npart // 10]] = 1.0
        damage0[pick[npart // 10: npart // 5]] = 0.3
        strain_f0[pick[npart // 10: npart // 4]] = 1e-3
        cloud["damage_n"], cloud["strain_f_n"] = damage0, strain_f0
    return dict(case, cloud=cloud, materials=[mat])


def form_solver(ndim, law, form):
    n = nlps()
    case = form_case(ndim, law, form)
    kw = {}
    if form == "damage":
        kw["params"] = n.default_params()
        kw["params"].driver_eigensoftening = 1
    S = gpu_setup(case, nsteps=NSTEPS, **kw)
    if form == "non_folded":
        S.debug_option("lazy_nodal", 0)
    elif form == "folded":
        S.debug_option("async_lists", 0)
    elif form == "deferred_move":
        S.debug_option("defer_move_min", 0)
    elif form == "deterministic":
        S.set_deterministic(True)
    elif form == "damage":
        S.set_explicit_damage(True)
    elif form == "loads":
        S.set_explicit_loads(n.BccSet(lr.contours(case)), lr.THICKNESS, lr.area0(case))
    gb = n.BccSet([dirichlet_plane(case, ndim - 1, 3, NSTEPS)])
    return S, gb


def three_steps(S, gb):
    S.set_resort_interval(2)  # the third step starts with a re-sort: the slots are not in the caller's order
    for t in range(3):
        S.explicit_step(gb, t, DT)


# 1. every form of the step
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("law", list(LAWS))
@pytest.mark.parametrize("ndim", [2, 3])
def test_snapshot_equals_download(ndim, law, form):
    n = nlps()
    S, gb = form_solver(ndim, law, form)
    S.set_snapshots(n.SNAP_ALL, 1)
    three_steps(S, gb)
    slot = S.snapshot_begin(7)
    ref = S.download_state()
    snap = S.snapshot_wait(slot)
    assert snap["tag"] == 7
    assert sorted(k for k in snap if k != "tag") == sorted([k for k, _ in n.SNAP_FIELDS] + ["x", "lambda", "beta"])
    assert_same(snap, ref, f"{ndim}-D {law} {form}")
    # the state is one worth comparing: the particles have moved and are stressed, the slots are permuted
    assert np.isfinite(ref["Stress"]).all() and np.abs(ref["Stress"]).max() > 1.0 and np.abs(ref["dis"]).max() > 0.0
    assert np.abs(ref["W"]).max() > 0.0 and not np.array_equal(ref["rho"], form_case(ndim, law, form)["cloud"]["rho"])
    if form == "damage":
        assert ref["Damage_n"].max() == 1.0 and ref["Strain_f_n"].max() > 0.0
    if law == "drucker-prager":
        assert np.abs(ref["b_e_n"] - ref["b_e_n"][0]).max() > 0.0 and ref["Kappa_n"].max() > 0.0
    S.snapshot_release(slot)
    # a subset leaves the others out (the state is now the materialised one)
    S.set_snapshots(["x", "Stress", "rho", "I0"], 2)
    slot = S.snapshot_begin(8)
    sub = S.snapshot_wait(slot, copy=False)
    assert sorted(sub) == ["I0", "Stress", "rho", "tag", "x", "x_GC"] and sub["tag"] == 8
    assert_same(sub, ref, f"{ndim}-D {law} {form}, subset")
    S.snapshot_release(slot)
    S.close()


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("by_caller", [0, 1])
def test_both_mappings_of_the_pack_across_resorts(ndim, by_caller):
    """one thread per caller's index through the inverse permutation (the shipped form: the map is rebuilt by the first
    begin behind a re-sort) and one thread per memory slot: the same snapshot at every step, re-sorts in between"""
    n = nlps()
    S, gb = form_solver(ndim, "hencky", "deferred_move")
    S.debug_option("snapshot_by_caller", by_caller)
    S.set_snapshots(n.SNAP_ALL, 1)
    S.set_resort_interval(2)
    for t in range(4):  # a re-sort at the head of the third step
        S.explicit_step(gb, t, DT)
        slot = S.snapshot_begin(t)
        ref = S.download_state()
        assert_same(S.snapshot_wait(slot), ref, f"{ndim}-D by_caller {by_caller}, step {t}")
        S.snapshot_release(slot)
    S.resort()
    slot = S.snapshot_begin(4)
    assert_same(S.snapshot_wait(slot), S.download_state(), f"{ndim}-D by_caller {by_caller}, behind resort()")
    S.close()


# 2. slots in flight across the steps that follow
@pytest.mark.parametrize("ndim", [2, 3])
def test_snapshot_survives_the_following_steps(ndim):
    n = nlps()
    case, nsteps = form_case(ndim, "neo-hookean", "deferred_move"), 6
    gb = n.BccSet([dirichlet_plane(case, ndim - 1, 3, nsteps)])
    S = gpu_setup(case, nsteps=nsteps)
    S.debug_option("defer_move_min", 0)
    S.set_snapshots(n.SNAP_ALL, 2)
    S.set_resort_interval(2)
    t = 0

    def steps(count):
        nonlocal t
        for _ in range(count):
            S.explicit_step(gb, t, DT)
            t += 1

    steps(1)
    a = S.snapshot_begin(t)
    ref_a = S.download_state()
    steps(2)
    b = S.snapshot_begin(t)
    ref_b = S.download_state()
    assert a != b
    steps(2)
    snap_b, snap_a = S.snapshot_wait(b), S.snapshot_wait(a)
    assert snap_a["tag"] == 1 and snap_b["tag"] == 3
    assert_same(snap_a, ref_a, "first slot, four steps later")
    assert_same(snap_b, ref_b, "second slot, two steps later")
    assert not np.array_equal(ref_a["x"], ref_b["x"])
    S.snapshot_release(a)
    c = S.snapshot_begin(t)
    ref_c = S.download_state()
    assert c == a
    steps(1)
    snap_c = S.snapshot_wait(c)
    assert snap_c["tag"] == 5
    assert_same(snap_c, ref_c, "the reused slot")
    assert_same(S.snapshot_wait(b), ref_b, "the slot that was not released")
    S.close()


def test_begin_leaves_the_pending_state_to_the_steps():
    """begin between deferred-move steps, no download in between: the run ends where a run without snapshots ends -- the
    closest nodes bit for bit, the fields to the tolerance test_gpu_async_lists.py holds two runs of one form to (the
    nodal sums are float atomics)."""
    from util import assert_close
    n = nlps()
    case, nsteps = form_case(3, "neo-hookean", "deferred_move"), 6
    gb = n.BccSet([dirichlet_plane(case, 2, 3, nsteps)])

    def run(snapshots):
        S = gpu_setup(case, nsteps=nsteps)
        S.debug_option("defer_move_min", 0)
        S.set_resort_interval(4)
        if snapshots:
            S.set_snapshots(["x", "dis", "Stress", "W", "rho", "I0"], 1)
        snaps = []
        for t in range(nsteps):
            S.explicit_step(gb, t, DT)
            if snapshots and t < nsteps - 1:
                slot = S.snapshot_begin(t)
                snaps.append(S.snapshot_wait(slot))
                S.snapshot_release(slot)
        out = S.download_state()
        S.close()
        return out, snaps

    with_snaps, snaps = run(True)
    without, _ = run(False)
    assert np.array_equal(with_snaps["I0"], without["I0"])
    for k in ("x", "dis", "vel", "acc", "F_n", "Stress", "J_n", "rho", "W"):
        assert_close(with_snaps[k], without[k], 1e-11, f"{k}: a run with snapshots vs one without")
    assert [s["tag"] for s in snaps] == list(range(nsteps - 1))
    assert np.abs(snaps[-1]["x"] - snaps[0]["x"]).max() > 0.0


# 3. level B and the implicit step
@pytest.mark.parametrize("ndim", [2, 3])
def test_after_level_b_stages_and_newmark_step(ndim):
    n = nlps()
    case, bcs, gravity, nsteps = _problem(ndim)
    S = gpu_setup(case, nsteps=nsteps)
    S.set_snapshots(n.SNAP_ALL, 1)

    def check(what):
        slot = S.snapshot_begin(0)
        ref = S.download_state()
        assert_same(S.snapshot_wait(slot), ref, what)
        S.snapshot_release(slot)
        return ref

    start = check("right after create")
    S.local_search()
    S.active_masks(bcs, 0)
    M = S.compute_nodal_lumped_mass()
    V, A = S.get_nodal_field_n(M)
    dU = 1e-3 * np.random.default_rng(4).normal(size=S.nactive * ndim)
    S.local_compatibility_conditions(dU)
    S.constitutive_update()
    check("after compatibility + constitutive (the n state is untouched)")
    S.update_particles_internal_variables()
    S.update_particles_kinetics_FLIP_PIC(1.0, dU, V, np.zeros_like(dU), np.zeros_like(dU))
    rolled = check("after roll_state + update_kinetics")
    assert not np.array_equal(rolled["F_n"], start["F_n"]) and not np.array_equal(rolled["x"], start["x"])
    S.close()
    S = gpu_setup(case, nsteps=nsteps)
    S.set_snapshots(n.SNAP_ALL, 1)
    info = S.newmark_step(bcs, 0, 2.0e-2, gravity, max_it=50, atol=1e-8, rtol=1e-10, stol=1e-8, linesearch="bt", ksp=DRIVER)
    assert info["reason"] > 0
    after = check("after a converged newmark_step")
    assert np.abs(after["Stress"]).max() > 0.0
    S.close()


# 4. the contract
def tiny_solver(ndim, npart, **kw):
    cells = [12, 11] if ndim == 2 else [9, 8, 8]
    lo = np.array([3.2] * ndim)
    hi = np.array([7.7, 6.9] if ndim == 2 else [5.8, 4.9, 4.6])
    return gpu_setup(_random_cloud_case(ndim, npart, 100 + npart, cells, lo, hi), nsteps=4, **kw)


def per_particle_bytes(mask, ndim):
    """8 D + 4 I of the header"""
    n, T, D = nlps(), 5 if ndim == 2 else 9, 0
    for b, (name, w) in enumerate(n.SNAP_FIELDS[:-1]):
        if (mask >> b) & 1:
            D += {"d": ndim, "T": T}.get(w, w)
    return 8 * D + (4 if mask & n.SNAP_BITS["I0"] else 0)


def test_contract():
    n = nlps()
    S, gb = form_solver(3, "neo-hookean", "async_lists")
    t = 0

    def step_and_check(what):
        """the handle is usable: a step, and a correct snapshot of it"""
        nonlocal t
        S.explicit_step(gb, t % NSTEPS, DT)
        t += 1
        slot = S.snapshot_begin(t)
        ref = S.download_state()
        snap = S.snapshot_wait(slot)
        assert snap["tag"] == t
        assert_same(snap, ref, what)
        S.snapshot_release(slot)

    for call in (lambda: S.snapshot_begin(0), lambda: S.snapshot_wait(0), lambda: S.snapshot_release(0), S.snapshot_bytes):
        with pytest.raises(n.NlpsError, match="no snapshots are set"):
            call()
    S.set_snapshots(n.SNAP_ALL, 2)
    per = per_particle_bytes(n.SNAP_ALL, 3)
    assert per == 8 * (5 * 3 + 3 * 9 + 3 + 10) + 4  # five vectors, three tensors, Back_stress, ten scalars, I0
    assert S.snapshot_bytes() == (2 * S.np * per + 4 * S.np, 2 * S.np * per)  # (+ the inverse permutation)
    for bad, msg in (((n.SNAP_ALL, 0), "slots outside"), ((n.SNAP_ALL, n.SNAP_MAX_SLOTS + 1), "slots outside"),
                     ((0, 2), "fields is 0"), ((1 << len(n.SNAP_FIELDS), 2), "bit outside"),
                     ((n.SNAP_ALL | (1 << 31), 2), "bit outside")):
        with pytest.raises(n.NlpsError, match=msg):
            S.set_snapshots(*bad)
        step_and_check(f"behind the refusal '{msg}'")  # (the snapshots set first are still the ones in force)
    for call in (lambda: S.snapshot_wait(0), lambda: S.snapshot_release(1), lambda: S.snapshot_wait(2), lambda: S.snapshot_release(-1)):
        with pytest.raises(n.NlpsError, match="was not begun"):
            call()
    step_and_check("behind wait / release on slots that were not begun")
    # every slot busy: in flight or unreleased
    a, b = S.snapshot_begin(1), S.snapshot_begin(2)
    ref = S.download_state()
    with pytest.raises(n.NlpsError, match="every slot is in flight or unreleased"):
        S.snapshot_begin(3)
    S.explicit_step(gb, t % NSTEPS, DT)
    t += 1
    assert_same(S.snapshot_wait(a), ref, "slot 0 behind a refused begin")
    assert_same(S.snapshot_wait(b), ref, "slot 1 behind a refused begin")
    S.snapshot_release(a)
    S.snapshot_release(b)
    step_and_check("behind a begin with every slot busy")
    # a no-op halo callback: the pack is rank-local
    S.set_halo_exchange(lambda dptr, nfield, elem, kind: 0)
    step_and_check("with a halo callback")
    S.set_halo_exchange(None)
    # off with a copy in flight, then a step; begin is refused again
    S.snapshot_begin(9)
    S.set_snapshots(None)
    S.explicit_step(gb, t % NSTEPS, DT)
    t += 1
    with pytest.raises(n.NlpsError, match="no snapshots are set"):
        S.snapshot_begin(0)
    # a subset, the formula again, and close() with a copy in flight
    mask = n.snapshot_mask(["x", "F_n", "W", "Back_stress", "I0"])
    S.set_snapshots(mask, 3)
    assert per_particle_bytes(mask, 3) == 8 * (3 + 9 + 1 + 3) + 4
    assert S.snapshot_bytes() == (3 * S.np * per_particle_bytes(mask, 3) + 4 * S.np, 3 * S.np * per_particle_bytes(mask, 3))
    step_and_check("a subset behind a replacement")
    S.snapshot_begin(10)
    S.close()
    # a migrated handle: refused by the setter, and by begin when the migration comes behind the set
    for set_first in (False, True):
        S, gb = form_solver(3, "neo-hookean", "async_lists")
        if set_first:
            S.set_snapshots(n.SNAP_ALL, 1)
        S.explicit_step(gb, 0, DT)
        n_down, n_up, _, _, _ = S.migration_select(0, 11)
        assert n_down == 0 and 0 < n_up < S.np
        S.migration_commit(0, 0, 0, 0)
        with pytest.raises(n.NlpsError, match="migrated"):
            S.snapshot_begin(0) if set_first else S.set_snapshots(n.SNAP_ALL, 1)
        S.explicit_step(gb, 1, DT)
        assert S.download_state()["x"].shape[0] == S.num_particles()
        S.close()


@pytest.mark.parametrize("ndim,npart", [(2, 0), (2, 1), (2, 37), (3, 1), (3, 333)])
def test_ragged_and_tiny_clouds(ndim, npart):
    n = nlps()
    S = tiny_solver(ndim, npart)
    S.set_snapshots(n.SNAP_ALL, 2)
    per = per_particle_bytes(n.SNAP_ALL, ndim)
    assert S.snapshot_bytes() == (2 * max(8, npart * per) + 4 * max(npart, 1), 2 * max(8, npart * per))
    none = n.BccSet([])
    for t in range(3):
        S.explicit_step(none, t, 2e-3)
        slot = S.snapshot_begin(t)
        ref = S.download_state()
        snap = S.snapshot_wait(slot)
        assert snap["x"].shape == (npart, ndim) and snap["I0"].shape == (npart,) and snap["I0"].dtype == np.int32
        assert_same(snap, ref, f"{ndim}-D, {npart} particles, step {t}")
        S.snapshot_release(slot)
    S.close()


def test_on_the_callers_stream():
    """a caller-owned non-blocking stream: wait needs no synchronisation of that stream"""
    import torch
    n = nlps()
    prev = torch.cuda.current_stream()
    ts = torch.cuda.Stream()
    torch.cuda.set_stream(ts)
    try:
        case = form_case(3, "neo-hookean", "async_lists")
        S = gpu_setup(case, nsteps=NSTEPS, stream=ts.cuda_stream)
        gb = n.BccSet([dirichlet_plane(case, 2, 3, NSTEPS)])
        S.set_snapshots(n.SNAP_ALL, 1)
        three_steps(S, gb)
        slot = S.snapshot_begin(3)
        snap = S.snapshot_wait(slot)  # (before the download: nothing but the slot's own event has been waited for)
        ref = S.download_state()
        assert_same(snap, ref, "on the caller's stream")
        S.snapshot_release(slot)
        S.close()
    finally:
        torch.cuda.set_stream(prev)


# 5. the VTK writer takes the snapshot as it is
@pytest.mark.parametrize("ndim", [2, 3])
def test_vtk_from_a_snapshot_is_byte_identical(ndim, tmp_path):
    import importlib
    gid = importlib.import_module("nl-partsol_amd.gid")
    n = nlps()
    S, gb = form_solver(ndim, "neo-hookean", "async_lists")
    S.set_snapshots(n.SNAP_VTK, 1)
    three_steps(S, gb)
    slot = S.snapshot_begin(3)
    ref = S.download_state()
    snap = S.snapshot_wait(slot, copy=False)
    flags = gid.VTK_X_GC | gid.VTK_P | gid.VTK_ENERGY
    gid.write_particles_vtk(tmp_path / "snap.vtk", 3, snap, flags)
    gid.write_particles_vtk(tmp_path / "down.vtk", 3, ref, flags)
    a, b = (tmp_path / "snap.vtk").read_bytes(), (tmp_path / "down.vtk").read_bytes()
    assert len(a) > 100 * S.np and a == b
    for block in (b"VELOCITY", b"STRESS", b"DEFORMATION-GRADIENT", b"DENSITY", b"ELEM_i", b"EPS"):
        assert block in a, block
    S.snapshot_release(slot)
    S.close()
