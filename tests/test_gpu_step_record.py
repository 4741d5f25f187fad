"""The step record (nlps_gpu_set_step_record): rows made on the device behind explicit_step / newmark_step
against the checker of step_record_ref.py applied to a download taken right after -- every one-rank form of the step, the
lazy state left alone, stored against re-formed W / tau, the damage step, the ring and the interval, record_now, Newmark,
the finish kernel's loop, the empty cloud and the refusals."""
import numpy as np
import pytest

import explicit_damage_ref as xr
import explicit_loads_ref as lr
import step_record_ref as rr
from test_gpu_explicit_damage import damage_solver
from test_gpu_newton_solve import DRIVER, _problem
from util import DP, NH, dirichlet_plane, gpu_setup, make_case, nlps

pytestmark = pytest.mark.gpu

ALL = 1023  # every NLPS_PROBE_ field


def probe_ids(npart, count=8, seed=3):
    """particles spread over the cloud, in no particular order"""
    return np.random.default_rng(seed).choice(npart, size=count, replace=False).astype(np.int32)


def step(S, bset, t):
    S.explicit_step(bset, t, lr.DT[t], lr.GAMMA, gravity=lr.gravity(S.ndim))


def check_last_row(S, bcs, t, kind, dt, time, probes, fields, what, reactions=True):
    """the newest row against a download (and the nodal arrays) taken right after it was read"""
    rec = S.read_step_records()
    r = rec["count"] - 1
    nodal = S.explicit_nodal() if reactions else None
    st = S.download_state()
    rr.check_head(rec, r, t, kind, dt, time, what)
    rr.check_globals(rec, r, st, S.ndim, what)
    if reactions:
        rr.check_reactions(rec, r, nodal, S.download_active(), bcs, t, S.ndim, what)
    else:
        assert np.isnan(rec["reactions"][r]).all(), f"{what}: reactions of a row that is not an explicit step"
    if len(probes):
        rr.check_probes(S, rec, r, st, probes, fields, what)
    return rec, st


def run_form(ndim, prepare=None, loads=False, laws=0, nsteps=4, nsets=1, case=None, energy=True):
    n = nlps()
    case = lr.loaded_case(ndim, laws) if case is None else case
    bcs = lr.dirichlet(case)
    S = gpu_setup(case, nsteps=lr.NSTEPS)
    if prepare:
        prepare(S)
    if loads:
        S.set_explicit_loads(n.BccSet(lr.contours(case)), lr.THICKNESS, lr.area0(case))
    probes = probe_ids(S.np)
    S.set_step_record(every=1, capacity=4, nsets=nsets, probes=probes, probe_fields=ALL)
    bset, time = n.BccSet(bcs), 0.0
    for t in range(nsteps):
        step(S, bset, t)
        time += lr.DT[t]
        rec, st = check_last_row(S, bcs, t, n.REC_KIND_EXPLICIT, lr.DT[t], time, probes, ALL, f"{ndim}-D step {t}")
        assert rec["total"] == t + 1 and rec["status"][-1] == 0.0
        assert np.abs(rec["reactions"][-1]).max() > 0.0 and (rec["strain"][-1] > 0.0 or not energy)
    S.close()


# 1. every one-rank form
@pytest.mark.parametrize("ndim", [2, 3])
def test_default_form(ndim):
    """the folded form with the lists of the next step on the side stream: W and tau re-formed in registers"""
    run_form(ndim)


@pytest.mark.parametrize("ndim", [2, 3])
def test_without_async_lists(ndim):
    run_form(ndim, prepare=lambda S: S.debug_option("async_lists", 0))


@pytest.mark.parametrize("ndim", [2, 3])
def test_non_folded_form(ndim):
    run_form(ndim, prepare=lambda S: S.debug_option("lazy_nodal", 0))


@pytest.mark.parametrize("ndim", [2, 3])
def test_with_contour_loads(ndim):
    """the reactions contain the contour tractions as explicit_nodal's do"""
    run_form(ndim, loads=True)


@pytest.mark.parametrize("ndim", [2, 3])
def test_with_resorts(ndim):
    """the probes keep addressing the caller's particles under a permutation of the slots"""
    def prepare(S):
        S.resort()
        S.set_resort_interval(2)
    run_form(ndim, prepare=prepare)


# 2. laziness
@pytest.mark.parametrize("ndim", [2, 3])
def test_the_record_leaves_the_lazy_state_alone(ndim):
    """A downloads after every step, B never does and reads all rows at the end, C never hears of a record: equal rows, and
    equal nodal arrays and particle state after the last step.  One field cannot be equal between A and B, with or without a
    record: every download of A re-makes rho = (rho J) / J_n and the next step takes rho J = rho J_n from it again
    (k_init_rhoj), two roundings per step that B and C never make; nothing in the step reads rho.  It is held to that
    bound, 2 NSTEPS 2^-53 relative, and B against C -- the record's own effect -- to equality like every other field."""
    n = nlps()
    case = lr.loaded_case(ndim)
    bcs = lr.dirichlet(case)
    probes = probe_ids(case["cloud"]["x"].shape[0])
    A, B, C = (gpu_setup(case, nsteps=lr.NSTEPS) for _ in range(3))
    rows = []
    for S in (A, B, C):
        S.set_deterministic(True)
    for S in (A, B):
        S.set_step_record(every=1, capacity=lr.NSTEPS, nsets=1, probes=probes, probe_fields=ALL)
    ba, bb, bc = n.BccSet(bcs), n.BccSet(bcs), n.BccSet(bcs)
    for t in range(lr.NSTEPS):
        step(A, ba, t)
        rows.append(A.read_step_records()["rows"][-1].copy())
        A.download_state()
        step(B, bb, t)
        step(C, bc, t)
    got = B.read_step_records()
    assert got["total"] == lr.NSTEPS and got["count"] == lr.NSTEPS
    assert np.array_equal(got["rows"], np.stack(rows), equal_nan=True)
    na, nb, nc = A.explicit_nodal(), B.explicit_nodal(), C.explicit_nodal()
    for k in na:
        assert np.array_equal(na[k], nb[k]) and np.array_equal(nb[k], nc[k]), f"nodal {k}"
    sa, sb, sc = A.download_state(), B.download_state(), C.download_state()
    for k in sa:
        assert np.array_equal(sb[k], sc[k]), f"{k}: with a record against without"
        if k == "rho":
            e = np.abs(sa[k] - sb[k]).max() / np.abs(sb[k]).max()
            print(f"rho of the handle that downloaded every step against the one that never did: {e:.2e}")
            assert e <= 2 * lr.NSTEPS * 2.0 ** -53
        else:
            assert np.array_equal(sa[k], sb[k]), k
    for S in (A, B, C):
        S.close()


# 3. laws: stored against re-formed W / tau
@pytest.mark.parametrize("name,laws,mode", [("hencky", 1, 0), ("drucker-prager", None, 0), ("mixed, per-law launches", (0, 1), 1),
                                            ("mixed, dispatch kernel", (0, 1), 2)])
def test_laws(name, laws, mode):
    if laws is None:
        case = make_case(3, [11, 10, 9], [3, 3, 2], [5, 4, 4], material=DP, velocity=[0.0, 0.0, -2.0])
    else:
        case = lr.loaded_case(3, laws)
    run_form(3, prepare=(lambda S: S.set_law_launch_mode(mode)) if mode else None, nsteps=2, case=case, energy=laws is not None)


# 4. damage
def test_damage_step():
    n = nlps()
    laws = 0
    S = damage_solver(xr.erosion_case(3, laws, Gf=xr.erosion_Gf(3, laws)))
    probes = probe_ids(S.np, 16)
    fields = n.PROBE_DAMAGE | n.PROBE_STRESS | n.PROBE_W
    S.set_step_record(every=1, capacity=2, probes=probes, probe_fields=fields)
    none, time, failed = n.BccSet([]), 0.0, []
    for t in range(4):
        S.explicit_step(none, t, xr.DT[t], xr.GAMMA)
        time += xr.DT[t]
        rec, st = check_last_row(S, [], t, n.REC_KIND_EXPLICIT, xr.DT[t], time, probes, fields, f"damage step {t}")
        failed.append(rec["failed"][-1])
        assert rec["Damage_max"][-1] == st["Damage_n"].max()
    assert failed[0] > 0 and failed[-1] >= failed[0] and rec["Damage_max"][-1] == 1.0
    S.close()


# 5. ring and interval
def test_ring_and_interval():
    n = nlps()
    case = lr.loaded_case(2)
    nsteps = 9
    bcs = [dirichlet_plane(case, 1, 3, nsteps)]
    dts = [1e-4 * (1.0 + 0.1 * t) for t in range(nsteps)]
    S = gpu_setup(case, nsteps=nsteps)
    S.set_step_record(every=2, capacity=3, nsets=1)
    bset = n.BccSet(bcs)
    for t in range(nsteps):
        S.explicit_step(bset, t, dts[t], lr.GAMMA, gravity=lr.gravity(2))
    rec = S.read_step_records()
    assert rec["total"] == 5 and rec["count"] == 3
    assert np.array_equal(rec["step"], [4.0, 6.0, 8.0])
    assert np.array_equal(rec["dt"], [dts[4], dts[6], dts[8]])
    want = np.cumsum(dts)
    assert np.all(np.abs(rec["time"] - want[[4, 6, 8]]) <= 1e-14 * want[[4, 6, 8]])
    assert abs(rec["time"][-1] - sum(dts)) <= 1e-14 * sum(dts)
    two = S.read_step_records(max_rows=2)
    assert two["total"] == 5 and two["count"] == 2 and np.array_equal(two["rows"], rec["rows"][1:], equal_nan=True)
    counts = S.read_step_records(counts_only=True)
    assert counts == {"total": 5, "count": 3}
    # the last row is the state as it stands
    st = S.download_state()
    rr.check_globals(rec, 2, st, 2, "step 8")
    S.close()


# 6. record_now
def test_record_now():
    n = nlps()
    case = lr.loaded_case(2)
    probes = probe_ids(case["cloud"]["x"].shape[0])
    S = gpu_setup(case, nsteps=lr.NSTEPS)
    S.set_step_record(every=1, capacity=4, nsets=2, probes=probes, probe_fields=ALL)
    S.record_now(7)
    rec, _ = check_last_row(S, [], 7, n.REC_KIND_NOW, 0.0, 0.0, probes, ALL, "straight after create", reactions=False)
    assert rec["total"] == 1 and rec["time"][0] == 0.0
    # level-B stages without a roll: the stored W / tau of the n+1 state
    bcs = lr.dirichlet(case)
    bset = n.BccSet(bcs)
    S.local_search()
    S.active_masks(bset, 0)
    dU = 1e-3 * np.random.default_rng(8).normal(size=S.nactive * 2)
    S.local_compatibility_conditions(dU)
    S.constitutive_update()
    S.record_now(-3)
    rec, st = check_last_row(S, [], -3, n.REC_KIND_NOW, 0.0, 0.0, probes, ALL, "after compatibility + constitutive", reactions=False)
    assert rec["total"] == 2 and rec["strain"][-1] > 0.0 and np.abs(st["Stress"]).max() > 0.0
    S.close()


# 7. Newmark
def test_newmark_rows():
    n = nlps()
    case, bcs, gravity, nsteps = _problem(2)
    dt = 2.0e-2
    kw = dict(max_it=50, atol=1e-8, rtol=1e-10, stol=1e-8, linesearch="bt", ksp=DRIVER)
    S = gpu_setup(case, nsteps=nsteps)
    probes = probe_ids(S.np)
    S.set_step_record(every=1, capacity=4, nsets=1, probes=probes, probe_fields=ALL)
    for t in range(2):
        info = S.newmark_step(bcs, t, dt, gravity, **kw)
        assert info["reason"] > 0
        rec, _ = check_last_row(S, [], t, n.REC_KIND_NEWMARK, dt, dt * (t + 1), probes, ALL, f"Newmark step {t}", reactions=False)
        assert rec["total"] == t + 1
    bad = S.newmark_step(bcs, 2, dt, gravity, **dict(kw, max_it=1))
    assert bad["reason"] <= 0
    assert S.read_step_records(counts_only=True)["total"] == 2
    S.close()


# 8. the finish kernel loops over more partials than it has threads
def test_finish_kernel_with_more_partials_than_threads():
    n = nlps()
    case = make_case(2, [146, 146], [3, 3], [140, 140], material=NH, velocity=[0.5, -1.0])
    case["cloud"]["vel"] = case["cloud"]["vel"] + 0.1 * np.random.default_rng(2).normal(size=case["cloud"]["vel"].shape)
    S = gpu_setup(case, nsteps=1)
    assert S.np == 78400
    bcs = [dirichlet_plane(case, 1, 3, 1)]
    S.set_step_record(every=1, capacity=1, nsets=1)
    S.explicit_step(n.BccSet(bcs), 0, 1e-4, 0.5, gravity=lr.gravity(2))
    check_last_row(S, bcs, 0, n.REC_KIND_EXPLICIT, 1e-4, 1e-4, [], 0, "78 400 particles")
    S.close()


# 9. the empty cloud and the refusals
def test_empty_cloud():
    n = nlps()
    case = lr.loaded_case(2)
    case["cloud"] = {k: (v[:0] if isinstance(v, np.ndarray) else v) for k, v in case["cloud"].items()}
    S = gpu_setup(case, nsteps=1)
    assert S.np == 0
    S.set_step_record(every=1, capacity=2)
    S.record_now(1)
    S.explicit_step(n.BccSet([]), 0, 1e-4, 0.5)
    rec = S.read_step_records()
    assert rec["total"] == 2
    for r in range(2):
        for k in ("mass", "kinetic", "strain", "volume", "vmax_comp", "vmax_norm", "EPS_max", "Damage_max", "failed", "np"):
            assert rec[k][r] == 0.0, k
        for k in ("momentum", "angular", "mass_x"):
            assert not rec[k][r].any(), k
        assert rec["J_min"][r] == np.inf and rec["J_max"][r] == -np.inf
    S.close()


def test_refusals_leave_the_handle_usable():
    """every refusal stores nothing: the step behind it writes the row of the record in force, which matches the checker"""
    n = nlps()
    case = lr.loaded_case(3)
    nsteps = 12
    bcs = lr.dirichlet(case, nsteps)
    S = gpu_setup(case, nsteps=nsteps)
    bset = n.BccSet(bcs)
    probes = probe_ids(S.np)
    good = dict(every=1, capacity=2, nsets=1, probes=probes, probe_fields=ALL)
    t, time = 0, 0.0

    def step_and_check(what):
        nonlocal t, time
        dt = lr.DT[t % 4]
        S.explicit_step(bset, t, dt, lr.GAMMA, gravity=lr.gravity(3))
        time += dt
        check_last_row(S, bcs, t, n.REC_KIND_EXPLICIT, dt, time, probes, ALL, what)
        t += 1

    with pytest.raises(n.NlpsError, match="no step record"):
        S.read_step_records()
    with pytest.raises(n.NlpsError, match="no step record"):
        S.record_now(0)
    S.set_step_record(**good)
    for bad, msg in ((dict(good, every=0), "every >= 1"), (dict(good, capacity=0), "capacity >= 1"),
                     (dict(good, nsets=-1), "negative count"),
                     (dict(good, probes=np.append(probes[:-1], S.np)), "probe index outside the cloud"),
                     (dict(good, probes=np.append(probes[:-1], -1)), "probe index outside the cloud"),
                     (dict(good, probe_fields=0), "probe_fields")):
        with pytest.raises(n.NlpsError, match=msg):
            S.set_step_record(**bad)
        step_and_check(f"behind the refusal '{msg}'")  # (the first record is still the one in force)
    S.set_halo_exchange(lambda dptr, nfield, elem, kind: 0)
    with pytest.raises(n.NlpsError, match="built for one rank"):
        S.set_step_record(**good)
    with pytest.raises(n.NlpsError, match="built for one rank"):
        S.explicit_step(bset, t, lr.DT[0], lr.GAMMA, gravity=lr.gravity(3))
    with pytest.raises(n.NlpsError, match="built for one rank"):
        S.record_now(0)
    S.set_halo_exchange(None)
    step_and_check("behind the halo refusals")
    S.set_halo_exchange(lambda dptr, nfield, elem, kind: 0)
    S.set_step_record(every=1, capacity=2)  # the particle sums alone are allowed on such a handle
    S.set_halo_exchange(None)
    S.set_step_record(**good)
    time = 0.0  # (a set starts the clock again)
    step_and_check("behind a replacement")
    S.set_step_record(every=None)
    S.explicit_step(bset, t, lr.DT[0], lr.GAMMA, gravity=lr.gravity(3))
    S.explicit_step(bset, t + 1, lr.DT[0], lr.GAMMA, gravity=lr.gravity(3))
    with pytest.raises(n.NlpsError, match="no step record"):
        S.read_step_records()
    with pytest.raises(n.NlpsError, match="no step record"):
        S.step_record_layout()
    S.close()


# 10. the host helper
def test_courant_dt():
    n = nlps()
    CFL, h, Cel = 0.6, 0.25, 1450.0
    assert n.courant_dt(CFL, h, Cel) == CFL * h / Cel
    row = np.zeros(n.REC_NGLOBAL)
    row[n.REC_COLUMNS["vmax_comp"][0]] = 37.5
    assert n.courant_dt(CFL, h, Cel, row) == CFL * h / (Cel + 37.5)
