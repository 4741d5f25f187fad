"""The checker of the step record (nlps_gpu_set_step_record): plain numpy over the dicts Solver.download_state()
and Solver.explicit_nodal() return.  The download is the independent code: it re-makes tau and W with k_copy_n_to_n1 and
permutes on the host; the record reduces on the device without making those arrays.

Tolerances (the issue's): a sum of n terms |got - want| <= 1e-12 sum|term| (the rounding bound is n 2^-53 sum|term|, 9e-12
of that at the largest n used, 78 400; only the order of summation differs, W is re-formed by the same code from the same
inputs); maxima, minima, counts, the head of a row and every probe value np.array_equal (the build compiles with
-ffp-contract=off); vmax_norm and time relative 1e-14."""
import numpy as np

SUM_TOL = 1e-12
EXACT = ("vmax_comp", "J_min", "J_max", "EPS_max", "Damage_max", "failed", "np")
PROBE_FIELDS = ("x_GC", "dis", "vel", "acc", "F_n", "Stress", "J_n", "EPS_n", "Damage_n", "W")  # ascending NLPS_PROBE_ bit


def _pad3(a):
    out = np.zeros((a.shape[0], 3))
    out[:, : a.shape[1]] = a
    return out


def sums(st, ndim):
    """name -> [terms per particle] of every sum of the global block ([np] or [np][3])"""
    m, v, x = st["mass"], _pad3(st["vel"]), _pad3(st["x_GC"])
    return {"mass": m, "momentum": m[:, None] * v, "angular": m[:, None] * np.cross(x, v), "mass_x": m[:, None] * x,
            "kinetic": 0.5 * m * (v * v).sum(axis=1), "strain": st["W"] * st["Vol_0"], "volume": st["Vol_0"] * st["J_n"]}


def extrema(st):
    n = st["mass"].size
    v = st["vel"]
    if n == 0:
        return {"vmax_comp": 0.0, "vmax_norm": 0.0, "J_min": np.inf, "J_max": -np.inf, "EPS_max": 0.0, "Damage_max": 0.0,
                "failed": 0.0, "np": 0.0}
    vv = np.zeros(n)
    for a in range(v.shape[1]):  # (the order of the kernel's sum: component by component)
        vv = vv + v[:, a] * v[:, a]
    return {"vmax_comp": np.abs(v).max(), "vmax_norm": np.sqrt(vv.max()), "J_min": st["J_n"].min(), "J_max": st["J_n"].max(),
            "EPS_max": st["EPS_n"].max(), "Damage_max": st["Damage_n"].max(), "failed": float((st["Damage_n"] == 1.0).sum()),
            "np": float(n)}


def check_sum(got, terms, what):
    want, scale = terms.sum(axis=0), np.abs(terms).sum(axis=0)
    err = np.abs(np.asarray(got) - want)
    print(f"{what}: |got - want| / sum|term| = {np.max(err / np.maximum(scale, 1e-300)):.2e}")
    assert np.all(err <= SUM_TOL * scale), f"{what}: got {got}, want {want}, sum|term| {scale}"


def check_globals(rec, r, st, ndim, what):
    """row r of a read_step_records() dict against the reductions over the download `st`"""
    for name, terms in sums(st, ndim).items():
        check_sum(rec[name][r], terms, f"{what} {name}")
    ex = extrema(st)
    for name in EXACT:
        assert np.array_equal(rec[name][r], ex[name]), f"{what} {name}: got {rec[name][r]!r}, want {ex[name]!r}"
    assert abs(rec["vmax_norm"][r] - ex["vmax_norm"]) <= 1e-14 * ex["vmax_norm"], f"{what} vmax_norm"
    assert not rec["rows"][r, 26:32].any(), f"{what}: the reserved slots"


def check_head(rec, r, step, kind, dt, time, what):
    for name, want in (("step", step), ("kind", kind), ("dt", dt)):
        assert np.array_equal(rec[name][r], float(want)), f"{what} {name}: got {rec[name][r]!r}, want {want!r}"
    assert abs(rec["time"][r] - time) <= 1e-14 * abs(time), f"{what} time: got {rec['time'][r]!r}, want {time!r}"


def nodes2mask(active):
    """masked numbering of the lattice nodes (running index over the active ones), -1 elsewhere"""
    a = np.asarray(active) != 0
    return np.where(a, np.cumsum(a) - 1, -1)


def reaction_terms(reaction, n2m, bc, step, ndim):
    """[nodes of the set][3]: the reaction of every dof of the set with dir == 1 at the step, 0 for the others"""
    R = np.asarray(reaction).reshape(-1, ndim)
    nodes = np.asarray(bc["nodes"])
    out = np.zeros((nodes.size, 3))
    m = n2m[nodes]
    for k in range(min(int(bc["dim"]), ndim)):
        if np.asarray(bc["dir"])[k, step] == 1:
            out[:, k] = np.where(m >= 0, R[np.maximum(m, 0), k], 0.0)
    return out


def check_reactions(rec, r, nodal, active, bcs, step, ndim, what):
    """the reaction block of row r: sets of the step against explicit_nodal()['reaction'], the others NaN"""
    got = rec["reactions"][r]
    n2m = nodes2mask(active)
    for s in range(got.shape[0]):
        if s < len(bcs):
            check_sum(got[s], reaction_terms(nodal["reaction"], n2m, bcs[s], step, ndim), f"{what} reaction of set {s}")
        else:
            assert np.isnan(got[s]).all(), f"{what}: set {s} is not one of the step's"


def check_probes(S, rec, r, st, probes, fields, what):
    got = rec["probes"][r]
    for name, sl in S.probe_slices(fields).items():
        want = st[name][probes]
        want = want.reshape(len(probes), -1)
        assert np.array_equal(got[:, sl], want), f"{what} probe {name}: largest difference {np.abs(got[:, sl] - want).max():.3e}"
