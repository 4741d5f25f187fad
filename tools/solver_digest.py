#!/usr/bin/env python3
"""Developer tool: what the device GMRES, MINRES, Lanczos, Newton and Newmark calls and the explicit step with the
handle's features on (the steps/ cases) return, as bits, for a host-side refactor that must not move any of them.
Fresh handles on the small clouds of the tests, deterministic mode on ahead of the first call; one JSON line per case:
{"case": name, "sha256": digest} with the digest over the output vector's bytes, the history's bytes and the integer
and float result fields, or {"case": name, "error": text} for a refused call.

    python tools/solver_digest.py            every case
    python tools/solver_digest.py --one      one GMRES(5) solve, one MINRES solve and one 8-step Lanczos run on the 3-D
                                             Neo-Hookean cloud (for `rocprofv3 --kernel-trace -- python ...`)
    python tools/solver_digest.py --steps    the steps/ cases alone
    python tools/solver_digest.py --steps-trace
                                             12 shipped-mode steps of the small 3-D cloud with loads, record probes and
                                             snapshots on, a re-sort every 4 (for `rocprofv3 --kernel-trace -- python ...`)
    python tools/solver_digest.py --compare parent1 parent2 new1 new2
                                             a case counts if the parent's two runs agree; exit 0 if every case counts
                                             and every counted case is equal on the new side, one JSON line either way
    python tools/solver_digest.py --launches kernel_trace.csv [list.txt] [--without KERNEL]
                                             length and SHA-256 of rocprofv3's ordered (kernel, grid, block) list, in
                                             the order of the launches; the list itself into list.txt.  --without: the
                                             launches of kernels whose name starts with KERNEL are counted apart and
                                             left out of the list

Two libraries are compared by running the tool twice, the other build through NLPS_GPU_LIB."""
import csv
import hashlib
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _compare(paths):
    runs = []
    for p in paths:
        rows = [json.loads(line) for line in open(p) if line.startswith("{")]
        runs.append({r["case"]: r.get("sha256", r.get("error")) for r in rows})
    p1, p2, n1, n2 = runs
    names = list(p1)
    missing = sorted(set().union(*runs) - set.intersection(*[set(r) for r in runs]))
    unstable = [k for k in names if k not in missing and p1[k] != p2[k]]
    counted = [k for k in names if k not in missing and k not in unstable]
    differ = [k for k in counted if not (n1[k] == n2[k] == p1[k])]
    print(json.dumps({"tool": "solver_digest --compare", "cases": len(names), "counted": len(counted),
                      "equal": len(counted) - len(differ), "parent_disagrees_with_itself": unstable,
                      "not_in_every_run": missing, "differ": differ}))
    sys.exit(0 if not (missing or unstable or differ) else 1)


def _launches(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))  # (the order of the host's launches)
    seq = [(r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], r["Workgroup_Size_X"],
            r["Workgroup_Size_Y"], r["Workgroup_Size_Z"]) for r in rows]
    args = sys.argv[sys.argv.index("--launches") + 1:]
    out = {"tool": "solver_digest --launches"}
    if "--without" in args:
        i = args.index("--without")
        name = args[i + 1]
        out["without"], out["left_out"] = name, sum(s[0].startswith(name) for s in seq)
        seq = [s for s in seq if not s[0].startswith(name)]
        del args[i:i + 2]
    text = "\n".join(" ".join(s) for s in seq)
    if len(args) > 1:
        open(args[1], "w").write(text + "\n")
    out.update(length=len(seq), kernels=len({s[0] for s in seq}), sha256=hashlib.sha256(text.encode()).hexdigest())
    print(json.dumps(out))
    sys.exit(0)


if "--compare" in sys.argv:
    _compare(sys.argv[sys.argv.index("--compare") + 1:][:4])
if "--launches" in sys.argv:
    _launches(sys.argv[sys.argv.index("--launches") + 1])

import ctypes as C  # noqa: E402

import torch  # noqa: E402

import minres_cases as mc  # noqa: E402
import solver_exit_cases as sx  # noqa: E402
from test_gpu_newton_solve import DRIVER, TIGHT, _alpha, _problem, _Step  # noqa: E402
from util import gpu_setup, nlps  # noqa: E402

N = nlps()
NHK, DPK = "neo-hookean", "drucker-prager"


def _bytes(v):
    if v is None:
        return b"none"
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    if isinstance(v, np.ndarray):
        return str(v.dtype).encode() + np.ascontiguousarray(v).tobytes()
    if isinstance(v, (bool, int, np.integer)):
        return struct.pack("<q", int(v))
    if isinstance(v, (float, np.floating)):
        return struct.pack("<d", float(v))
    return str(v).encode()


def emit(case, fn):
    """One line: the digest of what fn returns (a vector or None, and a dict of results), or the refusal's text."""
    try:
        vec, info = fn()
        hsh = hashlib.sha256(_bytes(vec))
        for k in sorted(info):
            hsh.update(k.encode() + _bytes(info[k]))
        line = {"case": case, "sha256": hsh.hexdigest()}
    except (N.NlpsError, ValueError) as e:
        line = {"case": case, "error": str(e)}
    print(json.dumps(line), flush=True)


def raw(S, status):
    """a C call made past the Python wrapper's own checks: its status and the handle's error text"""
    if status:
        raise N.NlpsError(S.L.nlps_gpu_last_error(S.h).decode())
    return None, {"status": status}


def ksp_struct(**kw):
    d = dict(pc=N.PC_KINDS["pbjacobi"], restart=30, max_it=100, x_is_guess=0, rtol=1e-5, atol=0.0, dtol=1e5, history=None)
    d.update(kw)
    return N.Ksp(**d)


def eroded_device(ndim, level):
    """sx.eroded_device in deterministic mode (a cloud with the damage hooks: both switches)"""
    case, dU, G, Gf = sx.erosion_case(ndim, 0, level)
    params = N.default_params()
    params.driver_eigenerosion = 1
    S = gpu_setup(case, nsteps=2, params=params)
    S.set_deterministic(True)
    S.set_deterministic_damage(True)
    S.local_search()
    _, d2m = S.active_masks(N.BccSet([]), 0)
    S.local_compatibility_conditions(dU)
    S.constitutive_update()
    S.nodal_internal_forces(np.zeros(S.nactive * ndim))
    return S


def lanczos(S, mass, **kw):
    info = S.tangent_lambda_max(mass, **kw)
    return info.pop("mode"), info


# ------------------------------------------------------------------------------------------------ --one
if "--one" in sys.argv:
    s = sx.linearised_device(3, NHK, deterministic=True)
    S, n = s["S"], s["na"] * 3
    S.tangent_operator(10.0, s["Mv"], True)
    b = mc.rhs(n, 29)
    emit("one gmres(5)", lambda: S.tangent_solve(b, pc="pbjacobi", restart=5, rtol=1e-8, max_it=400, history=True))
    S.set_linear_solver("minres")
    emit("one minres", lambda: S.tangent_solve(b, pc="pbjacobi", rtol=1e-8, max_it=2000, history=True))
    S.tangent_operator(0.0, None, True)
    emit("one lanczos(8)", lambda: lanczos(S, s["Mv"], seed=2, max_it=8, rtol=0.0, mode=True, history=True))
    S.close()
    sys.exit(0)


# ------------------------------------------------------------------------------------------------ steps/
def step_cases():
    """The explicit step with the handle's features coming, going and sharing the slot map across re-sorts (the scenarios
    of tests/test_gpu_feature_state.py), the plain step, and the fused damage residual: downloaded state, nodal arrays,
    record rows and snapshot blocks."""
    import explicit_damage_ref as xr
    import explicit_loads_ref as lr
    import test_gpu_feature_state as fs
    from test_gpu_implicit_damage import alpha_of, solver as implicit_solver

    def outputs(S, snaps=(), rows=False):
        nod, st = fs.results(S)
        info = {f"nodal {k}": v for k, v in nod.items() if isinstance(v, np.ndarray)}
        info.update({f"state {k}": v for k, v in st.items() if isinstance(v, np.ndarray)})
        for t, snap in enumerate(snaps):
            info.update({f"snapshot {t:02d} {k}": v for k, v in snap.items()})
        if rows:
            info["rows"] = S.read_step_records()["rows"]
        S.close()
        return None, info

    def stepped(handle, rows):
        S, bset = handle
        fs.run(S, bset)
        return outputs(S, rows=rows)

    def together(case, probes, by_caller):
        S, bset = fs.carrying(case, probes, ("record", "snapshots"), by_caller)
        return outputs(S, fs.run_with_downloads(S, bset, True, "digest"), rows=True)

    def damage(case):
        S = fs.damage_handle(case)
        fs.damage_steps(S, True)
        return outputs(S)

    def fused_damage_residual(ndim):
        case, dU, _, _ = sx.erosion_case(ndim, 0, "part")
        S = implicit_solver(case, "erosion", True, 2)
        S.set_deterministic(True)
        S.set_deterministic_damage(True)
        info, z = {}, None
        for k, scale in enumerate((1.0, 0.5, 0.25)):  # the runs are built, reused, dropped by a mode switch and built again
            if k == 2:
                S.set_deterministic(False)
                S.set_deterministic(True)
            if k != 1:
                S.local_search()
                S.active_masks(N.BccSet([]), 0)
                Mv, z = S.compute_nodal_lumped_mass(), np.zeros(S.nactive * ndim)
            info[f"residual {k}"] = np.array(S.lagrangian_evaluation(scale * dU, z, z, Mv, alpha_of(1.0e-3)[1]))
        info.update({f"state {k}": v for k, v in S.download_state().items() if isinstance(v, np.ndarray)})
        S.close()
        return None, info

    for ndim in (2, 3):
        case = lr.loaded_case(ndim)
        probes = fs.probe_ids(case["cloud"]["x"].shape[0])
        emit(f"steps/{ndim}-D plain", lambda: stepped(fs.loaded_solver(case, None, fs.prepare(case)), False))
        emit(f"steps/{ndim}-D record, loads set and removed", lambda: stepped(fs.had_loads(case, probes), True))
        emit(f"steps/{ndim}-D loads, record set and dropped", lambda: stepped(fs.had_record(case, probes), False))
        emit(f"steps/{ndim}-D loads, probes and snapshots", lambda: together(case, probes, 1))
        emit(f"steps/{ndim}-D loads, probes and snapshots, pack by slot", lambda: together(case, probes, 0))
        emit(f"steps/{ndim}-D fused damage residual", lambda: fused_damage_residual(ndim))
    emit("steps/3-D damage hooks, mode switches", lambda: damage(xr.erosion_case(3, 0, Gf=xr.erosion_Gf(3, 0))))


def traced_steps():
    """what `--steps-trace` runs under rocprofv3: the shipped (async, non-deterministic) step of one small 3-D Neo-Hookean
    cloud with loads, record probes and snapshots on, 12 steps, a re-sort every 4"""
    import explicit_loads_ref as lr
    import test_gpu_feature_state as fs
    case = lr.loaded_case(3)
    S, bset = fs.loaded_solver(case)
    S.set_resort_interval(4)
    fs.record(S, fs.probe_ids(S.np))
    S.set_snapshots(N.SNAP_ALL, 2)
    for t in range(12):
        fs.step(S, bset, fs.TABLE_STEP[t % fs.NSTEPS])
        slot = S.snapshot_begin(t)
        S.snapshot_wait(slot, copy=False)
        S.snapshot_release(slot)
    S.close()


if "--steps" in sys.argv:
    step_cases()
    sys.exit(0)
if "--steps-trace" in sys.argv:
    traced_steps()
    sys.exit(0)


# ------------------------------------------------------------------------------------------------ linear solves
def linear_cases(S, s, ndim, tag, pcs=mc.PCS, restarts=(30,)):
    """the cases GMRES and MINRES share, on the operator (ALPHA_1, Mv, Dirichlet on) of a linearised cloud"""
    n = s["na"] * ndim
    b, guess = sx.rhs(n, sx.SEED_ATOL), sx.rhs(n, sx.SEED_ATOL + 1)
    bn = float(np.linalg.norm(b))
    solve = lambda *a, **kw: S.tangent_solve(*a, history=True, **kw)  # noqa: E731
    for pc in pcs:
        for restart in restarts:
            emit(f"{tag} pc={pc} restart={restart}", lambda: solve(b, pc=pc, restart=restart, rtol=1e-8, max_it=150))
    emit(f"{tag} guess", lambda: solve(b, x=guess, rtol=1e-8, max_it=150))
    emit(f"{tag} guess, b=0", lambda: solve(np.zeros(n), x=guess))
    emit(f"{tag} b=0", lambda: solve(np.zeros(n)))
    bd, gd = torch.from_numpy(b).cuda(), torch.from_numpy(guess).cuda()
    emit(f"{tag} device vectors", lambda: solve(bd, rtol=1e-8, max_it=150))
    emit(f"{tag} device vectors, guess", lambda: solve(bd, x=gd, rtol=1e-8, max_it=150))
    for max_it in (0, 7):
        emit(f"{tag} max_it={max_it}", lambda: solve(b, rtol=1e-12, max_it=max_it))
    emit(f"{tag} atol 1e-6 ||b||", lambda: solve(b, rtol=0.0, atol=1e-6 * bn, max_it=400))
    emit(f"{tag} atol 10 ||b||", lambda: solve(b, rtol=0.0, atol=10.0 * bn))
    emit(f"{tag} dtol, a guess of 1e8", lambda: solve(b, x=1e8 * guess))
    emit(f"{tag} dtol 0.5", lambda: solve(b, dtol=0.5))
    for value in (np.nan, np.inf):
        bb = b.copy()
        bb[n // 3] = value
        emit(f"{tag} {value} in b", lambda: solve(bb))
        emit(f"{tag} {value} in b, guess", lambda: solve(bb, x=guess))
    emit(f"{tag} after the exits", lambda: solve(b, rtol=1e-10, max_it=400))


for ndim in (2, 3):
    for law in (NHK, DPK):
        s = sx.linearised_device(ndim, law, deterministic=True)
        S, n, Mv, d2m = s["S"], s["na"] * ndim, s["Mv"], s["d2m"]
        # ---- GMRES
        S.tangent_operator(sx.ALPHA_1, Mv, True)
        linear_cases(S, s, ndim, f"gmres {ndim}-D {law}", restarts=(1, 5, 30))
        fixed = np.flatnonzero(d2m == -1)
        for pc in ("none", "pbjacobi"):
            bh = sx.dyadic_rhs(n, fixed, sx.SEED_FIXED)
            emit(f"gmres {ndim}-D {law} happy pc={pc}", lambda: S.tangent_solve(bh, pc=pc, rtol=1e-10, history=True))
            emit(f"gmres {ndim}-D {law} happy pc={pc}, guess", lambda: S.tangent_solve(bh, x=-bh, pc=pc, rtol=1e-10, history=True))
            bn_ = sx.fixed_dof_rhs(d2m, sx.SEED_FIXED)
            emit(f"gmres {ndim}-D {law} happy normal pc={pc}", lambda: S.tangent_solve(bn_, pc=pc, rtol=1e-10, history=True))
        # ---- MINRES
        if law == NHK:
            S.set_linear_solver("minres")
            linear_cases(S, s, ndim, f"minres {ndim}-D")
            S.tangent_operator(mc.NEGATIVE_ALPHA, Mv, True)
            bf = mc.free_dof_rhs(d2m, mc.SEED_INDEFINITE_PC)
            emit(f"minres {ndim}-D indefinite pc", lambda: S.tangent_solve(bf, pc="jacobi", history=True))
            S.tangent_operator(mc.ALPHA_DYNAMIC, Mv, True)
            emit(f"minres {ndim}-D after the indefinite pc", lambda: S.tangent_solve(sx.rhs(n, 3), pc="jacobi", rtol=1e-10, history=True))
            S.set_linear_solver("gmres")
        # ---- Lanczos
        S.tangent_operator(0.0, None, True)
        tag = f"lanczos {ndim}-D {law}"
        v0 = sx.rhs(n, sx.SEED_LANCZOS)
        for mode in (True, False):
            emit(f"{tag} hashed mode={mode}", lambda: lanczos(S, Mv, seed=2, max_it=40, rtol=1e-8, mode=mode, history=True))
            emit(f"{tag} given v0 mode={mode}", lambda: lanczos(S, Mv, v0=v0, max_it=40, rtol=1e-8, mode=mode, history=True))
        emit(f"{tag} device vectors", lambda: lanczos(S, torch.from_numpy(Mv).cuda(), v0=torch.from_numpy(v0).cuda(), max_it=40,
                                                      rtol=1e-8, mode=True, history=True))
        emit(f"{tag} max_it=2 rtol=0", lambda: lanczos(S, Mv, seed=2, max_it=2, rtol=0.0, mode=True, history=True))
        emit(f"{tag} v0=0", lambda: lanczos(S, Mv, v0=np.zeros(n), mode=True, history=True))
        vn = np.ones(n)
        vn[n // 2] = np.nan
        emit(f"{tag} NaN in v0", lambda: lanczos(S, Mv, v0=vn, mode=True, history=True))
        free_dof = int(np.flatnonzero(d2m != -1)[0])
        for value in (0.0, -1.0, np.nan, np.inf):
            bad = Mv.copy()
            bad[free_dof] = value
            emit(f"{tag} mass {value}", lambda: lanczos(S, bad))
        emit(f"{tag} alpha_1 and mass", lambda: (S.tangent_operator(sx.ALPHA_1, Mv, True),
                                                lanczos(S, Mv, seed=9, max_it=60, rtol=1e-8, mode=True, history=True))[1])
        S.close()

for ndim in (2, 3):
    # the singular step: the operator is exactly zero
    S = eroded_device(ndim, "all")
    n = S.nactive * ndim
    S.tangent_operator(0.0, None, False)
    b, guess = sx.rhs(n, sx.SEED_SINGULAR), sx.rhs(n, sx.SEED_SINGULAR + 1)
    emit(f"gmres {ndim}-D singular step", lambda: S.tangent_solve(b, pc="none", history=True))
    emit(f"gmres {ndim}-D singular step, guess", lambda: S.tangent_solve(b, x=guess, pc="none", history=True))
    emit(f"gmres {ndim}-D zero operator, b=0", lambda: S.tangent_solve(np.zeros(n), x=guess, pc="none", history=True))
    emit(f"lanczos {ndim}-D zero operator", lambda: lanczos(S, S.compute_nodal_lumped_mass(), seed=sx.SEED_LANCZOS, mode=True, history=True))
    S.close()
    # the refused preconditioner, and the solves that follow on the same handle
    S = eroded_device(ndim, "part")
    n = S.nactive * ndim
    S.tangent_operator(0.0, None, False)
    b = sx.rhs(n, sx.SEED_REFUSAL)
    for k, kind in enumerate(("jacobi", "pbjacobi", "jacobi")):
        emit(f"gmres {ndim}-D refused {kind} ({k})", lambda: S.tangent_solve(b, pc=kind, history=True))
    emit(f"gmres {ndim}-D after the refusal", lambda: S.tangent_solve(b, pc="none", history=True, **sx.REFUSAL_KSP))
    S.tangent_operator(sx.ALPHA_1, S.compute_nodal_lumped_mass(), True)
    emit(f"gmres {ndim}-D a new operator with mass", lambda: S.tangent_solve(b, pc="pbjacobi", rtol=1e-10, history=True))
    S.close()


# ------------------------------------------------------------------------------------------------ Newton and Newmark
def newton(dev, start, **kw):
    dU, info = dev.solve(start, **kw)
    return dU, info


for ndim in (2, 3):
    case, bcs, gravity, nsteps = _problem(ndim)
    for solver in ("gmres", "minres"):
        for ls in ("basic", "bt"):
            S = gpu_setup(case, nsteps=nsteps)
            S.set_deterministic(True)
            S.set_linear_solver(solver)
            dev = _Step(S, bcs, 0, _alpha(1.0e-2), gravity)
            emit(f"newton {ndim}-D {solver} {ls}",
                 lambda: newton(dev, np.zeros(dev.n), linesearch=ls, ksp=TIGHT, max_it=12, rtol=1e-10, atol=0.0, stol=0.0))
            emit(f"newton {ndim}-D {solver} {ls} driver settings", lambda: newton(dev, np.zeros(dev.n), linesearch=ls, ksp=DRIVER))
            S.close()
        S = gpu_setup(case, nsteps=nsteps)
        S.set_deterministic(True)
        S.set_linear_solver(solver)
        for step in range(2):
            def newmark():
                info = S.newmark_step(bcs, step, 2.0e-2, gravity, ksp=DRIVER, max_it=50, atol=0.0, rtol=1e-10, stol=0.0)
                st = S.download_state()
                return np.concatenate([st[k].ravel() for k in ("x", "vel", "acc", "F_n", "Stress")]), info
            emit(f"newmark {ndim}-D {solver} step {step}", newmark)
        S.close()

# ------------------------------------------------------------------------------------------------ refusals
s = sx.linearised_device(3, NHK, deterministic=True)
S, n, Mv = s["S"], s["na"] * 3, s["Mv"]
b, x = sx.rhs(n, 3), np.zeros(n)
emit("refusal solve: no operator", lambda: S.tangent_solve(b))
emit("refusal lanczos: no operator", lambda: lanczos(S, Mv))
S.tangent_operator(sx.ALPHA_1, Mv, True)
k = ksp_struct()
emit("refusal solve: ksp NULL", lambda: raw(S, S.L.nlps_gpu_tangent_solve(S.h, N._vp(b), N._vp(x), None)))
emit("refusal solve: b NULL", lambda: raw(S, S.L.nlps_gpu_tangent_solve(S.h, None, N._vp(x), C.byref(k))))
emit("refusal solve: x NULL", lambda: raw(S, S.L.nlps_gpu_tangent_solve(S.h, N._vp(b), None, C.byref(k))))
for what, kw in (("pc 7", dict(pc=7)), ("pc -1", dict(pc=-1)), ("restart 0", dict(restart=0)), ("restart 257", dict(restart=257)),
                 ("max_it -1", dict(max_it=-1)), ("rtol -1", dict(rtol=-1.0)), ("rtol NaN", dict(rtol=float("nan"))),
                 ("atol -1", dict(atol=-1.0)), ("dtol 0", dict(dtol=0.0))):
    kk = ksp_struct(**kw)
    emit(f"refusal solve: {what}", lambda: raw(S, S.L.nlps_gpu_tangent_solve(S.h, N._vp(b), N._vp(x), C.byref(kk))))
emit("refusal solve: wrapper pc", lambda: S.tangent_solve(b, pc="ilu"))
S.set_linear_solver("minres")
for what, kw in (("restart 0 is not read", dict(restart=0)), ("max_it -1", dict(max_it=-1)), ("pc 7", dict(pc=7))):
    kk = ksp_struct(**kw)
    emit(f"refusal minres: {what}", lambda: raw(S, S.L.nlps_gpu_tangent_solve(S.h, N._vp(b), N._vp(x), C.byref(kk))))
S.set_linear_solver("gmres")
emit("refusal lanczos: eig NULL", lambda: raw(S, S.L.nlps_gpu_tangent_lambda_max(S.h, N._vp(Mv), None, None, None)))
emit("refusal lanczos: mass NULL", lambda: lanczos(S, None))
for max_it in (0, 257):
    emit(f"refusal lanczos: max_it {max_it}", lambda: lanczos(S, Mv, max_it=max_it))
emit("refusal lanczos: rtol -1", lambda: lanczos(S, Mv, rtol=-1.0))
S.local_search()
emit("refusal solve: stale", lambda: S.tangent_solve(b))
emit("refusal lanczos: stale", lambda: lanczos(S, Mv))
S.close()
for solver in ("gmres", "minres"):
    s = sx.linearised_device(2, NHK, deterministic=True)
    S, Mv = s["S"], s["Mv"]
    S.set_linear_solver(solver)
    S.tangent_operator(sx.ALPHA_1, Mv, True)
    S.set_halo_exchange(lambda dptr, nfield, elem, kind: 0)
    emit(f"refusal solve: halo callback, {solver}", lambda: S.tangent_solve(np.ones(s["na"] * 2)))
    emit(f"refusal lanczos: halo callback, {solver}", lambda: lanczos(S, Mv))
    S.set_halo_exchange(None)
    emit(f"refusal solve: after the halo callback, {solver}", lambda: S.tangent_solve(np.ones(s["na"] * 2), history=True))
    S.close()
for law in ("hencky", DPK):
    s = sx.linearised_device(3, law, deterministic=True)
    emit(f"refusal minres on a {law} cloud", lambda: (None, {"status": s["S"].set_linear_solver("minres")}))
    s["S"].tangent_operator(sx.ALPHA_1, s["Mv"], True)
    emit(f"refusal minres on a {law} cloud: restart 0 is read", lambda: s["S"].tangent_solve(sx.rhs(s["na"] * 3, 3), restart=0))
    s["S"].close()
# Newton
case, bcs, gravity, nsteps = _problem(2)
S = gpu_setup(case, nsteps=nsteps)
S.set_deterministic(True)
dev = _Step(S, bcs, 0, _alpha(1.0e-2), gravity)
z = np.zeros(dev.n)
al = np.ascontiguousarray(dev.alpha, dtype=np.float64)


def newton_raw(sn, dU=z, V=None, alpha=al):
    V = dev.V if V is None else V
    return raw(S, S.L.nlps_gpu_newton_solve(S.h, N._vp(dU), N._vp(V), N._vp(dev.A), N._vp(dev.M), N._d(alpha), None, None, 0, 0,
                                            1.0, None, None if sn is None else C.byref(sn)))


def snes_struct(**kw):
    d = dict(max_it=5, max_funcs=100, atol=1e-8, rtol=1e-10, stol=1e-8, divtol=1e4, linesearch="bt", ls_alpha=1e-4,
             ls_steptol=1e-12, ls_maxstep=1e8, ls_max_it=40, apply_dirichlet=True, ksp=TIGHT)
    edit = {k: kw.pop(k) for k in list(kw) if k.startswith("raw_")}
    d.update(kw)
    sn, keep = S._snes(**d)
    for k, v in edit.items():
        setattr(sn, k[4:], v)
    return sn, keep


emit("refusal newton: snes NULL", lambda: newton_raw(None))
sn0, keep0 = snes_struct()
emit("refusal newton: dU NULL", lambda: newton_raw(sn0, dU=None))
emit("refusal newton: alpha NULL", lambda: newton_raw(sn0, alpha=None))
for what, kw in (("atol -1", dict(atol=-1.0)), ("max_it -1", dict(max_it=-1)), ("linesearch 9", dict(raw_linesearch=9)),
                 ("ls_maxstep 0", dict(ls_maxstep=0.0)), ("ls_max_it -1", dict(ls_max_it=-1))):
    sn1, keep1 = snes_struct(**kw)
    emit(f"refusal newton: {what}", lambda: newton_raw(sn1))
for what, ksp in (("ksp restart 0", dict(TIGHT, restart=0)), ("ksp rtol -1", dict(TIGHT, rtol=-1.0))):
    emit(f"refusal newton: {what}", lambda: newton(dev, z.copy(), ksp=ksp))
S.set_halo_exchange(lambda dptr, nfield, elem, kind: 0)
emit("refusal newton: halo callback", lambda: newton(dev, z.copy(), ksp=TIGHT))
S.set_halo_exchange(None)
emit("newton after the refusals", lambda: newton(dev, z.copy(), linesearch="basic", ksp=TIGHT, max_it=12, rtol=1e-10, atol=0.0, stol=0.0))
S.close()

step_cases()
