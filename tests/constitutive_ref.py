"""Deformation gradients at which the per-particle laws can go wrong, and a 50-digit statement of the three closed-form
laws (Neo-Hookean, Hencky, compressible Newtonian fluid) to hold a double-precision implementation against.

The statements follow the reference's lines, like csrc/nlps_device.hpp and oracle/nlps_oracle.c do:
  Neo-Hookean ........ Constitutive/Hyperelastic/Neo-Hookean.c:18-85 (tau = lambda/2 (J^2 - 1) I + G (b - I); in 2-D the
                       zz slot is lambda/2 (J^2 - 1) and the energy's I1 is the trace of the 2 x 2 block)
  Hencky ............. Constitutive/Hyperelastic/Hencky.c:40-94, 233-285 (principal log strains of b = F F^T; in 2-D the
                       third eigenvalue is fixed at 1)
  Newtonian fluid .... Constitutive/Fluid/Newtonian-Fluid.c:17-79 (L = dt_F F^-1, Macdonald pressure; in 2-D the "trace"
                       is E[0] + E[2] = xx + yx and the zz slot is -p - 2/3 c0 trace, as upstream)
Nothing here is a Jacobi iteration and nothing is done in double: the float64 inputs (F, J, dt_F, the material's numbers)
are converted exactly to mpf, b is formed at 50 digits and its eigen-decomposition is mpmath's eigsy (tridiagonal QL).

The bound: forming b in double perturbs it by O(eps |b|), which moves log(lambda_min) by O(eps cond(b)),
which a modulus multiplies.  So an error is measured in units of 2^-52 * cond(b) * s with s = max(max|ref|, E) (the fluid:
max(max|tau_ref|, K_fluid); Neo-Hookean: max(|b|, 1) in place of cond(b), the law has no logarithm of an eigenvalue), and
a correct implementation stays below C_BOUND of these units.  The constant comes from the CPU oracle and LAPACK
(tests/test_constitutive_ref.py measures both), never from the device."""
import functools
import itertools

import numpy as np

try:
    import mpmath as mp
except ImportError:  # the tests that need the reference skip with this reason; nothing weaker takes its place
    mp = None

MP_SKIP = "mpmath is not installed: there is no 50-digit reference without it"
DPS = 50
EPS = 2.0 ** -52
LAWS = ("neo_hookean", "hencky", "fluid")
# units of 2^-52 cond(b) s: 64 unless the CPU oracle needs more than 16 (then four times its worst value), DESIGN.md §2
C_BOUND = {(law, ndim): 64.0 for law in LAWS for ndim in (2, 3)}

NH = {"type": 0, "E": 1.0e7, "nu": 0.3}
HENCKY = {"type": 1, "E": 1.0e7, "nu": 0.3}
FLUID = {"type": 6, "E": 0.0, "nu": 0.0, "p_ref": 1.0e3, "viscosity": 40.0, "compressibility": 2.0e5, "n_macdonald": 7.0}
MATERIAL = {"neo_hookean": NH, "hencky": HENCKY, "fluid": FLUID}


def tensor_width(ndim):
    return 5 if ndim == 2 else 9


# ------------------------------------------------------------------------------------------------ families of F
def _rotation(rng, ndim):
    if ndim == 2:  # rotation about z
        th = rng.uniform(0.3, 2.8)
        return np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    return Q


def equal_diagonal_cases(ndim):
    """Family (f): b with two EQUAL diagonal entries coupled by an off-diagonal delta whose square underflows.  3-D:
    F = I + delta e_i (x) e_j + big (e_k (x) e_i + |big| e_k (x) e_k), so b_ii == b_jj == 1 exactly, b_ij = delta,
    b_ik = big: every assignment of (i, j, k), big = +-0.1.  2-D: F = I + delta e_i (x) e_j (no third index)."""
    out = []
    for delta in (1e-160, 1e-200, 4.9e-324):
        if ndim == 2:
            for i, j in ((0, 1), (1, 0)):
                F = np.eye(2)
                F[i, j] = delta
                out.append((f"f:delta={delta:g},ij={i}{j}", F))
            continue
        for (i, j, k), big in itertools.product(itertools.permutations(range(3)), (0.1, -0.1)):
            F = np.eye(3)
            F[i, j] = delta
            F[k, i] = big
            F[k, k] = 1.1
            out.append((f"f:delta={delta:g},ijk={i}{j}{k},big={big:+g}", F))
    return out


@functools.lru_cache(maxsize=None)
def families(ndim, seed=20240607):
    """[(name, F[ndim, ndim] float64)].  The doubles these products round to ARE the inputs: both sides get them."""
    rng = np.random.default_rng(seed + ndim)
    R, Q = _rotation(rng, ndim), _rotation(rng, ndim)
    a, c = 1.3, 0.7
    d = ndim
    out = [("a:identity", np.eye(d)), ("a:rotation", R.copy())]

    def spectral(vals):
        return R @ np.diag(vals[:d] if d == 3 else vals) @ R.T

    if d == 3:
        out += [("b:aac", spectral([a, a, c])), ("b:aaa", spectral([a, a, a]))]
        out += [(f"c:gap={g:g}", spectral([a, a * (1.0 + g), c])) for g in (1e-6, 1e-9, 1e-13)]
        out += [(f"d:s={s:g}", Q @ np.diag([s, 1.0, 1.0 / s]) @ R.T) for s in (10.0, 100.0, 1000.0)]
    else:
        out += [("b:ac", spectral([a, c])), ("b:aa", spectral([a, a]))]
        out += [(f"c:gap={g:g}", spectral([a, a * (1.0 + g)])) for g in (1e-6, 1e-9, 1e-13)]
        out += [(f"d:s={s:g}", Q @ np.diag([s, 1.0 / s]) @ R.T) for s in (10.0, 100.0, 1000.0)]
    for gamma in (0.5, 5.0):
        F = np.eye(d)
        F[0, 1] = gamma
        out.append((f"e:shear={gamma:g}", F))
    out += equal_diagonal_cases(d)
    G = rng.normal(size=(d, d))
    out += [(f"g:I+{amp:g}G", np.eye(d) + amp * G) for amp in (1e-12, 1e-8)]
    out += [(f"h:J={J:g}", J ** (1.0 / d) * R) for J in (1e-3, 1e3)]
    return tuple((n, np.ascontiguousarray(F, dtype=np.float64)) for n, F in out)


def rate_tensor(ndim, k):
    """dt_F of case k for the fluid: entries of order one (velocity gradients of order |F^-1|), seeded per case"""
    return np.random.default_rng(7000 + 10 * k + ndim).normal(size=(ndim, ndim))


def tensor_row(A, ndim, zz=1.0):
    """d x d block -> the reference's row (T = 5 in 2-D with the zz slot, 9 in 3-D)"""
    row = np.zeros(tensor_width(ndim))
    row[: ndim * ndim] = np.asarray(A, dtype=np.float64).ravel()
    if ndim == 2:
        row[4] = zz
    return row


def shuffled_cloud(ncases, npart=3 * 64 + 7, seed=99):
    """Case index of every particle: the cases tiled to npart and shuffled, so that neighbouring lanes of a wave leave the
    eigen-solver's sweep loop after different counts and the last wave is ragged."""
    idx = np.resize(np.arange(ncases), npart)
    return np.random.default_rng(seed).permutation(idx)


# ------------------------------------------------------------------------------------------------ 50-digit laws
def _mpm(A):
    A = np.asarray(A, dtype=np.float64)
    return mp.matrix([[mp.mpf(float(x)) for x in row] for row in A])  # (float -> mpf is exact)


def _b_and_spectrum(F, ndim):
    Fm = _mpm(F)
    b = Fm * Fm.T
    w, V = mp.eigsy(b)
    w = [w[i] for i in range(ndim)]
    return b, w, V


def reference(law, mat, F, J, dtF, ndim):
    """{"tau": [T mpf], "W": mpf or None, "cond": float, "normb": float} of one particle at mp.dps = 50."""
    with mp.workdps(DPS):
        T = tensor_width(ndim)
        half = mp.mpf(1) / 2
        Jm = mp.mpf(float(J))
        b, w, V = _b_and_spectrum(F, ndim)
        wmax, wmin = max(w), min(w)
        out = {"cond": float(wmax / wmin), "normb": float(wmax), "W": None}
        tau = [mp.mpf(0)] * T
        if law == "fluid":
            n, K, p0, mu = (mp.mpf(float(mat[k])) for k in ("n_macdonald", "compressibility", "p_ref", "viscosity"))
            L = _mpm(dtF) * mp.inverse(_mpm(F))
            E = (L + L.T) * half
            p = Jm * (p0 + (K / n) * (mp.power(Jm, -n) - 1))
            c0 = Jm * mu
            trace = E[0, 0] + E[1, 0] if ndim == 2 else E[0, 0] + E[1, 1] + E[2, 2]
            vol = -p - mp.mpf(2) / 3 * c0 * trace
            for i in range(ndim):
                for j in range(ndim):
                    tau[i * ndim + j] = (vol if i == j else 0) + 2 * c0 * E[i, j]
            if ndim == 2:
                tau[4] = vol
            out["tau"] = tau
            return out
        E_, nu = mp.mpf(float(mat["E"])), mp.mpf(float(mat["nu"]))
        G = E_ / (2 * (1 + nu))
        lame = nu * E_ / ((1 - 2 * nu) * (1 + nu))
        if law == "neo_hookean":
            c0 = lame * half * (Jm * Jm - 1)
            for i in range(ndim):
                for j in range(ndim):
                    Id = 1 if i == j else 0
                    tau[i * ndim + j] = c0 * Id + G * (b[i, j] - Id)
            if ndim == 2:
                tau[4] = c0
            I1 = sum(b[i, i] for i in range(ndim))
            lj = mp.log(Jm)
            out["W"] = lame / 4 * (Jm * Jm - 1) - half * lame * lj - G * lj + half * G * (I1 - ndim)
        elif law == "hencky":
            Eh = [half * mp.log(x) for x in w] + ([mp.mpf(0)] if ndim == 2 else [])  # 2-D: third eigenvalue 1
            tr = Eh[0] + Eh[1] + Eh[2]
            Tp = [lame * tr + 2 * G * e for e in Eh]
            for i in range(ndim):
                for j in range(ndim):
                    tau[i * ndim + j] = sum(Tp[A] * V[i, A] * V[j, A] for A in range(ndim))
            if ndim == 2:
                tau[4] = Tp[2]
            out["W"] = half * (Tp[0] * Eh[0] + Tp[1] * Eh[1] + Tp[2] * Eh[2])
        else:
            raise ValueError(law)
        out["tau"] = tau
        return out


def eigen_reference(F, ndim):
    """(eigenvalues of b = F F^T ascending [mpf], |b|_2 as float), b formed at 50 digits"""
    with mp.workdps(DPS):
        _, w, _ = _b_and_spectrum(F, ndim)
        w = sorted(w)
        return w, float(max(abs(x) for x in w))


@functools.lru_cache(maxsize=None)
def references(law, ndim):
    """The reference of every case of families(ndim), computed once per (law, ndim) and shared; with each case's inputs:
    [{"name", "F", "J", "dtF", "tau", "W", "cond", "normb"}]"""
    out = []
    for k, (name, F) in enumerate(families(ndim)):
        J = float(np.linalg.det(F))
        dtF = rate_tensor(ndim, k)
        r = reference(law, MATERIAL[law], F, J, dtF, ndim)
        r.update(name=name, F=F, J=J, dtF=dtF)
        out.append(r)
    return tuple(out)


def abs_error(values, ref):
    """max |value - ref| over the entries, the difference taken at 50 digits; inf where a value is not finite"""
    values = np.atleast_1d(np.asarray(values, dtype=np.float64))
    if not np.all(np.isfinite(values)):
        return float("inf")
    with mp.workdps(DPS):
        return float(max(abs(mp.mpf(float(v)) - r) for v, r in zip(values, ref)))


def scale_of(law, mat, ref):
    with mp.workdps(DPS):
        return max(float(max(abs(t) for t in ref)), float(mat["compressibility"] if law == "fluid" else mat["E"]))


def unit_of(law, mat, r, ref):
    """2^-52 * cond(b) * s (Neo-Hookean: max(|b|, 1) for cond(b)) for the entries `ref` of case r"""
    amp = max(r["normb"], 1.0) if law == "neo_hookean" else r["cond"]
    return EPS * amp * scale_of(law, mat, ref)


def error_units(law, mat, r, tau, W=None):
    """(error of tau, error of W or 0.0), each in its unit; what a correct double implementation keeps below C_BOUND"""
    et = abs_error(tau, r["tau"]) / unit_of(law, mat, r, r["tau"])
    ew = 0.0
    if W is not None and r["W"] is not None:
        ew = abs_error([W], [r["W"]]) / unit_of(law, mat, r, [r["W"]])
    return et, ew


# ------------------------------------------------------------------------------------------------ numpy / LAPACK
def numpy_law(law, mat, F, J, dtF, ndim):
    """The same three laws in double with LAPACK (eigh, inv): the second, non-Jacobi witness that the bound is achievable"""
    T = tensor_width(ndim)
    tau = np.zeros(T)
    F = np.asarray(F, dtype=np.float64)
    b = F @ F.T
    if law == "fluid":
        n, K, p0, mu = mat["n_macdonald"], mat["compressibility"], mat["p_ref"], mat["viscosity"]
        L = dtF @ np.linalg.inv(F)
        E = 0.5 * (L + L.T)
        p = J * (p0 + (K / n) * (J ** (-n) - 1.0))
        c0 = J * mu
        trace = E[0, 0] + E[1, 0] if ndim == 2 else np.trace(E)
        vol = -p - (2.0 / 3.0) * c0 * trace
        tau[: ndim * ndim] = (vol * np.eye(ndim) + 2.0 * c0 * E).ravel()
        if ndim == 2:
            tau[4] = vol
        return tau, None
    G = mat["E"] / (2 * (1 + mat["nu"]))
    lame = mat["nu"] * mat["E"] / ((1 - 2 * mat["nu"]) * (1 + mat["nu"]))
    if law == "neo_hookean":
        c0 = lame * 0.5 * (J * J - 1.0)
        tau[: ndim * ndim] = (c0 * np.eye(ndim) + G * (b - np.eye(ndim))).ravel()
        if ndim == 2:
            tau[4] = c0
        W = 0.25 * lame * (J * J - 1) - 0.5 * lame * np.log(J) - G * np.log(J) + 0.5 * G * (np.trace(b) - ndim)
        return tau, float(W)
    w, V = np.linalg.eigh(b)
    Eh = np.zeros(3)
    Eh[:ndim] = 0.5 * np.log(w)
    Tp = lame * Eh.sum() + 2 * G * Eh
    tau[: ndim * ndim] = ((V * Tp[:ndim]) @ V.T).ravel()
    if ndim == 2:
        tau[4] = Tp[2]
    return tau, float(0.5 * Tp @ Eh)


# ------------------------------------------------------------------------------------------------ plastic laws
PLASTIC_LAWS = ("drucker_prager", "von_mises", "matsuoka_nakai", "lade_duncan")
AMPLITUDES = (1e-4, 1e-3, 1e-2, 5e-2)
TOL_RR, ITS_RR = 1e-10, 20  # what upstream's Matsuoka-Nakai reader sets (InOutFun/Material/Plasticity/Matsuoka-Nakai.c:82-83)


def plastic_material(law):
    from util import synth
    return {"drucker_prager": synth.drucker_prager_material, "von_mises": synth.von_mises_material,
            "matsuoka_nakai": lambda: synth.matsuoka_nakai_material(False),
            "lade_duncan": lambda: synth.matsuoka_nakai_material(True)}[law]()


def increments(ndim, amp, seed=515):
    """[(name, DF)]: families (b), (c), (e), (f), (g) as strain increments of amplitude amp around I; the second value is
    whether the case keeps its meaning only on an isotropic b_e_n (family (f): the equal diagonals of the trial state)"""
    rng = np.random.default_rng(seed + ndim)
    R = _rotation(rng, ndim)
    d = ndim
    p, m = 1.0 + amp, 1.0 - amp
    out = []
    if d == 3:
        out += [("b:aac", R @ np.diag([p, p, m]) @ R.T, False), ("b:aaa", R @ np.diag([p, p, p]) @ R.T, False)]
        out += [(f"c:gap={g:g}", R @ np.diag([p, p * (1.0 + g), m]) @ R.T, False) for g in (1e-6, 1e-9, 1e-13)]
    else:
        out += [("b:ac", R @ np.diag([p, m]) @ R.T, False), ("b:aa", R @ np.diag([p, p]) @ R.T, False)]
        out += [(f"c:gap={g:g}", R @ np.diag([p, p * (1.0 + g)]) @ R.T, False) for g in (1e-6, 1e-9, 1e-13)]
    F = np.eye(d)
    F[0, 1] = amp
    out.append(("e:shear", F, False))
    for name, F in equal_diagonal_cases(d):  # the large entries 0.1 -> amp
        DF = np.where(np.abs(np.abs(F) - 0.1) < 1e-12, np.sign(F) * amp, F)
        DF = np.where(np.abs(F - 1.1) < 1e-12, 1.0 + amp, DF)
        out.append((name, DF, True))
    G = rng.normal(size=(d, d))
    out += [(f"g:I+{a:g}G", np.eye(d) + a * G, False) for a in (1e-12, 1e-8, 0.5 * amp)]
    return [(f"{n},amp={amp:g}", np.ascontiguousarray(DF), iso) for n, DF, iso in out]


def elastic_states(law, mat, ndim, seed=77):
    """[(name, b_e_n row [T], isotropic)]: the state the increment starts from.  Drucker-Prager and Von-Mises: the unit
    tensor and b = F F^T of families (b) and (c) at amplitude 1e-4.  Matsuoka-Nakai and Lade-Duncan need compressive
    principal stresses (synth.frictional_states): an isotropic state at -20 and two states close to the surface."""
    from util import synth
    rng = np.random.default_rng(seed + ndim)
    d = ndim
    if law in ("matsuoka_nakai", "lade_duncan"):
        e = (1.0 - 2.0 * mat["nu"]) / mat["E"] * -20.0  # principal log strain of the hydrostatic stress -20
        rows = synth.frictional_states(ndim, mat, 2, seed=seed)
        return [("hydrostatic", tensor_row(np.exp(2 * e) * np.eye(d), d, np.exp(2 * e)), True),
                ("near-surface-0", rows[0], False), ("near-surface-1", rows[1], False)]
    R = _rotation(rng, d)
    p, m = 1.0 + 1e-4, 1.0 - 1e-4
    Fb = R @ np.diag([p, p, m][:d] if d == 3 else [p, m]) @ R.T
    Fc = R @ np.diag([p, p * (1.0 + 1e-9), m][:d] if d == 3 else [p, p * (1.0 + 1e-9)]) @ R.T
    return [("unit", tensor_row(np.eye(d), d), True), ("b", tensor_row(Fb @ Fb.T, d), False), ("c", tensor_row(Fc @ Fc.T, d), False)]


@functools.lru_cache(maxsize=None)
def plastic_cases(law, ndim, rr=None):
    """Every case of one plastic law with the CPU oracle's answer, computed once and shared (rr: the return mapping's
    (tolerance, iterations) instead of plastic_params' choice):
    [{"name", "DF" row, "b_e_n" row, "kappa_n", "eps_n", "cond" of the trial state, "status", "Stress", "W", "b_e_n1",
      "Kappa_n1", "EPS_n1", "C_ep", "Back_stress"}]"""
    from util import orc
    o = orc()
    mat = plastic_material(law)
    omat = o.make_materials([mat])[0]
    prm = plastic_params(o.default_params(), law, rr)
    kappa_n = mat["kappa_0"] if law != "von_mises" else 0.0
    eps_n = mat["eps_0"] if law in ("matsuoka_nakai", "lade_duncan") else 0.0
    def answer(DFrow, be):
        back = np.zeros(3)
        cep = np.zeros(ndim * ndim)
        st, tau, W, b1, k1, e1 = o.stress_one(ndim, omat, prm, DFrow, DFrow, 1.0, be, kappa_n, eps_n, back_stress=back, C_ep=cep)
        return {"status": st, "Stress": tau, "W": W, "b_e_n1": b1, "Kappa_n1": k1, "EPS_n1": e1, "C_ep": cep, "Back_stress": back}

    out = []
    for amp in AMPLITUDES:
        for dname, DF, needs_iso in increments(ndim, amp):
            for sname, be, iso in elastic_states(law, mat, ndim):
                if needs_iso and not iso:
                    continue
                DFrow = tensor_row(DF, ndim)
                btr = o.trial_b_e(DF, be[: ndim * ndim].reshape(ndim, ndim), ndim)
                out.append(dict(answer(DFrow, be), name=f"{dname}|{sname}", DF=DFrow, b_e_n=be, kappa_n=kappa_n, eps_n=eps_n,
                                cond=float(np.linalg.cond(btr))))
    # The oracle's own error at every case: how far its answer moves when every entry of DF and b_e_n moves by one ulp
    # (8 fixed sign patterns), in the units the comparison uses (the field's largest magnitude over the cases; C_ep: at
    # least E).  Where that exceeds the tolerance the iteration sits on one of its own decisions (a stopping test or a
    # line-search step within rounding of its threshold), and two correct implementations may differ by as much.
    ok = [c for c in out if c["status"] == 0]
    scale = {k: max([float(np.max(np.abs(c[k]))) for c in ok] + [mat["E"] if k == "C_ep" else 1e-300]) for k in PLASTIC_FIELDS}
    signs = np.random.default_rng(2718).choice([-1.0, 1.0], size=(8, 2 * tensor_width(ndim)))
    T = tensor_width(ndim)
    for c in out:
        own = 0.0
        for s in signs if c["status"] == 0 else ():
            a = answer(np.nextafter(c["DF"], c["DF"] + s[:T]), np.nextafter(c["b_e_n"], c["b_e_n"] + s[T:]))
            own = max([own] + [float(np.max(np.abs(a[k] - c[k]))) / scale[k] for k in PLASTIC_FIELDS])
        c["own_error"] = own
    return tuple(out)


PLASTIC_FIELDS = ("Stress", "W", "b_e_n1", "Kappa_n1", "EPS_n1", "C_ep", "Back_stress")
PLASTIC_TOL = 1e-10  # the project's tolerance for these fields


def plastic_params(prm, law, rr=None):
    """Drucker-Prager and Von-Mises: the defaults (1e-14, 10 iterations); the frictional laws: their reader's values"""
    if rr is not None:
        prm.tol_radial_returning, prm.max_iter_radial_returning = rr
    elif law in ("matsuoka_nakai", "lade_duncan"):
        prm.tol_radial_returning, prm.max_iter_radial_returning = TOL_RR, ITS_RR
    return prm
