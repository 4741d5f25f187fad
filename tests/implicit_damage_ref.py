"""One implicit Newmark step with the damage hooks, as a composition of the oracle's stage calls (the definition of
nlps_gpu_set_implicit_damage in include/nlps_gpu.h carried through nlps_gpu_newmark_step): search, active nodes, the
epsilon-neighbourhoods, lumped mass, nodal field, explicit trial, then snes_ref.newton over a residual that is, per
evaluation and in the order of U-Newmark-beta.c:1018-1036, compatibility, the constitutive update that skips failed
particles, the eigenerosion or eigensoftening hook, the internal forces and the inertial term; the tangent is the oracle's
with 1 - Damage_n1 (set_tangent_damage); after the solve the roll, Damage_n <- Damage_n1 and the kinetics update.  No
Dirichlet sets, no gravity (the scenarios of explicit_damage_ref.py have neither).  One thread, like the reference's
sequential eigensoftening loop."""
import functools

import numpy as np

import explicit_damage_ref as xr
import snes_ref
from newmark import newmark_parameters
from util import oracle_setup, orc

DT = xr.DT
DT_TWO_ITERATES = [5e-3]  # a single 2-D step that takes two Newton iterates
BETA, GAMMA = 0.25, 0.5
SNES = dict(max_it=50, rtol=1e-8, atol=0.0, stol=0.0, linesearch="bt")
FIELDS = ("x", "dis", "vel", "acc", "F_n", "J_n", "stress", "W")


class ImplicitDamageRef:
    """driver: "erosion" or "softening" """

    def __init__(self, case, driver):
        self.o = orc()
        self.case, self.driver = case, driver
        self.M, self.P, self.prm, self.mats = oracle_setup(case)
        n = self.P.np
        cloud = case["cloud"]
        zero = np.zeros(n)
        self.damage_n = np.array(cloud.get("damage_n", zero), dtype=np.float64)
        self.damage_n1 = self.damage_n.copy()
        self.strain_f = np.array(cloud.get("strain_f_n", zero), dtype=np.float64)  # StrainF_n and StrainF_n1 are one array
        if driver == "erosion":  # U-Newmark-beta.c:182-183
            self.beps = self.o.compute_beps(self.P, self.M, self.mats, initialize=True)
        else:  # :213-215: never initialised
            self.beps = (np.zeros(n, dtype=np.int32), np.full((n, self.o.BEPS_STRIDE), -1, dtype=np.int32))
        self.evals = []  # the margins of every residual evaluation of the last step
        self.info, self.na = None, 0

    def _neighbours(self, p):
        return self.beps[1][p, : self.beps[0][p]]

    def _hook(self):
        """the hook of one evaluation, with the quantities that decide it restated for the margins"""
        o, P, mats = self.o, self.P, self.mats
        nd = P.ndim
        T0 = xr.min_principal(P["stress"], nd)
        live = self.damage_n < 1.0
        diag = {"T0": T0, "T0_margin": float(np.min(np.abs(T0[live])) / np.abs(T0[live]).max())}
        if self.driver == "erosion":
            cand = np.where(live & (T0 > 0.0))[0]
            V, W, h = P["vol0"] * P["J_n1"], P["W"], self.case["h"]
            G = np.zeros(cand.size)
            for i, p in enumerate(cand):
                q = self._neighbours(p)
                lq = self.damage_n[q] < 1.0
                G[i] = mats[P["matidx"][p]].Ceps * h / (V[p] + V[q].sum()) * (V[p] * W[p] + (V[q][lq] * W[q][lq]).sum())
            diag.update(cand=cand, G=G)
            assert o.eigenerosion_hook(self.damage_n1, self.damage_n, P, mats, self.beps, h) == 0
        else:
            sf_before = self.strain_f.copy()
            assert o.eigensoftening_hook(self.damage_n1, self.damage_n, self.strain_f, P, mats, self.beps) == 0
            cand = np.where((self.damage_n == 0.0) & (T0 > 0.0))[0]
            m = P["mass"]
            Teps = np.zeros(cand.size)
            for i, p in enumerate(cand):  # (restated as in explicit_damage_ref.DamageRef)
                q = self._neighbours(p)
                term = m[p] * T0[p]
                lq = q[self.damage_n[q] < 1.0]
                if lq.size:
                    ql = lq[-1]
                    term = m[ql] * (T0[ql] * (1.0 - self.damage_n1[ql]) if ql < p else T0[ql])
                Teps[i] = term / (m[p] + m[q].sum())
            diag.update(cand=cand, Teps=Teps, started=(self.strain_f > 0) & (sf_before == 0))
        self.evals.append(diag)

    def step(self, dt):
        o = self.o
        threads = o.num_threads()
        o.set_num_threads(1)
        try:
            self._step(dt)
        finally:
            o.set_num_threads(threads)

    def _step(self, dt):
        o, P, M, prm, mats = self.o, self.P, self.M, self.prm, self.mats
        nd = P.ndim
        assert o.local_search(P, M, prm) == 0
        n2m, na = o.active_nodes(M)
        d2m = np.zeros(na * nd, dtype=np.int32)  # no Dirichlet set: every dof is free
        o.compute_beps(P, M, mats, beps=self.beps, initialize=False)
        mass = o.lumped_mass(P, M, n2m, na)
        V, A = o.nodal_field_n(mass, P, M, n2m, d2m, na)
        a = newmark_parameters(BETA, GAMMA, dt)
        self.evals = []

        def residual(x):
            x = np.ascontiguousarray(x, dtype=np.float64)
            assert o.compatibility(x, None, P, M, n2m) == 0
            assert o.constitutive_eroded(P, mats, prm, self.damage_n) == 0
            self._hook()
            R, st = o.internal_forces(P, M, n2m, d2m, na)
            assert st == 0
            return R + mass * (a["a1"] * x - a["a2"] * V - a["a3"] * A)

        def tangent():
            o.set_tangent_damage(self.damage_n1)
            try:
                K, _, st = o.tangent_matrix(P, M, mats, n2m, d2m, na, alpha_1=a["a1"], lumped_mass=mass, with_pattern=False)
            finally:
                o.set_tangent_damage(None)
            assert st == 0
            return K

        guess = dt * V + (0.5 * dt * dt) * A  # __form_initial_guess, explicit trial
        dU, info = snes_ref.newton(residual, tangent, guess, linear="dense", **SNES)
        self.info, self.na, self.n2m, self.dU = info, na, n2m, dU
        self.masked = {"M": mass, "V": V, "A": A, "alpha": [a["a1"], a["a2"], a["a3"], a["a4"], a["a5"], a["a6"]], "guess": guess}
        if info["reason"] <= 0:
            return
        dU_dt = a["a4"] * dU + (a["a5"] - 1.0) * V + a["a6"] * A
        dU_dt2 = a["a1"] * dU - a["a2"] * V - (a["a3"] + 1.0) * A
        o.roll_state(P)
        self.damage_n[:] = self.damage_n1  # U-Newmark-beta.c:1950-1956 (Strain_f: one array)
        assert o.update_kinetics(1.0, dU, V, dU_dt, dU_dt2, P, M, n2m) == 0

    def snapshot(self):
        s = {k: self.P[k].copy() for k in FIELDS}
        s.update(damage=self.damage_n1.copy(), strain_f=self.strain_f.copy(), na=self.na, info=self.info, evals=self.evals,
                 dU=self.dU.copy())
        return s


def _run(case, driver, dts):
    R = ImplicitDamageRef(case, driver)
    out = []
    for dt in dts:
        R.step(dt)
        out.append(R.snapshot())
    return out


@functools.lru_cache(maxsize=None)
def erosion_Gf(ndim, laws, dts=tuple(DT)):
    """midway between the two neighbours at the 0.75 quantile of step 0's G values in a run nobody fails in (the values
    of the step's last residual evaluation)"""
    s = _run(xr.erosion_case(ndim, laws, Gf=1e300), "erosion", dts[:1])[0]
    d = s["evals"][-1]
    assert d["cand"].size == s["damage"].size, "every particle is stretched in every principal direction"
    G = np.sort(d["G"])
    k = int(0.75 * G.size)
    return float(0.5 * (G[k - 1] + G[k]))


@functools.lru_cache(maxsize=None)
def erosion_reference(ndim, laws, dts=tuple(DT)):
    """snapshots after each of the steps (read-only: shared by the tests)"""
    return _run(xr.erosion_case(ndim, laws, Gf=erosion_Gf(ndim, laws, dts)), "erosion", dts)


@functools.lru_cache(maxsize=None)
def softening_ft(ndim, law):
    """the median smallest principal stress of the candidates of a first step nobody starts to fracture in"""
    R = ImplicitDamageRef(xr.softening_case(ndim, law, ft=1e300), "softening")
    R.step(DT[0])
    d = R.evals[-1]
    return float(np.median(d["T0"][d["cand"]]))


@functools.lru_cache(maxsize=None)
def softening_reference(ndim, law, dts=tuple(DT)):
    return _run(xr.softening_case(ndim, law, ft=softening_ft(ndim, law)), "softening", dts)
