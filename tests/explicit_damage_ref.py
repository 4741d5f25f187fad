"""The explicit step with the damage hooks, as a composition of the oracle's stage calls (the definition of
nlps_gpu_set_explicit_damage in include/nlps_gpu.h): orc_explicit_step with the hooks of the maintained driver at the
places U-Newmark-beta.c puts them.  Search, active nodes, lumped mass, shape functions, compatibility, the constitutive
update that skips failed particles, the epsilon-neighbourhoods, the two hooks and the internal forces are the oracle's;
the predictor, the projection of dU, the nodal equilibrium, the G2P and the corrector are restated here in numpy in the
oracle's loop order (no Dirichlet sets, no gravity: the scenarios below have neither).  One thread, like the reference's
sequential eigensoftening loop."""
import functools

import numpy as np

from util import make_case, oracle_setup, orc

DT = [1e-3, 1e-4, 1e-4, 1e-4]
GAMMA = 0.5
E, NU, CEPS = 1.0e6, 0.25, 1.5


def velocity_field(x, seed=7):
    u = np.random.default_rng(seed).uniform(size=(x.shape[0], 1))
    return 10.0 * (x - x.mean(axis=0)) * (1.0 + 0.5 * u)


def erosion_case(ndim, laws, Gf=0.0):
    """laws: one law, or several that are dealt to the particles in turn (a cloud of interleaved laws)"""
    laws = list(laws) if isinstance(laws, (list, tuple)) else [laws]
    mats = [{"type": l, "E": E, "nu": NU, "Ceps": CEPS, "Gf": Gf} for l in laws]
    if ndim == 3:
        case = make_case(3, [11, 10, 9], [3, 3, 2], [5, 4, 4], material=mats[0])  # 640 particles, 3 x 3 x 3 tiles
    else:
        case = make_case(2, [22, 12], [6, 3], [12, 6], material=mats[0])  # 288 particles across the tile boundary at node 16
    cloud = case["cloud"]
    cloud["vel"] = velocity_field(cloud["x"])
    case["materials"] = mats
    if len(mats) > 1:
        cloud["matidx"] = (np.arange(cloud["x"].shape[0]) % len(mats)).astype(np.int32)
    return case


def softening_case(ndim, law, ft=0.0):
    """the pre-damaged, partly moved cloud of test_gpu_eigensoftening.py with the velocity field of the erosion scenario"""
    rng = np.random.default_rng(33)
    mat = {"type": law, "E": E, "nu": NU, "Ceps": CEPS, "ft": ft, "heps": 2.0, "wcrit": 0.05}
    if ndim == 2:
        case = make_case(2, [14, 12], [3, 3], [7, 6], material=mat)
    else:
        case = make_case(3, [11, 10, 9], [3, 3, 2], [5, 4, 4], material=mat)
    cloud = case["cloud"]
    npart = cloud["x"].shape[0]
    dis = np.zeros_like(cloud["x"])
    dis[rng.uniform(size=npart) < 0.5] = 1e-3
    cloud["dis"] = dis
    damage0, strain_f0 = np.zeros(npart), np.zeros(npart)
    pick = rng.permutation(npart)
    damage0[pick[:npart // 10]] = 1.0
    damage0[pick[npart // 10: npart // 5]] = 0.3
    strain_f0[pick[npart // 10: npart // 4]] = 1e-3
    cloud["damage_n"] = damage0
    cloud["strain_f_n"] = strain_f0
    cloud["vel"] = velocity_field(cloud["x"])
    return case


def min_principal(stress, ndim):
    n = stress.shape[0]
    tau = stress[:, : ndim * ndim].reshape(n, ndim, ndim)
    return np.linalg.eigvalsh(0.5 * (tau + np.transpose(tau, (0, 2, 1))))[:, 0]


class DamageRef:
    """driver: None (the plain explicit step), "erosion" or "softening" """

    def __init__(self, case, driver=None):
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
        elif driver == "softening":  # :213-215: never initialised
            self.beps = (np.zeros(n, dtype=np.int32), np.full((n, self.o.BEPS_STRIDE), -1, dtype=np.int32))
        self.nodal, self.diag, self.n2m, self.na = {}, {}, None, 0

    def step(self, dt, gamma=GAMMA):
        o = self.o
        threads = o.num_threads()
        o.set_num_threads(1)
        try:
            self._step(dt, gamma)
        finally:
            o.set_num_threads(threads)

    def _neighbours(self, p):
        return self.beps[1][p, : self.beps[0][p]]

    def _step(self, dt, gamma):
        o, P, M, prm, mats = self.o, self.P, self.M, self.prm, self.mats
        nd, n = P.ndim, P.np
        assert o.local_search(P, M, prm) == 0
        n2m, na = o.active_nodes(M)
        mass = o.lumped_mass(P, M, n2m, na)
        # predictor
        P["d_dis"][:] = dt * P["vel"] + (0.5 * (dt * dt)) * P["acc"]
        P["vel"][:] += ((1 - gamma) * dt) * P["acc"]
        # nodal dU
        dU = np.zeros((na, nd))
        shape, rows = [], []
        for p in range(n):
            N = o.compute_N(P, M, p)
            r = n2m[P["list"][p, : N.size]]
            dU[r] += (P["mass"][p] * N)[:, None] * P["d_dis"][p]
            shape.append(N)
            rows.append(r)
        dU = dU.ravel()
        with np.errstate(divide="ignore", invalid="ignore"):
            dU = np.where(mass != 0.0, dU / mass, 0.0)
        # local state
        assert o.compatibility(dU, None, P, M, n2m) == 0
        assert (P["J_n1"] > 0.0).all()
        DF = P["DF"]
        if nd == 2:
            detDF = DF[:, 0] * DF[:, 3] - DF[:, 1] * DF[:, 2]
        else:
            detDF = (DF[:, 0] * DF[:, 4] * DF[:, 8] - DF[:, 0] * DF[:, 5] * DF[:, 7] + DF[:, 1] * DF[:, 5] * DF[:, 6] -
                     DF[:, 1] * DF[:, 3] * DF[:, 8] + DF[:, 2] * DF[:, 3] * DF[:, 7] - DF[:, 2] * DF[:, 4] * DF[:, 6])
        P["rho"][:] = P["rho"] / detDF
        self.diag = {}
        if self.driver is None:
            assert o.constitutive(P, mats, prm) == 0
        else:
            o.compute_beps(P, M, mats, beps=self.beps, initialize=False)
            assert o.constitutive_eroded(P, mats, prm, self.damage_n) == 0
            T0 = min_principal(P["stress"], nd)
            if self.driver == "erosion":
                cand = np.where((self.damage_n < 1.0) & (T0 > 0.0))[0]
                V = P["vol0"] * P["J_n1"]
                W = P["W"]
                h = self.case["h"]
                G = np.zeros(cand.size)
                for i, p in enumerate(cand):
                    q = self._neighbours(p)
                    live = self.damage_n[q] < 1.0
                    G[i] = mats[P["matidx"][p]].Ceps * h / (V[p] + V[q].sum()) * (V[p] * W[p] + (V[q][live] * W[q][live]).sum())
                self.diag = {"cand": cand, "G": G, "T0": T0}
                assert o.eigenerosion_hook(self.damage_n1, self.damage_n, P, mats, self.beps, h) == 0
            else:
                sf_before = self.strain_f.copy()
                assert o.eigensoftening_hook(self.damage_n1, self.damage_n, self.strain_f, P, mats, self.beps) == 0
                # T_eps of the first branch, restated: the own term, or the term of the LAST list entry with Damage_n < 1,
                # its stress scaled already iff it came earlier in the loop (damage_n1 of a neighbour depends on its own
                # data only, so the values after the loop are the values it had then)
                cand = np.where((self.damage_n == 0.0) & (T0 > 0.0))[0]
                m = P["mass"]
                Teps = np.zeros(cand.size)
                for i, p in enumerate(cand):
                    q = self._neighbours(p)
                    term = m[p] * T0[p]
                    live = q[self.damage_n[q] < 1.0]
                    if live.size:
                        ql = live[-1]
                        term = m[ql] * (T0[ql] * (1.0 - self.damage_n1[ql]) if ql < p else T0[ql])
                    Teps[i] = term / (m[p] + m[q].sum())
                self.diag = {"cand": cand, "Teps": Teps, "T0": T0, "started": (self.strain_f > 0) & (sf_before == 0)}
        # nodal forces and equilibrium
        fint, st = o.internal_forces(P, M, n2m, np.zeros(na * nd, dtype=np.int32), na)
        assert st == 0
        force = -fint
        with np.errstate(divide="ignore", invalid="ignore"):
            accel = np.where(mass != 0.0, 0.0 + force / mass, 0.0)
        # G2P (sums in list order) and corrector
        a2, u2 = accel.reshape(na, nd), dU.reshape(na, nd)
        for p in range(n):
            N, r = shape[p][:, None], rows[p]
            P["acc"][p] = np.cumsum(N * a2[r], axis=0)[-1]
            P["d_dis"][p] = np.cumsum(N * u2[r], axis=0)[-1]
        P["J_n"][:] = P["J_n1"]
        P["kappa_n"][:] = P["kappa_n1"]
        P["eps_n"][:] = P["eps_n1"]
        P["b_e_n"][:] = P["b_e_n1"]
        P["vel"][:] += (gamma * dt) * P["acc"]
        P["x"][:] += P["d_dis"]
        P["dis"][:] += P["d_dis"]
        P["F_n"][:] = P["F_n1"]
        self.damage_n[:] = self.damage_n1  # U-Newmark-beta.c:1950-1956 (Strain_f: one array)
        self.n2m, self.na = n2m, na
        self.nodal = {"mass": mass, "dU": dU, "force": force, "accel": accel}

    FIELDS = ("x", "dis", "vel", "acc", "F_n", "J_n", "rho", "stress", "W")

    def snapshot(self):
        s = {k: self.P[k].copy() for k in self.FIELDS}
        s.update(damage=self.damage_n1.copy(), strain_f=self.strain_f.copy(), na=self.na,
                 nodal={k: v.copy() for k, v in self.nodal.items()}, diag=self.diag)
        return s


def erosion_G_step1(ndim, laws):
    """energy release rates of step 1 in a run nobody fails in"""
    R = DamageRef(erosion_case(ndim, laws, Gf=1e300), "erosion")
    R.step(DT[0])
    assert R.diag["cand"].size == R.P.np, "every particle is stretched in every principal direction"
    return R.diag["G"]


@functools.lru_cache(maxsize=None)
def erosion_Gf(ndim, laws):
    """midway between two neighbours of the sorted step-1 values: a quarter of the cloud fails in step 1"""
    G = np.sort(erosion_G_step1(ndim, laws))
    k = int(0.75 * G.size)
    return float(0.5 * (G[k - 1] + G[k]))


@functools.lru_cache(maxsize=None)
def erosion_reference(ndim, laws, nsteps=4):
    """snapshots after each of the steps (read-only: shared by the tests)"""
    R = DamageRef(erosion_case(ndim, laws, Gf=erosion_Gf(ndim, laws)), "erosion")
    out = []
    for t in range(nsteps):
        R.step(DT[t])
        out.append(R.snapshot())
    return out


@functools.lru_cache(maxsize=None)
def softening_ft(ndim, law):
    """the median T0 of the candidates of a reference step 1"""
    R = DamageRef(softening_case(ndim, law, ft=1e300), "softening")
    R.step(DT[0])
    return float(np.median(R.diag["T0"][R.diag["cand"]]))


@functools.lru_cache(maxsize=None)
def softening_reference(ndim, law, nsteps=3):
    R = DamageRef(softening_case(ndim, law, ft=softening_ft(ndim, law)), "softening")
    out = []
    for t in range(nsteps):
        R.step(DT[t])
        out.append(R.snapshot())
    return out
