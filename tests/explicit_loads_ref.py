"""The explicit step with Neumann contours (nlps_gpu_set_explicit_loads), as a composition of the oracle's
stage calls in orc_explicit_step's order: search, active nodes and dofs, lumped mass, shape functions, compatibility, the
constitutive update, the internal forces and the contour tractions are the oracle's; the predictor, the projection of dU
with its Dirichlet sets, the nodal equilibrium with gravity and reactions, the G2P and the corrector are restated here in
numpy.  The one term orc_explicit_step does not have: orc.nodal_traction_forces accumulated into a zero vector with every
dof free, R -= N T A0, so force = -f_int - R (compute_Nodal_Nominal_traction_Forces, U-Verlet.c:805-902, called at :695).
tests/test_explicit_loads_ref.py shows that without loads the composition is orc.ExplicitStepper to rounding, and checks
the margins of the scenarios below."""
import functools

import numpy as np

import explicit_damage_ref as xr
from util import dirichlet_plane, oracle_setup, orc

NSTEPS = 4
DT = xr.DT
GAMMA = xr.GAMMA
THICKNESS = 0.5
TB = {2: 16, 3: 4}  # closest nodes per tile and axis (TileCfg)


def loaded_case(ndim, laws=0):
    """the multi-tile clouds of the erosion scenario (Neo-Hookean by default, a velocity field that moves particles
    across cells) without the driver"""
    return xr.erosion_case(ndim, laws)


def gravity(ndim):
    return np.array([0.0, -9.81] if ndim == 2 else [0.0, 0.0, -9.81])


def area0(case):
    """Phi.Area_0 of every particle (3-D), caller's order"""
    n = case["cloud"]["x"].shape[0]
    return np.random.default_rng(5).uniform(0.2, 0.3, size=n) if case["ndim"] == 3 else None


def outer_layer(x, axis, upper, count, seed):
    """`count` particles of the cloud's outermost layer along `axis`, spread over the whole layer"""
    c = x[:, axis]
    layer = np.where(c > c.max() - 0.25 if upper else c < c.min() + 0.25)[0]
    pick = np.random.default_rng(seed).permutation(layer.size)[:count]
    return np.sort(layer[pick]).astype(np.int32)


def contours(case, nsteps=NSTEPS, scale=1.0, all_off=False):
    """Two contours of 20 particles from two outer layers of the cloud, each across a tile boundary.  The values differ per
    step and direction; the second contour has direction 0 switched off at step 2, where it carries the first one's."""
    nd, x = case["ndim"], case["cloud"]["x"]
    rng = np.random.default_rng(91)
    if nd == 2:
        sets = [outer_layer(x, 1, True, 20, 1), outer_layer(x, 1, False, 20, 2)]  # top and bottom rows, across node 16 in x
    else:
        sets = [outer_layer(x, 0, True, 20, 1), outer_layer(x, 2, True, 20, 2)]  # the +x and the +z face
    out = []
    for k, ids in enumerate(sets):
        value = scale * rng.uniform(2.0e4, 8.0e4, size=(nd, nsteps)) * rng.choice([-1.0, 1.0], size=(nd, nsteps))
        d = np.ones((nd, nsteps), dtype=np.int32)
        if k == 1 and nsteps > 2:
            d[0, 2] = 0
        if all_off:
            d[:] = 0
        out.append({"nodes": ids, "dim": nd, "dir": d, "value": value})
    return out


def dirichlet(case, nsteps=NSTEPS):
    """the node plane under the cloud, every direction held: in the stencils of the lowest particles of the contours
    (2-D: the bottom row is the second contour; 3-D: the +x face reaches down to it)"""
    nd = case["ndim"]
    return [dirichlet_plane(case, nd - 1, 3 if nd == 2 else 2, nsteps)]


def lattice_index(nodes, grid_n, nd):
    """(i, j[, k]) of lattice nodes (x fastest)"""
    nodes = np.asarray(nodes)
    ijk = [nodes % grid_n[0], (nodes // grid_n[0]) % grid_n[1], nodes // (grid_n[0] * grid_n[1])]
    return np.stack(ijk[:nd], axis=1)


def carried_tractions(loads, step, nd):
    """the traction vector every contour applies at `step` (zero at the start of the step, U-Verlet.c:865-869)"""
    T, out = np.zeros(nd), []
    for l in loads:
        on = np.asarray(l["dir"])[:, step] == 1
        T = np.where(on, np.asarray(l["value"])[:, step], T)
        out.append(T.copy())
    return out


def total_traction(case, loads, step, thickness=THICKNESS, a0=None):
    """sum T A0 over the contour entries: what the nodal force sums to (partition of unity; the internal forces sum to 0)"""
    nd, vol0 = case["ndim"], case["cloud"]["vol0"]
    tot = np.zeros(nd)
    for l, T in zip(loads, carried_tractions(loads, step, nd)):
        A = vol0[l["nodes"]] / thickness if nd == 2 else a0[l["nodes"]]
        tot += T * A.sum()
    return tot


class LoadsRef:
    def __init__(self, case, bcs=(), loads=(), nsteps=NSTEPS, gravity=None, thickness=THICKNESS, area0=None):
        self.o = orc()
        self.case, self.bcs, self.loads, self.nsteps = case, list(bcs), list(loads), nsteps
        self.gravity, self.thickness, self.area0 = gravity, thickness, area0
        self.M, self.P, self.prm, self.mats = oracle_setup(case)
        self.bset = self.o.BccSet(self.bcs)
        self.nodal, self.n2m, self.na = {}, None, 0
        self.min_J = np.inf

    def step(self, t, dt, gamma=GAMMA):
        o = self.o
        threads = o.num_threads()
        o.set_num_threads(1)
        try:
            self._step(t, dt, gamma)
        finally:
            o.set_num_threads(threads)

    def _step(self, t, dt, gamma):
        o, P, M, prm, mats = self.o, self.P, self.M, self.prm, self.mats
        nd, n = P.ndim, P.np
        assert o.local_search(P, M, prm) == 0
        n2m, na = o.active_nodes(M)
        d2m, _ = o.active_dofs(n2m, na, nd, self.bset, t, self.nsteps)
        mass = o.lumped_mass(P, M, n2m, na)
        # predictor
        P["d_dis"][:] = dt * P["vel"] + (0.5 * (dt * dt)) * P["acc"]
        P["vel"][:] += ((1 - gamma) * dt) * P["acc"]
        # nodal dU and its Dirichlet values
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
        for b in self.bcs:
            d, v = np.asarray(b["dir"]), np.asarray(b["value"])
            for A in b["nodes"]:
                m = n2m[A]
                if m == -1:
                    continue
                for k in range(b["dim"]):
                    if d[k, t] == 1:
                        dU[m * nd + k] = v[k, t]
        # local state
        assert o.compatibility(dU, None, P, M, n2m) == 0
        self.min_J = min(self.min_J, float(P["J_n1"].min()))
        assert (P["J_n1"] > 0.0).all()
        DF = P["DF"]
        if nd == 2:
            detDF = DF[:, 0] * DF[:, 3] - DF[:, 1] * DF[:, 2]
        else:
            detDF = (DF[:, 0] * DF[:, 4] * DF[:, 8] - DF[:, 0] * DF[:, 5] * DF[:, 7] + DF[:, 1] * DF[:, 5] * DF[:, 6] -
                     DF[:, 1] * DF[:, 3] * DF[:, 8] + DF[:, 2] * DF[:, 3] * DF[:, 7] - DF[:, 2] * DF[:, 4] * DF[:, 6])
        P["rho"][:] = P["rho"] / detDF
        assert o.constitutive(P, mats, prm) == 0
        # nodal forces: -f_int and the contour tractions, on every dof
        free = np.zeros(na * nd, dtype=np.int32)
        fint, st = o.internal_forces(P, M, n2m, free, na)
        assert st == 0
        force = -fint
        if self.loads:
            R = np.zeros(na * nd)
            assert o.nodal_traction_forces(R, P, M, n2m, free, self.loads, t, self.nsteps, self.thickness, self.area0) == 0
            force = force - R
        # equilibrium: a = g + F / M on the free dofs, reactions on the fixed ones
        g = np.tile(np.zeros(nd) if self.gravity is None else np.asarray(self.gravity, dtype=np.float64), na)
        fixed = d2m == -1
        with np.errstate(divide="ignore", invalid="ignore"):
            accel = np.where((mass != 0.0) & ~fixed, g + force / mass, 0.0)
        reaction = np.where(fixed, force, 0.0)
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
        self.n2m, self.na, self.d2m = n2m, na, d2m
        self.nodal = {"mass": mass, "dU": dU, "force": force, "accel": accel, "reaction": reaction}

    FIELDS = ("x", "dis", "vel", "acc", "F_n", "J_n", "rho", "stress")

    def snapshot(self):
        s = {k: self.P[k].copy() for k in self.FIELDS}
        s.update(I0=self.P["I0"].copy(), na=self.na, n2m=self.n2m.copy(), d2m=self.d2m.copy(), nodal={k: v.copy() for k, v in self.nodal.items()})
        return s


@functools.lru_cache(maxsize=None)
def reference(ndim, laws=0, loaded=True, with_bcs=True, nsteps=NSTEPS):
    """snapshots after each of the steps (read-only: shared by the tests)"""
    case = loaded_case(ndim, laws)
    R = LoadsRef(case, dirichlet(case) if with_bcs else (), contours(case) if loaded else (), NSTEPS, gravity(ndim), THICKNESS,
                 area0(case))
    out = []
    for t in range(nsteps):
        R.step(t, DT[t])
        out.append(R.snapshot())
    return out
