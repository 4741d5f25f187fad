"""The explicit step of a cloud that holds the compressible Newtonian fluid (nlps_gpu_set_explicit_fluid), as
a composition of the oracle's stage calls in orc_explicit_step's order (stage order of U-Verlet.c).  Search, active nodes
and dofs, lumped mass, shape functions, compatibility WITH the rate tensors, the constitutive update of the solid laws,
the internal forces and the contour tractions are the oracle's; the fluid stress is tests/fluid_ref.py's; the predictor,
the projection of dU with its Dirichlet sets, the nodal equilibrium with gravity and reactions, the G2P and the corrector
are restated here in numpy, as tests/explicit_loads_ref.py restates them.

The definition: the nodal rate vector is the increment's mean rate over the step, dV_A = dU_A / dt, and the rate carried
over from the last step is zero.  So dt_F_n is zeroed in front of o.compatibility(dU, dU / dt, ..), and the oracle's own
formulas (compute-Strains.c:48-72, 176-207) give dt_DF = (DF - I) / dt and dt_F_n1 = dt_DF F_n = (F_n1 - F_n) / dt.
`carried=True` keeps the term DF dt_F_n of the Newmark path in, to show what dropping it avoids
(tests/test_explicit_fluid_ref.py); nothing else uses it.

tests/test_explicit_fluid_ref.py holds the numpy part to orc.ExplicitStepper on a Neo-Hookean cloud."""
import functools

import numpy as np

import explicit_damage_ref as xr
import fluid_ref
from util import dirichlet_plane, make_case, oracle_setup, orc

NSTEPS = 4
DT = 1e-4
GAMMA = 0.5
# tests/test_gpu_fluid.py's materials (restated: that module needs a GPU build to import)
FLUID = {"type": 6, "E": 0.0, "nu": 0.0, "p_ref": 1.0e3, "viscosity": 40.0, "compressibility": 2.0e5, "n_macdonald": 7.0}
SOFT_NH = {"type": 0, "E": 2.0e5, "nu": 0.3}
LO = {2: [6, 3], 3: [3, 3, 2]}  # the first cell of the cloud per axis


def gravity(ndim):
    return np.array([0.0, -9.81] if ndim == 2 else [0.0, -9.81, 0.0])


def fluid_case(ndim, materials=(FLUID,), layout=None):
    """the multi-tile clouds of explicit_damage_ref.erosion_case with its velocity field; several materials are dealt to
    the particles in turn ("interleaved") or by layers along the last axis ("layers"), as tests/test_gpu_fluid.py does"""
    materials = list(materials)
    if ndim == 3:
        case = make_case(3, [11, 10, 9], LO[3], [5, 4, 4], material=materials[0])  # 640 particles, 3 x 3 x 3 tiles
    else:
        case = make_case(2, [22, 12], LO[2], [12, 6], material=materials[0])  # 288 particles across the tile boundary at node 16
    cloud = case["cloud"]
    npart = cloud["x"].shape[0]
    cloud["vel"] = xr.velocity_field(cloud["x"])
    case["materials"] = materials
    if layout == "interleaved":
        cloud["matidx"] = (np.arange(npart) % len(materials)).astype(np.int32)
    elif layout == "layers":
        z = cloud["x"][:, ndim - 1]
        cloud["matidx"] = np.minimum(len(materials) - 1,
                                     ((z - z.min()) / (z.max() - z.min() + 1e-9) * len(materials)).astype(np.int32))
    return case


def dirichlet(case, nsteps=NSTEPS):
    """the node layer under the cloud (along y, the axis of gravity), its normal direction held at 0"""
    nd = case["ndim"]
    dirs = np.zeros((nd, nsteps), dtype=np.int32)
    dirs[1, :] = 1
    return [dirichlet_plane(case, 1, LO[nd][1], nsteps, dims=dirs)]


def face_contour(case, nsteps=NSTEPS):
    """one face of the cloud as a Neumann contour: every particle of the outermost +x layer, a traction per step"""
    nd, x = case["ndim"], case["cloud"]["x"]
    ids = np.where(x[:, 0] > x[:, 0].max() - 0.25)[0].astype(np.int32)
    rng = np.random.default_rng(17)
    value = rng.uniform(2.0e3, 8.0e3, size=(nd, nsteps)) * rng.choice([-1.0, 1.0], size=(nd, nsteps))
    return [{"nodes": ids, "dim": nd, "dir": np.ones((nd, nsteps), dtype=np.int32), "value": value}]


def area0(case):
    n = case["cloud"]["x"].shape[0]
    return np.random.default_rng(5).uniform(0.2, 0.3, size=n) if case["ndim"] == 3 else None


def det_block(t, nd):
    if nd == 2:
        return t[:, 0] * t[:, 3] - t[:, 1] * t[:, 2]
    return (t[:, 0] * t[:, 4] * t[:, 8] - t[:, 0] * t[:, 5] * t[:, 7] + t[:, 1] * t[:, 5] * t[:, 6] -
            t[:, 1] * t[:, 3] * t[:, 8] + t[:, 2] * t[:, 3] * t[:, 7] - t[:, 2] * t[:, 4] * t[:, 6])


class FluidStepRef:
    def __init__(self, case, bcs=(), loads=(), nsteps=NSTEPS, gravity=None, thickness=1.0, area0=None, carried=False):
        self.o = orc()
        self.case, self.bcs, self.loads, self.nsteps = case, list(bcs), list(loads), nsteps
        self.gravity, self.thickness, self.area0, self.carried = gravity, thickness, area0, carried
        self.materials = case["materials"]
        self.M, self.P, self.prm, _ = oracle_setup(case)
        self.F = fluid_ref.OracleFluid(self.o, self.P, self.M, self.prm, self.materials, case["ndim"])
        self.fluid = np.array([self.materials[m]["type"] == fluid_ref.FLUID_TYPE for m in self.P["matidx"]])
        self.bset = self.o.BccSet(self.bcs)
        self.nodal, self.n2m, self.na = {}, None, 0

    def step(self, t, dt, gamma=GAMMA):
        o = self.o
        threads = o.num_threads()
        o.set_num_threads(1)
        try:
            self._step(t, dt, gamma)
        finally:
            o.set_num_threads(threads)

    def _step(self, t, dt, gamma):
        o, P, M, prm = self.o, self.P, self.M, self.prm
        nd, n = P.ndim, P.np
        # 1. search, active nodes and dofs, lumped mass, predictor, nodal dU with its Dirichlet values
        assert o.local_search(P, M, prm) == 0
        n2m, na = o.active_nodes(M)
        d2m, _ = o.active_dofs(n2m, na, nd, self.bset, t, self.nsteps)
        mass = o.lumped_mass(P, M, n2m, na)
        P["d_dis"][:] = dt * P["vel"] + (0.5 * (dt * dt)) * P["acc"]
        P["vel"][:] += ((1 - gamma) * dt) * P["acc"]
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
        # 2. the local state with the rate tensors of the definition: dV = dU / dt, nothing carried
        if not self.carried:
            P["dt_F_n"][:] = 0.0
        assert o.compatibility(dU, dU / dt, P, M, n2m) == 0
        assert (P["J_n1"] > 0.0).all()
        # 3. the density
        P["rho"][:] = P["rho"] / det_block(P["DF"], nd)
        # 4. the constitutive update: the oracle's for the solids, fluid_ref's over the fluid rows
        self.F.stress()
        # 5. nodal forces (-f_int and the contour tractions, on every dof), equilibrium, reactions, G2P, corrector
        free = np.zeros(na * nd, dtype=np.int32)
        fint, st = o.internal_forces(P, M, n2m, free, na)
        assert st == 0
        force = -fint
        if self.loads:
            R = np.zeros(na * nd)
            assert o.nodal_traction_forces(R, P, M, n2m, free, self.loads, t, self.nsteps, self.thickness, self.area0) == 0
            force = force - R
        g = np.tile(np.zeros(nd) if self.gravity is None else np.asarray(self.gravity, dtype=np.float64), na)
        fixed = d2m == -1
        with np.errstate(divide="ignore", invalid="ignore"):
            accel = np.where((mass != 0.0) & ~fixed, g + force / mass, 0.0)
        reaction = np.where(fixed, force, 0.0)
        a2, u2 = accel.reshape(na, nd), dU.reshape(na, nd)
        for p in range(n):
            N, r = shape[p][:, None], rows[p]
            P["acc"][p] = np.cumsum(N * a2[r], axis=0)[-1]
            P["d_dis"][p] = np.cumsum(N * u2[r], axis=0)[-1]
        P["vel"][:] += (gamma * dt) * P["acc"]
        P["x"][:] += P["d_dis"]
        P["dis"][:] += P["d_dis"]
        # 6. the roll, dt_F_n <- dt_F_n1 included
        self.F_before = P["F_n"].copy()
        P["J_n"][:] = P["J_n1"]
        P["kappa_n"][:] = P["kappa_n1"]
        P["eps_n"][:] = P["eps_n1"]
        P["b_e_n"][:] = P["b_e_n1"]
        P["F_n"][:] = P["F_n1"]
        P["dt_F_n"][:] = P["dt_F_n1"]
        self.n2m, self.na, self.d2m = n2m, na, d2m
        self.nodal = {"mass": mass, "dU": dU, "force": force, "accel": accel, "reaction": reaction}

    FIELDS = ("x", "dis", "vel", "acc", "F_n", "J_n", "rho", "stress")
    RATES = ("dt_F_n", "dt_F_n1")

    def snapshot(self):
        s = {k: self.P[k].copy() for k in self.FIELDS + self.RATES + ("DF", "dt_DF", "W")}
        s.update(na=self.na, fluid=self.fluid.copy(), F_before=self.F_before.copy(),
                 nodal={k: v.copy() for k, v in self.nodal.items()})
        return s


@functools.lru_cache(maxsize=None)
def reference(ndim, materials=(0,), layout=None, loaded=False, nsteps=NSTEPS):
    """snapshots after each of the steps (read-only: shared by the tests).  materials: indices into (FLUID, SOFT_NH)"""
    case = fluid_case(ndim, [(FLUID, SOFT_NH)[m] for m in materials], layout)
    R = FluidStepRef(case, dirichlet(case), face_contour(case) if loaded else (), NSTEPS, gravity(ndim), 1.0, area0(case))
    out = []
    for t in range(nsteps):
        R.step(t, DT)
        out.append(R.snapshot())
    return out
