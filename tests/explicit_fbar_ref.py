"""The explicit step with F-bar on lattice-cell patches (nlps_gpu_set_explicit_fbar): the composition of the
oracle's stage calls of tests/explicit_fluid_ref.py (FluidStepRef) with ONE insertion between the compatibility and the
constitutive update, as include/nlps_gpu.h defines it:

  patch of a particle   c_k = clamp(floor((x_k - origin_k) / h), 0, n_k - 2), patch = c_k // block[k], x in front of the step
  patch sums            Vn = sum J_n Vol_0, Vn1 = sum J_n1 Vol_0 over ALL particles of the patch, J_patch = Vn1 / Vn
  per particle          c = (J_patch / det DF)^(1/ndim), Fbar_n1 = alpha F_n1 + (1 - alpha) c DF Fbar_n (2-D: the in-plane
                        block, zz of F_n1), Jbar_n1 = Jbar_n J_patch; a material with alpha < 0 forms them with alpha = 0
  the law               F_n1 / J_n1 of the rows whose material has alpha >= 0 are swapped for the barred values around the
                        stress call and restored in front of internal_forces; the fluid's rate dt_F_n1 stays unbarred
  the roll              Fbar_n <- Fbar_n1, Jbar_n <- Jbar_n1

tests/test_explicit_fbar_ref.py holds this file to orc.ExplicitStepper and to the definition on the CPU."""
import functools

import numpy as np

import explicit_damage_ref as xr
import explicit_fluid_ref as xf
from util import DP, dirichlet_plane, make_case

NSTEPS = 4
DT = xf.DT
GAMMA = xf.GAMMA
NH49 = {"type": 0, "E": 2.0e5, "nu": 0.49}  # near-incompressible: lambda / mu = 49
FLUID, SOFT_NH = xf.FLUID, xf.SOFT_NH
SOFT_HENCKY = {"type": 1, "E": 2.0e5, "nu": 0.3}
MATS = (NH49, FLUID, SOFT_NH, SOFT_HENCKY, DP)
# clouds around node 16 of every axis: with block 3 the cells 15 - 17 form one patch across the seam between tiles (a 2-D
# tile is 16 x 16 nodes, a 3-D tile 4 x 4 x 4: node 16 starts a tile in both)
CLOUD = {2: dict(cells=[22, 20], lo=[12, 12], blk=[7, 6]),    # tests/test_gpu_tiles_2d.py's corner: 168 particles, cells 12 - 18 x 12 - 17
         3: dict(cells=[20, 20, 20], lo=[14, 14, 14], blk=[4, 4, 4])}  # 512 particles, cells 14 - 17 per axis


def fbar_case(ndim, materials=(0,), layout=None):
    """materials: indices into MATS; several are dealt in turn ("interleaved") or by halves along x ("tiles": the seam at
    node 16 separates them, one law per tile)"""
    c = CLOUD[ndim]
    mats = [MATS[m] for m in materials]
    case = make_case(ndim, c["cells"], c["lo"], c["blk"], material=mats[0])
    cloud = case["cloud"]
    n = cloud["x"].shape[0]
    cloud["vel"] = xr.velocity_field(cloud["x"])
    case["materials"] = mats
    if layout == "interleaved":
        cloud["matidx"] = (np.arange(n) % len(mats)).astype(np.int32)
    elif layout == "tiles":
        cloud["matidx"] = np.where(cloud["x"][:, 0] < 16.0, 0, len(mats) - 1).astype(np.int32)
    for i, m in enumerate(mats):  # Kappa_n = kappa_0 at start, as util.make_case does for a cloud of one such material
        if m["type"] == 2:
            cloud["kappa_n"][cloud["matidx"] == i] = m["kappa_0"]
    return case


def dirichlet(case, nsteps=NSTEPS):
    """the node layer under the cloud (along y, the axis of gravity), its normal direction held at 0"""
    nd = case["ndim"]
    dirs = np.zeros((nd, nsteps), dtype=np.int32)
    dirs[1, :] = 1
    return [dirichlet_plane(case, 1, CLOUD[nd]["lo"][1], nsteps, dims=dirs)]


def patch_of(x, origin, h, grid_n, block):
    """[np] patch number of every particle and the number of patches (the header's definition)"""
    nd = x.shape[1]
    block = [int(block)] * nd if np.isscalar(block) else list(block)[:nd]
    pid, mul, cells = np.zeros(x.shape[0], dtype=np.int64), 1, []
    for k in range(nd):
        c = np.clip(np.floor((x[:, k] - origin[k]) / h).astype(np.int64), 0, grid_n[k] - 2)
        cells.append(c)
        npk = (max(1, grid_n[k] - 1) + block[k] - 1) // block[k]
        pid += mul * (c // block[k])
        mul *= npk
    return pid, mul, np.stack(cells, axis=1)


def fbar_update(nd, pid, npatch, vol0, J_n, J_n1, DF, F_n1, Fbar_n, Jbar_n, alpha_p):
    """the insertion: (Fbar_n1, Jbar_n1, J_patch per particle, Vn, Vn1)"""
    Vn = np.bincount(pid, weights=J_n * vol0, minlength=npatch)
    Vn1 = np.bincount(pid, weights=J_n1 * vol0, minlength=npatch)
    Jp = Vn1[pid] / Vn[pid]
    q = Jp / xf.det_block(DF, nd)
    c = np.sqrt(q) if nd == 2 else np.cbrt(q)
    n = F_n1.shape[0]
    B = lambda a: a[:, : nd * nd].reshape(n, nd, nd)  # noqa: E731
    a = np.maximum(alpha_p, 0.0)[:, None, None]
    bar = a * B(F_n1) + (1.0 - a) * c[:, None, None] * np.einsum("pik,pkj->pij", B(DF), B(Fbar_n))
    Fbar_n1 = F_n1.copy()  # (2-D: the zz entry is F_n1's)
    Fbar_n1[:, : nd * nd] = bar.reshape(n, nd * nd)
    return Fbar_n1, Jbar_n * Jp, Jp, Vn, Vn1, c


class FbarStepRef(xf.FluidStepRef):
    """alpha: one entry per material (< 0: the material does not read F-bar); noop: the insertion is made and nothing is
    swapped (what every alpha < 0 would mean, which the setter refuses)"""

    def __init__(self, case, alpha, block=1, bcs=(), loads=(), nsteps=NSTEPS, gravity=None, thickness=1.0, area0=None,
                 Fbar_n=None, Jbar_n=None):
        super().__init__(case, bcs, loads, nsteps, gravity, thickness, area0)
        P = self.P
        self.alpha = np.asarray(alpha, dtype=np.float64)
        self.alpha_p = self.alpha[P["matidx"]]
        self.block = block
        self.Fbar_n = P["F_n"].copy() if Fbar_n is None else np.array(Fbar_n, dtype=np.float64)
        self.Jbar_n = P["J_n"].copy() if Jbar_n is None else np.array(Jbar_n, dtype=np.float64)
        self.last = {}
        inner = self.F.stress

        def stress():
            nd = P.ndim
            pid, npatch, cells = patch_of(P["x"], case["origin"], case["h"], case["grid_n"], self.block)
            F1, J1, Jp, Vn, Vn1, c = fbar_update(nd, pid, npatch, P["vol0"], P["J_n"], P["J_n1"], P["DF"], P["F_n1"],
                                                 self.Fbar_n, self.Jbar_n, self.alpha_p)
            self.Fbar_n1, self.Jbar_n1 = F1, J1
            self.last = dict(pid=pid, cells=cells, x=P["x"].copy(), Jp=Jp, Vn=Vn, Vn1=Vn1, c=c, DF=P["DF"].copy(),
                             J_n=P["J_n"].copy(), J_n1=P["J_n1"].copy(), vol0=P["vol0"].copy())
            rows = self.alpha_p >= 0.0
            keepF, keepJ = P["F_n1"].copy(), P["J_n1"].copy()
            P["F_n1"][rows] = F1[rows]
            P["J_n1"][rows] = J1[rows]
            try:
                return inner()
            finally:
                P["F_n1"][:] = keepF
                P["J_n1"][:] = keepJ
        self.F.stress = stress

    def _step(self, t, dt, gamma):
        super()._step(t, dt, gamma)
        self.Fbar_n, self.Jbar_n = self.Fbar_n1, self.Jbar_n1  # the roll, extended

    def snapshot(self):
        s = super().snapshot()
        s.update(Fbar_n=self.Fbar_n.copy(), Jbar_n=self.Jbar_n.copy(), last={k: v.copy() for k, v in self.last.items()})
        s.update({k: self.P[k].copy() for k in ("kappa_n", "eps_n", "b_e_n")})  # (the plastic laws' internal variables)
        s.update({k: self.P[k].copy() for k in ("lambda", "beta", "I0")})  # (what a restart hands to the search)
        return s


def gravity(ndim):
    return xf.gravity(ndim)


@functools.lru_cache(maxsize=None)
def reference(ndim, materials=(0,), alpha=(0.0,), block=1, layout=None, loaded=False, nsteps=NSTEPS):
    """snapshots after each of the steps (read-only: shared by the tests); alpha None: the plain step of the same cloud"""
    case = fbar_case(ndim, materials, layout)
    loads = xf.face_contour(case) if loaded else ()
    if alpha is None:
        R = xf.FluidStepRef(case, dirichlet(case), loads, NSTEPS, gravity(ndim), 1.0, xf.area0(case))
    else:
        R = FbarStepRef(case, alpha, block, dirichlet(case), loads, NSTEPS, gravity(ndim), 1.0, xf.area0(case))
    out = []
    for t in range(nsteps):
        R.step(t, DT)
        out.append(R.snapshot())
    return out
