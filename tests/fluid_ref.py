"""numpy restatement of the compressible Newtonian-fluid law, the checker of the fluid tests.

Written from the reference's lines (nl-partsol/src of migmolper/NL-PartSol @ v1), not from the device code:
  stress ................. Constitutive/Fluid/Newtonian-Fluid.c:17-79
  velocity gradient ...... Particles/compute-Strains.c:249-341 (L = dFdt F^-1)
  stiffness density ...... Constitutive/Fluid/Newtonian-Fluid.c:83-190
  what feeds them ........ Constitutive/Constitutive.c:84-108 (F_n1, dt_F_n1, J_n1) and :298-314 (+ F_n, alpha_4)
  the Jacobian loop ...... Formulations/Displacements/U-Newmark-beta.c:1646-1830
Nothing reference-built pins this law (the committed bridge zeroes Viscosity, Compressibility and n_Macdonald_model), so
the oracle does everything around the law and these functions do the law.

Tensors are the reference's rows: T = 5 in 2-D (xx, xy, yx, yy, zz), 9 in 3-D; the d x d block is the first d*d entries.
A material is a dict with p_ref, viscosity, compressibility, n_macdonald (type 6)."""
import numpy as np

FLUID_TYPE = 6


def block(t, ndim):
    return np.asarray(t, dtype=np.float64)[: ndim * ndim].reshape(ndim, ndim)


def velocity_gradient(F, dFdt):
    """spatial_velocity_gradient__Particles__: L = dFdt F^-1; LinAlgError where dgetrf reports a singular F"""
    return dFdt @ np.linalg.inv(F)


def pressure(mat, J):
    """:35"""
    n, K, p0 = mat["n_macdonald"], mat["compressibility"], mat["p_ref"]
    return J * (p0 + (K / n) * (J ** (-n) - 1.0))


def stress_terms(mat, F, dFdt, J, ndim):
    """The three parts of the stress row, each of length T: the p0 term, the K/n volumetric term, the viscous term."""
    T = 5 if ndim == 2 else 9
    n, K, p0, mu = mat["n_macdonald"], mat["compressibility"], mat["p_ref"], mat["viscosity"]
    L = velocity_gradient(block(F, ndim), block(dFdt, ndim))
    E = 0.5 * (L + L.T)
    Ef = E.ravel()
    trace_E = Ef[0] + Ef[2] if ndim == 2 else Ef[0] + Ef[4] + Ef[8]  # :59 -- in 2-D that is xx + yx, as upstream
    c0 = J * mu
    Id = np.eye(ndim)
    terms = np.zeros((3, T))
    terms[0, : ndim * ndim] = (-J * p0 * Id).ravel()
    terms[1, : ndim * ndim] = (-J * (K / n) * (J ** (-n) - 1.0) * Id).ravel()
    terms[2, : ndim * ndim] = (2.0 * c0 * E - (2.0 / 3.0) * c0 * trace_E * Id).ravel()
    if ndim == 2:  # :74
        terms[0, 4] = -J * p0
        terms[1, 4] = -J * (K / n) * (J ** (-n) - 1.0)
        terms[2, 4] = -(2.0 / 3.0) * c0 * trace_E
    return terms


def stress(mat, F, dFdt, J, ndim):
    """compute_Kirchhoff_Stress_Newtonian_Fluid__Constitutive__ for one particle, :35-75 as written: the stress row [T]"""
    T = 5 if ndim == 2 else 9
    p = pressure(mat, J)
    c0 = J * mat["viscosity"]
    L = velocity_gradient(block(F, ndim), block(dFdt, ndim))
    E = (0.5 * (L + L.T)).ravel()
    Id = np.eye(ndim).ravel()
    trace_E = E[0] + E[2] if ndim == 2 else E[0] + E[4] + E[8]  # :59
    out = np.zeros(T)
    for q in range(ndim * ndim):
        out[q] = -p * Id[q] + 2.0 * c0 * E[q] - (2.0 / 3.0) * c0 * trace_E * Id[q]
    if ndim == 2:
        out[4] = -p - (2.0 / 3.0) * c0 * trace_E  # :74
    return out


def stress_cloud(materials, matidx, F_n1, dt_F_n1, J_n1, ndim, out):
    """The fluid particles' rows of `out` (the oracle's Stress array) overwritten; returns their mask."""
    sel = np.array([materials[m]["type"] == FLUID_TYPE for m in matidx])
    for p in np.nonzero(sel)[0]:
        out[p, :] = stress(materials[matidx[p]], F_n1[p], dt_F_n1[p], J_n1[p], ndim)
    return sel


def stiffness_density(dNa1, dNb1, dNa_n, dNb_n, F_n, F_n1, dFdt, J, alpha4, mat, ndim):
    """compute_stiffness_density_Newtonian_Fluid__Constitutive__ for one pair of nodes, statement by statement
    (:108-187); alpha = the row node, beta = the column node.  d x d."""
    n, K, p0, mu = mat["n_macdonald"], mat["compressibility"], mat["p_ref"], mat["viscosity"]
    p = J * (p0 + (K / n) * (J ** (-n) - 1.0))
    dp = -K * J ** (1.0 - n)
    c0 = J * mu
    c1 = p + dp + (2.0 / 3.0) * alpha4 * c0
    c2 = p + alpha4 * c0
    L = velocity_gradient(block(F_n1, ndim), block(dFdt, ndim))
    E = 0.5 * (L + L.T)
    E_a, E_b = E @ dNa1, E @ dNb1
    Lt_a, Lt_b = L.T @ dNa1, L.T @ dNb1
    b_n = block(F_n, ndim) @ block(F_n, ndim).T
    len0 = dNb_n @ (b_n @ dNa_n)
    S = np.zeros((ndim, ndim))
    for i in range(ndim):
        for j in range(ndim):
            S[i, j] = (-c1 * dNa1[i] * dNb1[j] + c2 * dNa1[j] * dNb1[i] + 2.0 * c0 * E_a[i] * dNb1[j]
                       - 2.0 * c0 * E_b[i] * dNa1[j] + alpha4 * c0 * (i == j) * len0 - c0 * len0 * L[i, j]
                       - c0 * dNb1[i] * Lt_a[j] + (2.0 / 3.0) * c0 * dNa1[i] * Lt_b[j])
    return S


def stiffness_density_all_pairs(dN1, dN, F_n, F_n1, dFdt, J, alpha4, mat, ndim):
    """stiffness_density for every (alpha, beta) of one particle at once, the same eight terms: [nn, nn, d, d].
    (tests/test_fluid_ref.py holds it to the per-pair form above.)"""
    n, K, p0, mu = mat["n_macdonald"], mat["compressibility"], mat["p_ref"], mat["viscosity"]
    p = J * (p0 + (K / n) * (J ** (-n) - 1.0))
    dp = -K * J ** (1.0 - n)
    c0 = J * mu
    c1 = p + dp + (2.0 / 3.0) * alpha4 * c0
    c2 = p + alpha4 * c0
    L = velocity_gradient(block(F_n1, ndim), block(dFdt, ndim))
    E = 0.5 * (L + L.T)
    Ea, Lta = dN1 @ E.T, dN1 @ L            # rows: E dN_A, L^T dN_A
    b_n = block(F_n, ndim) @ block(F_n, ndim).T
    len0 = (dN @ b_n.T) @ dN.T               # [alpha, beta] = (b_n dN_alpha) . dN_beta
    Id = np.eye(ndim)
    nn = dN1.shape[0]
    x, ea, lta = dN1.ravel(), Ea.ravel(), Lta.ravel()   # index (alpha, i) or (beta, j)
    # rows (alpha, i), columns (beta, j): the terms with alpha's factor on i and beta's on j (first, third, eighth of
    # :178-185) and the two that carry lenght_0 (fifth, sixth) ...
    S = np.outer(x, -c1 * x + (2.0 / 3.0) * c0 * lta) + np.outer(2.0 * c0 * ea, x) + np.kron(len0, alpha4 * c0 * Id - c0 * L)
    # ... those with alpha's factor on j and beta's on i (second, fourth, seventh), made as rows (alpha, j), columns (beta, i)
    Sw = np.outer(x, c2 * x - 2.0 * c0 * ea) + np.outer(lta, -c0 * x)
    S = S.reshape(nn, ndim, nn, ndim) + Sw.reshape(nn, ndim, nn, ndim).transpose(0, 3, 2, 1)
    return S.transpose(0, 2, 1, 3)           # [alpha, beta, i, j]


def dense_tangent(o, P, M, n2m, d2m, nactive, pair_blocks, alpha_1=0.0, lumped_mass=None):
    """__jacobian_evaluation, dense, masked numbering: for every particle and every pair (A, B) of its members the block
    V0 x stiffness density at rows (A, i), columns (B, j); alpha_1 M on the diagonal (:1797-1807); Dirichlet dofs become
    identity rows and columns (:1822).  pair_blocks(p, dN_n1, dN_n) -> [nn, nn, d, d], the stiffness densities of particle
    p's pairs, with dN_n from the oracle and dN_n1 = DF^-T dN_n (push_forward_dN__MeshTools__)."""
    ndim = P.ndim
    ntot = nactive * ndim
    K = np.zeros(ntot * ntot)
    idx, val = [], []

    def flush():  # the += of a batch of particles, repeated indices summed
        if idx:
            K[:] += np.bincount(np.concatenate(idx), weights=np.concatenate(val), minlength=ntot * ntot)
            idx.clear()
            val.clear()

    for p in range(P.np):
        dN = o.compute_dN(P, M, p)
        nn = dN.shape[0]
        DF = block(P["DF"][p], ndim)
        dN1 = dN @ np.linalg.inv(DF)          # row A: DF^-T dN_A
        blocks = pair_blocks(p, dN1, dN)
        nodes = n2m[P.lists(p)]
        assert nodes.shape[0] == nn and np.all(nodes >= 0)
        # rows (A, i), columns (B, j) of every pair: K[row, col] += V0 * blocks[A, B, i, j]
        dofs = (nodes[:, None] * ndim + np.arange(ndim)[None, :]).ravel()
        idx.append((dofs[:, None] * ntot + dofs[None, :]).ravel())
        val.append(P["vol0"][p] * blocks.transpose(0, 2, 1, 3).reshape(-1))
        if len(idx) == 16:
            flush()
    flush()
    K = K.reshape(ntot, ntot)
    if lumped_mass is not None:
        K[np.arange(ntot), np.arange(ntot)] += alpha_1 * np.asarray(lumped_mass)
    if d2m is not None:
        fixed = np.nonzero(np.asarray(d2m) == -1)[0]
        K[fixed, :] = 0.0
        K[:, fixed] = 0.0
        K[fixed, fixed] = 1.0
    return K


def neo_hookean_pair_blocks(o, P, mats, ndim):
    """pair_blocks of the oracle's per-pair Neo-Hookean stiffness (orc.stiffness_density_neo_hookean): pins the loop."""
    def f(p, dN1, dN):
        nn = dN.shape[0]
        out = np.zeros((nn, nn, ndim, ndim))
        for A in range(nn):
            for B in range(nn):
                out[A, B] = o.stiffness_density_neo_hookean(dN1[A], dN1[B], dN[A], dN[B], P["F_n"][p][: ndim * ndim],
                                                            P["J_n1"][p], mats[P["matidx"][p]], ndim)
        return out
    return f


def neo_hookean_all_pairs(dN1, dN, F_n, J, mat, ndim):
    """compute_stiffness_density_Neo_Hookean (Hyperelastic/Neo-Hookean.c:89-141) for every pair of one particle at once,
    [nn, nn, d, d]: the Neo-Hookean half of a mixed cloud (tests/test_fluid_ref.py holds it to orc.py's per-pair one)."""
    E, nu = mat["E"], mat["nu"]
    G = E / (2 * (1 + nu))
    lam = nu * E / ((1 - nu * 2) * (1 + nu))
    c0 = lam * J * J
    c1 = G - 0.5 * lam * (J * J - 1)
    nn = dN1.shape[0]
    b_n = block(F_n, ndim) @ block(F_n, ndim).T
    len0 = (dN @ b_n.T) @ dN.T
    x = dN1.ravel()
    S = (c0 * np.outer(x, x) + np.kron(G * len0, np.eye(ndim))).reshape(nn, ndim, nn, ndim)
    S = S + (c1 * np.outer(x, x)).reshape(nn, ndim, nn, ndim).transpose(0, 3, 2, 1)
    return S.transpose(0, 2, 1, 3)


def fluid_pair_blocks(P, materials, alpha4, ndim, solid=None):
    """pair_blocks of the fluid law from the oracle's particle arrays; particles of another law go to `solid`."""
    def f(p, dN1, dN):
        mat = materials[P["matidx"][p]]
        if mat["type"] != FLUID_TYPE:
            return solid(p, dN1, dN)
        return stiffness_density_all_pairs(dN1, dN, P["F_n"][p], P["F_n1"][p], P["dt_F_n1"][p], P["J_n1"][p], alpha4,
                                           mat, ndim)
    return f


class OracleFluid:
    """__lagrangian_evaluation and __jacobian_evaluation of a cloud that holds the fluid law: the oracle does the
    compatibility with rates, the internal, traction and inertial forces, numpy does the stress and the tangent blocks.
    A mixed cloud runs the oracle's constitutive update with the fluid's table entry replaced by a Neo-Hookean one
    (Neo-Hookean touches only Stress and W), then the fluid particles' stress is overwritten."""

    def __init__(self, o, P, M, prm, materials, ndim):
        self.o, self.P, self.M, self.prm, self.materials, self.ndim = o, P, M, prm, materials, ndim
        self.solid = [m for m in materials if m["type"] != FLUID_TYPE]
        stand_in = {"type": 0, "E": 1.0, "nu": 0.25}
        self.mats = o.make_materials([stand_in if m["type"] == FLUID_TYPE else m for m in materials])

    def stress(self):
        P = self.P
        if self.solid:
            assert self.o.constitutive(P, self.mats, self.prm) == 0
        return stress_cloud(self.materials, P["matidx"], P["F_n1"], P["dt_F_n1"], P["J_n1"], self.ndim, P["stress"])

    def residual(self, n2m, d2m, na, dU, Un_dt, Un_dt2, Mv, a, gravity, loads=None, step=0, nsteps=1, thickness=1.0,
                 area0=None):
        """U-Newmark-beta.c:1018-1036, as _oracle_residual of tests/test_gpu_lagrangian.py"""
        o, P, M = self.o, self.P, self.M
        dU_dt = a["a4"] * dU + (a["a5"] - 1) * Un_dt + a["a6"] * Un_dt2
        assert o.compatibility(dU, dU_dt, P, M, n2m) == 0
        self.stress()
        R, st = o.internal_forces(P, M, n2m, d2m, na)
        assert st == 0
        if loads:
            assert o.nodal_traction_forces(R, P, M, n2m, d2m, loads, step, nsteps, thickness, area0) == 0
        free = d2m != -1
        bvec = np.tile(np.asarray(gravity, dtype=np.float64), na)
        R[free] += (Mv * (a["a1"] * dU - a["a2"] * Un_dt - a["a3"] * Un_dt2 - bvec))[free]
        return R

    def tangent(self, n2m, d2m, na, alpha4, alpha_1=0.0, lumped_mass=None):
        o, P = self.o, self.P
        solid = None
        if self.solid:
            assert all(m["type"] == 0 for m in self.solid), "the solid half of a mixed test cloud is Neo-Hookean"
            solid = lambda p, dN1, dN: neo_hookean_all_pairs(dN1, dN, P["F_n"][p], P["J_n1"][p],  # noqa: E731
                                                             self.materials[P["matidx"][p]], self.ndim)
        return dense_tangent(o, P, self.M, n2m, d2m, na, fluid_pair_blocks(P, self.materials, alpha4, self.ndim, solid),
                             alpha_1, lumped_mass)
