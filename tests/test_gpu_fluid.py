"""The compressible Newtonian-fluid law (NLPS_MAT_NEWTONIAN_FLUID, Constitutive/Fluid/Newtonian-Fluid.c) on the implicit
path: level-B stages, the fused residual with the rate tensors in registers, mixed clouds, both tangents, the Newton solve,
the one-call Newmark step, the explicit step's refusal and the failure path.  The checker is tests/fluid_ref.py (numpy, from
the reference's lines) with the oracle doing everything around the law."""
import numpy as np
import pytest

import fluid_ref
import snes_ref
from newmark import newmark_parameters
from test_gpu_lagrangian import _moved_case
from test_gpu_tangent_operator import _check_apply, _check_blocks, _coo_dense
from util import assert_close, dirichlet_plane, gpu_setup, nlps, orc

pytestmark = pytest.mark.gpu

TOL = 1e-10      # states and residuals (tests/test_gpu_lagrangian.py)
TOL_K = 1e-9     # the tangent
# p0 = 1 kPa against K (J - 1) ~ 2e5 x 1e-3 and 2 mu sym(L) ~ 80 x O(1): each of the three stress terms is at least 1 % of the
# stress norm on the test clouds (asserted by _three_terms)
FLUID = {"type": 6, "E": 0.0, "nu": 0.0, "p_ref": 1.0e3, "viscosity": 40.0, "compressibility": 2.0e5, "n_macdonald": 7.0}
SOFT_NH = {"type": 0, "E": 2.0e5, "nu": 0.3}
# fnorm_history against the numpy Newton, entries at or above 1e-7 fnorm0: ten times the largest relative difference measured
# on the MI355X over the cases of test_newton_solve
HISTORY_TOL = 1.2e-10
RATES = (("dt_DF", "dt_DF"), ("dt_F_n1", "dt_F_n1"))
STATE = (("DF", "DF"), ("F_n1", "F_n1"), ("J_n1", "J_n1"), ("Stress", "stress")) + RATES


class _Case:
    """A moved cloud (tests/test_gpu_lagrangian.py::_moved_case) with the fluid law, searched and masked on both sides."""

    def __init__(self, ndim, materials=None, layout=None, nsteps=3, step=1, seed=11, dt=2.0e-3, twin=False):
        self.o, self.n, self.ndim, self.nsteps, self.step = orc(), nlps(), ndim, nsteps, step
        o = self.o
        self.rng = rng = np.random.default_rng(seed)
        materials = [FLUID] if materials is None else materials
        case, self.M, P, self.prm, _ = _moved_case(ndim, FLUID, nsteps, rng)
        cloud = case["cloud"]
        npart = cloud["x"].shape[0]
        cloud["dt_F_n"] = 0.1 * rng.normal(size=P["F_n"].shape)   # a rate history: dt_F_n1 = dt_DF F_n + DF dt_F_n
        if ndim == 2:
            cloud["dt_F_n"][:, 4] = 0.0
        case["materials"] = materials
        if layout == "interleaved":
            cloud["matidx"] = (np.arange(npart) % len(materials)).astype(np.int32)
        elif layout == "layers":
            z = cloud["x"][:, ndim - 1]
            cloud["matidx"] = np.minimum(len(materials) - 1, ((z - z.min()) / (z.max() - z.min() + 1e-9) * len(materials))
                                         .astype(np.int32))
        self.case, self.materials = case, materials
        self.P = o.OracleParticles(cloud)
        self.F = fluid_ref.OracleFluid(o, self.P, self.M, self.prm, materials, ndim)
        self.bcs_list = [dirichlet_plane(case, ndim - 1, 3, nsteps)]
        self.bcs = self.n.BccSet(self.bcs_list)
        self.S = gpu_setup(case, init=False, nsteps=nsteps)
        self.S2 = gpu_setup(case, init=False, nsteps=nsteps) if twin else None
        self.a = newmark_parameters(0.25, 0.5, dt)
        self.alpha = [self.a[k] for k in ("a1", "a2", "a3", "a4", "a5", "a6")]
        self.grav = [0.0] * (ndim - 1) + [-9.81]
        self.begin_step(step)

    def begin_step(self, step):
        o, S = self.o, self.S
        self.step = step
        assert o.local_search(self.P, self.M, self.prm) == 0
        S.local_search()
        self.n2m, self.na = o.active_nodes(self.M)
        self.d2m, _ = o.active_dofs(self.n2m, self.na, self.ndim, o.BccSet(self.bcs_list), step, self.nsteps)
        n2m, d2m = S.active_masks(self.bcs, step)
        assert np.array_equal(n2m, self.n2m) and np.array_equal(d2m, self.d2m)
        self.Mv = o.lumped_mass(self.P, self.M, self.n2m, self.na)
        self.V, self.A = o.nodal_field_n(self.Mv, self.P, self.M, self.n2m, self.d2m, self.na)
        self.ntot = self.na * self.ndim

    def velocity_increment(self, dU):  # __compute_nodal_velocity_increments, U-Newmark-beta.c:1834-1870
        return self.a["a4"] * dU + (self.a["a5"] - 1) * self.V + self.a["a6"] * self.A

    def residual_ref(self, dU):
        return self.F.residual(self.n2m, self.d2m, self.na, np.asarray(dU), self.V, self.A, self.Mv, self.a, self.grav)

    def tangent_ref(self, alpha4=None, alpha_1=None, dirichlet=True):
        return self.F.tangent(self.n2m, self.d2m if dirichlet else None, self.na, self.a["a4"] if alpha4 is None else alpha4,
                              self.a["a1"] if alpha_1 is None else alpha_1, self.Mv)

    def residual_gpu(self, dU, flags=0, S=None):
        return (S or self.S).lagrangian_evaluation(np.ascontiguousarray(dU), self.V, self.A, self.Mv, self.alpha, self.grav,
                                                   flags=flags)

    def advance(self, dU, gpu=True, ref=True):
        """the roll and the particle update, on both sides"""
        dV = self.velocity_increment(dU)
        dA = self.a["a1"] * dU - self.a["a2"] * self.V - (self.a["a3"] + 1) * self.A
        if ref:
            self.o.roll_state(self.P)
            self.o.update_kinetics(1.0, dU, self.V, dV, dA, self.P, self.M, self.n2m)
        if gpu:
            self.S.update_particles_internal_variables()
            self.S.update_particles_kinetics_FLIP_PIC(1.0, dU, self.V, dV, dA)

    def compare_state(self, what, tol=TOL, S=None):
        st = (S or self.S).download_state()
        for k, ok in STATE:
            assert_close(st[k], self.P[ok], tol, f"{what}: {k}")
        assert np.array_equal(st["W"], np.zeros(self.P.np)) or len(self.materials) > 1, "the fluid law writes no W"
        return st

    def close(self):
        self.S.close()
        if self.S2:
            self.S2.close()


def _three_terms(c):
    """Each of the p0 term, the K/n volumetric term and the viscous term is at least 1 % of the fluid's stress norm."""
    P = c.P
    fl = np.array([c.materials[m]["type"] == 6 for m in P["matidx"]])
    t = np.array([fluid_ref.stress_terms(c.materials[P["matidx"][p]], P["F_n1"][p], P["dt_F_n1"][p], P["J_n1"][p], c.ndim)
                  for p in np.nonzero(fl)[0]])
    total = np.linalg.norm(P["stress"][fl])
    shares = [np.linalg.norm(t[:, k]) / total for k in range(3)]
    print("stress term shares (p0, K/n, viscous):", shares)
    assert min(shares) >= 0.01, shares


@pytest.mark.parametrize("ndim", [2, 3])
def test_level_b_stages(ndim):
    """nlps_gpu_compatibility with dU_dt, nlps_gpu_constitutive, nlps_gpu_internal_forces one by one"""
    c = _Case(ndim)
    S, o, P = c.S, c.o, c.P
    dU = 1e-3 * c.rng.normal(size=c.ntot)
    dV = c.velocity_increment(dU)
    assert o.compatibility(dU, dV, P, c.M, c.n2m) == 0
    c.F.stress()
    _three_terms(c)
    with pytest.raises(c.n.NlpsError, match="nlps_gpu_compatibility: .*dU_dt is required"):
        S.local_compatibility_conditions(dU)  # (the stress would be made from stale rates)
    S.local_compatibility_conditions(dU, dV)
    S.constitutive_update()
    c.compare_state("level B")
    R_o, st = o.internal_forces(P, c.M, c.n2m, c.d2m, c.na)
    assert st == 0
    R_g = S.nodal_internal_forces(np.zeros(c.ntot))
    assert_close(R_g, R_o, TOL, "level B: internal forces")
    c.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_fused_residual(ndim):
    """Three dU in a row from one n state (the SNES iterates), the same through the separate stages and with device-resident
    vectors: residual, DF, F_n1, J_n1, Stress and both rate tensors; then the roll (dt_F_n <- dt_F_n1) and the kinetics."""
    import torch
    c = _Case(ndim)
    S, P = c.S, c.P
    variants = [("fused", 1e-3, 0, False), ("fused again", 2e-3, 0, False), ("fused, third", 1e-3, 0, False),
                ("separate stages", 2e-3, S.LAGR_SEPARATE, False), ("separate, rates flag", 1e-3, S.LAGR_SEPARATE | S.LAGR_RATES, False),
                ("rates flag alone", 2e-3, S.LAGR_RATES, False), ("device vectors", 1e-3, 0, True)]
    for what, amp, flags, on_device in variants:
        dU = amp * c.rng.normal(size=c.ntot)
        R_o = c.residual_ref(dU)
        if what == "fused":
            _three_terms(c)
        if on_device:
            dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (dU, c.V, c.A, c.Mv)]
            R_d = torch.full((c.ntot,), 7.0, dtype=torch.float64, device="cuda")
            S.lagrangian_evaluation(dev[0], dev[1], dev[2], dev[3], c.alpha, c.grav, out=R_d)
            R_g = R_d.cpu().numpy()
        else:
            R_g = c.residual_gpu(dU, flags)
        assert_close(R_g, R_o, TOL, f"{what}: residual")
        assert np.all(R_g[c.d2m == -1] == 0.0), "Dirichlet dofs carry no residual"
        st = c.compare_state(what)
        assert_close(st["dt_F_n"], P["dt_F_n"], TOL, f"{what}: the n state is not touched")
    rate_n1 = P["dt_F_n1"].copy()
    assert np.abs(rate_n1).max() > 0 and np.abs(rate_n1 - P["dt_F_n"]).max() > 1e-3 * np.abs(rate_n1).max()
    c.advance(dU)
    st = S.download_state()
    assert np.array_equal(P["dt_F_n"], rate_n1)
    assert_close(st["dt_F_n"], rate_n1, TOL, "dt_F_n after the roll is the previous dt_F_n1")
    for k, ok in (("x", "x"), ("vel", "vel"), ("acc", "acc"), ("F_n", "F_n"), ("J_n", "J_n"), ("rho", "rho")):
        assert_close(st[k], P[ok], TOL, f"{k} after roll + kinetics")
    c.close()


@pytest.mark.parametrize("layout", ["interleaved", "layers"])
def test_mixed_cloud(layout):
    """Fluid + Neo-Hookean in one 3-D cloud: the fluid's launch in the rate-carrying mode, the solid's in MODE 3 (one launch
    per law: the run-time dispatch kernel does not hold the fluid law and is refused), and through the separate stages."""
    c = _Case(3, materials=[FLUID, SOFT_NH], layout=layout)
    S, P = c.S, c.P
    fl = P["matidx"] == 0
    assert 0 < np.count_nonzero(fl) < P.np
    with pytest.raises(c.n.NlpsError, match="dispatch kernel does not hold Newtonian-Fluid-Compressible"):
        S.set_law_launch_mode(2)
    for mode, flags in ((1, 0), (1, S.LAGR_SEPARATE)):
        S.set_law_launch_mode(mode)
        for amp in (1e-3, 2e-3):
            what = f"mixed {layout}, launch mode {mode}, flags {flags}"
            dU = amp * c.rng.normal(size=c.ntot)
            R_o = c.residual_ref(dU)
            R_g = c.residual_gpu(dU, flags)
            assert_close(R_g, R_o, TOL, f"{what}: residual")
            assert np.all(R_g[c.d2m == -1] == 0.0)
            st = S.download_state()
            for k, ok in STATE[:4]:
                assert_close(st[k], P[ok], TOL, f"{what}: {k}")
            for k, ok in RATES:  # the rate tensors are the fluid particles' (a fused solid launch does not make them)
                assert_close(st[k][fl], P[ok][fl], TOL, f"{what}: {k} of the fluid particles")
    _three_terms(c)
    assert np.abs(P["stress"][~fl]).max() > 0 and np.abs(P["W"][~fl]).max() > 0
    # the tangent of the mixed cloud: never the upper-half shortcut of a Neo-Hookean cloud
    S.set_tangent_alpha4(c.a["a4"])
    K = _coo_dense(S, c.ntot, c.a["a1"], c.Mv, True)
    K_ref = c.tangent_ref()
    assert_close(K, K_ref, TOL_K, f"mixed {layout}: assembled tangent")
    # (the mass term alpha_1 M sets max |K|; rounding alone leaves an asymmetry of ~1e-16 of it)
    assert np.abs(K_ref - K_ref.T).max() > 1e-10 * np.abs(K_ref).max()
    S.tangent_operator(c.a["a1"], c.Mv, True)
    _check_apply(S, K, c.ntot, c.rng, f"mixed {layout}")
    c.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_tangent(ndim):
    """COO matrix, matrix-free products and diagonal blocks against the dense numpy tangent, with alpha_4 and without;
    the setter changes exactly the alpha_4 terms."""
    c = _Case(ndim)
    S = c.S
    dU = 1e-3 * c.rng.normal(size=c.ntot)
    c.residual_ref(dU)
    c.residual_gpu(dU)
    a4 = c.a["a4"]
    mats = {}
    for alpha4, alpha_1, mass, dirichlet in ((None, 0.0, None, False), (a4, 0.0, None, False), (a4, c.a["a1"], c.Mv, True)):
        what = f"fluid {ndim}-D (alpha_4={alpha4}, alpha_1={alpha_1}, dirichlet={dirichlet})"
        if alpha4 is not None:
            S.set_tangent_alpha4(alpha4)  # (None: the default of a new handle, 0)
        K_ref = c.F.tangent(c.n2m, c.d2m if dirichlet else None, c.na, alpha4 or 0.0, alpha_1, mass)
        K = _coo_dense(S, c.ntot, alpha_1, mass, dirichlet)
        assert_close(K, K_ref, TOL_K, f"{what}: assembled COO")
        S.tangent_operator(alpha_1, mass, dirichlet)
        for _ in range(3):
            x = c.rng.normal(size=c.ntot)
            assert_close(S.tangent_apply(x), K_ref @ x, TOL_K, f"{what}: apply", scale=np.abs(K_ref).max() * np.abs(x).max())
        _check_apply(S, K, c.ntot, c.rng, what)
        _check_blocks(S, K, c.na, ndim, what)
        B = S.tangent_block_diagonal()
        ref = np.stack([K_ref[A * ndim:(A + 1) * ndim, A * ndim:(A + 1) * ndim] for A in range(c.na)])
        assert_close(B, ref, TOL_K, f"{what}: block diagonal", scale=np.abs(K_ref).max())
        mats[(alpha4, dirichlet)] = (K, K_ref)
    (K0, K0_ref), (K4, K4_ref) = mats[(None, False)], mats[(a4, False)]   # without the mass term: max |K| is the stiffness
    assert np.abs(K4_ref - K4_ref.T).max() > 1e-4 * np.abs(K4_ref).max(), "not symmetric"
    # what alpha_4 adds: 2/3 alpha_4 c0 in c1, alpha_4 c0 in c2 and alpha_4 c0 lenght_0 on the diagonal, nothing else
    d_gpu, d_ref = K4 - K0, K4_ref - K0_ref
    assert np.abs(d_ref).max() > 1e-2 * np.abs(K4_ref).max()
    assert_close(d_gpu, d_ref, TOL_K, "the alpha_4 terms", scale=np.abs(K4_ref).max())
    c.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_newton_solve(ndim):
    """Three time steps of nlps_gpu_newton_solve against snes_ref.newton over the numpy residual and tangent."""
    c = _Case(ndim, step=0)
    S = c.S
    tight = dict(pc="pbjacobi", restart=200, max_it=2000, rtol=1e-12)
    kw = dict(max_it=12, rtol=1e-10, atol=0.0, stol=0.0)
    worst = 0.0
    for step in range(3):
        what = f"fluid {ndim}-D step {step}"
        if step:
            c.begin_step(step)
        dU, info = S.newton_solve(np.zeros(c.ntot), c.V, c.A, c.Mv, c.alpha, c.grav, linesearch="basic", ksp=tight, **kw)
        xr, ir = snes_ref.newton(c.residual_ref, c.tangent_ref, np.zeros(c.ntot), linesearch="basic", linear="dense", **kw)
        print(what, "device", info["fnorm_history"], "reference", ir["fnorm_history"])
        assert info["reason"] == snes_ref.CONVERGED_FNORM_RELATIVE and info["iterations"] >= 2, info
        for k in ("reason", "iterations", "function_evaluations"):
            assert info[k] == ir[k], f"{what}: {k} {info[k]} vs the reference's {ir[k]}\n{info}\n{ir}"
        assert np.all(info["lambda_history"] == 1.0) and info["linear_iterations"] == info["ksp_iterations"].sum() > 0
        assert_close(dU, xr, 1e-8, f"{what}: dU", scale=np.abs(xr).max())
        hd, hr = info["fnorm_history"], ir["fnorm_history"]
        big = hr >= 1e-7 * hr[0]  # (below that the entries are summation noise of the residual's atomics)
        # In 2-D the first two entries of every step count.  In 3-D the step at this dt is so nearly linear that the second
        # entry (5.5e-8 fnorm0) is already under the threshold: there the history check holds entry 0 only, and the
        # post-update state is held by the counts, dU to 1e-8 and the particle state to 1e-10 below.  (At dt = 1e-2 the
        # second 3-D entry is 5.1e-6 fnorm0 in the numpy Newton; the bound for that dt has to be measured on the device
        # before the test can move there.)
        assert big[:2].all() or ndim == 3, f"{what}: the first two entries are above 1e-7 fnorm0: {hr}"
        err = float((np.abs(hd - hr)[big] / hr[big]).max())
        worst = max(worst, err)
        print(what, "fnorm_history: largest relative difference %.3e" % err)
        assert err <= HISTORY_TOL, f"{what}: fnorm_history, relative {err:.3e}\n{hd}\n{hr}"
        c.residual_ref(dU)  # the state the solve leaves is the one of an evaluation at the returned dU
        c.compare_state(what)
        c.advance(dU)
    print(f"fluid {ndim}-D: fnorm_history worst relative difference {worst:.3e}")
    c.close()


@pytest.mark.parametrize("ndim", [2, 3])
def test_newmark_step(ndim):
    """nlps_gpu_newmark_step over three steps against the separate calls on a twin handle."""
    c = _Case(ndim, step=0, twin=True)
    S, S2 = c.S, c.S2
    dt = 2.0e-3
    kw = dict(max_it=50, atol=1e-8, rtol=1e-10, stol=1e-8, linesearch="bt", ksp=dict(pc="jacobi", restart=30, max_it=10000, rtol=1e-5))
    dU_out = np.zeros(S.nnodes * ndim)
    for step in range(3):
        info = S.newmark_step(c.bcs, step, dt, c.grav, dU_out=dU_out, **kw)
        S2.local_search()
        S2.active_masks(c.bcs, step)
        M = S2.compute_nodal_lumped_mass()
        V, A = S2.get_nodal_field_n(M)
        guess = S2.form_initial_guess(V, A, dt, c.bcs, step)
        dU, ir = S2.newton_solve(guess, V, A, M, c.alpha, c.grav, **kw)
        dV, dA = S2.compute_nodal_kinetic_increments(dU, V, A, c.alpha)
        S2.update_particles_internal_variables()
        S2.update_particles_kinetics_FLIP_PIC(1.0, dU, V, dV, dA)
        print(f"step {step}", info["fnorm_history"], info["ksp_iterations"], ir["fnorm_history"], ir["ksp_iterations"])
        assert info["nactive"] == S2.nactive and info["reason"] > 0 and info["iterations"] >= 1
        for k in ("reason", "iterations", "function_evaluations", "linear_iterations"):
            assert info[k] == ir[k], f"step {step}: {k} {info[k]} vs {ir[k]}"
        n = S2.nactive * ndim
        assert_close(dU_out[:n], dU, 1e-8, f"step {step}: dU", scale=np.abs(dU).max())
    a, b = S.download_state(), S2.download_state()
    for k in ("x", "vel", "acc", "F_n", "Stress", "J_n", "dt_F_n"):
        assert_close(a[k], b[k], 1e-8, f"after three steps: {k}")
    assert np.abs(a["dt_F_n"]).max() > 0
    c.close()


def test_the_explicit_step_refuses_the_law():
    c = _Case(3)
    S = c.S
    with pytest.raises(c.n.NlpsError, match="nlps_gpu_explicit_step.*Newtonian-Fluid-Compressible"):
        S.explicit_step(c.bcs, 0, 1e-4)
    # the handle stays usable: the search and the masks of before are still good for a residual evaluation
    dU = 1e-3 * c.rng.normal(size=c.ntot)
    assert_close(c.residual_gpu(dU), c.residual_ref(dU), TOL, "residual after the refusal")
    c.close()


@pytest.mark.parametrize("flags", [0, 2])
def test_a_singular_F_fails_the_residual_call(flags):
    """spatial_velocity_gradient__Particles__ fails where F_n1 does not invert (compute-Strains.c:286-324): status flag 8
    and an error from the call, fused and through the separate stages."""
    n = nlps()
    rng = np.random.default_rng(5)
    nsteps, step, ndim = 2, 1, 3
    case, M, P, prm, _ = _moved_case(ndim, FLUID, nsteps, rng)
    good = gpu_setup(case, init=False, nsteps=nsteps)
    case["cloud"] = dict(case["cloud"])
    F_n = case["cloud"]["F_n"].copy()
    F_n[F_n.shape[0] // 2, :] = 0.0   # F_n1 = DF F_n = 0
    case["cloud"]["F_n"] = F_n
    bad = gpu_setup(case, init=False, nsteps=nsteps)
    for S, fails in ((good, False), (bad, True)):
        S.local_search()
        n2m, d2m = S.active_masks(n.BccSet([dirichlet_plane(case, ndim - 1, 3, nsteps)]), step)
        na = int(n2m.max()) + 1
        a = newmark_parameters(0.25, 0.5, 2.0e-3)
        alpha = [a[k] for k in ("a1", "a2", "a3", "a4", "a5", "a6")]
        z, Mv = np.zeros(na * ndim), np.ones(na * ndim)
        dU = 1e-3 * np.random.default_rng(6).normal(size=na * ndim)
        if not fails:
            R = S.lagrangian_evaluation(dU, z, z, Mv, alpha, [0.0, 0.0, 0.0], flags=flags)
            assert np.all(np.isfinite(R)) and S.status_flags() == 0
        else:
            with pytest.raises(n.NlpsError):
                S.lagrangian_evaluation(dU, z, z, Mv, alpha, [0.0, 0.0, 0.0], flags=flags)
            assert S.status_flags() & 8
        S.close()
