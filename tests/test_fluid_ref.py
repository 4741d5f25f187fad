"""The checker of the fluid tests holds itself (tests/fluid_ref.py, no GPU): the stress against closed forms, upstream's
2-D trace, the vectorised pair blocks against the statement-by-statement stiffness density, and the dense Jacobian loop
against the oracle's assembled Neo-Hookean tangent."""
import numpy as np
import pytest

import fluid_ref
from util import NH, dirichlet_plane, make_case, oracle_setup, orc

WATER = {"type": 6, "E": 0.0, "nu": 0.0, "p_ref": 1.0e3, "viscosity": 0.7, "compressibility": 2.0e5, "n_macdonald": 7.0}


def _row(A, ndim):
    T = 5 if ndim == 2 else 9
    r = np.zeros(T)
    r[: ndim * ndim] = np.asarray(A, dtype=np.float64).ravel()
    if ndim == 2:
        r[4] = 1.0
    return r


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("s", [0.9, 1.0, 1.2])
def test_a_fluid_at_rest_carries_its_pressure_only(ndim, s):
    """dt_F = 0 and F = s I: tau = -pressure(J) I exactly, in the plane and out of it"""
    J = s ** ndim
    tau = fluid_ref.stress(WATER, _row(s * np.eye(ndim), ndim), _row(np.zeros((ndim, ndim)), ndim) * 0.0, J, ndim)
    n, K, p0 = WATER["n_macdonald"], WATER["compressibility"], WATER["p_ref"]
    p = J * (p0 + (K / n) * (J ** (-n) - 1.0))
    expect = _row(-p * np.eye(ndim), ndim)
    if ndim == 2:
        expect[4] = -p
    assert np.array_equal(tau, expect)
    if s == 1.0:
        assert p == p0


def test_simple_shear_gives_mu_gamma_dot():
    """F = I and dt_F a simple shear rate: tau_xy = tau_yx = mu gamma_dot, the diagonal is the pressure"""
    gd = 3.5
    dF = np.zeros((3, 3))
    dF[0, 1] = gd
    tau = fluid_ref.stress(WATER, _row(np.eye(3), 3), _row(dF, 3), 1.0, 3).reshape(3, 3)
    assert tau[0, 1] == pytest.approx(WATER["viscosity"] * gd, rel=1e-15) and tau[1, 0] == tau[0, 1]
    assert np.allclose(np.diag(tau), -WATER["p_ref"], rtol=1e-15) and tau[0, 2] == tau[1, 2] == 0.0


def test_the_2d_trace_is_upstreams():
    """Newtonian-Fluid.c:59 adds E[0] + E[2] of the 2 x 2 row, xx + yx.  With L_yx != L_yy a corrected trace fails."""
    L = np.array([[0.3, 0.8], [-0.2, 1.1]])
    E = 0.5 * (L + L.T)
    assert abs(E[1, 0] - E[1, 1]) > 0.1
    tau = fluid_ref.stress(WATER, _row(np.eye(2), 2), _row(L, 2), 1.0, 2)
    mu, p0 = WATER["viscosity"], WATER["p_ref"]
    upstream = E[0, 0] + E[1, 0]
    corrected = E[0, 0] + E[1, 1]
    assert tau[0] == pytest.approx(-p0 + 2 * mu * E[0, 0] - (2.0 / 3.0) * mu * upstream, rel=1e-14)
    assert tau[4] == pytest.approx(-p0 - (2.0 / 3.0) * mu * upstream, rel=1e-14)      # :74
    assert abs(tau[4] - (-p0 - (2.0 / 3.0) * mu * corrected)) > 0.1
    assert tau[1] == pytest.approx(2 * mu * E[0, 1], rel=1e-14) and tau[1] == tau[2]


def test_the_three_terms_sum_to_the_stress():
    rng = np.random.default_rng(2)
    for ndim in (2, 3):
        F = np.eye(ndim) + 0.1 * rng.normal(size=(ndim, ndim))
        dF = rng.normal(size=(ndim, ndim))
        J = np.linalg.det(F)
        t = fluid_ref.stress_terms(WATER, _row(F, ndim), _row(dF, ndim), J, ndim)
        full = fluid_ref.stress(WATER, _row(F, ndim), _row(dF, ndim), J, ndim)
        assert np.abs(t.sum(axis=0) - full).max() <= 1e-15 * np.abs(t).max()
        assert all(np.abs(t[k]).max() > 0 for k in range(3))


def test_a_singular_F_is_an_error():
    with pytest.raises(np.linalg.LinAlgError):
        fluid_ref.stress(WATER, _row(np.zeros((3, 3)), 3), _row(np.ones((3, 3)), 3), 0.5, 3)


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("alpha4", [0.0, 250.0])
def test_all_pairs_is_the_per_pair_stiffness_density(ndim, alpha4):
    rng = np.random.default_rng(7 + ndim)
    nn = 6
    dN, dN1 = rng.normal(size=(nn, ndim)), rng.normal(size=(nn, ndim))
    F_n = _row(np.eye(ndim) + 0.1 * rng.normal(size=(ndim, ndim)), ndim)
    F_n1 = _row(np.eye(ndim) + 0.1 * rng.normal(size=(ndim, ndim)), ndim)
    dF = _row(rng.normal(size=(ndim, ndim)), ndim)
    J = np.linalg.det(fluid_ref.block(F_n1, ndim))
    allp = fluid_ref.stiffness_density_all_pairs(dN1, dN, F_n, F_n1, dF, J, alpha4, WATER, ndim)
    scale = np.abs(allp).max()
    asym = 0.0
    for A in range(nn):
        for B in range(nn):
            one = fluid_ref.stiffness_density(dN1[A], dN1[B], dN[A], dN[B], F_n, F_n1, dF, J, alpha4, WATER, ndim)
            assert np.abs(allp[A, B] - one).max() <= 1e-14 * scale
            asym = max(asym, np.abs(allp[A, B] - allp[B, A].T).max())
    assert asym > 1e-8 * scale, "the fluid tangent is not symmetric (rounding is 1e-16 of the scale)"


@pytest.mark.parametrize("ndim", [2, 3])
def test_the_dense_loop_reproduces_the_oracles_neo_hookean_tangent(ndim):
    """fluid_ref.dense_tangent with orc.py's per-pair Neo-Hookean stiffness as the block function is the oracle's assembled
    tangent to 1e-12 of its norm: the particle / pair loop, the push-forward, the mass term and the Dirichlet rows are
    pinned before the fluid blocks go through them."""
    o = orc()
    rng = np.random.default_rng(4)
    nsteps, step = 2, 0
    if ndim == 2:
        case = make_case(2, [10, 9], [3, 3], [3, 2], material=NH, velocity=[0.5, -1.0])
    else:
        case = make_case(3, [7, 7, 7], [2, 2, 2], [2, 1, 1], material=NH, velocity=[0.5, 0.2, -1.0])
    M, P, prm, mats = oracle_setup(case)
    assert o.local_search(P, M, prm) == 0
    n2m, na = o.active_nodes(M)
    d2m, _ = o.active_dofs(n2m, na, ndim, o.BccSet([dirichlet_plane(case, ndim - 1, 2, nsteps)]), step, nsteps)
    assert np.count_nonzero(d2m == -1) > 0
    Mv = o.lumped_mass(P, M, n2m, na)
    dU = 1e-3 * rng.normal(size=na * ndim)
    assert o.compatibility(dU, None, P, M, n2m) == 0 and o.constitutive(P, mats, prm) == 0
    K_o, _, st = o.tangent_matrix(P, M, mats, n2m, d2m, na, alpha_1=4.0e4, lumped_mass=Mv, with_pattern=False)
    assert st == 0
    K = fluid_ref.dense_tangent(o, P, M, n2m, d2m, na, fluid_ref.neo_hookean_pair_blocks(o, P, mats, ndim), 4.0e4, Mv)
    assert np.linalg.norm(K - K_o) <= 1e-12 * np.linalg.norm(K_o)
    # the vectorised Neo-Hookean blocks a mixed cloud's reference uses, through the same loop
    K2 = fluid_ref.dense_tangent(o, P, M, n2m, d2m, na, lambda p, dN1, dN: fluid_ref.neo_hookean_all_pairs(
        dN1, dN, P["F_n"][p], P["J_n1"][p], NH, ndim), 4.0e4, Mv)
    assert np.linalg.norm(K2 - K_o) <= 1e-12 * np.linalg.norm(K_o)
    free = d2m != -1
    assert np.abs(K_o[np.ix_(free, free)]).max() > 0
