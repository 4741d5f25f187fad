"""The eigenerosion and eigensoftening hooks inside the explicit step (nlps_gpu_set_explicit_damage) against
the composition of the oracle's stage calls (explicit_damage_ref.py; its scenarios and their margins are checked on the
CPU by test_explicit_damage_ref.py)."""
import numpy as np
import pytest

import explicit_damage_ref as xr
from test_gpu_eigenerosion import stretch_field
from test_gpu_parity import masks
from util import assert_close, gpu_setup, nlps, orc, relerr

pytestmark = pytest.mark.gpu

PARTICLE = (("Stress", "stress"), ("W", "W"), ("x_GC", "x"), ("dis", "dis"), ("vel", "vel"), ("acc", "acc"), ("F_n", "F_n"),
            ("J_n", "J_n"), ("rho", "rho"))
NODAL = ("mass", "dU", "force", "accel")


def damage_solver(case, driver="erosion", nsteps=4):
    n = nlps()
    params = n.default_params()
    if driver == "erosion":
        params.driver_eigenerosion = 1
    elif driver == "softening":
        params.driver_eigensoftening = 1
    S = gpu_setup(case, nsteps=nsteps, params=params)
    if driver:
        S.set_explicit_damage(True)
    return S


def compare(S, snap, what, tol=1e-9):
    nod = S.explicit_nodal()
    assert S.nactive == snap["na"], what
    for k in NODAL:
        assert_close(nod[k], snap["nodal"][k], tol, f"{what} nodal {k}")
    st = S.download_state()
    assert np.array_equal(st["Damage_n1"], snap["damage"]), f"{what}: Damage_n1"
    assert np.array_equal(st["Damage_n"], snap["damage"]), f"{what}: Damage_n after the roll"
    for k, ok in PARTICLE:
        assert_close(st[k], snap[ok], tol, f"{what} {k}")
    return st


def run_erosion(ndim, laws, prepare=None):
    n = nlps()
    ref = xr.erosion_reference(ndim, laws)
    S = damage_solver(xr.erosion_case(ndim, laws, Gf=xr.erosion_Gf(ndim, laws)))
    if prepare:
        prepare(S)
    none = n.BccSet([])
    for t, snap in enumerate(ref):
        S.explicit_step(none, t, xr.DT[t], xr.GAMMA)
        compare(S, snap, f"step {t}")
    S.close()


@pytest.mark.parametrize("ndim,law", [(2, 0), (3, 0), (3, 1)])
def test_eigenerosion_steps(ndim, law):
    run_erosion(ndim, law)


def test_eigenerosion_steps_with_resorts():
    """the snapshot tables under a permutation of the slots, the damage fields travelling with the periodic re-sort"""
    def prepare(S):
        S.resort()
        S.set_resort_interval(2)
    run_erosion(3, 0, prepare)


def test_eigenerosion_steps_interleaved_laws():
    """Neo-Hookean and Hencky particles in turn: the state half of a cloud of several laws (the launch form the library
    picks for it)"""
    run_erosion(3, (0, 1))


def test_eigenerosion_steps_interleaved_laws_per_law_launches():
    """the same cloud with one launch of the state half per law present (nlps_gpu_set_law_launch_mode 1; the library's own
    choice for laws in turn is the kernel that dispatches on the law)"""
    run_erosion(3, (0, 1), prepare=lambda S: S.set_law_launch_mode(1))


def test_level_b_force_evaluation_on_top_of_damage_steps():
    """the state a damage step leaves is the state the level-B stages expect"""
    o = orc()
    n = nlps()
    ndim = 3
    case = xr.erosion_case(ndim, 0, Gf=xr.erosion_Gf(ndim, 0))
    R = xr.DamageRef(case, "erosion")
    S = damage_solver(case)
    none = n.BccSet([])
    for t in range(2):
        R.step(xr.DT[t])
        S.explicit_step(none, t, xr.DT[t], xr.GAMMA)
    M, P, prm, mats = R.M, R.P, R.prm, R.mats
    assert o.local_search(P, M, prm) == 0
    S.local_search()
    n2m, d2m, na = masks(S, M, [], 2, 4)
    o.compute_beps(P, M, mats, beps=R.beps, initialize=False)
    dU = stretch_field(M, n2m, na, ndim, 0.02, np.random.default_rng(3))
    assert o.compatibility(dU, None, P, M, n2m) == 0
    assert o.constitutive_eroded(P, mats, prm, R.damage_n) == 0
    assert o.eigenerosion_hook(R.damage_n1, R.damage_n, P, mats, R.beps, case["h"]) == 0
    R_o, st = o.internal_forces(P, M, n2m, d2m, na)
    assert st == 0
    S.local_compatibility_conditions(dU)
    S.constitutive_update()
    R_g = S.nodal_internal_forces(np.zeros(na * ndim))
    d = S.download_state()
    assert np.array_equal(d["Damage_n"], R.damage_n)
    assert np.array_equal(d["Damage_n1"], R.damage_n1)
    assert R.damage_n1.sum() > R.damage_n.sum(), "the level-B evaluation has to fail further particles"
    assert_close(d["Stress"], P["stress"], 1e-10, "scaled Kirchhoff stress")
    assert_close(R_g, R_o, 1e-10, "internal forces")
    S.close()


def test_unreachable_threshold_is_the_plain_step():
    """Gf = 1e300 with the switch on against a handle created without the driver: the non-folded damage form against the
    plain step, 1e-12 (the project's bound for equivalent launch forms)"""
    n = nlps()
    ndim = 3
    case = xr.erosion_case(ndim, 0, Gf=1e300)
    A = damage_solver(case)
    B = damage_solver(case, driver=None)
    none = n.BccSet([])
    worst = 0.0
    for t in range(3):
        A.explicit_step(none, t, xr.DT[t], xr.GAMMA)
        B.explicit_step(none, t, xr.DT[t], xr.GAMMA)
        na, nb = A.explicit_nodal(), B.explicit_nodal()
        assert A.nactive == B.nactive
        for k in NODAL:
            worst = max(worst, relerr(na[k], nb[k]))
            assert_close(na[k], nb[k], 1e-12, f"step {t} nodal {k}")
        a, b = A.download_state(), B.download_state()
        assert not a["Damage_n1"].any()
        for k in [k for k, _ in PARTICLE] + ["DF", "F_n1", "J_n1"]:
            worst = max(worst, relerr(a[k], b[k]))
            assert_close(a[k], b[k], 1e-12, f"step {t} {k}")
    print(f"damage form with an unreachable Gf against the plain step: worst relative difference {worst:.2e}")
    A.close()
    B.close()


@pytest.mark.parametrize("ndim,law", [(2, 0), (3, 0)])
def test_eigensoftening_steps(ndim, law):
    n = nlps()
    ref = xr.softening_reference(ndim, law)
    S = damage_solver(xr.softening_case(ndim, law, ft=xr.softening_ft(ndim, law)), "softening", nsteps=3)
    none = n.BccSet([])
    for t, snap in enumerate(ref):
        S.explicit_step(none, t, xr.DT[t], xr.GAMMA)
        d = S.download_state()
        assert np.array_equal(d["Strain_f_n1"] > 0, snap["strain_f"] > 0), f"step {t}: which particles start to fracture"
        assert_close(d["Strain_f_n1"], snap["strain_f"], 1e-9, f"step {t}: fracture strain")
        assert_close(d["Strain_f_n"], snap["strain_f"], 1e-9, f"step {t}: rolled fracture strain")
        assert_close(d["Damage_n1"], snap["damage"], 1e-9, f"step {t}: damage")
        assert_close(d["Damage_n"], snap["damage"], 1e-9, f"step {t}: rolled damage")
        assert_close(d["Stress"], snap["stress"], 1e-9, f"step {t}: scaled Kirchhoff stress")
        for k, ok in (("x_GC", "x"), ("vel", "vel"), ("F_n", "F_n")):
            assert_close(d[k], snap[ok], 1e-9, f"step {t} {k}")
    S.close()


def test_refusals_leave_the_handle_usable():
    n = nlps()
    none = n.BccSet([])
    case = xr.erosion_case(3, 0, Gf=1e300)
    S = damage_solver(case)
    S.set_explicit_damage(False)
    with pytest.raises(n.NlpsError, match="level-B stages only"):  # switch off: today's message
        S.explicit_step(none, 0, 1e-4)
    S.local_search()
    S.set_explicit_damage(True)
    S.set_deterministic(True)
    with pytest.raises(n.NlpsError, match="deterministic"):
        S.explicit_step(none, 0, 1e-4)
    S.local_search()
    S.set_deterministic(False)
    S.set_halo_exchange(lambda dptr, nfield, elem, kind: 0)
    with pytest.raises(n.NlpsError, match="ghost particles"):
        S.explicit_step(none, 0, 1e-4)
    S.local_search()
    S.set_halo_exchange(None)
    S.explicit_step(none, 0, 1e-4)  # and with everything back in place it steps
    S.close()
    P = damage_solver(case, driver=None)
    with pytest.raises(n.NlpsError, match="without driver_eigenerosion"):
        P.set_explicit_damage(True)
    P.local_search()
    P.explicit_step(none, 0, 1e-4)
    P.close()
