"""The checker of the explicit step with Neumann contours (tests/explicit_loads_ref.py) on the CPU: without loads the
composition is orc.ExplicitStepper to rounding, and the scenarios of tests/test_gpu_explicit_loads.py have the margins
that keep a GPU test from passing vacuously."""
import numpy as np
import pytest

import explicit_loads_ref as lr
from util import assert_close, dirichlet_plane, make_case, oracle_setup, orc, relerr


@pytest.mark.parametrize("ndim", [2, 3])
def test_composition_without_loads_is_the_oracle_step(ndim):
    """3 steps with a Dirichlet plane and gravity against orc_explicit_step, 1e-13"""
    o = orc()
    nsteps = 3
    if ndim == 3:
        case = make_case(3, [10, 10, 10], [3, 3, 3], [4, 4, 4], velocity=[0.0, 0.0, -10.0])
        bcs = [dirichlet_plane(case, 2, 2, nsteps)]
    else:
        case = make_case(2, [14, 12], [3, 3], [7, 6], velocity=[0.0, -10.0])
        bcs = [dirichlet_plane(case, 1, 2, nsteps)]
    g = lr.gravity(ndim)
    M, P, prm, mats = oracle_setup(case)
    stepper = o.ExplicitStepper(P, M, mats, prm, o.BccSet(bcs), nsteps, gravity=g)
    R = lr.LoadsRef(case, bcs, (), nsteps, g)
    for t in range(nsteps):
        assert stepper.step(t, 1e-3) == 0
        R.step(t, 1e-3)
        assert stepper.out.nactive == R.na
        for k in ("mass", "dU", "force", "accel", "reaction"):
            assert_close(R.nodal[k], stepper.nodal(k), 1e-13, f"step {t} nodal {k}")
        assert np.abs(stepper.nodal("reaction")).max() > 0.0, "the plane has to hold something"
        for k in lr.LoadsRef.FIELDS:
            assert_close(R.P[k], P[k], 1e-13, f"step {t} {k}")


@pytest.mark.parametrize("ndim,laws", [(2, 0), (3, 0), (3, (0, 1))])
def test_scenario_margins(ndim, laws):
    loaded = lr.reference(ndim, laws, True)
    plain = lr.reference(ndim, laws, False)
    case = lr.loaded_case(ndim, laws)
    loads = lr.contours(case)
    # the contours: 20 particles each, from outer layers, across a tile boundary
    I0 = oracle_setup(case)[1]["I0"]
    gn = case["grid_n"]
    for l in loads:
        assert len(l["nodes"]) == 20 and len(set(l["nodes"].tolist())) == 20
        ijk = lr.lattice_index(I0[l["nodes"]], gn, ndim)
        tiles = {tuple(t) for t in (ijk // lr.TB[ndim]).tolist()}
        assert len(tiles) >= 2, "a contour has to cross a tile boundary"
    assert (loads[1]["dir"][0] == [1, 1, 0, 1]).all(), "the carry-over step"
    T2 = lr.carried_tractions(loads, 2, ndim)
    assert T2[1][0] == loads[0]["value"][0, 2] and T2[1][1] == loads[1]["value"][1, 2]
    # the loaded run is another run from the first step on
    e = relerr(loaded[0]["acc"], plain[0]["acc"])
    print(f"{ndim}-D laws {laws}: particle acceleration, loaded against unloaded after step 1: {e:.3e}")
    assert e >= 1e-3
    # every J_n1 stays positive (LoadsRef asserts it in every step; J_n is J_n1 after the corrector)
    for s in loaded + plain:
        assert (s["J_n"] > 0.0).all()
    # a fixed dof carries a traction share: its reaction differs from the unloaded run
    for t, (a, b) in enumerate(zip(loaded[:1], plain[:1])):
        assert a["na"] == b["na"] and np.array_equal(a["d2m"], b["d2m"])
        fixed = a["d2m"] == -1
        assert fixed.any()
        d = np.abs(a["nodal"]["reaction"] - b["nodal"]["reaction"])[fixed]
        scale = np.abs(b["nodal"]["reaction"]).max()
        print(f"{ndim}-D: largest change of a reaction {d.max():.3e} of {scale:.3e}")
        assert d.max() > 1e-3 * scale


@pytest.mark.parametrize("ndim", [2, 3])
def test_partition_of_unity(ndim):
    """no Dirichlet sets: the nodal force sums to sum T A0 over the contour entries (the internal forces sum to zero);
    independent of the oracle's traction routine"""
    case = lr.loaded_case(ndim)
    loads, a0 = lr.contours(case), lr.area0(case)
    R = lr.LoadsRef(case, (), loads, lr.NSTEPS, lr.gravity(ndim), lr.THICKNESS, a0)
    for t in range(lr.NSTEPS):
        R.step(t, lr.DT[t])
        got = R.nodal["force"].reshape(-1, ndim).sum(axis=0)
        want = lr.total_traction(case, loads, t, lr.THICKNESS, a0)
        e = np.abs(got - want).max() / np.abs(want).max()
        print(f"{ndim}-D step {t}: sum of the nodal force {got}, sum T A0 {want}, relative {e:.2e}")
        assert e <= 1e-10
