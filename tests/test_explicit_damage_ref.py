"""The reference of the explicit step with the damage hooks (explicit_damage_ref.py) against the oracle's own explicit
step with the hooks off, and the margins of the scenarios the GPU tests (test_gpu_explicit_damage.py) compare on: no
candidate may sit on a threshold, and the damage has to grow over the steps."""
import numpy as np
import pytest

import explicit_damage_ref as xr
from util import oracle_setup, orc, relerr


@pytest.mark.parametrize("ndim", [2, 3])
def test_composition_without_hooks_is_the_oracles_explicit_step(ndim):
    """1e-12 of each field's maximum: rounding of the reassociated sums with room (the oracle step and the composition make the same sums in the same order: no difference seen in 2-D or 3-D)"""
    o = orc()
    case = xr.erosion_case(ndim, 0)
    R = xr.DamageRef(case, None)
    M, P, prm, mats = oracle_setup(case)
    stepper = o.ExplicitStepper(P, M, mats, prm, o.BccSet([]), 3)
    worst = 0.0
    for t in range(3):
        R.step(xr.DT[t])
        assert stepper.step(t, xr.DT[t], xr.GAMMA) == 0
        assert R.na == stepper.out.nactive
        for k in ("mass", "dU", "force", "accel"):
            e = relerr(R.nodal[k], stepper.nodal(k))
            worst = max(worst, e)
            assert e <= 1e-12, f"step {t} nodal {k}: {e:.3e}"
        for k in xr.DamageRef.FIELDS + ("DF", "F_n1", "J_n1", "d_dis"):
            e = relerr(R.P[k], P[k])
            worst = max(worst, e)
            assert e <= 1e-12, f"step {t} {k}: {e:.3e}"
    print(f"composition against orc.ExplicitStepper, {ndim}-D: worst relative difference {worst:.2e}")


@pytest.mark.parametrize("ndim,laws", [(2, 0), (3, 0), (3, 1), (3, (0, 1))])
def test_eigenerosion_scenario_margins(ndim, laws):
    ref = xr.erosion_reference(ndim, laws)
    Gf = xr.erosion_Gf(ndim, laws)
    npart = ref[0]["damage"].size
    failed = [int(s["damage"].sum()) for s in ref]
    margin = np.inf
    for t, s in enumerate(ref):
        d = s["diag"]
        G, w0 = d["G"], d["T0"][d["cand"]]
        assert d["cand"].size > 0
        assert np.all(np.abs(G - Gf) >= 1e-6 * Gf), f"step {t}: a candidate sits on the threshold"
        assert np.all(np.abs(w0) >= 1e-6 * np.abs(w0).max()), f"step {t}: a principal stress next to zero decides a candidate"
        margin = min(margin, float(np.min(np.abs(G - Gf)) / Gf))
        assert np.all((s["damage"] == 0.0) | (s["damage"] == 1.0))
    assert np.all(xr.erosion_G_step1(ndim, laws) > 0.0)
    assert 0 < failed[0] < npart
    assert failed[2] > failed[0]
    print(f"eigenerosion {ndim}-D laws {laws}: failed {failed} of {npart}, smallest G margin {margin:.1e}")
    if laws == 0:
        assert failed == ([72, 79, 156, 158] if ndim == 2 else [160, 160, 307, 325])


@pytest.mark.parametrize("ndim,law", [(2, 0), (3, 0)])
def test_eigensoftening_scenario_margins(ndim, law):
    ref = xr.softening_reference(ndim, law)
    ft = xr.softening_ft(ndim, law)
    started = 0
    for t, s in enumerate(ref):
        d = s["diag"]
        assert np.all(np.abs(d["Teps"] - ft) >= 1e-6 * ft), f"step {t}: a candidate sits on the threshold"
        started += int(d["started"].sum())
    assert started > 0, "some particle has to start to fracture"
    assert np.any((ref[-1]["damage"] > 0.0) & (ref[-1]["damage"] < 1.0))
    print(f"eigensoftening {ndim}-D: {started} particles start to fracture over {len(ref)} steps")
