"""The reference of the implicit Newmark step with the damage hooks (implicit_damage_ref.py) and the margins of the
scenarios the GPU tests (test_gpu_implicit_damage.py) compare on: every step converges, no candidate sits on a threshold
at any residual evaluation, the failed share is neither nothing nor everything, and some particle fails after the first
step, so that later evaluations skip failed particles (Damage_n == 1)."""
import numpy as np
import pytest

import implicit_damage_ref as ir
import snes_ref

MARGIN = 1e-6


def _margins(ref, key, threshold):
    """smallest relative distance of a candidate from the threshold, and of a live particle's smallest principal stress
    from zero, over every residual evaluation of every step"""
    m, t0 = np.inf, np.inf
    for t, s in enumerate(ref):
        assert s["info"]["reason"] > 0, f"step {t}: {s['info']}"
        assert len(s["evals"]) == s["info"]["function_evaluations"]
        for e, d in enumerate(s["evals"]):
            assert d["cand"].size > 0
            v = d[key]
            assert np.all(np.abs(v - threshold) >= MARGIN * threshold), f"step {t} evaluation {e}: a candidate sits on the threshold"
            assert d["T0_margin"] >= MARGIN, f"step {t} evaluation {e}: a principal stress next to zero decides a candidate"
            m = min(m, float(np.min(np.abs(v - threshold)) / threshold))
            t0 = min(t0, d["T0_margin"])
    return m, t0


@pytest.mark.parametrize("ndim,dts", [(2, tuple(ir.DT)), (3, tuple(ir.DT)), (2, tuple(ir.DT_TWO_ITERATES))])
def test_eigenerosion_scenario(ndim, dts):
    ref = ir.erosion_reference(ndim, 0, dts)
    Gf = ir.erosion_Gf(ndim, 0, dts)
    npart = ref[0]["damage"].size
    failed = [int(s["damage"].sum()) for s in ref]
    margin, t0 = _margins(ref, "G", Gf)
    its = [s["info"]["iterations"] for s in ref]
    print(f"eigenerosion {ndim}-D dt {dts}: failed {failed} of {npart}, iterates {its}, smallest G margin {margin:.1e}, "
          f"smallest |T0| / max |T0| {t0:.1e}")
    for s in ref:
        assert s["info"]["reason"] == snes_ref.CONVERGED_FNORM_RELATIVE
        assert np.all((s["damage"] == 0.0) | (s["damage"] == 1.0))
    assert 0 < failed[-1] < npart
    if len(dts) > 1:
        assert failed[-1] > failed[0], "a particle fails in a step later than the first"
        later = ref[-1]["evals"][0]
        assert later["cand"].size < npart, "the later steps skip failed particles"
    else:
        assert its[0] >= 2, "the solve is exercised beyond one iterate"


@pytest.mark.parametrize("ndim", [2, 3])
def test_eigensoftening_scenario(ndim):
    """The softening scenario meets every condition but one: no particle FAILS in a later step, with any ft.  Damage grows
    by heps / wcrit = 40 times the growth of the smallest principal Almansi strain since the particle started to fracture;
    the velocity field strains the cloud by 10 to 15 per unit time, 0.013 to 0.02 over the four steps, so that no damage
    grows by more than 0.8 and the pre-damaged particles (0.3, fracture strain 1e-3 on record) end below 1 -- ft only
    decides who starts.  The Newmark-step GPU tests therefore run the eigenerosion scenarios, and eigensoftening is
    compared at the level of the residual (test_gpu_implicit_damage.py)."""
    ref = ir.softening_reference(ndim, 0)
    ft = ir.softening_ft(ndim, 0)
    margin, t0 = _margins(ref, "Teps", ft)
    npart = ref[0]["damage"].size
    failed = [int((s["damage"] == 1.0).sum()) for s in ref]
    started = [int(sum(d["started"].sum() for d in s["evals"])) for s in ref]
    partial = (ref[-1]["damage"] > 0.0) & (ref[-1]["damage"] < 1.0)
    print(f"eigensoftening {ndim}-D: failed {failed} of {npart}, started {started}, smallest T_eps margin {margin:.1e}, "
          f"smallest |T0| / max |T0| {t0:.1e}")
    assert 0 < failed[-1] < npart
    assert sum(started) > 0, "some particle has to start to fracture"
    assert partial.any()
    assert np.any(ref[-1]["damage"][partial] > ref[0]["damage"][partial]), "damage grows over the later steps"
