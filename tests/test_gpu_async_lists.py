"""Async lists: in the folded one-rank explicit step the search of the next step is a kernel of its own in front of K5,
and the activation and list kernels of the next step run on the library's side stream beside K5, into a twin set of
lists that the next step adopts.  `debug_option("async_lists", 0)` keeps the sequence with the search riding on K5 and
the lists built in front of K2.  Both forms must give the same closest nodes and neighbour lists, bit for bit, and the
same state to the tolerances of two equivalent launch forms (test_folded_step_matches_the_nodal_kernels)."""
import functools

import numpy as np
import pytest

from util import assert_close, dirichlet_plane, gpu_setup, make_case, nlps

pytestmark = pytest.mark.gpu

DT = 2e-3  # 40 steps at |v| ~ 10: 0.8 h along the last axis, so most particles change closest node, some change tile


def lists_equal(nn, a, b):
    col = np.arange(a.shape[1])[None, :]
    valid = col < nn[:, None]
    return bool(np.all(np.where(valid, a, 0) == np.where(valid, b, 0)))


def the_case(ndim):
    if ndim == 3:  # 4 096 particles over several 4^3-node tiles
        return make_case(3, [16, 16, 16], [4, 4, 4], [8, 8, 8], velocity=[3.0, 1.0, -10.0])
    return make_case(2, [24, 24], [4, 4], [16, 16], velocity=[3.0, -10.0])


def between(S, gb, what, t):
    """One API call between two runs of steps; returns the number of the next step."""
    if what == "download_state":
        S.download_state()
    elif what == "explicit_nodal":
        S.explicit_nodal()
    elif what == "local_search":
        S.local_search()
    elif what == "resort":
        S.resort()
    elif what == "timing":
        S.set_timing(True)
        S.explicit_step(gb, t, DT)
        S.set_timing(False)
        t += 1
    elif what == "lazy_nodal":
        S.debug_option("lazy_nodal", 0)
    return t


def run(ndim, async_lists, nsteps, resort=None, what=None, stream=None, plane=2):
    """nsteps steps; with `what`, that call comes after the third step and three more steps follow it.  Returns the
    solver and the closest nodes of the initial search.  The nodes of layer `plane` are held: 2 for the long runs, which
    fly 0.8 h before they are compared, 3 -- one layer under the block, inside the stencil of its lowest particles -- for
    the short ones, so that stress and acceleration are the cloud's answer to the wall from the first step on and not
    the rounding noise of a rigid flight."""
    case = the_case(ndim)
    total = nsteps + 1
    gb = nlps().BccSet([dirichlet_plane(case, ndim - 1, plane, total)])
    S = gpu_setup(case, nsteps=total, stream=stream)
    if not async_lists:
        S.debug_option("async_lists", 0)
    if resort:
        S.set_resort_interval(resort)
    I0_start = S.download_state()["I0"].copy()
    t = 0
    for _ in range(nsteps if what is None else 3):
        S.explicit_step(gb, t, DT)
        t += 1
    if what is not None:
        t = between(S, gb, what, t)
        for _ in range(3):
            S.explicit_step(gb, t, DT)
            t += 1
    return S, I0_start


def results(S, stream=None):
    if stream is not None:
        stream.synchronize()  # the caller's stream alone; the downloads below copy through the default stream
    out = (S.download_state(), S.download_lists(), S.explicit_nodal(), S.nactive, S.status_flags())
    S.close()
    return out


@functools.lru_cache(maxsize=None)
def serial(ndim, nsteps, resort=None, what=None, plane=2):
    S, I0_start = run(ndim, False, nsteps, resort, what, plane=plane)
    return results(S), I0_start


def compare(a, b, what):
    (sa, (na, la), noda, nacta, fa), (sb, (nb, lb), nodb, nactb, fb) = a, b
    assert fa == fb, f"{what}: status flags {fa:#x} vs {fb:#x}"
    assert np.array_equal(sa["I0"], sb["I0"]), f"{what}: closest nodes differ"
    assert np.array_equal(na, nb) and lists_equal(na, la, lb), f"{what}: neighbour lists differ"
    assert np.abs(sb["Stress"]).max() > 1.0 and np.abs(sb["acc"]).max() > 1.0  # (fields, not rounding noise)
    for k in ("x", "vel", "acc", "F_n", "Stress", "J_n", "rho"):
        assert_close(sa[k], sb[k], 1e-11, f"{k}: {what}")
    assert nacta == nactb
    for k in ("mass", "dU", "force", "accel", "reaction"):
        assert_close(noda[k], nodb[k], 1e-10, f"nodal {k}: {what}", scale=1e-12)


@pytest.mark.parametrize("ndim", [3, 2])
def test_async_lists_match_the_serial_form(ndim):
    """40 steps across node and tile boundaries, with a re-sort every 7 steps so that re-sorts fall between lists built
    ahead (the step in front of a re-sort builds none)."""
    ref, I0_start = serial(ndim, 40, 7)
    S, _ = run(ndim, True, 40, 7)
    got = results(S)
    moved = np.mean(ref[0]["I0"] != I0_start)
    print(f"{ndim}-D: {100 * moved:.1f} % of the closest nodes changed over the run")
    assert moved >= 0.05, "the run does not move enough particles to another node to see a stale list"
    compare(got, ref, "async lists vs serial")


@pytest.mark.parametrize("what", ["download_state", "explicit_nodal", "local_search", "resort", "timing", "lazy_nodal"])
def test_api_calls_between_async_steps(what):
    """Every entry that reads or rebuilds what the side stream has made ahead: 3 steps, the call, 3 more steps."""
    ref, _ = serial(3, 6, None, what, 3)
    S, _ = run(3, True, 6, None, what, plane=3)
    compare(results(S), ref, f"async lists vs serial, {what} between the steps")


def test_async_lists_on_the_callers_stream():
    """The side work is joined into the handle's stream at the end of every step: after synchronising the caller's
    non-blocking stream alone, a read through another stream sees the finished state."""
    import torch
    ref, _ = serial(3, 10, None, None, 3)
    prev = torch.cuda.current_stream()
    ts = torch.cuda.Stream()
    torch.cuda.set_stream(ts)
    try:
        S, _ = run(3, True, 10, stream=ts.cuda_stream, plane=3)
        got = results(S, stream=ts)
    finally:
        torch.cuda.set_stream(prev)
    compare(got, ref, "async lists on the caller's stream vs serial")
