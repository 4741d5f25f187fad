"""Deferred move: an async step (test_gpu_async_lists) with the step record off whose successor does not start with a
re-sort leaves `x += d_dis; dis += d_dis` to K2 of the next step.  Its search marks the particles K5 would have moved,
K5 stores acc and vel alone, and the whole list stage of the next step runs beside it.  Between two steps a move is
pending; everything that reads or writes x / dis, reorders the particles or rebuilds lists from them applies it first
(materialise_move), so the state at every boundary of the API is the one of `debug_option("async_lists", 0)`, where K5
moves the particle itself.  Clouds under 100 000 particles keep the in-place K5 by default, so the deferred runs here
lower that bound (`debug_option("defer_move_min", 0)`).  The clouds, DT and `compare` are those of test_gpu_async_lists: the smallest shapes at which
particles change node and tile."""
import functools

import numpy as np
import pytest

from test_gpu_async_lists import DT, compare, results, the_case
from util import assert_close, dirichlet_plane, gpu_setup, make_case, nlps

pytestmark = pytest.mark.gpu

CALLS = ["download_state", "download_lists", "local_search", "resort", "explicit_nodal", "step_record", "timing",
         "lazy_nodal", "upload", "shape_functions", "record_now"]


def call(S, gb, what, t, case):
    """One API call between two runs of steps; returns the number of the next step."""
    if what == "download_state":
        S.download_state()
    elif what == "download_lists":
        S.download_lists()
    elif what == "local_search":
        S.local_search()
    elif what == "resort":
        S.resort()
    elif what == "explicit_nodal":
        S.explicit_nodal()
    elif what == "step_record":  # on from here: the following steps keep the in-place K5
        S.set_step_record(every=1, capacity=8)
    elif what == "record_now":  # a row of the state as it stands, then the record goes again: deferred steps follow
        S.set_step_record(every=1, capacity=8)
        S.record_now(7)
        S.set_step_record(every=None)
    elif what == "timing":  # the bracketed step runs the same K2 and K5 forms, every kernel on the handle's stream
        S.set_timing(True)
        S.explicit_step(gb, t, DT)
        S.set_timing(False)
        t += 1
    elif what == "lazy_nodal":
        S.debug_option("lazy_nodal", 0)
    elif what == "upload":  # the top sixth of the block (fewer than the spare capacity of create, np / 4) leaves and comes
        cut = 10            # straight back as immigrants: rows written into the state
        n_down, n_up, _, _, up = S.migration_select(0, cut)
        assert n_down == 0 and 0 < n_up < S.np
        S.migration_commit(up, n_up, 0, 0)
    elif what == "shape_functions":
        S.shape_functions(0, 64)
    return t


def run(ndim, deferred, pre, post=0, what=None, resort=None, stream=None, case=None, plane=3):
    """`pre` steps, then with `what` that call and `post` more steps.  The nodes of layer `plane` of the last axis are
    held (one layer under the block: stress and acceleration are the cloud's answer to the wall from the first step)."""
    case = the_case(ndim) if case is None else case
    total = pre + post + 2
    gb = nlps().BccSet([dirichlet_plane(case, ndim - 1, plane, total)])
    S = gpu_setup(case, nsteps=total, stream=stream)
    if deferred:  # (clouds under 100 000 particles keep the in-place K5 unless told otherwise)
        S.debug_option("defer_move_min", 0)
    else:
        S.debug_option("async_lists", 0)
    if resort:
        S.set_resort_interval(resort)
    t = 0
    for _ in range(pre):
        S.explicit_step(gb, t, DT)
        t += 1
    if what is not None:
        t = call(S, gb, what, t, case)
    for _ in range(post):
        S.explicit_step(gb, t, DT)
        t += 1
    return S


@functools.lru_cache(maxsize=None)
def serial(ndim, pre, post=0, what=None, resort=None, plane=3):
    return results(run(ndim, False, pre, post, what, resort, plane=plane))


@pytest.mark.parametrize("ndim", [3, 2])
@pytest.mark.parametrize("nsteps", [1, 2])
def test_download_behind_a_deferred_step(ndim, nsteps):
    """A download straight after one step -- a move is pending and no K2 comes -- and after two."""
    compare(results(run(ndim, True, nsteps)), serial(ndim, nsteps), f"download after {nsteps} deferred step(s)")


@pytest.mark.parametrize("what", CALLS)
def test_calls_between_deferred_steps(what):
    """Three steps, the call with the move of the third pending, three more steps."""
    compare(results(run(3, True, 3, 3, what)), serial(3, 3, 3, what), f"deferred move, {what} between the steps")


@pytest.mark.parametrize("ndim", [3, 2])
def test_deferred_move_across_resorts(ndim):
    """Forty steps with a re-sort every 7: the step in front of a re-sort runs the in-place K5, the others defer.  A
    particle moved twice or never shows in x and, a step later, in the closest nodes."""
    ref = serial(ndim, 40, resort=7, plane=2)  # (layer 2: the block falls 0.8 h before it is compared)
    compare(results(run(ndim, True, 40, resort=7, plane=2)), ref, "deferred move across re-sorts")


def rising_case(ndim):
    """The cloud of the_case, flying upward and placed so that the closest nodes of its top particles lie in the last but
    one node layer, nl - 2: their 5-wide stencils leave the grid by one layer while every closest node, every particle
    and every cell that is searched stays inside (the top of the block is one whole cell under the last layer and rises
    0.02 h per step)."""
    if ndim == 3:
        return make_case(3, [16, 16, 16], [4, 4, 7], [8, 8, 8], velocity=[3.0, 1.0, 10.0])
    return make_case(2, [24, 24], [4, 7], [16, 16], velocity=[3.0, 10.0])


@pytest.mark.parametrize("ndim", [3, 2])
def test_particles_whose_stencil_leaves_the_grid(ndim):
    """Particles the next lists might leave out.  bin_particle leaves a particle out (status 16) when the node layers of
    its stencil, CLAMPED to the grid, leave the node window; closest_node_update never steps outside the grid.  The
    deferred form needs the whole grid as window (async form), where the clamped stencil cannot leave it: here the case
    raises no flag at all and every particle stays listed, in both forms -- so the rule of k_search_ahead for a mark
    that K2 did not take has no particle to act on, and what this test holds is that flags, closest nodes, x and dis
    of every particle, the clipped ones included, are the serial form's."""
    case = rising_case(ndim)
    nl = case["grid_n"][ndim - 1]
    top = nl - 1  # the wall: the last node layer, inside the stencil of the top particles
    a = run(ndim, True, 6, case=case, plane=top)
    b = run(ndim, False, 6, case=case, plane=top)
    fa, fb = a.status_flags(), b.status_flags()
    sa, sb = a.download_state(), b.download_state()
    a.close()
    b.close()
    plane = int(np.prod(case["grid_n"][:ndim - 1]))
    layers = sb["I0"] // plane
    print(f"{ndim}-D: flags {fa:#x} / {fb:#x}, {int(np.sum(layers >= nl - 2))} particles with a clipped stencil")
    assert np.any(layers >= nl - 2), "no stencil leaves the grid"
    assert layers.max() <= nl - 1
    assert fa == fb, f"status flags {fa:#x} vs {fb:#x}"
    assert np.array_equal(sa["I0"], sb["I0"])
    assert np.abs(sb["dis"]).max() > 0.0
    for k in ("x", "dis"):
        assert_close(sa[k], sb[k], 1e-11, f"{k}: rising cloud")


def test_deferred_move_on_the_callers_stream():
    """After synchronising the caller's non-blocking stream alone, a read through another stream sees the moved state."""
    import torch
    ref = serial(3, 5)
    prev = torch.cuda.current_stream()
    ts = torch.cuda.Stream()
    torch.cuda.set_stream(ts)
    try:
        S = run(3, True, 5, stream=ts.cuda_stream)
        got = results(S, stream=ts)
    finally:
        torch.cuda.set_stream(prev)
    compare(got, ref, "deferred move on the caller's stream")


@pytest.mark.parametrize("nsteps", [1, 4])
def test_close_with_a_move_pending(nsteps):
    """close() straight behind a step: a move is pending and the side chain has just been joined."""
    S = run(3, True, nsteps)
    S.close()
    S2 = run(3, True, 1)  # (the device is fine)
    assert S2.status_flags() == 0
    S2.close()
