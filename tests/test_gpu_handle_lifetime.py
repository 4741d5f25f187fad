"""A handle gives back what it took: rounds of create / use / close in one process do not lower the free device memory.

Every round touches each lazily allocated family of the handle (the re-sort twin, the canonical lists, the Dirichlet
sets, the staging of host vectors, the assembled tangent and its per-call temporaries, the matrix-free operator, the
GMRES, Newton and Newmark work vectors with their pinned words, the temporaries of shape_functions) and closes it.

What the figure is: free memory after round 2 minus free memory after round 40 (torch.cuda.mem_get_info).  The
block the owning types were introduced over, phase_d (128 KiB, allocated at create and missing from the old free
list), exists only in developer builds with -DNLPS_PHASE_TIMING=1, so the product build before the owning types loses
nothing through it and a quarter of its loss is no usable bound; that the block is freed now follows from the code
alone (it is a DevBuf member like the others).  BOUND_MIB is therefore the guard against large leaks: 1 MiB over 38
handles, which a block of 32 KiB or more kept per handle (38 x 32 KiB = 1.19 MiB) trips."""
import numpy as np
import pytest

from test_gpu_newton_solve import DRIVER, _alpha, _problem, _Step
from util import gpu_setup

pytestmark = pytest.mark.gpu

MIB = float(1 << 20)
BOUND_MIB = 1.0
ROUNDS = 40


def one_round():
    case, bcs, gravity, nsteps = _problem(2)
    dt = 1.0e-2
    alpha = _alpha(dt)
    S = gpu_setup(case, nsteps=nsteps)  # (initialise_shapefun)
    S.set_resort_interval(1)
    for _ in range(2):  # the second step re-sorts: the twin of the field block is made and swapped in
        S.explicit_step(bcs, 0, 1.0e-4, gravity=gravity)
    st = _Step(S, bcs, 0, alpha, gravity)  # local search, active_masks, M, Un_dt, Un_dt2
    R = S.lagrangian_evaluation(np.zeros(st.n), st.V, st.A, st.M, alpha, gravity)
    rows, cols, vals = S.jacobian_evaluation(alpha[0], st.M, True)
    pat = S.create_sparsity_pattern()
    S.tangent_operator(alpha[0], st.M, True)
    blocks = S.tangent_block_diagonal()
    x, ksp = S.tangent_solve(R, pc="pbjacobi")
    info = S.newmark_step(bcs, 0, dt, gravity, ksp=DRIVER)
    N, dN = S.shape_functions()
    # (the calls are checked where they are tested; here they only have to have run)
    assert np.isfinite(R).all() and vals.size == rows.size == cols.size > 0 and pat.size == st.n
    assert blocks.shape[0] == S.nactive and ksp["reason"] > 0 and np.isfinite(x).all()
    assert info["reason"] > 0 and N.shape[0] == dN.shape[0] == S.np
    S.close()


def loss_over_rounds(rounds=ROUNDS):
    """free memory after round 2 minus free memory after the last round, in bytes (rounds 1 and 2 absorb the runtime's
    own first-use allocations: code objects, hipcub, torch's context)"""
    import torch
    free2 = None
    for r in range(1, rounds + 1):
        one_round()
        torch.cuda.synchronize()
        if r == 2:
            free2 = torch.cuda.mem_get_info()[0]
    return free2 - torch.cuda.mem_get_info()[0]


def test_forty_handles_give_their_memory_back():
    loss = loss_over_rounds()
    print("free memory after round 2 minus after round %d: %.3f MiB (bound %.3f MiB)" % (ROUNDS, loss / MIB, BOUND_MIB))
    assert loss <= BOUND_MIB * MIB, "%d handles kept %.3f MiB of device memory (bound %.3f MiB)" % (
        ROUNDS - 2, loss / MIB, BOUND_MIB)
