"""The cases of the device MINRES tests (tests only), described once for tests/test_minres_ref.py (the numpy reference alone on
the CPU oracle's matrices: the conditions) and tests/test_gpu_minres.py (the device beside that reference on the dense
matrix of its own COO).  Neo-Hookean throughout, Dirichlet rows on; the clouds are solver_exit_cases.linearised_* and wide_*.

The iteration-count margins are max(2, 3 x spread), spread = the largest difference among the reference's own counts on
K, b and eight copies moved by one relative eps (test_minres_ref.perturbed_counts): what two orders of summation do to a
long short-recurrence solve.  Measured:
  GAP         3-D, alpha_1 = 10, rtol 1e-5, about 230 steps: counts 229 .. 233, spread 3 on eight copies (4 on another four)
  INDEFINITE  3-D, alpha_1 = 0, rtol 1e-5, about 200 steps: jacobi 203 .. 205, pbjacobi 189 .. 190, spread 2
  WIDE        2-D n = 1610, alpha_1 = 10, rtol 1e-8: jacobi 211 eight times, pbjacobi 220 .. 221, spread 1
  DENSE       alpha_1 = 4e4, rtol 1e-10, 12 to 14 steps: spread 0 (held to "within 1", no margin)
No function here calls a solver under test."""
import numpy as np

ALPHA_DYNAMIC = 4.0e4
PCS = ("none", "jacobi", "pbjacobi")

# 1. the dynamic regime against a dense solve
DENSE = dict(alpha_1=ALPHA_DYNAMIC, rtol=1e-10, seed=5,
             # without a preconditioner the identity rows beside the stiffness stall the true residual near 2e-9 ||b||
             # (reference: x is within 1e-9 of the dense solve from step 500 on): both sides run to max_it
             max_it={"none": 800, "jacobi": 2000, "pbjacobi": 2000})
# 2. where GMRES(30) does not get there: the seed is one at which the reference GMRES(30) is above tol after 1500 steps
GAP = dict(alpha_1=10.0, rtol=1e-5, seed=23, margin=12, pcs=("jacobi", "pbjacobi"))
# 3. an indefinite tangent, b = K x_true
INDEFINITE = dict(alpha_1=0.0, rtol=1e-5, seed=6, margin=6, pcs=("jacobi", "pbjacobi"))
# 4. several 512-element tiles with a ragged tail
WIDE = dict(alpha_1=10.0, rtol=1e-8, seed=31, margin=3, pcs=("jacobi", "pbjacobi"), counts={"jacobi": 211, "pbjacobi": 221})
# 6. a Jacobi preconditioner that is not positive definite: alpha_1 so far below zero that every free diagonal entry of
# K = stiffness + alpha_1 M is negative, while the Dirichlet rows keep their 1.  b on the free dofs only: r0 . M^-1 r0 < 0.
NEGATIVE_ALPHA = -4.0e8
SEED_INDEFINITE_PC = 17


def rhs(n, seed):
    return np.random.default_rng(seed).normal(size=n)


def free_dof_rhs(d2m, seed):
    """normal deviates on the free dofs (d2m != -1), exactly 0 on the fixed ones"""
    b = np.random.default_rng(seed).normal(size=d2m.shape[0])
    b[d2m == -1] = 0.0
    return b


def history_error(h, href, count=10):
    """the GMRES tests' measure over the first `count` entries"""
    k = min(count, len(h), len(href))
    return float((np.abs(h[:k] - href[:k]) / np.maximum(href[:k], 1e-12 * href[0])).max())
