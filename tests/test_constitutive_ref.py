"""The CPU oracle's closed-form laws and its eigen-solver against the 50-digit statement of tests/constitutive_ref.py, over
every family of deformation gradients, in 2-D and 3-D.

This is the evidence that the bound of constitutive_ref (C_BOUND units of 2^-52 cond(b) s) is achievable by a correct
double-precision implementation -- the oracle's cyclic Jacobi and LAPACK's eigh both keep it -- and the first check of the
oracle's eigen-solver against a decomposition that is neither a Jacobi iteration nor done in double.  The oracle has no
fluid law (Constitutive.c:84-108 is restated in tests/fluid_ref.py): that numpy statement stands in its place.
`python tests/test_constitutive_ref.py` prints the table of DESIGN.md §2."""
import numpy as np
import pytest

import constitutive_ref as cr
import fluid_ref
from util import orc

pytestmark = pytest.mark.skipif(cr.mp is None, reason=cr.MP_SKIP)

EPS = cr.EPS


def oracle_law(law, r, ndim):
    """(status, tau[T], W or None) of the double-precision implementation under test for case r"""
    mat = cr.MATERIAL[law]
    if law == "fluid":
        return 0, fluid_ref.stress(mat, cr.tensor_row(r["F"], ndim), cr.tensor_row(r["dtF"], ndim, 0.0), r["J"], ndim), None
    o = orc()
    Frow = cr.tensor_row(r["F"], ndim)
    st, tau, W, _, _, _ = o.stress_one(ndim, o.make_materials([mat])[0], o.default_params(), Frow, cr.tensor_row(np.eye(ndim), ndim),
                                       r["J"], cr.tensor_row(np.eye(ndim), ndim), 0.0, 0.0)
    return st, tau, W


def worst_units(law, ndim, which):
    """worst error (units of the bound) over the families, with the case's name: which = "oracle" or "numpy" """
    mat = cr.MATERIAL[law]
    worst, name = 0.0, ""
    for r in cr.references(law, ndim):
        if which == "oracle":
            st, tau, W = oracle_law(law, r, ndim)
            assert st == 0, f"{law} {ndim}-D {r['name']}: the oracle returns status {st}"
        else:
            tau, W = cr.numpy_law(law, mat, r["F"], r["J"], r["dtF"], ndim)
        e = max(cr.error_units(law, mat, r, tau, W))
        if e > worst or not np.isfinite(e):
            worst, name = e, r["name"]
    return worst, name


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("law", cr.LAWS)
def test_oracle_law_meets_the_50_digit_statement(law, ndim):
    worst, name = worst_units(law, ndim, "oracle")
    print(f"{law} {ndim}-D: worst {worst:.3g} units at {name} (bound {cr.C_BOUND[law, ndim]:g})")
    assert worst <= cr.C_BOUND[law, ndim], f"{law} {ndim}-D: {worst:.3g} units of 2^-52 cond(b) s at {name}"


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("law", cr.LAWS)
def test_lapack_law_meets_the_50_digit_statement(law, ndim):
    worst, name = worst_units(law, ndim, "numpy")
    print(f"{law} {ndim}-D: worst {worst:.3g} units at {name} (bound {cr.C_BOUND[law, ndim]:g})")
    assert worst <= cr.C_BOUND[law, ndim], f"{law} {ndim}-D: {worst:.3g} units of 2^-52 cond(b) s at {name}"


@pytest.mark.parametrize("ndim", [2, 3])
def test_oracle_sym_eigen_on_every_case(ndim):
    """orc.sym_eigen on the double b of every case: orthonormal vectors, ascending values, values within 16 eps |b| of the
    eigenvalues of the b formed at 50 digits (forming b in double costs at most ndim eps |b| of that)."""
    o = orc()
    for name, F in cr.families(ndim):
        b = F @ F.T
        st, w, V = o.sym_eigen(b)
        assert st == 0, name
        assert np.linalg.norm(V.T @ V - np.eye(ndim), 2) <= 16 * EPS, f"{name}: eigenvectors not orthonormal"
        assert np.all(np.diff(w) >= 0.0), f"{name}: eigenvalues not ascending"
        w_ref, normb = cr.eigen_reference(F, ndim)
        assert cr.abs_error(w, w_ref) <= 16 * EPS * normb, f"{name}: eigenvalues {w}"
        # and the vectors belong to the matrix it was given: the backward error of a Jacobi iteration is a few eps |b|
        # per rotation, at most 3 rotations in each of about 10 sweeps
        assert np.max(np.abs((V * w) @ V.T - b)) <= 64 * EPS * normb, f"{name}: V w V^T != b"


def test_case_families_are_what_they_claim():
    """the equal-diagonal family really meets the eigen-solver with df == 0 and an off-diagonal whose square underflows"""
    n = 0
    for name, F in cr.families(3):
        if not name.startswith("f:"):
            continue
        b = F @ F.T
        # (below 1.5e-154 the square is subnormal or zero: it has lost bits or all of them)
        pairs = [(i, j) for i in range(3) for j in range(i + 1, 3) if b[i, i] == b[j, j] and 0.0 < abs(b[i, j]) < 1.5e-154]
        assert len(pairs) == 1, name
        assert np.max(np.abs(b - np.diag(np.diag(b)))) == 0.1 * 1.0, name
        n += 1
    assert n == 36
    conds = {name: np.linalg.cond(F @ F.T) for name, F in cr.families(3) if name.startswith("d:")}
    assert [round(np.log10(conds[f"d:s={s:g}"])) for s in (10.0, 100.0, 1000.0)] == [4, 8, 12]
    assert len(cr.shuffled_cloud(len(cr.families(3)))) == 3 * 64 + 7


if __name__ == "__main__":  # the table of DESIGN.md §2
    print("| law | ndim | worst oracle | at | worst numpy/LAPACK | at | c |")
    print("|---|---|---|---|---|---|---|")
    for law in cr.LAWS:
        for ndim in (2, 3):
            wo, no = worst_units(law, ndim, "oracle")
            wn, nn = worst_units(law, ndim, "numpy")
            print(f"| {law} | {ndim} | {wo:.3g} | {no} | {wn:.3g} | {nn} | {cr.C_BOUND[law, ndim]:g} |")
