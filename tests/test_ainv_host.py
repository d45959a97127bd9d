"""Host construction of the AINV and DIAG preconditioners (gg_host_ainv,
gg_host_diag) against the plain-Python restatement (tests/ainv_ref.py).  CPU
only -- no device is touched."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import ainv_ref as R
from conftest import fixture_path
from ggmres import GGError, host as H, matrices as M

GG_EINVAL, GG_EZEROPIVOT = -1, -3


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name == "pert16":
        return R.pert(16)
    if name == "pert16x17":
        return R.pert(16, 17)                      # 272 rows: a ragged last slice
    if name == "power_law":
        return M.power_law(3000, 33000, seed=7)    # a 1,435-entry row in Z
    if name == "sherman1":
        return M.read_rua(fixture_path("sherman1.rua"))
    if name == "9pt_10x10":
        return M.read_mtx(fixture_path("9pt_10x10.mtx"))   # n < one block
    if name == "lap37x64":
        return M.laplacian_5pt(37, 64)             # 37 slices
    if name == "two_rows":
        return R.two_dense_rows(2400)              # 2400-entry rows in Z and Wt
    raise KeyError(name)


MATRICES = ["pert16", "power_law", "sherman1", "9pt_10x10", "lap37x64", "pert16x17", "two_rows"]


@functools.lru_cache(maxsize=None)
def reference(name, tol=0.1):
    """the restatement's factors, computed once and shared"""
    return R.ainv(matrix(name), tol)


def same_csr(a, b):
    return (np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and
            np.array_equal(a.data, b.data))


@pytest.mark.parametrize("name", MATRICES)
def test_host_ainv_bitexact_vs_restatement(ggmres_lib, name):
    Z, Wt, dinv = H.ainv(matrix(name), 0.1)
    Zr, Wtr, dr = reference(name)
    assert same_csr(Z, Zr), "Z"
    assert same_csr(Wt, Wtr), "Wt"
    assert np.array_equal(dinv, dr)
    assert np.all(np.isfinite(dinv))


@pytest.mark.parametrize("name", MATRICES)
def test_host_ainv_triangular_unit_diagonal(ggmres_lib, name):
    Z, Wt, _ = H.ainv(matrix(name), 0.1)
    n = Z.shape[0]
    for T, lower in ((Z, True), (Wt, False)):
        rows = np.repeat(np.arange(n), np.diff(T.indptr))
        assert np.all(T.indices <= rows) if lower else np.all(T.indices >= rows)
        assert np.all(np.diff(T.indices)[np.diff(rows) == 0] > 0)     # ascending columns
        assert np.array_equal(T.diagonal(), np.ones(n))


def test_host_ainv_exact_inverse_without_dropping(ggmres_lib):
    """tol = 0: M = Wt diag(dinv) Z is A^-1 up to rounding (the restatement gives
    2.6e-15 on this matrix; the transposed order Z^T D Wt^T gives 0.67)."""
    A = matrix("pert16")
    Z, Wt, dinv = H.ainv(A, 0.0)
    Mi = (Wt @ sp.diags(dinv) @ Z).toarray()
    dev = np.max(np.abs(Mi @ A.toarray() - np.eye(A.shape[0])))
    print(f"max|M A - I| = {dev:.3e}")
    assert dev <= 1e-10
    Zr, Wtr, dr = reference("pert16", 0.0)
    assert same_csr(Z, Zr) and same_csr(Wt, Wtr) and np.array_equal(dinv, dr)


def test_host_ainv_zero_pivot(ggmres_lib):
    with pytest.raises(GGError) as e:
        H.ainv(sp.csr_matrix(np.array([[0.0, 1.0], [1.0, 0.0]])), 0.1)
    assert e.value.code == GG_EZEROPIVOT
    with pytest.raises(R.ZeroPivot):
        R.ainv(sp.csr_matrix(np.array([[0.0, 1.0], [1.0, 0.0]])), 0.1)


@pytest.mark.parametrize("tol", [-1.0, float("nan")])
def test_host_ainv_bad_tolerance(ggmres_lib, tol):
    with pytest.raises(GGError) as e:
        H.ainv(matrix("pert16"), tol)
    assert e.value.code == GG_EINVAL


def test_numpy_gmres_matches_the_oracle():
    """The NumPy GMRES the GPU tests compare against (ainv_ref.gmres_left with
    the device-order dot) is bit-identical to the oracle's order-matched
    gmres_left when given the oracle's own ILU(0) operator."""
    import oracle as O
    from helpers import device_layout
    A = matrix("pert16")
    n = A.shape[0]
    b = A @ np.ones(n)
    L, U = O.ilu0(A)
    O.set_dot_order(*device_layout(n))
    try:
        o = O.gmres_left(A, L, U, b, m=10, max_iter=3000, tol=1e-10)     # m = 10: restarts
    finally:
        O.set_dot_order(None)
    g = R.gmres_left(A, lambda v: O.lusolve(L, U, v), b, m=10, max_iter=3000, tol=1e-10, dot=R.device_dot(n))
    assert o["ret"] == g["ret"] == 0 and o["iters"] == g["iters"] > 10 and o["inner"] == g["inner"]
    assert np.array_equal(o["hist"], g["hist"]) and np.array_equal(o["x"], g["x"])


def test_host_diag_nearest_column_first_wins(ggmres_lib):
    # row 0: diagonal present; row 1: no diagonal, columns 0 and 2 equally near
    # (the first wins); row 2: no diagonal, column 0 nearer than none else;
    # row 3: columns 1 and 2, column 2 nearer
    A = sp.csr_matrix((np.array([4.0, -1.0, 5.0, 8.0, 2.0, 3.0, -2.5]),
                       np.array([0, 3, 0, 2, 0, 1, 2], np.int32),
                       np.array([0, 2, 4, 5, 7], np.int32)), shape=(4, 4))
    inv = H.diag(A)
    assert np.array_equal(inv, 1.0 / np.array([4.0, 5.0, 2.0, -2.5]))
    assert np.array_equal(inv, R.diag_nearest(A))
    for name in ("pert16", "sherman1"):
        assert np.array_equal(H.diag(matrix(name)), R.diag_nearest(matrix(name)))
        assert np.array_equal(H.diag(matrix(name)), 1.0 / matrix(name).diagonal())


def test_host_diag_empty_row_and_zero_value(ggmres_lib):
    A = sp.csr_matrix((np.array([1.0, 2.0]), np.array([0, 2], np.int32), np.array([0, 1, 1, 2], np.int32)),
                      shape=(3, 3))
    with pytest.raises(GGError) as e:
        H.diag(A)
    assert e.value.code == GG_EZEROPIVOT
    B = sp.csr_matrix((np.array([1.0, 0.0]), np.array([0, 1], np.int32), np.array([0, 1, 2], np.int32)),
                      shape=(2, 2))
    with pytest.raises(GGError) as e:
        H.diag(B)
    assert e.value.code == GG_EZEROPIVOT
