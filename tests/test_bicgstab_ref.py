"""CPU: the NumPy restatement of the BiCGStab solve (tests/bicgstab_ref.py) and
the constants of its interface."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import bicgstab_ref as B
import oracle as O
from conftest import REPO
from ggmres import matrices as M
from helpers import rel_err


def cyclic_shift(n=272):
    """row i has a single 1 at column (i + 1) mod n"""
    A = sp.csr_matrix((np.ones(n), (np.arange(n), (np.arange(n) + 1) % n)), shape=(n, n))
    A.sort_indices()
    return A


@pytest.mark.parametrize("name", ["7pt_10_upwind", "5pt_10x10_upwind"])
def test_bicgstab_solves_nonsymmetric_grids(name):
    """ILU(0) from the oracle, NumPy dots, b = A 1, tol 1e-10: the solution is
    within 1e-8 relative of a direct solve"""
    A = M.grid_7pt(10, upwind=0.1) if name == "7pt_10_upwind" else M.laplacian_5pt(10, 10, upwind=0.2)
    assert abs(A - A.T).max() > 0.0
    n = A.shape[0]
    b = A @ np.ones(n)
    L, U = O.ilu0(A)
    ret, x, iters, relres, hist = B.bicgstab(A, lambda v: O.lusolve(L, U, v), b, None, 500, 1e-10, None)
    assert ret == 0 and 0 < iters < 100
    assert hist.size == iters + 1 and hist[-1] == relres < 1e-10
    assert np.all(hist[:-1] >= 1e-10)
    exact = spla.spsolve(A.tocsc(), b)
    assert rel_err(x, exact) <= 1e-8


def test_laplacian_5pt_upwind():
    """the default is the matrix it always was; upwind scales west by 1 + u and east by 1 - u"""
    A0 = M.laplacian_5pt(7, 5)
    A1 = M.laplacian_5pt(7, 5, upwind=0.0)
    assert np.array_equal(A0.indptr, A1.indptr) and np.array_equal(A0.indices, A1.indices)
    assert np.array_equal(A0.data, A1.data) and abs(A0 - A0.T).max() == 0.0
    A = M.laplacian_5pt(7, 5, upwind=0.2).toarray()
    assert A[8, 7] == -1.0 * (1 + 0.2) and A[8, 9] == -1.0 * (1 - 0.2)
    assert A[8, 1] == A[8, 15] == -1.0 and A[8, 8] == 4.0
    assert A[7, 6] == 0.0 and A[6, 7] == 0.0          # no wrap across the line's ends


def test_bicgstab_statuses():
    A = M.laplacian_5pt(8, 9, upwind=0.2)
    n = A.shape[0]
    b = A @ np.ones(n)
    ident = lambda v: v.copy()                               # noqa: E731
    full = B.bicgstab(A, ident, b, None, 500, 1e-10, None)
    assert full[0] == 0 and full[2] > 5
    cut = B.bicgstab(A, ident, b, None, 5, 1e-10, None)      # exhaustion: the same first entries
    assert cut[0] == 1 and cut[2] == 5 and np.array_equal(cut[4], full[4][:6])
    zero = B.bicgstab(A, ident, np.zeros(n), None, 500, 1e-10, None)
    assert zero[0] == 0 and zero[2] == 0 and zero[4].tolist() == [0.0]
    at = B.bicgstab(A, ident, b, np.ones(n), 500, 1e-10, None)    # the exact solution as x0
    assert at[0] == 0 and at[2] == 0


def test_bicgstab_breakdown_on_the_cyclic_shift():
    """b = e_0, x0 = 0, no preconditioner: r = rt = p = e_0 and v = A e_0 =
    e_271 (the only row with column 0 is the last), so rt . v is a sum of
    exact zeros in any order"""
    n = 272
    A = cyclic_shift(n)
    b = np.zeros(n)
    b[0] = 1.0
    x0 = np.zeros(n)
    ret, x, iters, relres, hist = B.bicgstab(A, lambda v: v.copy(), b, x0, 500, 1e-10, None)
    assert ret == B.BREAKDOWN and iters == 0 and np.array_equal(x, x0)
    assert hist.tolist() == [1.0] and relres == 1.0


def test_header_constants_match_python():
    import ggmres
    h = open(os.path.join(REPO, "include", "ggmres.h")).read()
    flag = re.search(r"#define\s+GG_SOLVE_BICGSTAB\s+(0x[0-9a-fA-F]+|\d+)", h)
    assert flag and int(flag.group(1), 0) == ggmres.SOLVE_BICGSTAB == 0x8
    assert ggmres.SOLVE_BICGSTAB & (ggmres.SOLVE_CG | ggmres.SOLVE_CGS2 | ggmres.SOLVE_SHARED_DEVICE) == 0
