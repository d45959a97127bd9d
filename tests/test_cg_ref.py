"""CPU: the NumPy restatement of the CG solve (tests/cg_ref.py) and the
constants of its interface."""
import os
import re

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import ainv_ref as R
import cg_ref as C
import oracle as O
from conftest import REPO, fixture_path
from ggmres import matrices as M
from helpers import device_layout, rel_err


@pytest.mark.parametrize("name", ["5pt_10x10", "7pt_10x10x10"])
def test_pcg_solves_the_fixtures(name):
    """ILU(0) from the oracle, NumPy dots, b = A 1, tol 1e-10: the solution is
    within 1e-8 relative of a direct solve"""
    A = M.read_mtx(fixture_path(name + ".mtx"))
    assert abs(A - A.T).max() == 0.0
    n = A.shape[0]
    b = A @ np.ones(n)
    L, U = O.ilu0(A)
    ret, x, iters, relres, hist = C.pcg(A, lambda v: O.lusolve(L, U, v), b, None, 500, 1e-10, None)
    assert ret == 0 and 0 < iters < 100
    assert hist.size == iters + 1 and hist[-1] == relres < 1e-10 <= hist[-2]
    exact = spla.spsolve(A.tocsc(), b)
    assert rel_err(x, exact) <= 1e-8


def test_pcg_statuses():
    A = M.laplacian_5pt(8, 9)
    n = A.shape[0]
    b = A @ np.ones(n)
    ident = lambda v: v.copy()                               # noqa: E731
    full = C.pcg(A, ident, b, None, 500, 1e-10, None)
    assert full[0] == 0
    cut = C.pcg(A, ident, b, None, 5, 1e-10, None)           # exhaustion: the same first entries
    assert cut[0] == 1 and cut[2] == 5 and np.array_equal(cut[4], full[4][:6])
    zero = C.pcg(A, ident, np.zeros(n), None, 500, 1e-10, None)
    assert zero[0] == 0 and zero[2] == 0 and zero[4].tolist() == [0.0]
    at = C.pcg(A, ident, b, np.ones(n), 500, 1e-10, None)    # the exact solution as x0
    assert at[0] == 0 and at[2] == 0
    neg = C.pcg(-A, ident, -b, None, 500, 1e-10, None)       # p.Ap < 0 in the first iteration
    assert neg[0] == C.BREAKDOWN and neg[2] == 0 and np.all(np.isfinite(neg[1]))


@pytest.mark.parametrize("n", [100, 272, 2368, 40000])
def test_layout_dot_natural_is_device_dot(n):
    """on the natural layout layout_dot is ainv_ref.device_dot, bit for bit"""
    lay2nat, G = device_layout(n)
    rng = np.random.default_rng(n)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    assert C.layout_dot(lay2nat, G)(x, y) == R.device_dot(n)(x, y)


def test_layout_dot_wavefront_layout():
    """a 2D band layout: the same products in other slots -- the exact sum of the
    products within a few ulps of their absolute sum, padding contributing nothing"""
    nx, ny = 60, 52
    lay2nat, G = device_layout(nx * ny, nx=nx)
    assert lay2nat.size > nx * ny and (lay2nat < 0).any()
    rng = np.random.default_rng(1)
    x, y = rng.standard_normal(nx * ny), rng.standard_normal(nx * ny)
    d = C.layout_dot(lay2nat, G)(x, y)
    import math
    assert abs(d - math.fsum(x * y)) <= 64 * np.finfo(float).eps * np.abs(x * y).sum()


def test_header_constants_match_python():
    import ggmres
    h = open(os.path.join(REPO, "include", "ggmres.h")).read()
    flag = re.search(r"#define\s+GG_SOLVE_CG\s+(0x[0-9a-fA-F]+|\d+)", h)
    code = re.search(r"GG_EBREAKDOWN\s*=\s*(-?\d+)", h)
    assert flag and int(flag.group(1), 0) == ggmres.SOLVE_CG == 0x4
    assert code and int(code.group(1)) == ggmres.EBREAKDOWN == C.BREAKDOWN == -8
