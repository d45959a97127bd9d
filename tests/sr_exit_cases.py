"""The exits of the CG and BiCGStab control kernels (k_cg_xr, k_cg_p, k_bi_s,
k_bi_xr, k_bi_p; csrc/kernels/short_recurrence.hip), one small system per exit.

A plain module shared by tests/test_sr_exit_cases.py (CPU: every case reaches
the exit it is named for, in two summation orders) and the GPU tests
(tests/test_gpu_sr_exits.py: the device against the restatement, bit for bit).

Each Case holds the matrix, the preconditioner kind ("none", "ilu0", or "lu"
with its factors), b, x0, the method ("cg" / "bicgstab"), the tolerance and what
the restatement must report: `why` (cg_ref.pcg / bicgstab_ref.bicgstab's
info["why"]), `ret`, and `iters` -- a count, or a (lo, hi) window for the cases
whose scalars are rounded sums (the summation order may move the iteration by
one or two; the window is a condition on the reference alone).

The exact cases are block-diagonal matrices of tiny integer or dyadic blocks:
every product and every partial sum of every dot is an exactly representable
number, so the scalars are the same in any summation order and a true zero is a
true zero on the device as well.  Their `x`, `relres` and `hist` are worked out
by hand below and checked by the CPU test.

`pq_zero` (p.Ap an exact zero, the boundary of "not > 0") and `rtv0` (the cyclic
shift of tests/test_gpu_bicgstab.py, rt.v = 0 at iteration 0) complete the set.

The non-finite cases (`rho0_inf`, `nan`) use 2 I without a preconditioner: no
inf or NaN enters a triangular solve or any other kernel that polls for a value.
"""
import functools
import math
from typing import NamedTuple, Optional

import numpy as np
import scipy.sparse as sp

import bicgstab_ref as B
import cg_ref as C
import oracle as O
from ggmres import matrices as M

BREAKDOWN = C.BREAKDOWN
BI_TOL = 1e-12
CG_TOL = 1e-10


class Case(NamedTuple):
    name: str
    method: str                     # "cg" | "bicgstab"
    A: sp.csr_matrix
    precond: str                    # "none" | "ilu0" | "lu"
    b: np.ndarray
    x0: np.ndarray
    tol: float
    why: str
    ret: int
    iters: object                   # int, or (lo, hi) inclusive for the rounded cases
    factors: Optional[tuple] = None     # (L, U) oracle CSR for "lu"
    relres: Optional[float] = None      # exact cases: the expected values
    x: Optional[np.ndarray] = None
    hist: Optional[list] = None

    @property
    def exact(self):
        return not isinstance(self.iters, tuple)

    def iters_ok(self, k):
        return k == self.iters if self.exact else self.iters[0] <= k <= self.iters[1]


def block_diag(rows, count):
    """count copies of one block on the diagonal; rows = the block's rows, each a
    list of (column, value) in ascending column order.  Entries are stored as
    given, an explicit 0.0 included"""
    m = len(rows)
    rp, ci, v = [0], [], []
    for k in range(count):
        for row in rows:
            for c, val in row:
                ci.append(k * m + c)
                v.append(float(val))
            rp.append(len(ci))
    return sp.csr_matrix((np.array(v), np.array(ci, np.int32), np.array(rp, np.int32)), shape=(m * count,) * 2)


def _dense_rows(block):
    return [[(c, val) for c, val in enumerate(row) if val != 0] for row in block]


def _shifted(A, sigma):
    S = (sp.csr_matrix(A) - sigma * sp.identity(A.shape[0], format="csr")).tocsr()
    S.sort_indices()
    return S


def _negated(A):
    S = (-sp.csr_matrix(A)).tocsr()
    S.sort_indices()
    return S


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case"""
    out = []
    n2, n3 = 272, 273
    z2, z3 = np.zeros(n2), np.zeros(n3)

    # ---- BiCGStab, no preconditioner, tol 1e-12, x0 = 0 ----------------------
    # [[1,1],[0,0]] with b = (1,1): r = rt = p = (1,1), v = (2,0), alpha = 1,
    # s = (-1,1), t = A s = 0, tt = 0 -> omega = 0; x = p, r = s, res = 1, and
    # rt.r = 0 as well: omega is the scalar that gets named
    oblique = block_diag([[(0, 1.0), (1, 1.0)], [(1, 0.0)]], 136)
    out.append(Case("omega", "bicgstab", oblique, "none", np.ones(n2), z2, BI_TOL, "omega", BREAKDOWN, 1,
                    relres=1.0, x=np.ones(n2), hist=[1.0, 1.0]))
    # alpha = omega = -1/2, r = (-1/4, 0, 1/4) after the first iteration: rt.r = 0
    rho_mid = block_diag(_dense_rows([[-1, -1, -1], [-1, -1, 0], [0, 0, -1]]), 91)
    out.append(Case("rho_mid", "bicgstab", rho_mid, "none", np.ones(n3), z3, BI_TOL, "rho", BREAKDOWN, 1,
                    relres=0.35355339059327384, x=np.tile([-0.25, -0.5, -0.75], 91),
                    hist=[1.0, 0.35355339059327384]))
    # the first iteration moves everything; rt.v = 0 in the second
    rtv_mid = block_diag(_dense_rows([[-1, -1, -1], [-1, -1, -1], [0, 0, -1]]), 91)
    out.append(Case("rtv_mid", "bicgstab", rtv_mid, "none", np.tile([1.0, 0.0, 0.0], 91), z3, BI_TOL, "rtv",
                    BREAKDOWN, 1, relres=0.7071067811865476, x=np.tile([-1.0, 0.5, 0.0], 91),
                    hist=[1.0, 0.7071067811865476]))
    # 2 I: alpha = 1/2, s = 0 exactly at the half step, t = 0, omega = 0 -- and
    # the solve has converged: convergence is tested before breakdown
    two_i = block_diag([[(0, 2.0)]], n2)
    out.append(Case("lucky", "bicgstab", two_i, "none", np.full(n2, 3.0), z2, BI_TOL, "conv", 0, 1,
                    relres=0.0, x=np.full(n2, 1.5), hist=[1.0, 0.0]))
    # the omega matrix with b = (1,0): v = p = r, alpha = 1, s = 0, omega = 0, converged
    out.append(Case("lucky_oblique", "bicgstab", oblique, "none", np.tile([1.0, 0.0], 136), z2, BI_TOL, "conv", 0, 1,
                    relres=0.0, x=np.tile([1.0, 0.0], 136), hist=[1.0, 0.0]))
    # r.r overflows: normb = inf, res0 = inf / inf, rho = inf at the start
    out.append(Case("rho0_inf", "bicgstab", two_i, "none", np.full(n2, 1e200), z2, BI_TOL, "rho0", BREAKDOWN, 0,
                    relres=math.nan, x=z2, hist=[math.nan]))
    # the cyclic shift, b = e_0: every product of rt . v is an exact zero at iteration 0
    shift = sp.csr_matrix((np.ones(n2), (np.arange(n2), (np.arange(n2) + 1) % n2)), shape=(n2, n2))
    shift.sort_indices()
    e0 = np.zeros(n2)
    e0[0] = 1.0
    out.append(Case("rtv0", "bicgstab", shift, "none", e0, z2, BI_TOL, "rtv", BREAKDOWN, 0,
                    relres=1.0, x=z2, hist=[1.0]))

    # ---- CG, tol 1e-10, x0 = 0 -------------------------------------------------
    lap = sp.csr_matrix(M.laplacian_5pt(16, 17))
    lap.sort_indices()
    neg = _negated(lap)
    rnd = np.random.default_rng(1).standard_normal(n2)
    # negative definite, no preconditioner: r.z = r.r > 0 at the start, p.Ap < 0
    # in the first iteration -- k_cg_xr's exit, nothing has moved
    out.append(Case("pq0", "cg", neg, "none", neg @ np.ones(n2), z2, CG_TOL, "pq", BREAKDOWN, 0))
    # [[0,1],[1,0]] with b = (1,0): p = r = (1,0), q = (0,1), every product of p.Ap
    # an exact zero -- the boundary of "not > 0" (a kernel testing pq < 0 goes on)
    swap = block_diag([[(1, 1.0)], [(0, 1.0)]], 136)
    out.append(Case("pq_zero", "cg", swap, "none", np.tile([1.0, 0.0], 136), z2, CG_TOL, "pq", BREAKDOWN, 0,
                    relres=1.0, x=z2, hist=[1.0]))
    # indefinite shifts of the grid: p.Ap turns negative after x and r have moved
    # (iteration 6, p.Ap = -1157.6; iteration 17, p.Ap = -8.6e4 with plain dots)
    out.append(Case("pq_mid", "cg", _shifted(lap, 0.3), "none", rnd, z2, CG_TOL, "pq", BREAKDOWN, (4, 8)))
    out.append(Case("pq_late", "cg", _shifted(lap, 0.07), "none", rnd, z2, CG_TOL, "pq", BREAKDOWN, (14, 20)))
    # an indefinite M = diag(1 / d), d = 1 except -1 at every 40th row, given as
    # the factors L = I, U = diag(d): r.z turns negative (iteration 2, r.z = -18.5)
    d = np.ones(n2)
    d[39::40] = -1.0
    eye = O.csr(sp.identity(n2, format="csr"))
    out.append(Case("rz_mid", "cg", lap, "lu", rnd, z2, CG_TOL, "rz", BREAKDOWN, (1, 4),
                    factors=(eye, O.csr(sp.diags(d).tocsr()))))
    # ILU(0) of a negative definite matrix is negative definite: r.z < 0 at the start
    out.append(Case("rz0", "cg", neg, "ilu0", neg @ np.ones(n2), z2, CG_TOL, "rz0", BREAKDOWN, 0))
    # r.r, r.z and p.Ap overflow to inf (> 0: no exit), alpha = inf / inf, x and
    # r all NaN, r.z = NaN: "NaN counts as not > 0" in k_cg_p
    out.append(Case("nan", "cg", two_i, "none", np.full(n2, 1e200), z2, CG_TOL, "rz", BREAKDOWN, 1,
                    relres=math.nan, x=np.full(n2, math.nan), hist=[math.nan, math.nan]))
    return {c.name: c for c in out}


def names(method=None):
    return [k for k, c in cases().items() if method in (None, c.method)]


def minv(case):
    """the restatement's preconditioner of a case"""
    if case.precond == "none":
        return lambda v: np.array(v, np.float64, copy=True)
    if case.precond == "ilu0":
        L, U = O.ilu0(case.A)
    else:
        L, U = case.factors
    return lambda v: O.lusolve(L, U, v)


def reference(case, dot=None, max_iter=3000, info=None):
    """the restatement's (ret, x, iters, relres, hist) of a case with the dots in `dot`"""
    run = C.pcg if case.method == "cg" else B.bicgstab
    return run(case.A, minv(case), case.b, case.x0, max_iter, case.tol, dot, info=info)


def configure(solver, case):
    """the case's matrix and preconditioner on a ggmres.Solver"""
    solver.set_matrix(case.A)
    if case.precond == "lu":
        solver.set_precond_lu(*case.factors)
    else:
        getattr(solver, "set_precond_" + case.precond)()
