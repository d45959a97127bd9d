"""The orthogonalization launch's tail: the Hessenberg column rotated on chip as
its entries arrive (kernels/arnoldi.h givens_absorb / givens_finish / givens_column,
the cs / sn preload of k_arnoldi_persist), and the launches gated off around it.

Every case compares x, the result record (ret, iters, inner, restarts, relres)
and the whole residual history BIT FOR BIT with the order-matched oracle
(helpers.device_layout, the device's division restated by oracle.set_div_mode):
the change reorders memory accesses, never arithmetic.

ILU(0) on the 60 x 52 grid and on C1 (100 x 100), with GG_DIV_FMA and with the
exact division:
  * restart lengths 1 (no stored rotation, gen_rot only), 2 (one), 30, and 33 /
    70 (the cs / sn preload spans more than 32 entries / more than its 64 LDS
    entries: C1 runs indices up to 69, whose rotations 64.. come from memory);
  * convergence in mid-cycle with cycle pipelining on: the launches enqueued
    behind the converged iteration run gated off (the `done` half of the gate);
  * max_iter = 7 at restart 30: the `nit` half of the gate;
  * after each of those two a second solve with another right-hand side on the
    same solver equals a fresh solver's bits -- the gated launches left granules,
    election words, flags and LDS alone;
  * a diagonal system (M^-1 A = I): hn = 0 at i = 0, inv = 0, v_1 = 0.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import ggmres
import oracle as O
from ggmres import matrices as M
from helpers import device_layout

pytestmark = pytest.mark.gpu

GRIDS = {"60x52": (60, 52), "c1_100x100": (100, 100)}
DIVS = {"fma": ggmres.DIV_FMA, "exact": ggmres.DIV_EXACT}
_MODE = {ggmres.DIV_EXACT: 0, ggmres.DIV_RCP: 1, ggmres.DIV_FMA: 2}


def record(r):
    return (r["ret"], r["iters"], r["inner"], r["restarts"], r["relres"])


def check_bits(g, o):
    assert (g["ret"], g["iters"], g["inner"]) == (o["ret"], o["iters"], o["inner"])
    for key in ("restarts", "relres"):
        if key in o:
            assert g[key] == o[key], key
    assert np.array_equal(g["hist"], o["hist"])
    assert np.array_equal(g["x"], o["x"])


def same_bits(a, b):
    assert record(a) == record(b)
    assert np.array_equal(a["hist"], b["hist"])
    assert np.array_equal(a["x"], b["x"])


class System:
    """one grid with one division: the matrix, its factors, a solver set up on
    it and the oracle in the solver's order (shared by the module's tests)"""

    def __init__(self, grid, div):
        self.nx, self.ny = GRIDS[grid]
        self.A = M.laplacian_5pt(self.nx, self.ny)
        self.n = self.A.shape[0]
        self.L, self.U = O.ilu0(self.A)
        self.div = DIVS[div]
        self.s = self.new_solver()
        self.mul = (_MODE[self.s.division_active(0)], _MODE[self.s.division_active(1)])

    def new_solver(self):
        s = ggmres.Solver(0)
        s.set_division(self.div)
        s.set_matrix(self.A)
        s.set_precond_ilu0()
        assert s.uses_wavefront
        return s

    def oracle(self, b, **kw):
        O.set_dot_order(*device_layout(self.n, self.nx))
        O.set_div_mode(*self.mul)
        try:
            return O.gmres_left(self.A, self.L, self.U, b, **kw)
        finally:
            O.set_dot_order(None)
            O.set_div_mode()

    def rhs(self, which):
        return M.rhs_ones(self.A) if which == 0 else M.rhs_uniform(self.n)


_systems = {}


@pytest.fixture(params=[(g, d) for g in sorted(GRIDS) for d in sorted(DIVS)], ids=lambda p: f"{p[0]}-{p[1]}")
def system(request):
    if request.param not in _systems:
        _systems[request.param] = System(*request.param)
    return _systems[request.param]


@pytest.fixture(scope="module", autouse=True)
def _close_solvers():
    yield
    for sy in _systems.values():
        sy.s.close()
    _systems.clear()


@pytest.mark.parametrize("m", [1, 2, 30, 33, 70])
def test_restart_lengths(system, m):
    """(max_iter bounds the short restarts, which do not converge: ret = 1)"""
    b = system.rhs(0)
    kw = dict(max_iter=150, tol=1e-10)
    g = system.s.solve(b, restart=m, **kw)
    assert system.s.mgs_kernel().startswith("k_arnoldi_persist<")
    check_bits(g, system.oracle(b, m=m, **kw))


def _then_second_solve(system, kw):
    """a second solve, another right-hand side, on the solver the gated launches
    ran on: a fresh solver's bits, and the oracle's"""
    b2 = system.rhs(1)
    g2 = system.s.solve(b2, **kw)
    fresh = system.new_solver()
    try:
        f2 = fresh.solve(b2, **kw)
    finally:
        fresh.close()
    same_bits(g2, f2)
    check_bits(g2, system.oracle(b2, m=kw["restart"], max_iter=kw["max_iter"], tol=kw["tol"]))


def test_converged_mid_cycle_gates_the_rest(system):
    """a loose tolerance met well below index m - 1: the rest of the enqueued
    cycle (and the cycle pipelined behind it) runs gated off"""
    b = system.rhs(0)
    # (the oracle meets 1e-2 at index 16 of the first cycle on the small grid,
    # 1e-3 at index 6 of the second on C1)
    kw = dict(restart=30, max_iter=3000, tol=1e-2 if system.nx == 60 else 1e-3)
    g = system.s.solve(b, **kw)
    o = system.oracle(b, m=30, max_iter=3000, tol=kw["tol"])
    assert g["ret"] == 0 and 5 <= (g["inner"] - 1) % 30 <= 20, g["inner"]   # mid-cycle
    check_bits(g, o)
    _then_second_solve(system, kw)


def test_max_iter_cuts_the_cycle(system):
    b = system.rhs(0)
    kw = dict(restart=30, max_iter=7, tol=1e-10)
    g = system.s.solve(b, **kw)
    assert g["ret"] == 1 and g["iters"] == 7
    check_bits(g, system.oracle(b, m=30, max_iter=7, tol=1e-10))
    _then_second_solve(system, kw)


@pytest.mark.parametrize("div", sorted(DIVS))
def test_diagonal_system(div):
    """A = 2 I on a 64 x 64 grid, b = ones: v_0 = 1/64 exactly, <w, v_0> = 1,
    w - v_0 = 0, so hn = 0 at i = 0 (gen_rot's dy == 0 branch, inv = 0, v_1 = 0)
    and the residual is 0"""
    nx = 64
    A = sp.csr_matrix(2.0 * sp.identity(nx * nx, format="csr"))
    A.sort_indices()
    n = A.shape[0]
    b = np.ones(n)
    L, U = O.ilu0(A)
    s = ggmres.Solver(0)
    try:
        s.set_division(DIVS[div])
        s.set_matrix(A)
        s.set_precond_ilu0()
        mul = (_MODE[s.division_active(0)], _MODE[s.division_active(1)])
        lay = s.layout()
        g = s.solve(b, restart=30, max_iter=100, tol=1e-10)
    finally:
        s.close()
    O.set_dot_order(*lay)
    O.set_div_mode(*mul)
    try:
        o = O.gmres_left(A, L, U, b, m=30, max_iter=100, tol=1e-10)
    finally:
        O.set_dot_order(None)
        O.set_div_mode()
    assert g["ret"] == 0 and g["inner"] == 1 and g["hist"][-1] == 0.0
    check_bits(g, o)
    assert np.array_equal(g["x"], np.full(n, 0.5))
