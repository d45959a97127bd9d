"""GPU: GMRES, CG and BiCGStab read their control blocks back through one pair
of pinned slots on the solver (csrc/gg_solver.h ReadPipe).  Solves of the three
methods in turn on one solver, profiled, must each give the bits and the
profile counts of the same solve on a fresh solver.

The matrix is the 60 x 52 five-point grid with ILU(0).  Serial-order CPU
restatements give 121 iterations for GMRES(10) at tol 1e-10 (more than twelve
restart cycles), 75 for CG and 53 for BiCGStab at tol 1e-12: every method
posts to both slots several times, which the test asserts so that it cannot
pass without slot reuse.
"""
import numpy as np
import pytest

import ggmres
from ggmres import matrices as M

pytestmark = pytest.mark.gpu
CG, BICGSTAB = ggmres.SOLVE_CG, ggmres.SOLVE_BICGSTAB
CHUNK = {CG: 32, BICGSTAB: 16}      # csrc/cg.hip Cg::kChunk, csrc/bicgstab.hip BiCgStab::kChunk
KINDS = (ggmres.PROF_SPMV, ggmres.PROF_PRECOND, ggmres.PROF_MGS)
SOLVES = [("GMRES(10)", dict(restart=10, tol=1e-10)),
          ("CG", dict(tol=1e-12, flags=CG)),
          ("BiCGStab", dict(tol=1e-12, flags=BICGSTAB)),
          ("GMRES(10) again", dict(restart=10, tol=1e-10))]


def make(A):
    s = ggmres.Solver(0)
    s.set_matrix(A)
    s.set_precond_ilu0()
    s.profile(True)
    return s


def counts(s):
    return np.array([s.profile_get(k)[0] for k in KINDS])


def test_methods_in_turn_on_one_solver_match_fresh_solvers():
    A = M.laplacian_5pt(60, 52)
    b = A @ np.ones(A.shape[0])
    fresh = []
    for _, kw in SOLVES[:3]:
        s = make(A)
        try:
            fresh.append((s.solve(b, max_iter=3000, **kw), counts(s)))
        finally:
            s.close()
    fresh.append(fresh[0])
    s = make(A)
    try:
        before = counts(s)
        for (what, kw), (f, fc) in zip(SOLVES, fresh):
            g = s.solve(b, max_iter=3000, **kw)
            after = counts(s)
            gc, before = after - before, after
            print(f"{what}: ret {g['ret']} iters {g['iters']} restarts {g['restarts']} relres {g['relres']:.3e} "
                  f"counts {gc.tolist()}; fresh iters {f['iters']} restarts {f['restarts']} counts {fc.tolist()}")
            flags = kw.get("flags", 0)
            if flags:
                assert f["iters"] > 2 * CHUNK[flags], what
            else:
                assert f["restarts"] > 2, what
            assert g["ret"] == f["ret"] == 0, what
            for k in ("iters", "inner", "restarts", "relres"):
                assert g[k] == f[k], (what, k)
            assert np.array_equal(g["hist"], f["hist"]), what
            assert np.array_equal(g["x"], f["x"]), what
            assert np.array_equal(gc, fc), what
            assert fc[0] > 0 and fc[1] > 0 and (fc[2] > 0) == (flags == 0), what
    finally:
        s.close()
