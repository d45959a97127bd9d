"""GPU: the many-RHS BiCGStab solve (gg_solve_bicgstab_batch*,
gg_transient_bicgstab_batch; gpu-gmres_amd/csrc/bicgstab_batch.hip).

The batch's contract is tests/test_gpu_cg_batch.py's: every scenario is exactly
the single-RHS solve, here gg_solve(GG_SOLVE_BICGSTAB) on the same solver --
status, iteration count, relres, residual history and solution are
bit-identical (np.array_equal, NaN equal to NaN for relres and history) to the
single BiCGStab solve on that right-hand side alone, which
tests/test_gpu_bicgstab.py pins to the restatement tests/bicgstab_ref.py; one
test checks the batch against that restatement directly.  Exact division unless
a case says otherwise.

The cases are tests/bi_batch_cases.py's; tests/test_bicgstab_batch_cases.py
holds the restatement with plain dots to the counts named in comments here.
The device's reduction order may move a count, so every assertion on a count
is made on the single solves the test runs itself, never on the batch.
"""
import ctypes

import numpy as np
import pytest

import bi_batch_cases as K
import bicgstab_ref as R
import cg_ref as C
import ggmres
import oracle as O
from ggmres import matrices as M

pytestmark = pytest.mark.gpu
BI = ggmres.SOLVE_BICGSTAB
CG = ggmres.SOLVE_CG


def make(A, kind="ilu0", division=ggmres.DIV_EXACT):
    s = ggmres.Solver(0)
    s.set_matrix(A)
    if kind == "ainv":
        s.set_precond_ainv(0.1)
    else:
        getattr(s, "set_precond_" + kind)()
    s.set_division(division)
    return s


def singles(s, B, X0, max_iter=3000, tol=1e-10):
    return [s.solve(B[q], x0=X0[q], max_iter=max_iter, tol=tol, flags=BI) for q in range(B.shape[0])]


def same_as_singles(g, ref, what):
    """every scenario of the batch g against its single solve"""
    S = len(ref)
    assert len(g["status"]) == S and g["x"].shape[0] == S and len(g["hist"]) == S, what
    for q, r in enumerate(ref):
        assert (g["status"][q], g["iters"][q], g["inner"][q], g["restarts"][q]) == \
               (r["ret"], r["iters"], r["iters"], 0), (what, q)
        assert np.array_equal(g["relres"][q], r["relres"], equal_nan=True), (what, q)
        assert np.array_equal(g["hist"][q], r["hist"], equal_nan=True), (what, q)
        assert np.array_equal(g["x"][q], r["x"]), (what, q)
    stat = [r["ret"] for r in ref]
    want = ggmres.EBREAKDOWN if ggmres.EBREAKDOWN in stat else (1 if 1 in stat else 0)
    assert g["ret"] == want, what


def same_batches(g, f, what):
    """a batch against another batch (a fresh solver's)"""
    assert g["ret"] == f["ret"], what
    for k in ("status", "iters", "inner", "restarts"):
        assert g[k] == f[k], (what, k)
    assert np.array_equal(g["relres"], f["relres"], equal_nan=True), what
    assert len(g["hist"]) == len(f["hist"]), what
    for q in range(len(f["hist"])):
        assert f["hist"][q].size > 0 and np.array_equal(g["hist"][q], f["hist"][q], equal_nan=True), (what, q)
    assert np.array_equal(g["x"], f["x"]), what


@pytest.mark.parametrize("division", [ggmres.DIV_EXACT, ggmres.DIV_FMA, ggmres.DIV_RCP])
@pytest.mark.parametrize("max_iter,tol", [(3000, 1e-10),     # converges: 31 .. 34 cold, 0 for b = 0, 21 and 11 warm
                                          (3000, 0.05),      # 9 .. 17, 0 warm: gated launches behind every end
                                          (6, 1e-300)])      # max_iter cuts every scenario
def test_bicgstab_batch_bitexact_vs_single(max_iter, tol, division):
    A, B, X0 = K.band()
    s = make(A, division=division)
    try:
        assert s.uses_wavefront and s.batch_engine
        ref = singles(s, B, X0, max_iter, tol)
        counts = [r["iters"] for r in ref]
        print(f"division {division} max_iter {max_iter} tol {tol}: single-solve counts {counts}")
        if tol == 1e-10:
            # scenarios end several chunks of the read-back apart while others go on
            assert all(r["ret"] == 0 for r in ref)
            assert K.diverse(counts)
        elif tol == 0.05:
            assert all(r["ret"] == 0 for r in ref) and 0 < max(counts) < 32
        else:
            for q, r in enumerate(ref):
                assert (r["ret"], r["iters"]) == ((1, 6) if np.any(B[q]) else (0, 0)), q
        g = s.solve_bicgstab_batch(B, X0, max_iter=max_iter, tol=tol)
        same_as_singles(g, ref, "S = 9")
        assert g["ret"] == (1 if tol == 1e-300 else 0)
        for k in (1, 2):                                # one scenario; a pair
            # flags 0 means BiCGStab too
            gk = s.solve_bicgstab_batch(B[:k], X0[:k], max_iter=max_iter, tol=tol, flags=0)
            same_as_singles(gk, ref[:k], f"S = {k}")
    finally:
        s.close()


def test_bicgstab_batch_bitexact_vs_restatement():
    """37 x 64 upwinded (27 .. 28 iterations), 4 scenarios, each against
    bicgstab_ref.bicgstab with the dots summed in the solver's order:
    test_gpu_bicgstab.same_bits's bar"""
    A, B, X0 = K.nat()
    S = B.shape[0]
    L, U = O.ilu0(A)
    s = make(A)
    try:
        assert s.uses_wavefront and s.batch_engine
        lay2nat, G = s.layout()
        dot = C.layout_dot(lay2nat, G)
        g = s.solve_bicgstab_batch(B, X0, max_iter=3000, tol=1e-10)
    finally:
        s.close()
    refs = [R.bicgstab(A, lambda v: O.lusolve(L, U, v), B[q], X0[q], 3000, 1e-10, dot) for q in range(S)]
    assert max(o[2] for o in refs) > 20 and refs[2][2] == 0
    for q, (ret, x, iters, relres, hist) in enumerate(refs):
        assert g["status"][q] == ret == 0, q
        assert g["iters"][q] == g["inner"][q] == iters and g["restarts"][q] == 0, q
        assert g["hist"][q].shape == hist.shape and np.array_equal(g["hist"][q], hist), q
        assert g["relres"][q] == relres, q
        assert np.array_equal(g["x"][q], x), q
    assert g["ret"] == 0


def test_bicgstab_batch_breakdown_at_the_start_and_rezeroing():
    """`small`: b = 1e200 * 1 overflows rho at the start (k_bi_p<START>'s exit:
    relres NaN, x untouched) beside two ordinary solves and one that converges
    at the start.  Then the three good right-hand sides on the same solver:
    a fresh solver's bits, so nothing that was not finite stayed in the arena"""
    A, B, X0 = K.small()
    good = [0, 2, 3]
    f = make(A)
    try:
        fresh = f.solve_bicgstab_batch(B[good], X0[good])
    finally:
        f.close()
    s = make(A)
    try:
        assert s.batch_engine
        ref = singles(s, B, X0)
        assert [r["iters"] for r in ref][1:3] == [0, 0] and min(ref[0]["iters"], ref[3]["iters"]) > 8
        g = s.solve_bicgstab_batch(B, X0)
        msg = ggmres.lib().gg_last_error().decode()
        assert g["status"] == [0, -8, 0, 0] and g["ret"] == ggmres.EBREAKDOWN == -8
        assert np.isnan(g["relres"][1])
        assert np.all(np.isfinite(g["x"]))
        same_as_singles(g, ref, "small")
        assert "scenario 1 at iteration 0" in msg and "rho" in msg, msg
        # the same arena (S = 4 again: kept, not zeroed anew) with a good
        # right-hand side where the broken scenario was
        g4 = s.solve_bicgstab_batch(B[[0, 3, 2, 3]], X0)
        same_as_singles(g4, [ref[0], ref[3], ref[2], ref[3]], "S = 4 after a breakdown")
        again = s.solve_bicgstab_batch(B[good], X0[good])
        assert again["ret"] == 0
        same_batches(again, fresh, "after a breakdown")
    finally:
        s.close()


def broken(ref):
    """(scenario, iteration) of the lowest scenario of the single solves that broke down"""
    q = [r["ret"] for r in ref].index(-8)
    return q, ref[q]["iters"]


@pytest.mark.parametrize("path", ["batched", "scenario by scenario"])
def test_bicgstab_batch_breakdowns_after_iteration_0(path, monkeypatch):
    """`tiny`: right-hand sides so small that the scalars underflow -- k_bi_s's
    and k_bi_p's exits at several iterations greater than 0 in one batch, after
    x and r have moved, beside scenarios that converge and one that converged
    at the start; with max_iter = 4 a mix of -8, 1 and 0 in one launch sequence.
    Exponents: bi_batch_cases.TINY_EXPONENTS, -162 .. -153 (on the device: rt.v
    at iteration 0, omega at 2, 6, 8, 10 and 12, convergences at 5 .. 14)."""
    A, B, X0 = K.tiny()
    s = make(A)
    try:
        assert s.uses_wavefront and s.batch_engine
        ref = singles(s, B, X0)
        stat = [(r["ret"], r["iters"]) for r in ref]
        print(f"single solves: {stat}")
        # on the single solves alone: breakdowns at two or more distinct iterations
        # greater than 0, a convergence after iterations, a convergence at the start
        assert len({k for ret, k in stat if ret == -8 and k > 0}) >= 2
        assert any(ret == 0 and k > 0 for ret, k in stat) and (0, 0) in stat
        ref4 = singles(s, B, X0, max_iter=4)
        stat4 = [(r["ret"], r["iters"]) for r in ref4]
        print(f"single solves, max_iter 4: {stat4}")
        assert {ret for ret, _ in stat4} == {-8, 1, 0} and (1, 4) in stat4
        if path != "batched":
            monkeypatch.setenv("GG_BATCH_SEQ", "1")
            assert not s.batch_engine
        for what, run, r in (("S = 12", lambda: s.solve_bicgstab_batch(B, X0), ref),
                             ("S = 3", lambda: s.solve_bicgstab_batch(B[:3], X0[:3]), ref[:3]),
                             ("S = 12, max_iter 4", lambda: s.solve_bicgstab_batch(B, X0, max_iter=4), ref4)):
            g = run()
            msg = ggmres.lib().gg_last_error().decode()
            same_as_singles(g, r, f"{path} {what}")
            q, k = broken(r)
            assert g["ret"] == ggmres.EBREAKDOWN == -8, what
            assert f"scenario {q} at iteration {k}: " in msg, (what, msg)
            # the scalar and its value: the single solve's own message ends in
            # "rho|rt.v|omega = VAL (zero or not finite)"
            s.solve(B[q], x0=X0[q], max_iter=4 if "max_iter" in what else 3000, tol=1e-10, flags=BI)
            single_msg = ggmres.lib().gg_last_error().decode()
            scalar = single_msg.rsplit(": ", 1)[1]
            assert scalar.split(" = ")[0] in ("rho", "rt.v", "omega") and msg.endswith(scalar), \
                (what, msg, single_msg)
    finally:
        s.close()


@pytest.mark.parametrize("case", ["ainv", "diag", "grid3d", "forced"])
def test_bicgstab_batch_scenario_by_scenario(case, monkeypatch):
    """configurations without batched launches (AINV, DIAG, the 3D tile
    wavefront) and the forced scenario-by-scenario path: the single solves'
    results"""
    if case == "grid3d":
        A = M.grid_7pt(20, upwind=0.1)
        n = A.shape[0]
        B = K.rhs_set(A, 3, seed=7)
        X0 = np.zeros((3, n))
        X0[1] = 1e-2 * np.random.default_rng(9).standard_normal(n)
    else:
        A, B, X0 = K.nat()
    s = make(A, case if case in ("ainv", "diag") else "ilu0")
    try:
        ref = singles(s, B, X0)
        assert all(r["ret"] == 0 for r in ref) and ref[0]["iters"] > 20
        if case == "forced":
            assert s.batch_engine
            batched = s.solve_bicgstab_batch(B, X0)
            monkeypatch.setenv("GG_BATCH_SEQ", "1")
        assert not s.batch_engine
        g = s.solve_bicgstab_batch(B, X0)
        same_as_singles(g, ref, case)
        if case == "forced":
            monkeypatch.delenv("GG_BATCH_SEQ")
            same_as_singles(batched, ref, "batched")
    finally:
        s.close()


def test_bicgstab_batch_refusals():
    from helpers import make_split
    A = K.small_matrix()
    n = A.shape[0]
    L = ggmres.lib()
    b = np.tile(A @ np.ones(n), 2)
    x = np.zeros(2 * n)
    res = (ggmres.Result * 2)()

    def call(s, nrhs=2, ld=n, flags=BI, fn=L.gg_solve_bicgstab_batch):
        o = ggmres.Options(30, 100, 1e-8, flags)
        x[:] = 0.0
        return fn(s.h, nrhs, b, ld, x, ld, ctypes.byref(o), res)
    s = ggmres.Solver(0)
    try:
        assert call(s) == -5                            # GG_ESTATE: no matrix
        s.set_matrix(A)
        assert call(s) == -5                            # GG_ESTATE: no preconditioner
        s.set_precond_ilu0()
        assert call(s) == 0
        for kw in (dict(flags=CG), dict(flags=ggmres.SOLVE_SHARED_DEVICE), dict(flags=ggmres.SOLVE_CGS2),
                   dict(flags=CG | BI), dict(nrhs=0), dict(ld=n - 1)):
            assert call(s, **kw) == -1, kw               # GG_EINVAL
            assert call(s) == 0 and res[1].status == 0 and res[1].iters > 8, kw       # still solves
        o = ggmres.Options(0, 100, 1e-8, BI)            # restart is validated
        assert L.gg_solve_bicgstab_batch(s.h, 2, b, n, x, n, ctypes.byref(o), res) == -1
        assert call(s) == 0 and res[1].iters > 8
        o = ggmres.Options(30, 100, 1e-8, CG)
        ports = np.zeros(1, np.int32)
        tot = np.zeros(2, np.int32)
        rc = L.gg_transient_bicgstab_batch(s.h, 2, 1, 1e-2, np.ones(n), np.zeros(3, np.int32), ports, ports, ports,
                                           np.zeros(1), 0, ports, x, ctypes.byref(o), np.zeros(1), tot)
        assert rc == -1
        assert call(s) == 0 and res[1].iters > 8
        P = make_split(A, identity_perm=True)
        s.set_precond_split(P.L, P.U, P.middle, P.perm_row, P.perm_col, P.lscale, P.rscale)
        assert call(s) == -1
        s.set_precond_user(lambda op, i, o, n: 0)
        assert call(s) == -1
        s.set_precond_ilu0()
        assert call(s) == 0 and res[1].iters > 8
        # the existing refusals stay: the GMRES batch defines no flags, the CG batch refuses BiCGStab's
        assert call(s, flags=BI, fn=L.gg_solve_batch) == -1
        assert call(s, flags=BI, fn=L.gg_solve_cg_batch) == -1
    finally:
        s.close()


def test_transient_bicgstab_batch_bitexact_vs_single():
    """24 x 24 upwinded, A = G + C/h, 6 steps: three seeded PULSE scenarios and
    one without sources (its right-hand side stays zero: every step converges
    at the start, 0 iterations)"""
    h = 1e-2
    A = M.transient(M.laplacian_5pt(24, upwind=0.2), c=1e-3, h=h)
    n = A.shape[0]
    cdiag = np.full(n, 1e-3 / h)
    sc = [M.pulse_sources(n, frac=0.01, h=h, seed=100 + k) for k in range(3)]
    sc.append((np.zeros(0, np.int32), np.zeros((0, 7))))
    S = len(sc)
    ports = np.array([0, n - 1], np.int32)
    X0 = np.zeros((S, n))
    s = make(A)
    try:
        assert s.batch_engine
        g = s.transient_bicgstab_batch(6, h, cdiag, sc, ports, X0, restart=30, max_iter=3000, tol=1e-10)
        for q, (nodes, pulses) in enumerate(sc):
            r = s.transient(6, h, cdiag, nodes, pulses, ports, X0[q], restart=30, max_iter=3000, tol=1e-10, flags=BI)
            assert r["ret"] == 0
            assert (r["iters_total"] > 0) == (q < 3), q
            assert g["iters_total"][q] == r["iters_total"], q
            assert np.array_equal(g["ports"][q], r["ports"]) and np.array_equal(g["x"][q], r["x"]), q
        assert g["iters_total"][3] == 0
        assert g["ret"] == 0 and np.max(np.abs(g["ports"][:3])) > 0 and not np.any(g["x"][3])
    finally:
        s.close()


def test_bicgstab_batch_second_grid_in_the_same_arena():
    """test_gpu_cg_batch.test_cg_batch_second_grid_in_the_same_arena for BiCGStab:
    60 x 52, then 60 x 40 (both upwinded) on the same solver -- the same nrhs,
    Ppad (8192) and granule counts, rows of the first grid where the second
    pads.  The second grid's batch is a fresh solver's, bit for bit."""
    A = [M.laplacian_5pt(60, 52, upwind=0.2), M.laplacian_5pt(60, 40, upwind=0.2)]
    B = [K.rhs_set(a, 3, seed=3) for a in A]
    f = make(A[1])
    try:
        fresh = f.solve_bicgstab_batch(B[1], max_iter=3000, tol=1e-10)
    finally:
        f.close()
    s = ggmres.Solver(0)
    try:
        lay = []
        for a, b in zip(A, B):
            s.set_matrix(a)
            s.set_precond_ilu0()
            s.set_division(ggmres.DIV_EXACT)
            assert s.uses_wavefront and s.batch_engine
            lay.append(s.layout())
            g = s.solve_bicgstab_batch(b, max_iter=3000, tol=1e-10)
    finally:
        s.close()
    assert lay[0][0].size == lay[1][0].size == 8192 and lay[0][1] == lay[1][1]
    assert [np.count_nonzero(l >= 0) for l, _ in lay] == [60 * 52, 60 * 40]
    assert np.any((lay[0][0] >= 0) & (lay[1][0] < 0))
    assert fresh["ret"] == 0 and max(fresh["iters"]) > 20 and fresh["iters"][2] == 0
    same_batches(g, fresh, "second grid")


def test_batches_and_single_solves_alternate_on_one_solver():
    """GMRES, CG and BiCGStab batches and single solves on one solver (the
    symmetric 40 x 33 grid, so that CG applies): each gives a fresh solver's
    bits, and batch_history follows the last batch"""
    A = M.laplacian_5pt(40, 33)
    B = K.rhs_set(A, 5, seed=13)
    steps = [("solve_batch", lambda s: s.solve_batch(B[:3], restart=30, max_iter=2000, tol=1e-10)),
             ("solve_bicgstab_batch 5", lambda s: s.solve_bicgstab_batch(B, max_iter=2000, tol=1e-10)),
             ("solve_cg_batch", lambda s: s.solve_cg_batch(B[:3], max_iter=2000, tol=1e-10)),
             ("solve_bicgstab_batch 2", lambda s: s.solve_bicgstab_batch(B[3:5], max_iter=2000, tol=1e-10)),
             ("solve BiCGStab", lambda s: s.solve(B[1], max_iter=2000, tol=1e-10, flags=BI)),
             ("solve_bicgstab_batch 5 again", lambda s: s.solve_bicgstab_batch(B, max_iter=2000, tol=1e-10)),
             ("solve", lambda s: s.solve(B[1], restart=30, max_iter=2000, tol=1e-10)),
             ("solve_batch again", lambda s: s.solve_batch(B[:3], restart=30, max_iter=2000, tol=1e-10))]
    fresh = []
    for _, run in steps:
        f = make(A)
        try:
            fresh.append(run(f))
        finally:
            f.close()
    s = make(A)
    try:
        assert s.batch_engine
        last_batch = None
        for (what, run), f in zip(steps, fresh):
            g = run(s)
            assert g["ret"] == f["ret"] == 0, what
            assert g["iters"] == f["iters"], what
            assert np.array_equal(g["x"], f["x"]), what
            if isinstance(f["hist"], list):
                last_batch = f
                assert len(g["hist"]) == len(f["hist"]), what
                for a, b in zip(g["hist"], f["hist"]):
                    assert a.size > 0 and np.array_equal(a, b), what
            else:
                assert np.array_equal(g["hist"], f["hist"]), what
                # a single solve leaves the last batch's histories where they were
                for q, b in enumerate(last_batch["hist"]):
                    assert np.array_equal(s.batch_history(q), b), (what, q)
            if "bicgstab_batch" in what:
                assert s.batch_mgs_kernel() == "", what
    finally:
        s.close()
