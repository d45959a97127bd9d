"""GPU: the many-RHS conjugate-gradient solve (gg_solve_cg_batch*,
gg_transient_cg_batch; gpu-gmres_amd/csrc/cg_batch.hip).

The batch's contract carries over from tests/test_gpu_batch.py: every scenario
is exactly the single-RHS solve, here gg_solve(GG_SOLVE_CG) -- status,
iteration count, relres, residual history and solution are bit-identical
(np.array_equal) to the single CG solve on that right-hand side alone, which
tests/test_gpu_cg.py pins to the restatement tests/cg_ref.py; one test checks
the batch against that restatement directly.  Exact division unless a case
says otherwise.

Iteration counts named in comments are those of cg_ref.pcg with plain dots; the
device's reduction order may move a count by one or two, so every assertion on
a count is made on a reference the test computes itself, never on the batch.
"""
import ctypes

import numpy as np
import pytest

import cg_ref as C
import ggmres
import oracle as O
from ggmres import matrices as M

pytestmark = pytest.mark.gpu
CG = ggmres.SOLVE_CG


def rhs_set(A, S, seed):
    """test_gpu_batch._rhs_set's pattern: b = A 1, random normal, zeros, 1e3 * uniform, repeated"""
    n = A.shape[0]
    rng = np.random.default_rng(seed)
    out = []
    for q in range(S):
        k = q % 4
        if k == 0:
            out.append(A @ np.ones(n))
        elif k == 1:
            out.append(rng.standard_normal(n))
        elif k == 2:
            out.append(np.zeros(n))
        else:
            out.append(1e3 * rng.uniform(-1, 1, n))
    return np.array(out)


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
    return [s.solve(B[q], x0=X0[q], max_iter=max_iter, tol=tol, flags=CG) for q in range(B.shape[0])]


def same_as_singles(g, ref, what):
    """every scenario of the batch g against its single solve"""
    S = len(ref)
    assert len(g["status"]) == S and g["x"].shape[0] == S and len(g["hist"]) == S, what
    for q, r in enumerate(ref):
        assert (g["status"][q], g["iters"][q], g["inner"][q], g["restarts"][q]) == \
               (r["ret"], r["iters"], r["iters"], 0), (what, q)
        assert g["relres"][q] == r["relres"], (what, q)
        assert np.array_equal(g["hist"][q], r["hist"]), (what, q)
        assert np.array_equal(g["x"][q], r["x"]), (what, q)
    stat = [r["ret"] for r in ref]
    want = ggmres.EBREAKDOWN if ggmres.EBREAKDOWN in stat else (1 if 1 in stat else 0)
    assert g["ret"] == want, what


def band_case():
    """60 x 52: one 64-line band with padded steps; 9 scenarios (the batched SpMV
    carries 8 per launch: groups of 8 + 1), three of them warm starts"""
    A = M.laplacian_5pt(60, 52)
    n = A.shape[0]
    S = 9
    B = rhs_set(A, S, seed=3)
    rng = np.random.default_rng(9)
    X0 = np.zeros((S, n))
    X0[1] = 1e-2 * rng.standard_normal(n)
    X0[4] = 1.0 + 1e-5 * rng.standard_normal(n)        # b = A 1: 36 iterations instead of 65
    X0[8] = 1.0 + 1e-7 * rng.standard_normal(n)        # b = A 1: 16
    return A, B, X0


@pytest.mark.parametrize("division", [ggmres.DIV_EXACT, ggmres.DIV_FMA, ggmres.DIV_RCP])
@pytest.mark.parametrize("max_iter,tol", [(3000, 1e-10),     # converges: 65 .. 72 cold, 0 for b = 0, 36 and 16 warm
                                          (3000, 0.05),      # 10 .. 13: launches gated off behind every end
                                          (12, 1e-300)])     # max_iter cuts every scenario
def test_cg_batch_bitexact_vs_single(max_iter, tol, division):
    A, B, X0 = band_case()
    S = B.shape[0]
    s = make(A, division=division)
    try:
        assert s.uses_wavefront and s.batch_engine
        ref = singles(s, B, X0, max_iter, tol)
        counts = [r["iters"] for r in ref]
        print(f"division {division} max_iter {max_iter} tol {tol}: single-solve counts {counts}")
        if tol == 1e-10:
            # scenarios end several chunks of the read-back apart while others go on
            assert all(r["ret"] == 0 for r in ref)
            assert len(set(counts)) >= 4 and 0 in counts
            assert max(counts) > 2 * min(c for c in counts if c > 0)
        elif tol == 0.05:
            # early ends a few iterations apart: the host is a chunk ahead, so launches
            # run gated off behind every scenario's end
            assert all(r["ret"] == 0 for r in ref) and 0 < max(counts) < 32
        else:
            for q, r in enumerate(ref):
                assert (r["ret"], r["iters"]) == ((1, 12) if np.any(B[q]) else (0, 0)), q
        g = s.solve_cg_batch(B, X0, max_iter=max_iter, tol=tol)
        same_as_singles(g, ref, "S = 9")
        assert g["ret"] == (1 if tol == 1e-300 else 0)
        for k in (1, 2):                                # one scenario; a pair
            gk = s.solve_cg_batch(B[:k], X0[:k], max_iter=max_iter, tol=tol, flags=0)     # flags 0 means CG too
            same_as_singles(gk, ref[:k], f"S = {k}")
    finally:
        s.close()


def test_cg_batch_bitexact_vs_restatement():
    """37 x 64 (56 .. 62 iterations), 4 scenarios, each against cg_ref.pcg with
    the dots summed in the solver's order: test_gpu_cg.same_bits's bar"""
    A = M.laplacian_5pt(37, 64)
    n = A.shape[0]
    S = 4
    B = rhs_set(A, S, seed=5)                           # (scenario 2 is the zero vector)
    X0 = np.zeros((S, n))
    X0[1] = 1e-2 * np.random.default_rng(9).standard_normal(n)      # a warm start
    L, U = O.ilu0(A)
    s = make(A)
    try:
        assert s.uses_wavefront and s.batch_engine
        lay2nat, G = s.layout()
        dot = C.layout_dot(lay2nat, G)
        g = s.solve_cg_batch(B, X0, max_iter=3000, tol=1e-10)
    finally:
        s.close()
    refs = [C.pcg(A, lambda v: O.lusolve(L, U, v), B[q], X0[q], 3000, 1e-10, dot) for q in range(S)]
    assert max(o[2] for o in refs) > 40 and refs[2][2] == 0
    for q, (ret, x, iters, relres, hist) in enumerate(refs):
        assert g["status"][q] == ret == 0, q
        assert g["iters"][q] == g["inner"][q] == iters and g["restarts"][q] == 0, q
        assert g["hist"][q].shape == hist.shape and np.array_equal(g["hist"][q], hist), q
        assert g["relres"][q] == relres, q
        assert np.array_equal(g["x"][q], x), q
    assert g["ret"] == 0


def test_cg_batch_smallest_layout():
    """272 rows: fewer than one pad unit per reduction block (23 .. 24 iterations)"""
    A = M.laplacian_5pt(16, 17)
    n = A.shape[0]
    rng = np.random.default_rng(4)
    B = np.array([A @ np.ones(n), rng.standard_normal(n), 1e3 * rng.uniform(-1, 1, n)])
    X0 = np.zeros((3, n))
    s = make(A)
    try:
        assert s.batch_engine
        ref = singles(s, B, X0)
        assert all(r["ret"] == 0 and r["iters"] > 15 for r in ref)
        same_as_singles(s.solve_cg_batch(B, X0), ref, "16 x 17")
    finally:
        s.close()


def test_cg_batch_breakdown_stays_in_its_scenario():
    """a negative definite matrix with ILU(0), itself negative definite: r.z =
    r.Mr < 0 at the start for every nonzero right-hand side (k_cg_p<START>'s
    exit, tests/sr_exit_cases.py `rz0`; k_cg_xr never runs); the zero one
    converges at the start"""
    import scipy.sparse as sp
    A = -sp.csr_matrix(M.laplacian_5pt(16, 17))
    A.sort_indices()
    A = A.tocsr()
    n = A.shape[0]
    B = np.array([A @ np.ones(n), np.zeros(n), np.random.default_rng(6).standard_normal(n)])
    X0 = np.zeros((3, n))
    L, U = O.ilu0(A)
    for q, want in enumerate([(C.BREAKDOWN, 0), (0, 0), (C.BREAKDOWN, 0)]):
        o = C.pcg(A, lambda v: O.lusolve(L, U, v), B[q], None, 3000, 1e-10)
        assert (o[0], o[2]) == want, q
    s = make(A)
    try:
        assert s.batch_engine
        ref = singles(s, B, X0)
        g = s.solve_cg_batch(B, X0)
        msg = ggmres.lib().gg_last_error().decode()
        assert g["status"] == [-8, 0, -8] and g["ret"] == ggmres.EBREAKDOWN == -8
        assert np.all(np.isfinite(g["x"]))
        same_as_singles(g, ref, "breakdown")
        assert msg and "scenario 0" in msg
        # still usable: the zero right-hand side alone converges at the start
        z = s.solve_cg_batch(B[1:2], X0[1:2])
        assert z["ret"] == 0 and z["iters"] == [0]
    finally:
        s.close()


def indefinite_case():
    """60 x 52 shifted by -0.02 I (indefinite), ILU(0): with cg_ref.pcg's plain
    dots p.Ap turns negative at iterations 5, 10, 9 and 6 (scenarios 0, 1, 3, 5),
    b = 0 converges at the start (2) and the warm start converges in 9 (4,
    relres 8.2e-11) -- breakdowns after x and r have moved, at different
    iterations, while other scenarios go on through the same launches"""
    import scipy.sparse as sp
    A = (sp.csr_matrix(M.laplacian_5pt(60, 52)) - 0.02 * sp.identity(60 * 52, format="csr")).tocsr()
    A.sort_indices()
    n = A.shape[0]
    one = A @ np.ones(n)
    B = np.array([one, np.random.default_rng(1).standard_normal(n), np.zeros(n),
                  np.random.default_rng(3).standard_normal(n), one, np.random.default_rng(2).standard_normal(n)])
    X0 = np.zeros((6, n))
    X0[4] = 1.0 + 1e-8 * np.random.default_rng(9).standard_normal(n)
    return A, B, X0


def broken(ref):
    """(scenario, iteration) of the lowest scenario of the single solves that broke down"""
    q = [r["ret"] for r in ref].index(-8)
    return q, ref[q]["iters"]


@pytest.mark.parametrize("path", ["batched", "scenario by scenario"])
def test_cg_batch_breakdowns_after_iteration_0(path, monkeypatch):
    """k_cg_xr's exit at several iterations greater than 0 in one batch, beside a
    scenario that converges and one that converged at the start; with max_iter =
    8 a mix of -8, 1 and 0 in one launch sequence"""
    A, B, X0 = indefinite_case()
    s = make(A)
    try:
        assert s.uses_wavefront and s.batch_engine
        ref = singles(s, B, X0)
        stat = [(r["ret"], r["iters"]) for r in ref]
        print(f"single solves: {stat}")
        # on the single solves alone: breakdowns at three or more distinct iterations
        # greater than 0, a convergence after iterations, a convergence at the start
        assert len({k for ret, k in stat if ret == -8 and k > 0}) >= 3
        assert any(ret == 0 and k > 0 for ret, k in stat) and (0, 0) in stat
        ref8 = singles(s, B, X0, max_iter=8)
        stat8 = [(r["ret"], r["iters"]) for r in ref8]
        print(f"single solves, max_iter 8: {stat8}")
        assert {ret for ret, _ in stat8} == {-8, 1, 0} and (1, 8) in stat8
        if path != "batched":
            monkeypatch.setenv("GG_BATCH_SEQ", "1")      # test_cg_batch_scenario_by_scenario's mechanism
            assert not s.batch_engine
        for what, g, r in (("S = 6", s.solve_cg_batch(B, X0), ref),
                           ("S = 2", s.solve_cg_batch(B[:2], X0[:2]), ref[:2]),
                           ("S = 6, max_iter 8", s.solve_cg_batch(B, X0, max_iter=8), ref8)):
            msg = ggmres.lib().gg_last_error().decode()
            same_as_singles(g, r, f"{path} {what}")
            q, k = broken(r)
            assert g["ret"] == ggmres.EBREAKDOWN == -8, what
            assert f"scenario {q} at iteration {k} " in msg, (what, msg)
    finally:
        s.close()


def test_cg_batch_pq_breakdown_at_iteration_0():
    """tests/sr_exit_cases.py `pq0` (negative definite, no preconditioner: r.z =
    r.r > 0, p.Ap < 0 in the first iteration) through the batch entry: k_cg_xr's
    exit at iteration 0, scenario by scenario (no batched launches without
    triangular factors)"""
    import sr_exit_cases as X
    c = X.cases()["pq0"]
    n = c.A.shape[0]
    B = np.array([c.b, np.zeros(n), np.random.default_rng(6).standard_normal(n)])
    X0 = np.zeros((3, n))
    for q, want in enumerate([("pq", 0), ("conv0", 0), ("pq", 0)]):
        info = {}
        o = X.reference(c._replace(b=B[q]), info=info)
        assert (info["why"], o[2]) == want, q
    s = make(c.A, "none")
    try:
        assert not s.batch_engine
        ref = singles(s, B, X0)
        g = s.solve_cg_batch(B, X0)
        msg = ggmres.lib().gg_last_error().decode()
        assert g["status"] == [-8, 0, -8] and g["iters"] == [0, 0, 0] and g["ret"] == ggmres.EBREAKDOWN
        assert np.array_equal(g["x"], X0)
        same_as_singles(g, ref, "pq0")
        assert "scenario 0 at iteration 0 " in msg
    finally:
        s.close()


@pytest.mark.parametrize("case", ["ainv", "diag", "grid3d", "forced"])
def test_cg_batch_scenario_by_scenario(case, monkeypatch):
    """configurations without batched launches (AINV, DIAG, the 3D tile
    wavefront) and the forced scenario-by-scenario path: the single solves'
    results"""
    A = M.grid_7pt(20) if case == "grid3d" else M.laplacian_5pt(37, 64)
    n = A.shape[0]
    B = rhs_set(A, 3, seed=7)
    X0 = np.zeros((3, n))
    X0[1] = 1e-2 * np.random.default_rng(9).standard_normal(n)
    s = make(A, case if case in ("ainv", "diag") else "ilu0")
    try:
        ref = singles(s, B, X0)
        assert all(r["ret"] == 0 for r in ref) and ref[0]["iters"] > 30
        if case == "forced":
            assert s.batch_engine
            batched = s.solve_cg_batch(B, X0)
            monkeypatch.setenv("GG_BATCH_SEQ", "1")
        assert not s.batch_engine
        g = s.solve_cg_batch(B, X0)
        same_as_singles(g, ref, case)
        if case == "forced":
            monkeypatch.delenv("GG_BATCH_SEQ")
            same_as_singles(batched, ref, "batched")
    finally:
        s.close()


def test_cg_batch_refusals():
    from helpers import make_split
    A = M.laplacian_5pt(16, 17)
    n = A.shape[0]
    L = ggmres.lib()
    b = np.tile(A @ np.ones(n), 2)
    x = np.zeros(2 * n)
    res = (ggmres.Result * 2)()

    def call(s, nrhs=2, ld=n, flags=CG, fn=L.gg_solve_cg_batch):
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
        for kw in (dict(flags=ggmres.SOLVE_BICGSTAB), dict(flags=ggmres.SOLVE_SHARED_DEVICE),
                   dict(flags=ggmres.SOLVE_CGS2), dict(flags=CG | ggmres.SOLVE_BICGSTAB),
                   dict(nrhs=0), dict(ld=n - 1)):
            assert call(s, **kw) == -1, kw               # GG_EINVAL
            assert call(s) == 0 and res[1].status == 0 and res[1].iters > 10, kw      # still solves
        o = ggmres.Options(0, 100, 1e-8, CG)            # restart is validated
        assert L.gg_solve_cg_batch(s.h, 2, b, n, x, n, ctypes.byref(o), res) == -1
        o = ggmres.Options(30, 100, 1e-8, ggmres.SOLVE_BICGSTAB)
        ports = np.zeros(1, np.int32)
        tot = np.zeros(2, np.int32)
        rc = L.gg_transient_cg_batch(s.h, 2, 1, 1e-2, np.ones(n), np.zeros(3, np.int32), ports, ports, ports,
                                     np.zeros(1), 0, ports, x, ctypes.byref(o), np.zeros(1), tot)
        assert rc == -1
        P = make_split(A, identity_perm=True)
        s.set_precond_split(P.L, P.U, P.middle, P.perm_row, P.perm_col, P.lscale, P.rscale)
        assert call(s) == -1
        s.set_precond_user(lambda op, i, o, n: 0)
        assert call(s) == -1
        s.set_precond_ilu0()
        assert call(s) == 0
    finally:
        s.close()


def test_transient_cg_batch_bitexact_vs_single():
    """24 x 24, A = G + C/h, 6 steps: three seeded PULSE scenarios (22 .. 24 CG
    iterations per step) and one without sources (its right-hand side stays
    zero: every step converges at the start)"""
    h = 1e-2
    A = M.transient(M.laplacian_5pt(24), c=1e-3, h=h)
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
        g = s.transient_cg_batch(6, h, cdiag, sc, ports, X0, restart=30, max_iter=3000, tol=1e-10)
        for q, (nodes, pulses) in enumerate(sc):
            r = s.transient(6, h, cdiag, nodes, pulses, ports, X0[q], restart=30, max_iter=3000, tol=1e-10, flags=CG)
            assert r["ret"] == 0
            assert (r["iters_total"] > 0) == (q < 3), q
            assert g["iters_total"][q] == r["iters_total"], q
            assert np.array_equal(g["ports"][q], r["ports"]) and np.array_equal(g["x"][q], r["x"]), q
        assert g["ret"] == 0 and np.max(np.abs(g["ports"][:3])) > 0 and not np.any(g["x"][3])
    finally:
        s.close()


def test_cg_batch_second_grid_in_the_same_arena():
    """test_gpu_batch.test_solve_batch_second_grid_in_the_same_arena for CG: 60 x 52,
    then 60 x 40 on the same solver -- the same nrhs, Ppad (8192) and granule
    counts, rows of the first grid where the second pads.  The second grid's
    batch is a fresh solver's, bit for bit."""
    A = [M.laplacian_5pt(60, 52), M.laplacian_5pt(60, 40)]
    B = [rhs_set(a, 3, seed=3) for a in A]
    f = make(A[1])
    try:
        fresh = f.solve_cg_batch(B[1], max_iter=3000, tol=1e-10)
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
            g = s.solve_cg_batch(b, max_iter=3000, tol=1e-10)
    finally:
        s.close()
    assert lay[0][0].size == lay[1][0].size == 8192 and lay[0][1] == lay[1][1]
    assert [np.count_nonzero(l >= 0) for l, _ in lay] == [60 * 52, 60 * 40]
    assert np.any((lay[0][0] >= 0) & (lay[1][0] < 0))
    assert fresh["ret"] == 0 and max(fresh["iters"]) > 30 and fresh["iters"][2] == 0
    assert g["ret"] == fresh["ret"]
    for k in ("status", "iters", "inner", "restarts", "relres"):
        assert g[k] == fresh[k], k
    for q in range(3):
        assert np.array_equal(g["hist"][q], fresh["hist"][q]), q
        assert np.array_equal(g["x"][q], fresh["x"][q]), q


def test_cg_and_gmres_batches_alternate_on_one_solver():
    """each solve on a solver that ran the others gives a fresh solver's bits"""
    A = M.laplacian_5pt(40, 33)
    n = A.shape[0]
    B = rhs_set(A, 5, seed=13)
    steps = [("solve_batch", lambda s: s.solve_batch(B[:3], restart=30, max_iter=2000, tol=1e-10)),
             ("solve_cg_batch 5", lambda s: s.solve_cg_batch(B, max_iter=2000, tol=1e-10)),
             ("solve_batch again", lambda s: s.solve_batch(B[:3], restart=30, max_iter=2000, tol=1e-10)),
             ("solve_cg_batch 2", lambda s: s.solve_cg_batch(B[3:5], max_iter=2000, tol=1e-10)),
             ("solve CG", lambda s: s.solve(B[1], max_iter=2000, tol=1e-10, flags=CG)),
             ("solve", lambda s: s.solve(B[1], restart=30, max_iter=2000, tol=1e-10))]
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
        for (what, run), f in zip(steps, fresh):
            g = run(s)
            assert g["ret"] == f["ret"] == 0, what
            assert g["iters"] == f["iters"], what
            assert np.array_equal(g["x"], f["x"]), what
            if isinstance(f["hist"], list):
                assert len(g["hist"]) == len(f["hist"]), what
                for a, b in zip(g["hist"], f["hist"]):
                    assert a.size > 0 and np.array_equal(a, b), what
            else:
                assert np.array_equal(g["hist"], f["hist"]), what
    finally:
        s.close()
