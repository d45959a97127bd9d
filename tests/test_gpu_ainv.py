"""GPU: the AINV and DIAG preconditioners (gg_set_precond_ainv / _diag) against
the fp64 restatements of tests/ainv_ref.py.

Bars: the apply is bit-exact whichever SpMV kernel a factor takes (sliced or
CSR-stream) for every factor row of at most 2048 entries (a block's capacity);
a longer row is summed by the SpMV's strided block reduction, within the
project's 1e-13 |A||x| bar (test_spmv_long_rows); a GMRES solve agrees with the NumPy
GMRES of ainv_ref (the oracle's recurrence, dots summed in the solver's order)
in return code and iteration count, its history within 1e-10 per entry
(hist_close) and its solution within 1e-8 relative.
"""
import functools

import numpy as np
import pytest

import ainv_ref as R
import ggmres
import oracle as O
from conftest import fixture_path
from ggmres import matrices as M
from helpers import hist_close, rel_err

pytestmark = pytest.mark.gpu
HIST_RTOL = 1e-10
GG_APPLY_MINV = ggmres.APPLY_MINV


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name == "pert16":
        return R.pert(16)
    if name == "pert24":
        return R.pert(24)
    if name == "pert16x17":
        return R.pert(16, 17)                      # 272 rows: a ragged last slice
    if name == "power_law":
        return M.power_law(3000, 33000, seed=7)    # a 1,435-entry row in Z: CSR-stream, one packed block
    if name == "sherman1":
        return M.read_rua(fixture_path("sherman1.rua"))
    if name == "9pt_10x10":
        return M.read_mtx(fixture_path("9pt_10x10.mtx"))   # n < one block
    if name == "lap37x64":
        return M.laplacian_5pt(37, 64)             # 37 slices
    if name == "lap16x17":
        return M.laplacian_5pt(16, 17)             # 272 rows, sliced factors: a ragged last slice
    if name == "two_rows":
        return R.two_dense_rows(2400)          # 2400-entry rows in Z and Wt: the long-row path
    raise KeyError(name)


SPMV_CAP = 2048        # gg_internal.h kSpmvCap: entries one SpMV block sums serially
APPLY_MATS = ["pert16", "power_law", "sherman1", "9pt_10x10", "lap37x64", "pert16x17", "lap16x17"]
# both factors take the sliced form (checked against the rule below); the others the CSR-stream kernel
SLICED = ["pert16", "9pt_10x10", "lap37x64", "lap16x17"]


def sliced(T):
    """DevCsr::upload's rule for the sliced (ELL) form: per 64-row slice the
    longest row; at most 64 wide and padded entries <= 1.25 nnz + one slice"""
    n = T.shape[0]
    w = np.diff(T.indptr)
    ws = [int(w[k:k + 64].max()) for k in range(0, n, 64)]
    return max(ws) <= 64 and 64 * sum(ws) <= int(1.25 * T.nnz) + 64 * max(ws)


@functools.lru_cache(maxsize=None)
def factors(name):
    """the restatement's factors at the reference's tolerance, computed once"""
    return R.ainv(matrix(name), 0.1)


@functools.lru_cache(maxsize=None)
def reference_solve(name, kind):
    A = matrix(name)
    n = A.shape[0]
    b = A @ np.ones(n)
    if kind == "ainv":
        Z, Wt, dinv = factors(name)
        minv = lambda v: R.ainv_apply(Z, Wt, dinv, v)      # noqa: E731
    else:
        inv = R.diag_nearest(A)
        minv = lambda v: v * inv                           # noqa: E731
    return R.gmres_left(A, minv, b, m=30, max_iter=3000, tol=1e-10, dot=R.device_dot(n))


def make(A, kind="ainv"):
    s = ggmres.Solver(0)
    s.set_matrix(A)
    if kind == "ainv":
        s.set_precond_ainv(0.1)
    else:
        s.set_precond_diag()
    return s


@pytest.mark.parametrize("path", ["default", "csr"])
@pytest.mark.parametrize("name", APPLY_MATS)
def test_ainv_apply_bitexact(monkeypatch, name, path):
    if path == "csr":
        monkeypatch.setenv("GG_SPMV_CSR", "1")     # every factor on the CSR-stream kernel
    A = matrix(name)
    Z, Wt, dinv = factors(name)
    assert (sliced(Z) and sliced(Wt)) == (name in SLICED)
    assert max(np.diff(Z.indptr).max(), np.diff(Wt.indptr).max()) <= SPMV_CAP     # serial sums throughout
    if name == "power_law":
        assert np.diff(Z.indptr).max() == 1435     # one row filling most of a packed block
    s = make(A)
    try:
        assert s.ainv_fused == 0                   # no one-launch kernel in this build
        # the form each factor really took on the device (not only the rule restated above)
        want = (0, 0) if path == "csr" else (int(sliced(Z)), int(sliced(Wt)))
        assert s.ainv_sliced() == want
        if path == "default" and name in SLICED:
            assert s.ainv_sliced() == (1, 1)       # k_spmv_sell_mul and k_spmv_sell run below
        rng = np.random.default_rng(3)
        for _ in range(2):
            v = rng.standard_normal(A.shape[0])
            out = s.precond_apply(GG_APPLY_MINV, v)
            assert np.array_equal(out, O.spmv(Wt, dinv * O.spmv(Z, v)))
        assert s.ainv_nnz() == (Z.nnz, Wt.nnz)
    finally:
        s.close()


def test_ainv_apply_long_rows():
    """Factor rows above a block's capacity (2048 entries) take the SpMV's
    long-row path in both products (the multiply epilogue in the first): a
    strided block reduction, within 1e-13 of the serial sum on the scale
    |A||x| as in test_spmv_long_rows.  Here row n-1 of Z and row 0 of Wt hold
    2400 entries.  With t = dinv o (Z v): a long row c of Z puts an error
    E_c <= 1e-13 |dinv_c| (|Z||v|)_c on t_c, which a row r of Wt carries on as
    at most (|Wt| E)_r; a long row r of Wt adds 1e-13 (|Wt||t|)_r of its own
    (that term also covers the re-rounding of a short row's sum over the
    perturbed t, a few eps).  Every row that is short and touches no long row's
    t stays bit-exact."""
    A = matrix("two_rows")
    n = A.shape[0]
    Z, Wt, dinv = factors("two_rows")
    zl, wl = np.diff(Z.indptr), np.diff(Wt.indptr)
    assert zl[n - 1] == n > SPMV_CAP and wl[0] == n > SPMV_CAP
    zlong, wlong = zl > SPMV_CAP, wl > SPMV_CAP
    s = make(A)
    try:
        assert s.ainv_sliced() == (0, 0)
        v = np.random.default_rng(6).standard_normal(n)
        out = s.precond_apply(GG_APPLY_MINV, v)
    finally:
        s.close()
    t = dinv * O.spmv(Z, v)
    ref = O.spmv(Wt, t)
    E = np.where(zlong, 1e-13 * np.abs(dinv) * (abs(Z) @ np.abs(v)), 0.0)
    touched = wlong | ((abs(Wt) @ zlong.astype(float)) > 0)
    assert 0 < touched.sum() < n // 2
    bound = np.where(touched, abs(Wt) @ E + 1e-13 * (abs(Wt) @ np.abs(t)), 0.0)
    dev = np.abs(out - ref)
    print(f"long rows: {int(touched.sum())} rows touched, max deviation {dev.max():.3e}, "
          f"max deviation / bound {np.max(dev[touched] / bound[touched]):.3e}")
    assert np.array_equal(out[~touched], ref[~touched])
    assert np.all(dev <= bound)


def test_ainv_kind_and_queries():
    A = matrix("pert16")
    s = make(A)
    try:
        assert ggmres.lib().gg_precond_kind(s.h) == 7 == ggmres.PRECOND_AINV
        assert s.trsv_kernel(0) == "" and s.trsv_kernel(1) == ""
        assert s.trsv_levels(0) == 0 and s.trsv_levels(1) == 0
        assert not s.uses_wavefront and not s.batch_engine
        Z, Wt, _ = factors("pert16")
        n = A.shape[0]
        want = sum(12.0 * T.nnz + 4.0 * (n + 1) + 16.0 * n for T in (Z, Wt)) + 8.0 * n
        assert s.bytes_precond() == want
        s.set_precond_diag()
        assert ggmres.lib().gg_precond_kind(s.h) == 8 == ggmres.PRECOND_DIAG
        assert s.trsv_kernel(0) == "" and s.ainv_fused == 0 and not s.batch_engine
        v = np.random.default_rng(4).standard_normal(n)
        assert np.array_equal(s.precond_apply(GG_APPLY_MINV, v), v * R.diag_nearest(A))
    finally:
        s.close()


def check_solve(g, o, what):
    assert g["ret"] == o["ret"] == 0, (what, g["ret"], o["ret"])
    assert g["iters"] == o["iters"], (what, g["iters"], o["iters"])
    ok, msg = hist_close(g["hist"], o["hist"], HIST_RTOL)
    xe = rel_err(g["x"], o["x"])
    print(f"{what}: {g['iters']} iterations, history {msg}, x rel err {xe:.3e}")
    assert ok, (what, msg)
    assert xe <= 1e-8, (what, xe)


@pytest.mark.parametrize("name", ["pert16", "pert24", "sherman1", "lap37x64"])
def test_ainv_gmres_vs_numpy(name):
    """GMRES(30), tol 1e-10, b = A 1: more than 30 iterations, so a restart is
    crossed.  Measured on an MI355X: history and x bit-identical to the NumPy
    GMRES on all four (max rel dev 0, x rel err 0; DESIGN.md "AINV / DIAG")."""
    A = matrix(name)
    o = reference_solve(name, "ainv")
    assert o["iters"] > 30
    s = make(A)
    try:
        g = s.solve(A @ np.ones(A.shape[0]), restart=30, max_iter=3000, tol=1e-10)
    finally:
        s.close()
    check_solve(g, o, f"AINV {name}")


def test_diag_gmres_vs_numpy():
    A = matrix("pert16")
    o = reference_solve("pert16", "diag")
    s = make(A, "diag")
    try:
        g = s.solve(A @ np.ones(A.shape[0]), restart=30, max_iter=3000, tol=1e-10)
    finally:
        s.close()
    check_solve(g, o, "DIAG pert16")


def test_ainv_shared_device_solve_identical():
    """GG_SOLVE_SHARED_DEVICE is accepted (the apply's launches wait on nothing)
    and changes only the orthogonalization's launch form: the same bits"""
    A = matrix("pert16")
    b = A @ np.ones(A.shape[0])
    s = make(A)
    try:
        f = s.solve(b, restart=30, max_iter=3000, tol=1e-10)
        sh = s.solve(b, restart=30, max_iter=3000, tol=1e-10, flags=ggmres.SOLVE_SHARED_DEVICE)
        assert s.ainv_fused == 0
    finally:
        s.close()
    assert sh["ret"] == f["ret"] == 0 and sh["iters"] == f["iters"] > 30
    assert np.array_equal(sh["hist"], f["hist"]) and np.array_equal(sh["x"], f["x"])


def test_ainv_solve_batch_scenario_by_scenario():
    A = matrix("pert16")
    n = A.shape[0]
    rng = np.random.default_rng(5)
    B = np.stack([A @ np.ones(n), rng.standard_normal(n), A @ rng.standard_normal(n)])
    s = make(A)
    try:
        assert s.batch_engine is False
        r = s.solve_batch(B, restart=30, max_iter=3000, tol=1e-10)
        assert r["ret"] == 0
        for q in range(3):
            g = s.solve(B[q], restart=30, max_iter=3000, tol=1e-10)
            assert g["ret"] == 0 and r["status"][q] == 0
            assert r["iters"][q] == g["iters"] and r["relres"][q] == g["relres"]
            assert np.array_equal(r["x"][q], g["x"])
    finally:
        s.close()


def test_ainv_profile_brackets_the_apply():
    A = matrix("pert16")
    s = make(A)
    try:
        s.profile(True)
        g = s.solve(A @ np.ones(A.shape[0]), restart=30, max_iter=3000, tol=1e-10)
        launches, ms = s.profile_get(ggmres.PROF_PRECOND)
        assert g["inner"] <= launches <= g["inner"] + g["restarts"] + 1 and ms > 0.0
        s.profile(False)
    finally:
        s.close()


def test_ainv_transient_matches_solve_loop():
    """gg_transient with AINV: every step is the same solve gg_solve runs on
    the step's right-hand side (warm start), so the port waveform and the
    final state are bit-identical to that loop."""
    nx = 16
    h = 1e-2
    A = M.transient(R.pert(nx), c=1e-3, h=h)
    n = A.shape[0]
    cdiag = np.full(n, 1e-3 / h)
    nodes = np.array([3, 40, 200], np.int32)
    pulses = np.array([[0.0, 1.0, 0.0, 2e-2, 2e-2, 5e-2, 0.2]] * 3)
    ports = np.array([0, n // 2, n - 1], np.int32)
    s = make(A)
    try:
        r = s.transient(4, h, cdiag, nodes, pulses, ports, np.zeros(n), restart=30, max_iter=3000, tol=1e-10)
        x = np.zeros(n)
        for it in range(1, 5):
            u = np.array([O.pulse(q, it, h) for q in pulses])
            w = O.transient_rhs(cdiag, nodes, u, x)
            g = s.solve(w, x0=x, restart=30, max_iter=3000, tol=1e-10)
            assert g["ret"] == 0
            x = g["x"]
            assert np.array_equal(r["ports"][:, it], x[ports])
        assert r["ret"] == 0 and np.array_equal(r["x"], x)
    finally:
        s.close()
