"""GPU: the preconditioned BiCGStab solve (GG_SOLVE_BICGSTAB, csrc/bicgstab.hip)
against its NumPy restatement tests/bicgstab_ref.py.

Bar: return code, iteration count, the whole residual history, relres and x are
bit-identical (np.array_equal) to bicgstab_ref.bicgstab run with the dots summed
in the solver's own order (cg_ref.layout_dot over Solver.layout()) -- the SpMV
rows, the triangular-solve rows and the vector updates are serial fp64
expressions the restatement repeats, the dots are the only reordered sums.
Every solve here is b = A 1, x0 = 0, tol 1e-12, exact division unless a test
says otherwise; every matrix of the parity cases is nonsymmetric.

Iteration counts of the reference with plain NumPy dots at tol 1e-12: 38 (60 x
52 upwind grid, ILU0), 24 (the same, ILU(1)), 60 (20^3 upwind grid), 40
(permuted 40 x 33), 100 / 100 / 57 (37 x 64 with NONE / DIAG / AINV(0.1)), 16
(16 x 17).  Each case but the 272-row one asserts, on the reference alone, more
iterations than one default chunk of the driver (16).
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import ainv_ref as R
import bicgstab_ref as B
import cg_ref as C
import ggmres
import oracle as O
from ggmres import matrices as M
from helpers import rel_err

pytestmark = pytest.mark.gpu
BI = ggmres.SOLVE_BICGSTAB
CHUNK = 16                      # csrc/bicgstab.hip BiCgStab::kChunk
TOL = 1e-12


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name == "band2d":
        return M.laplacian_5pt(60, 52, upwind=0.2)     # one 64-line band, padded steps
    if name == "tile3d":
        return M.grid_7pt(20, upwind=0.1)              # 3 x 3 tiles of 8 lines x 8 planes
    if name == "flow":
        A = sp.csr_matrix(M.laplacian_5pt(40, 33, upwind=0.2))
        p = np.random.default_rng(11).permutation(A.shape[0])
        Bp = A[p][:, p].tocsr()                        # P A P^T: no grid left
        Bp.sort_indices()
        return Bp
    if name == "nat":
        return M.laplacian_5pt(37, 64, upwind=0.2)     # natural layout, 37 slices
    if name == "small":
        return M.laplacian_5pt(16, 17, upwind=0.2)     # 272 rows
    if name == "sym":
        return M.laplacian_5pt(60, 52)
    if name == "shift":
        n = 272                                        # row i: a single 1 at column (i + 1) mod n
        A = sp.csr_matrix((np.ones(n), (np.arange(n), (np.arange(n) + 1) % n)), shape=(n, n))
        A.sort_indices()
        return A
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def minv(name, kind):
    """the restatement's preconditioner, built once"""
    A = matrix(name)
    if kind == "ilu0":
        L, U = O.ilu0(A)
        return lambda v: O.lusolve(L, U, v)
    if kind == "iluk1":
        L, U = O.iluk(A, 1)
        return lambda v: O.lusolve(L, U, v)
    if kind == "none":
        return lambda v: np.array(v, np.float64, copy=True)
    if kind == "diag":
        inv = R.diag_nearest(A)
        return lambda v: v * inv
    if kind == "ainv":
        Z, Wt, dinv = R.ainv(A, 0.1)
        return lambda v: R.ainv_apply(Z, Wt, dinv, v)
    raise KeyError(kind)


def make(name, kind):
    s = ggmres.Solver(0)
    s.set_matrix(matrix(name))
    if kind == "iluk1":
        s.set_precond_iluk(1)
    else:
        getattr(s, "set_precond_" + kind)(*((0.1,) if kind == "ainv" else ()))
    return s


def rhs(name):
    A = matrix(name)
    return A @ np.ones(A.shape[0])


_REF = {}


def reference(s, name, kind, max_iter=3000, tol=TOL, b=None, x0=None):
    """bicgstab_ref.bicgstab in the solver's reduction order; the default solve
    of a case is computed once and shared (the layout of a case does not change)"""
    key = (name, kind, max_iter, tol) if b is None and x0 is None else None
    if key in _REF:
        return _REF[key]
    lay2nat, G = s.layout()
    assert G == s.reduce_blocks
    out = B.bicgstab(matrix(name), minv(name, kind), rhs(name) if b is None else b, x0, max_iter, tol,
                     C.layout_dot(lay2nat, G))
    if key:
        _REF[key] = out
    return out


def same_bits(g, o, what):
    ret, x, iters, relres, hist = o
    print(f"{what}: device ret {g['ret']} iters {g['iters']} relres {g['relres']:.3e}; "
          f"reference ret {ret} iters {iters} relres {relres:.3e}")
    assert g["ret"] == ret, what
    assert g["iters"] == g["inner"] == iters and g["restarts"] == 0, what
    assert g["hist"].shape == hist.shape, what
    if not np.array_equal(g["hist"], hist):
        k = int(np.flatnonzero(g["hist"] != hist)[0])
        raise AssertionError(f"{what}: history differs first at entry {k}: {g['hist'][k]!r} vs {hist[k]!r}")
    assert g["relres"] == relres, what
    assert np.array_equal(g["x"], x), (what, rel_err(g["x"], x))


CASES = [("band2d", "ilu0"), ("band2d", "iluk1"), ("tile3d", "ilu0"), ("flow", "ilu0"), ("nat", "none"),
         ("nat", "diag"), ("nat", "ainv"), ("small", "ilu0")]


@pytest.mark.parametrize("name,kind", CASES)
def test_bicgstab_bit_identical_to_the_restatement(name, kind):
    A = matrix(name)
    assert abs(A - A.T).max() > 0.0
    s = make(name, kind)
    try:
        if name in ("band2d", "tile3d"):
            assert s.uses_wavefront
        if name == "flow":
            assert not s.uses_wavefront
            assert s.trsv_kernel(0) == "k_trsv_flow"
        if name == "tile3d":
            assert "tile3d" in s.trsv_kernel(0)
        o = reference(s, name, kind)
        if name == "small":
            assert 12 <= o[2] <= 20                # 16 with plain dots; the order may move it a little
        else:
            assert o[2] > CHUNK                    # more than one chunk of gated iterations
        g = s.solve(rhs(name), restart=30, max_iter=3000, tol=TOL, flags=BI)
        assert s.mgs_kernel() == ""
    finally:
        s.close()
    assert g["ret"] == 0
    same_bits(g, o, f"BiCGStab {name} {kind}")
    assert rel_err(g["x"], np.ones(len(g["x"]))) < 1e-9


def test_bicgstab_exhaustion():
    s = make("band2d", "ilu0")
    try:
        full = reference(s, "band2d", "ilu0")
        assert full[2] > 20
        g = s.solve(rhs("band2d"), max_iter=20, tol=TOL, flags=BI)
        o = reference(s, "band2d", "ilu0", max_iter=20)
    finally:
        s.close()
    assert g["ret"] == 1 and g["iters"] == 20
    assert g["hist"].size == 21 and np.array_equal(g["hist"], full[4][:21])
    same_bits(g, o, "BiCGStab max_iter 20")


def test_bicgstab_launches_past_convergence_change_nothing():
    """The history is not monotone: on the band case it reaches 0.1140 at
    iteration 5 and climbs above 0.3 again before it falls for good.  tol 0.115
    stops there; the first chunk is 16 iterations and the host is one chunk
    ahead, so more than 25 iterations' launches run gated off behind the end"""
    tol = 0.115
    s = make("band2d", "ilu0")
    try:
        full = reference(s, "band2d", "ilu0")
        o = reference(s, "band2d", "ilu0", tol=tol)
        assert o[0] == 0 and 5 <= o[2] <= 25
        assert np.all(full[4][:o[2]] >= tol) and full[4][o[2]] < tol
        assert np.any(full[4][o[2] + 1:] > tol)                            # it would have come back up
        g = s.solve(rhs("band2d"), max_iter=3000, tol=tol, flags=BI)
        same_bits(g, o, f"BiCGStab tol {tol}")
        n = s.n
        z = s.solve(np.zeros(n), max_iter=3000, tol=TOL, flags=BI)         # b = 0, x0 = 0
        assert z["ret"] == 0 and z["iters"] == 0 and z["hist"].tolist() == [0.0]
        assert np.array_equal(z["x"], np.zeros(n))
        one = np.ones(n)                                                   # x0 = the exact solution
        e = s.solve(rhs("band2d"), x0=one, max_iter=3000, tol=TOL, flags=BI)
        oe = reference(s, "band2d", "ilu0", x0=one)
        assert e["ret"] == 0 and e["iters"] == 0 and np.array_equal(e["x"], one)
        same_bits(e, oe, "BiCGStab exact x0")
    finally:
        s.close()


def test_bicgstab_breakdown_on_the_cyclic_shift():
    """b = e_0, x0 = 0, no preconditioner: r = rt = p = e_0 and v = A e_0 = e_271
    (column 0 appears in the last row alone), so every product of rt . v is an
    exact zero and the sum is 0 in any order: breakdown before anything moved"""
    n = 272
    b = np.zeros(n)
    b[0] = 1.0
    x0 = np.zeros(n)
    s = make("shift", "none")
    try:
        o = reference(s, "shift", "none", b=b, x0=x0)
        assert o[0] == B.BREAKDOWN and o[2] == 0
        g = s.solve(b, x0=x0, max_iter=3000, tol=TOL, flags=BI)
        msg = ggmres.lib().gg_last_error().decode()
        detail = ggmres.lib().gg_strerror(ggmres.EBREAKDOWN)
    finally:
        s.close()
    assert g["ret"] == ggmres.EBREAKDOWN == -8 and g["iters"] == 0
    assert np.all(np.isfinite(g["x"])) and np.array_equal(g["x"], x0)
    same_bits(g, o, "BiCGStab breakdown")
    assert "rt.v" in msg and "iteration 0" in msg
    assert b"BICGSTAB" in detail


def test_bicgstab_refusals():
    from helpers import make_split
    A = matrix("small")
    b = rhs("small")
    s = ggmres.Solver(0)
    try:
        s.set_matrix(A)
        P = make_split(A, identity_perm=True)
        s.set_precond_split(P.L, P.U, P.middle, P.perm_row, P.perm_col, P.lscale, P.rscale)
        with pytest.raises(ggmres.GGError) as e:
            s.solve(b, flags=BI)
        assert e.value.code == -1
        s.set_precond_user(lambda op, i, o, n: 0)
        with pytest.raises(ggmres.GGError) as e:
            s.solve(b, flags=BI)
        assert e.value.code == -1
        s.set_precond_user(lambda op, i, o, n: 0, split=True)
        with pytest.raises(ggmres.GGError) as e:
            s.solve(b, flags=BI)
        assert e.value.code == -1
        s.set_precond_ilu0()
        with pytest.raises(ggmres.GGError) as e:
            s.solve(b, flags=BI | ggmres.SOLVE_CG)
        assert e.value.code == -1
        with pytest.raises(ggmres.GGError) as e:
            s.solve_batch(np.stack([b, b]), flags=BI)
        assert e.value.code == -1
        assert s.solve(b, flags=BI)["ret"] == 0            # the solver is still usable
    finally:
        s.close()


@pytest.mark.parametrize("mode", [ggmres.DIV_FMA, ggmres.DIV_RCP])
def test_bicgstab_fast_division(mode):
    """tolerance parity: converges, x within 1e-8 relative of the exact-division
    x (test_gpu_cg's bar)"""
    s = make("band2d", "ilu0")
    try:
        ex = s.solve(rhs("band2d"), max_iter=3000, tol=TOL, flags=BI)
        s.set_division(mode)
        assert s.division_active(1) == mode
        f = s.solve(rhs("band2d"), max_iter=3000, tol=TOL, flags=BI)
    finally:
        s.close()
    assert ex["ret"] == 0 and f["ret"] == 0
    xe = rel_err(f["x"], ex["x"])
    print(f"division mode {mode}: {f['iters']} iterations (exact {ex['iters']}), x rel err {xe:.3e}")
    assert xe <= 1e-8


def test_bicgstab_shared_device_same_bits():
    s = make("band2d", "ilu0")
    try:
        a = s.solve(rhs("band2d"), max_iter=3000, tol=TOL, flags=BI)
        b = s.solve(rhs("band2d"), max_iter=3000, tol=TOL, flags=BI | ggmres.SOLVE_SHARED_DEVICE)
    finally:
        s.close()
    assert a["ret"] == b["ret"] == 0 and a["iters"] == b["iters"] > CHUNK
    assert np.array_equal(a["hist"], b["hist"]) and np.array_equal(a["x"], b["x"])


def test_bicgstab_transient_matches_solve_loop():
    """gg_transient with the flag: every step is the solve gg_solve runs on the
    step's right-hand side (warm start; the first chunk sized from the previous
    step changes no bits), the pattern of test_cg_transient_matches_solve_loop"""
    h = 1e-2
    A = M.transient(M.laplacian_5pt(24, upwind=0.2), c=1e-3, h=h)
    assert abs(A - A.T).max() > 0.0
    n = A.shape[0]
    cdiag = np.full(n, 1e-3 / h)
    nodes = np.array([3, 40, 200], np.int32)
    pulses = np.array([[0.0, 1.0, 0.0, 2e-2, 2e-2, 5e-2, 0.2]] * 3)
    ports = np.array([0, n - 1], np.int32)
    s = ggmres.Solver(0)
    try:
        s.set_matrix(A)
        s.set_precond_ilu0()
        r = s.transient(5, h, cdiag, nodes, pulses, ports, np.zeros(n), restart=30, max_iter=3000, tol=1e-10,
                        flags=BI)
        x = np.zeros(n)
        total = 0
        for it in range(1, 6):
            u = np.array([O.pulse(q, it, h) for q in pulses])
            w = O.transient_rhs(cdiag, nodes, u, x)
            g = s.solve(w, x0=x, restart=30, max_iter=3000, tol=1e-10, flags=BI)
            assert g["ret"] == 0 and g["restarts"] == 0
            total += g["iters"]
            x = g["x"]
            assert np.array_equal(r["ports"][:, it], x[ports])
        assert r["ret"] == 0 and np.array_equal(r["x"], x) and r["iters_total"] == total > 0
    finally:
        s.close()


def test_gmres_and_cg_after_bicgstab_are_unchanged():
    """GMRES on a solver that ran BiCGStab gives the bits of a fresh solver and
    reports its own orthogonalization kernel again; so does CG on the symmetric
    grid (BiCGStab's r, p and v live in the work space both of them use)"""
    for name, flags in (("band2d", 0), ("sym", ggmres.SOLVE_CG)):
        b = rhs(name)
        fresh = make(name, "ilu0")
        try:
            f = fresh.solve(b, restart=30, max_iter=3000, tol=1e-10, flags=flags)
            fk = fresh.mgs_kernel()
        finally:
            fresh.close()
        s = make(name, "ilu0")
        try:
            c1 = s.solve(b, max_iter=3000, tol=TOL, flags=BI)      # before any GMRES work space exists
            assert s.mgs_kernel() == ""
            g1 = s.solve(b, restart=30, max_iter=3000, tol=1e-10, flags=flags)
            k1 = s.mgs_kernel()
            c2 = s.solve(b, max_iter=3000, tol=TOL, flags=BI)
            assert s.mgs_kernel() == ""
            g2 = s.solve(b, restart=30, max_iter=3000, tol=1e-10, flags=flags)
        finally:
            s.close()
        assert f["ret"] == 0 and f["iters"] > 30 and k1 == fk
        assert c1["ret"] == 0 and c1["iters"] > CHUNK
        for g in (g1, g2):
            assert g["ret"] == 0 and g["iters"] == f["iters"] and g["restarts"] == f["restarts"]
            assert np.array_equal(g["hist"], f["hist"]) and np.array_equal(g["x"], f["x"])
        assert np.array_equal(c1["hist"], c2["hist"]) and np.array_equal(c1["x"], c2["x"])


def test_bicgstab_agrees_with_cg_on_a_symmetric_grid():
    s = make("sym", "ilu0")
    try:
        c = s.solve(rhs("sym"), max_iter=3000, tol=TOL, flags=ggmres.SOLVE_CG)
        g = s.solve(rhs("sym"), max_iter=3000, tol=TOL, flags=BI)
    finally:
        s.close()
    assert c["ret"] == 0 and g["ret"] == 0
    xe = rel_err(g["x"], c["x"])
    print(f"symmetric 60 x 52: BiCGStab {g['iters']} iterations, CG {c['iters']}, x rel err {xe:.3e}")
    assert xe <= 1e-8


def test_bicgstab_profile_brackets():
    """both halves of an iteration are bracketed: two SpMVs and two
    preconditioner applications (a forward and a backward solve each) per
    executed iteration, no orthogonalization"""
    s = make("band2d", "ilu0")
    try:
        s.profile(True)
        g = s.solve(rhs("band2d"), max_iter=3000, tol=TOL, flags=BI)
        counts = {k: s.profile_get(k) for k in (ggmres.PROF_SPMV, ggmres.PROF_PRECOND, ggmres.PROF_TRSV_L,
                                                ggmres.PROF_TRSV_U, ggmres.PROF_MGS)}
        s.profile(False)
    finally:
        s.close()
    assert g["ret"] == 0 and g["iters"] > CHUNK
    for k in (ggmres.PROF_SPMV, ggmres.PROF_PRECOND, ggmres.PROF_TRSV_L, ggmres.PROF_TRSV_U):
        assert counts[k][0] == 2 * g["iters"] and counts[k][1] > 0.0
    assert counts[ggmres.PROF_MGS][0] == 0
