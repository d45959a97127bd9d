"""GPU: every exit of the CG and BiCGStab control kernels (k_cg_xr, k_cg_p,
k_bi_s, k_bi_xr, k_bi_p; csrc/kernels/short_recurrence.hip) against the
restatements tests/cg_ref.py and tests/bicgstab_ref.py, branch by branch.

The cases are tests/sr_exit_cases.py's; tests/test_sr_exit_cases.py shows on the
CPU that each reaches the exit it is named for, and every test here asserts it
again on the reference it compares with (the restatement with its dots summed
in the solver's order, cg_ref.layout_dot over Solver.layout()).

Bar: test_gpu_cg.same_bits / test_gpu_bicgstab.same_bits -- return code,
iteration count, the whole residual history, relres and x identical to the
reference -- with NaN equal to NaN (np.array_equal(..., equal_nan=True)), since
two cases end with a NaN residual.  No tolerance anywhere; the iteration windows
of the rounded cases are conditions on the reference alone.

The max_iter tests run the chunk loop's boundaries (short_recurrence.h: the host
enqueues chunks of kChunk iterations, one chunk ahead of the state it has read)
on the 60 x 52 ILU(0) cases of test_gpu_cg.py and test_gpu_bicgstab.py.
"""
import re

import numpy as np
import pytest

import cg_ref as C
import ggmres
import sr_exit_cases as X
import test_gpu_bicgstab as TB
import test_gpu_cg as TC

pytestmark = pytest.mark.gpu
FLAG = {"cg": ggmres.SOLVE_CG, "bicgstab": ggmres.SOLVE_BICGSTAB}
CG_CHUNK = 32                   # csrc/cg.hip Cg::kChunk
BI_CHUNK = TB.CHUNK             # csrc/bicgstab.hip BiCgStab::kChunk
BI_NAME = {"rho0": "rho", "rho": "rho", "rtv": "rt.v", "omega": "omega"}


def eq(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def same_bits(g, o, what):
    """test_gpu_cg.same_bits with NaN equal to NaN in the history, relres and x"""
    ret, x, iters, relres, hist = o
    print(f"{what}: device ret {g['ret']} iters {g['iters']} relres {g['relres']!r}; "
          f"reference ret {ret} iters {iters} relres {relres!r}")
    assert g["ret"] == ret, what
    assert g["iters"] == g["inner"] == iters and g["restarts"] == 0, what
    assert g["hist"].shape == hist.shape, what
    if not eq(g["hist"], hist):
        k = int(np.flatnonzero(~((g["hist"] == hist) | (np.isnan(g["hist"]) & np.isnan(hist))))[0])
        raise AssertionError(f"{what}: history differs first at entry {k}: {g['hist'][k]!r} vs {hist[k]!r}")
    assert eq(g["relres"], relres), what
    assert eq(g["x"], x), what


def same_solve(a, b, what):
    """two device solves with the same bits"""
    assert (a["ret"], a["iters"], a["inner"], a["restarts"]) == (b["ret"], b["iters"], b["inner"], b["restarts"]), what
    assert eq(a["relres"], b["relres"]) and eq(a["hist"], b["hist"]) and eq(a["x"], b["x"]), what


def last_error():
    return ggmres.lib().gg_last_error().decode()


@pytest.mark.parametrize("name", X.names())
def test_exit_bit_identical_to_the_restatement(name):
    c = X.cases()[name]
    flags = FLAG[c.method]
    run = lambda s, b, fl=flags: s.solve(b, x0=c.x0, max_iter=3000, tol=c.tol, flags=fl)      # noqa: E731
    s = ggmres.Solver(0)
    try:
        X.configure(s, c)
        lay2nat, G = s.layout()
        assert G == s.reduce_blocks
        info = {}
        o = X.reference(c, C.layout_dot(lay2nat, G), info=info)
        print(f"{name}: reference ret {o[0]} iters {o[2]} why {info['why']} bad {info['bad']!r}")
        assert info["why"] == c.why and o[0] == c.ret and c.iters_ok(o[2])         # still the intended exit
        if name == "lucky_oblique":
            # right after the `omega` breakdown on this solver: nothing of it survives
            # in the control block
            first = run(s, X.cases()["omega"].b)
            assert first["ret"] == ggmres.EBREAKDOWN and "omega" in last_error()
        g = run(s, c.b)
        msg = last_error()
        same_bits(g, o, f"{c.method} {name}")
        if c.x is not None:                                                        # the table's exact values
            assert eq(g["x"], c.x) and eq(g["relres"], c.relres) and eq(g["hist"], c.hist)
        if c.ret != X.BREAKDOWN:
            assert g["ret"] == 0
            return
        assert g["ret"] == ggmres.EBREAKDOWN == -8
        print(f"{name}: {msg}")
        assert re.search(rf"iteration {o[2]}\b", msg), msg
        if c.method == "bicgstab":
            assert BI_NAME[c.why] + " = " in msg
            if name == "rho0_inf":
                assert "inf" in msg
        # the solver after a breakdown: b = 0 converges at the start, then the same
        # breakdown with the same bits (the control block and the re-armed state)
        z = run(s, np.zeros(s.n))
        assert z["ret"] == 0 and z["iters"] == 0 and z["hist"].tolist() == [0.0]
        assert np.array_equal(z["x"], c.x0)
        again = run(s, c.b)
        assert last_error() == msg
        same_solve(again, g, f"{name} again")
        if name in ("pq_mid", "rho_mid"):
            shared = run(s, c.b, flags | ggmres.SOLVE_SHARED_DEVICE)
            same_solve(shared, g, f"{name} shared device")
    finally:
        s.close()


def boundaries(T, flags, K, tol):
    """max_iter on the chunk loop's boundaries: 0, 1, one chunk, two chunks, one
    short of the count, the count"""
    s = T.make("band2d", "ilu0")
    try:
        full = T.reference(s, "band2d", "ilu0")
        N = full[2]
        assert full[0] == 0 and N > 2 * K              # two whole chunks end short of the count
        for m in dict.fromkeys((0, 1, K, 2 * K, N - 1, N)):
            o = T.reference(s, "band2d", "ilu0", max_iter=m)
            g = s.solve(T.rhs("band2d"), max_iter=m, tol=tol, flags=flags)
            if m < N:
                assert g["ret"] == 1 and g["iters"] == m and g["hist"].size == m + 1, m
            else:
                assert g["ret"] == 0 and g["iters"] == N, m
            same_bits(g, o, f"max_iter {m}")
            assert np.array_equal(g["hist"], full[4][:g["iters"] + 1]), m
    finally:
        s.close()


def test_cg_max_iter_on_the_chunk_boundaries():
    boundaries(TC, ggmres.SOLVE_CG, CG_CHUNK, 1e-10)


def test_bicgstab_max_iter_on_the_chunk_boundaries():
    boundaries(TB, ggmres.SOLVE_BICGSTAB, BI_CHUNK, TB.TOL)
