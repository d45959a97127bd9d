"""CPU: the restatement tests/bicgstab_ref.py on the BiCGStab batch's cases
(tests/bi_batch_cases.py) -- ILU(0) from the oracle, plain dots, tol 1e-10.
tests/test_gpu_bicgstab_batch.py compares the batch with the single solves bit
for bit; what makes that comparison worth something is the variety of the
scenarios' ends, and this file holds the cases to it without a device: counts
several read-back chunks apart, a breakdown at the start, breakdowns after x
and r have moved at several iterations, convergence at the start."""
import functools

import numpy as np

import bi_batch_cases as K
import bicgstab_ref as R
import oracle as O


@functools.lru_cache(maxsize=None)
def solved(case, max_iter=3000, tol=1e-10):
    """[(ret, iters, why, relres, x)] per scenario of a case"""
    A, B, X0 = getattr(K, case)()
    L, U = O.ilu0(A)
    out = []
    for q in range(B.shape[0]):
        info = {}
        ret, x, it, res, _ = R.bicgstab(A, lambda v: O.lusolve(L, U, v), B[q], X0[q], max_iter, tol, info=info)
        out.append((ret, it, info["why"], res, x))
    return out


def test_band_counts():
    r = solved("band")
    assert [o[0] for o in r] == [0] * 9
    counts = [o[1] for o in r]
    assert counts == [34, 33, 0, 33, 21, 34, 0, 31, 11]
    assert K.diverse(counts)
    # at least 4 distinct counts with 0 among them; the largest more than twice the smallest positive
    assert len(set(counts)) >= 4 and 0 in counts
    assert max(counts) > 2 * min(c for c in counts if c > 0)


def test_band_early_ends_and_exhaustion():
    r = solved("band", 3000, 0.05)
    assert [o[0] for o in r] == [0] * 9
    assert [o[1] for o in r] == [17, 9, 0, 9, 0, 14, 0, 10, 0]
    _, B, _ = K.band()
    r = solved("band", 6, 1e-300)
    for q, o in enumerate(r):
        assert (o[0], o[1]) == ((1, 6) if np.any(B[q]) else (0, 0)), q


def test_nat_counts():
    r = solved("nat")
    assert [(o[0], o[1]) for o in r] == [(0, 27), (0, 28), (0, 0), (0, 28)]


def test_small_exits():
    r = solved("small")
    assert [(o[0], o[1], o[2]) for o in r] == [(0, 14, "conv"), (R.BREAKDOWN, 0, "rho0"), (0, 0, "conv0"),
                                               (0, 14, "conv")]
    assert np.isnan(r[1][3]) and np.all(np.isfinite(r[1][4]))


def test_tiny_breakdowns_after_x_and_r_moved():
    r = solved("tiny")
    got = {e: (o[0], o[1], o[2]) for e, o in zip(K.TINY_EXPONENTS, r)}
    assert got[-162] == (R.BREAKDOWN, 0, "rtv")
    assert [got[e] for e in (-161, -159, -157, -155, -154)] == \
        [(R.BREAKDOWN, k, "omega") for k in (2, 6, 8, 10, 12)]
    assert all(got[e][0] == 0 for e in (-160, -158, -156, -153))
    stat = [(o[0], o[1]) for o in r]
    assert len({k for ret, k in stat if ret == R.BREAKDOWN and k > 0}) >= 3
    assert sum(1 for ret, k in stat if ret == R.BREAKDOWN and k == 0) == 1
    assert any(ret == 0 and k > 10 for ret, k in stat)
    assert stat[-2] == (0, 14) and stat[-1] == (0, 0)


def test_tiny_ordinary_above_the_underflow():
    A = K.small_matrix()
    n = A.shape[0]
    L, U = O.ilu0(A)
    g = np.random.default_rng(6).standard_normal(n)
    for e in (-151, -100, 0):
        ret, _, it, _, _ = R.bicgstab(A, lambda v: O.lusolve(L, U, v), 10.0 ** e * g, None, 3000, 1e-10)
        assert (ret, it) == (0, 14), e
