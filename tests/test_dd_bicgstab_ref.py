"""CPU: the sharded BiCGStab restatement (tests/dd_bicgstab_ref.py) takes, on every
system of the GPU tests (tests/test_gpu_dd_bicgstab*.py), the exit its GPU test
claims -- on B = P A P^T with the ILU(0) of B and the natural block layout's
segments (dd_cg_ref.natural_segments; the device's segments differ inside a
segment only, so the decisive order check is the GPU's) -- and the sharded order
is visible in the history at all.

Iteration counts here (b = A 1, tol 1e-10): 89 / 90 / 99 on the 200 x 160 grids,
78 on 160 x 200, 60 and 58 on the 3D grids, 45 on sherman1, 35 on 60 x 60, 24 on
the small 40 x 30 system, 52 on the mixed one.
"""
import functools

import numpy as np
import pytest

import bicgstab_ref as R
import dd_bicgstab_ref as Q
import dd_cg_ref as D
import oracle as O
from ggmres import host

K = Q.K_CHUNK


@functools.lru_cache(maxsize=None)
def plan_of(key):
    """(B, L, U, q, segments, G, b) of a LAYOUT_CASES name, "small", "mixed" (b = A 1)
    or an EXACT_BLOCKS name (its own b), b in B's order"""
    if key in Q.EXACT_BLOCKS:
        A, b = Q.exact_system(key)
        P, method = 2, host.PART_BLOCKS
    else:
        A, P, method = Q.system(Q.named(key))
        b = A @ np.ones(A.shape[0])
    plan = host.DDPlan(A, P, method)
    B = host.permute(A, plan.pinv, plan.q)
    L, U = O.ilu0(B)
    segs, G = D.natural_segments(plan)
    return B, L, U, plan, segs, G, b[plan.q]


def run(key, b=None, **kw):
    B, L, U, plan, segs, G, b1 = plan_of(key)
    info = {}
    return Q.solve(B, L, U, b1 if b is None else b, segs, G, info=info, **kw), info


@functools.lru_cache(maxsize=None)
def default(key):
    return run(key)


def test_chunk_is_half_of_cgs():
    assert Q.K_CHUNK * 2 == D.K_CHUNK


@pytest.mark.parametrize("key", sorted(Q.LAYOUT_CASES) + ["small", "mixed"])
def test_layout_cases_converge(key):
    B = plan_of(key)[0]
    (ret, x, iters, relres, hist), info = default(key)
    print(f"{key}: {iters} iterations, relres {relres:.3e}")
    assert ret == 0 and info["why"] == "conv" and 2 * K + 2 < iters < 3000
    assert hist.size == iters + 1 and relres < 1e-10 <= hist[-2]
    assert np.linalg.norm(x - 1.0) < 1e-6 * np.sqrt(B.shape[0])


def test_the_sharded_order_is_visible():
    """the history with the dots in the sharded order differs from the plain np.dot
    one in at least one bit on at least one system"""
    seen = 0
    for key in ("small", "7pt_16_P4_bisect", "sherman1_P4"):
        B, L, U, plan, segs, G, b = plan_of(key)
        assert len(segs) > 1
        plain = R.bicgstab(B, lambda v: O.lusolve(L, U, v), b)
        hist = default(key)[0][4]
        k = min(hist.size, plain[4].size)
        seen += not np.array_equal(hist[:k], plain[4][:k])
    assert seen >= 1


def test_chunk_boundaries_on_the_small_system():
    (ret, x, iters, relres, hist), info = default("small")
    assert ret == 0 and iters > 2 * K + 2
    for mi in (0, 1, K, 2 * K, iters - 1):
        (r1, x1, it1, rr1, h1), i1 = run("small", max_iter=mi)
        assert r1 == 1 and i1["why"] == "exhausted" and it1 == mi
        assert np.array_equal(h1, hist[:mi + 1])
    (r1, x1, it1, rr1, h1), i1 = run("small", max_iter=iters)
    assert r1 == 0 and i1["why"] == "conv" and it1 == iters
    # a chunk's last iteration, the next chunk's first (BiCGStab's history is not
    # monotone: these four are record lows, the second chunk's boundary is not)
    for k in (K, K + 1, 3 * K, 3 * K + 1):
        (r1, x1, it1, rr1, h1), i1 = run("small", tol=Q.tol_ending_at(hist, k))
        assert r1 == 0 and i1["why"] == "conv" and it1 == k


def test_start_exits():
    B, L, U, plan, segs, G, b = plan_of("small")
    (ret, x, iters, relres, hist), info = run("small", b=np.zeros(B.shape[0]))
    assert ret == 0 and info["why"] == "conv0" and iters == 0 and hist.tolist() == [0.0]
    xs = default("small")[0][1]
    (ret, x, iters, relres, hist), info = run("small", x0=xs, tol=1e-8)
    assert ret == 0 and info["why"] == "conv0" and iters == 0 and np.array_equal(x, xs)


def test_nan_in_b_is_rho_at_the_start():
    B, L, U, plan, segs, G, b = plan_of("small")
    b = b.copy()
    b[plan.pinv[7]] = np.nan
    (ret, x, iters, relres, hist), info = run("small", b=b)
    assert ret == Q.BREAKDOWN and info["why"] == "rho0" and iters == 0 and np.isnan(info["bad"])
    assert hist.size == 1 and np.isnan(hist[0]) and np.array_equal(x, np.zeros(B.shape[0]))


@pytest.mark.parametrize("name", sorted(Q.EXACT_BLOCKS))
def test_exact_breakdowns(name):
    """the exit and every number are the same in the sharded order and in np.dot's:
    the scalars are exact sums; the connectors are the separator and no block is cut"""
    why, its = Q.EXACT_BLOCKS[name][2:]
    B, L, U, plan, segs, G, b = plan_of(name)
    m = 3 * Q.EXACT_COUNT
    assert plan.nsep == 2 and sorted(plan.q[plan.begin[2]:]) == [m, m + 1]
    assert all(np.all(np.diff(plan.q[plan.begin[p]:plan.begin[p + 1]]) == 1) for p in range(2))
    (ret, x, iters, relres, hist), info = run(name)
    assert ret == Q.BREAKDOWN and info["why"] == why and iters == its and info["bad"] == 0.0
    assert hist.size == its + 1 and np.all(np.isfinite(hist)) and np.all(np.isfinite(x))
    info2 = {}
    p = R.bicgstab(B, lambda v: O.lusolve(L, U, v), b, info=info2)
    assert info2 == info and p[2] == iters and np.array_equal(p[1], x)
    # the history's square roots aside, which see a rounded quotient of exact sums
    assert np.array_equal(p[4], hist)
