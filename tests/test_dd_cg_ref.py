"""CPU: the sharded CG restatement (tests/dd_cg_ref.py) against the pieces it is
built from, and the exits the GPU tests (tests/test_gpu_dd_cg.py) rely on.

  * one segment: shard_dot is cg_ref.layout_dot, bit for bit;
  * several segments: shard_dot is the oracle's sharded order -- the NumPy GMRES
    restatement (ainv_ref.gmres_left) run with it gives the history and x of
    oracle.gmres_left under oracle.set_dot_order_shards, bit for bit;
  * every system of the GPU tests takes, on B = P A P^T with the ILU(0) of B and
    the natural block layout's segments, the exit its GPU test claims: conv,
    conv0, exhausted, rz0, pq, rz -- and the chunk-boundary tolerances exist.

The partition is host.DDPlan's (the solver's own, tests/test_gpu_dd.py
test_dd_layout); the device's segments differ from natural_segments inside a
segment only, so the decisive order check is the GPU's.
"""
import functools

import numpy as np
import pytest

import ainv_ref as R
import cg_ref as C
import dd_cg_ref as D
import oracle as O
from ggmres import host

K = D.K_CHUNK


@functools.lru_cache(maxsize=None)
def plan_of(key):
    """(B, L, U, q, segments, G) of a LAYOUT_CASES name, "small", "mixed" or a BREAKDOWNS kind"""
    if key in D.LAYOUT_CASES:
        A, P, method = D.system(D.LAYOUT_CASES[key])
    elif key in D.BREAKDOWNS:
        _, P, method = D.system(D.SMALL)
        A = D.breakdown_matrix(key)
    else:
        A, P, method = D.system({"small": D.SMALL, "mixed": D.MIXED}[key])
    plan = host.DDPlan(A, P, method)
    B = host.permute(A, plan.pinv, plan.q)
    L, U = O.ilu0(B)
    segs, G = D.natural_segments(plan)
    return B, L, U, plan.q.copy(), segs, G


def run(key, b=None, **kw):
    """b, x0 and x in B's order; b = 1 by default"""
    B, L, U, q, segs, G = plan_of(key)
    b = np.ones(B.shape[0]) if b is None else b
    info = {}
    return D.solve(B, L, U, b, segs, G, info=info, **kw), info


def rhs_ones(key):
    B = plan_of(key)[0]
    return B @ np.ones(B.shape[0])          # A 1 in B's order is B 1 (a permutation of the ones)


@pytest.mark.parametrize("ppad,G", [(512, 1), (2048, 3), (153600, 300), (40960, 7)])
def test_one_segment_is_layout_dot(ppad, G):
    rng = np.random.default_rng(5)
    n = ppad - 37
    lay = np.full(ppad, -1, np.int64)
    lay[rng.permutation(ppad)[:n]] = np.arange(n)       # a scattered layout with padding
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    a, b = D.shard_dot([lay], G)(x, y), C.layout_dot(lay, G)(x, y)
    assert a == b


@pytest.mark.parametrize("key", ["small", "7pt_16_P4_bisect", "5pt_160x200_P8_grid"])
def test_several_segments_are_the_oracles_sharded_order(key):
    B, L, U, q, segs, G = plan_of(key)
    assert len(segs) > 1
    b = rhs_ones(key)
    O.set_dot_order_shards(list(segs), G)
    try:
        ref = O.gmres_left(B, L, U, b, m=30, max_iter=40, tol=1e-300)
    finally:
        O.set_dot_order(None)
    serial = O.gmres_left(B, L, U, b, m=30, max_iter=40, tol=1e-300)
    mine = R.gmres_left(B, lambda v: O.lusolve(L, U, v), b, m=30, max_iter=40, tol=1e-300,
                        dot=D.shard_dot(segs, G))
    assert np.array_equal(mine["hist"], ref["hist"]) and np.array_equal(mine["x"], ref["x"])
    assert not np.array_equal(ref["hist"], serial["hist"])      # the order is visible at all


@pytest.mark.parametrize("key", sorted(D.LAYOUT_CASES) + ["mixed"])
def test_layout_cases_converge(key):
    B = plan_of(key)[0]
    (ret, x, iters, relres, hist), info = run(key, b=rhs_ones(key))
    print(f"{key}: {iters} iterations, relres {relres:.3e}")
    assert ret == 0 and info["why"] == "conv" and iters > 30
    assert hist.size == iters + 1 and relres < 1e-10 <= hist[-2]
    assert np.linalg.norm(x - 1.0) < 1e-7 * np.sqrt(B.shape[0])


def test_warm_start_exhausts():
    B = plan_of("5pt_200x160_P2")[0]
    x0 = np.random.default_rng(9).standard_normal(B.shape[0])
    (ret, x, iters, relres, hist), info = run("5pt_200x160_P2", b=rhs_ones("5pt_200x160_P2"), x0=x0, max_iter=40)
    assert ret == 1 and info["why"] == "exhausted" and iters == 40 and hist.size == 41


def test_chunk_boundaries_on_the_small_system():
    b = rhs_ones("small")
    (ret, x, iters, relres, hist), info = run("small", b=b)
    assert ret == 0 and iters > 2 * K + 2
    for mi in (0, 1, K - 1, K, K + 1, 2 * K):
        (r1, x1, it1, rr1, h1), i1 = run("small", b=b, max_iter=mi, tol=1e-300)
        assert r1 == 1 and i1["why"] == "exhausted" and it1 == mi
        assert np.array_equal(h1, hist[:mi + 1])
    for k in (K, K + 1):                        # a chunk's last iteration, the next chunk's first
        (r1, x1, it1, rr1, h1), i1 = run("small", b=b, tol=D.tol_ending_at(hist, k))
        assert r1 == 0 and i1["why"] == "conv" and it1 == k


def test_start_exits():
    B = plan_of("small")[0]
    n = B.shape[0]
    (ret, x, iters, relres, hist), info = run("small", b=np.zeros(n))
    assert ret == 0 and info["why"] == "conv0" and iters == 0 and hist.tolist() == [0.0]
    b = rhs_ones("small")
    (_, xs, _, _, _), _ = run("small", b=b)                          # the converged solution
    (ret, x, iters, relres, hist), info = run("small", b=b, x0=xs, tol=1e-8)
    assert ret == 0 and info["why"] == "conv0" and iters == 0 and np.array_equal(x, xs)


@pytest.mark.parametrize("kind", sorted(D.BREAKDOWNS))
def test_breakdowns(kind):
    why, its = D.BREAKDOWNS[kind]
    (ret, x, iters, relres, hist), info = run(kind)
    assert ret == C.BREAKDOWN and info["why"] == why and iters == its, (info, iters)
    assert not info["bad"] > 0.0 and hist.size == its + 1
