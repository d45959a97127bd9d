"""CPU: the sharded transient restatement (tests/dd_transient_ref.py) on the
natural block layout (dd_cg_ref.natural_segments) takes, on the systems of
tests/test_gpu_dd_transient.py, the exits those tests rely on -- conditions, not
counts: the device's layout may move a count by one.

Measured here from x = 0 with c = 1e-3, h = 1e-2 (CG and GMRES(30) alike):
  small, tol 1e-7    20, 19, 18, 18, 18, 18, 17, 17, 17, 17
  small, tol 1e-10   28, 27, 26, 26, 26, 26, 25, 25, 25, 25
  mixed, tol 1e-7    25, 24, 23, 22, 22, 22
"""
import functools

import numpy as np
import pytest

import dd_cg_ref as D
import dd_transient_ref as T
import oracle as O
from ggmres import host

K = T.K_CHUNK


@functools.lru_cache(maxsize=None)
def plan_of(name):
    A, cdiag, P, method, nsteps = T.system(name)
    plan = host.DDPlan(A, P, method)
    B = host.permute(A, plan.pinv, plan.q)
    L, U = O.ilu0(B)
    segs, G = D.natural_segments(plan)
    return B, L, U, plan.q.copy(), segs, G, cdiag, nsteps


def run(name, flags, **kw):
    B, L, U, q, segs, G, cdiag, nsteps = plan_of(name)
    n = B.shape[0]
    nodes, sources = T.mixed_sources(n)
    return T.transient(B, L, U, q, segs, G, nsteps, T.H_STEP, cdiag, nodes, sources, T.default_ports(n),
                       np.zeros(n), flags=flags, restart=30, **kw)


@pytest.mark.parametrize("flags", [0, T.SOLVE_CG])
@pytest.mark.parametrize("name,tol", [("small", 1e-7), ("small", 1e-10), ("mixed", 1e-7)])
def test_every_step_converges_across_a_chunk(name, tol, flags):
    o = run(name, flags, tol=tol)
    counts = [i for _, i in o["steps"]]
    print(f"{name} tol {tol:g} flags {flags}: {counts}")
    assert o["ret"] == 0 and all(r == 0 for r, _ in o["steps"])
    assert len(counts) == plan_of(name)[7] and min(counts) > K          # every CG step crosses a chunk
    assert len(set(counts)) > 1                                         # the hint changes from step to step
    assert o["iters_total"] == sum(counts)
    if tol == 1e-10:
        assert max(counts) > 3 * K                                      # three chunks in play
    assert np.all(np.isfinite(o["x"])) and np.all(o["ports"][:, 0] == 0.0) and np.any(o["ports"][:, -1] != 0.0)


@pytest.mark.parametrize("flags", [0, T.SOLVE_CGS2, T.SOLVE_CG])
def test_exhausted_steps(flags):
    o = run("small", flags, tol=1e-7, max_iter=5)
    assert o["ret"] == 1 and o["steps"] == [(1, 5)] * plan_of("small")[7]
    assert o["iters_total"] == 5 * plan_of("small")[7]


def test_the_bisected_3d_system_converges():
    o = run("7pt_16_bisect", T.SOLVE_CG, tol=1e-7)
    assert o["ret"] == 0 and all(r == 0 and i > 0 for r, i in o["steps"])


def test_cg_breakdown_keeps_the_state():
    """the negated matrix: every step breaks down before its first iteration, x stays"""
    _, cdiag, P, method, _ = T.system("small")
    S = D.breakdown_matrix("negated")
    plan = host.DDPlan(S, P, method)
    B = host.permute(S, plan.pinv, plan.q)
    L, U = O.ilu0(B)
    segs, G = D.natural_segments(plan)
    n = S.shape[0]
    nodes, sources = T.mixed_sources(n)
    x0 = np.linspace(0.5, 1.5, n)
    o = T.transient(B, L, U, plan.q, segs, G, 3, T.H_STEP, cdiag, nodes, sources, T.default_ports(n), x0,
                    flags=T.SOLVE_CG, restart=30)
    assert o["ret"] == -8 and o["steps"] == [(-8, 0)] * 3 and o["iters_total"] == 0
    assert np.array_equal(o["x"], x0) and np.array_equal(o["ports"], np.tile(x0[T.default_ports(n)][:, None], 4))
