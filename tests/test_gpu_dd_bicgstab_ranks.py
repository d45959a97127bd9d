"""The sharded BiCGStab solve and transient across PROCESSES on one GPU (GG_DD_IPC),
as tests/test_gpu_dd_cg_ranks.py does for CG: P fresh processes
(tests/dd_bicgstab_rank_worker.py), one shard each, at P = 2 and P = 4 -- never
more than four GPU processes.  Every rank must agree, each writes exactly the
rows and ports it holds, and the merged results are bit-identical to the same
decomposition in one process (GG_DD_LOCAL) and to the restatement
(tests/dd_bicgstab_ref.py) in the sharded order.

The control flow checked besides the values: chunks enqueued ahead of the state
read and three ungated all-gathers per enqueued iteration, so a solve that ends
inside a chunk -- or breaks down at its start -- is followed by exchanges on
every rank alike; the GMRES solve each rank runs last would time out or diverge
had the ranks' sequence counters (or the fused SpMV's epochs) come apart.
"""
import os
import sys

import numpy as np
import pytest

import dd_bicgstab_ref as Q
import oracle as O
import test_gpu_dd_cg_ranks as CR
from conftest import REPO
from ggmres import host
from ggmres.dd import DD
from test_gpu_dd_ranks import merge

pytestmark = pytest.mark.gpu
WORKER = os.path.join(REPO, "tests", "dd_bicgstab_rank_worker.py")
sys.path.insert(0, os.path.join(REPO, "tests"))
import dd_bicgstab_rank_worker as W  # noqa: E402

_LOCAL = {}


def local(case):
    """once per case: the plan, the rows each rank holds, the GG_DD_LOCAL runs and the restatements"""
    if case not in _LOCAL:
        A, cdiag, P, method = W.system(case)
        n = A.shape[0]
        loc = DD(P, device=0)
        loc.set_system(A, method)
        pinv, q = loc.perm()
        nsep = loc.info()["nsep"]
        segs, G = zip(*[loc.dot_layout(p) for p in range(P)])
        got = W.runs(loc, A, cdiag)
        loc.close()
        plan = host.DDPlan(A, P, method)
        assert np.array_equal(plan.q, q) and plan.nsep == nsep
        B = host.permute(A, pinv, q)
        L, U = O.ilu0(B)
        b, bn, nodes, sources, ports = W.inputs(A, q, nsep)
        sys_ = (B, L, U)
        lay = (list(segs), G[0])
        ref = {
            "conv": Q.solve(*sys_, b[q], *lay),
            "tail": Q.solve(*sys_, b[q], *lay, max_iter=Q.K_CHUNK + 1, tol=1e-300),
            "brk": Q.solve(*sys_, bn[q], *lay),
            "tr": Q.transient(*sys_, q, *lay, W.NSTEPS, Q.H_STEP, cdiag, nodes, sources, ports, np.zeros(n),
                              tol=1e-7),
        }
        held = []                                   # rank r: interior r and the separator
        for r in range(P):
            m = np.zeros(n, bool)
            m[q[plan.begin[r]:plan.begin[r + 1]]] = True
            m[q[plan.begin[P]:]] = True
            held.append(m)
        _LOCAL[case] = (q, ports, held, got, ref)
    return _LOCAL[case]


def check(rs, case):
    P = len(rs)
    q, ports, held, got, ref = local(case)
    solves = ("conv", "tail", "brk", "gmres")
    for k, r in enumerate(rs):                      # every rank: the same plan, the same control flow
        assert np.array_equal(r["q"], q)
        assert r["info"][1] == P and r["info"][8] == 1
        assert np.array_equal(r["own"], held[k]), k
        for name in W.RUNS:
            assert int(r[f"ret_{name}"]) == int(rs[0][f"ret_{name}"]), name
            assert int(r[f"iters_{name}"]) == int(rs[0][f"iters_{name}"]), name
        for name in solves:
            assert np.array_equal(r[f"hist_{name}"], rs[0][f"hist_{name}"], equal_nan=True), name
        # each rank wrote exactly the rows and the ports it holds (both preset to NaN)
        assert np.array_equal(np.isnan(r["x_tr"]), ~held[k]), k
        assert np.array_equal(~np.isnan(r["ports_tr"]), np.tile(held[k][ports][:, None], W.NSTEPS + 1)), k
    assert all(held[k][ports[-1]] and held[k][ports[-2]] for k in range(P))     # separator ports: every rank
    r0 = rs[0]
    for name in solves:
        g = got[name]
        x = merge(rs, f"x_{name}")                  # the separator replica agrees on every rank
        assert (int(r0[f"ret_{name}"]), int(r0[f"iters_{name}"])) == (g["ret"], g["iters"]), name
        assert np.array_equal(r0[f"hist_{name}"], g["hist"], equal_nan=True), name
        assert np.array_equal(x, g["x"]), name
        if name in ref:
            ret, xr, iters, relres, hist = ref[name]
            assert (g["ret"], g["iters"]) == (ret, iters), name
            assert g["relres"] == relres or (np.isnan(relres) and np.isnan(g["relres"])), name
            assert np.array_equal(g["hist"], hist, equal_nan=True) and np.array_equal(x[q], xr), name
    g, o = got["tr"], ref["tr"]
    x, pv = merge(rs, "x_tr"), merge(rs, "ports_tr")
    assert int(r0["ret_tr"]) == g["ret"] == o["ret"] == 0
    assert int(r0["iters_tr"]) == g["iters_total"] == o["iters_total"]
    assert np.array_equal(x, g["x"]) and np.array_equal(x, o["x"])
    assert np.array_equal(pv, g["ports"]) and np.array_equal(pv, o["ports"])
    assert min(i for _, i in o["steps"]) > Q.K_CHUNK                    # every hinted step crosses a chunk
    assert got["conv"]["ret"] == 0 and got["gmres"]["ret"] == 0
    assert got["tail"]["ret"] == 1 and got["tail"]["iters"] == Q.K_CHUNK + 1
    assert got["brk"]["ret"] == Q.BREAKDOWN and got["brk"]["iters"] == 0


@pytest.mark.parametrize("case", sorted(W.CASES))
def test_dd_bicgstab_ipc_ranks_match_local_and_restatement(case, tmp_path, monkeypatch):
    P = W.CASES[case][3]
    monkeypatch.setattr(CR, "WORKER", WORKER)       # run_ranks' process handling, this file's worker
    check(CR.run_ranks(f"bi:{case}", P, tmp_path, timeout=240, env_extra={"GG_DD_XK": "0"}), case)
