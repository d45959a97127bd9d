"""The sharded transient loop across PROCESSES on one GPU (GG_DD_IPC), as
tests/test_gpu_dd_cg_ranks.py does for the CG solve: P fresh processes
(tests/dd_transient_rank_worker.py), one shard each.  Every rank must agree, must
have written exactly the rows of x and of the port matrix it holds, and the
merged results must be bit-identical to the same decomposition in one process
(GG_DD_LOCAL) and to the restatement (tests/dd_transient_ref.py).

What this adds to the one-process tests is the control flow: a hinted first chunk
changes how many ungated exchanges each step enqueues, on every rank alike only
because the hint is read from the replicated control block -- the GMRES solve
each rank runs last would time out or diverge had the ranks' sequence counters
(or the fused SpMV's epochs) come apart.
"""
import os
import sys

import numpy as np
import pytest

import dd_transient_ref as T
import oracle as O
import test_gpu_dd_cg_ranks as CR
from conftest import REPO
from ggmres import host
from ggmres.dd import DD
from test_gpu_dd_ranks import merge

pytestmark = pytest.mark.gpu
WORKER = os.path.join(REPO, "tests", "dd_transient_rank_worker.py")
sys.path.insert(0, os.path.join(REPO, "tests"))
import dd_transient_rank_worker as W  # noqa: E402

_LOCAL = {}


def local(case):
    """once per case: the plan, the GG_DD_LOCAL runs and the restatements of the transients"""
    if case not in _LOCAL:
        A, cdiag, method = W.system(case)
        P = int(case.split("_P")[1][0])
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
        nodes, sources, ports = W.inputs(A, q, nsep)
        kw = dict(restart=30, tol=1e-7)
        args = (B, L, U, q, list(segs), G[0], W.NSTEPS, T.H_STEP, cdiag, nodes, sources, ports, np.zeros(n))
        ref = {
            "cg": T.transient(*args, flags=T.SOLVE_CG, **kw),
            "cgs2": T.transient(*args, flags=T.SOLVE_CGS2, **kw),
            "tail": T.transient(*args, flags=T.SOLVE_CG, max_iter=T.K_CHUNK + 1, **kw),
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
    for r in rs:                                    # every rank: the same plan, the same control flow
        assert np.array_equal(r["q"], q)
        assert r["info"][1] == P and r["info"][8] == 1
        for name in W.RUNS:
            assert int(r[f"ret_{name}"]) == int(rs[0][f"ret_{name}"]), name
            assert int(r[f"iters_{name}"]) == int(rs[0][f"iters_{name}"]), name
        assert np.array_equal(r["hist_gmres"], rs[0]["hist_gmres"])
    # each rank wrote exactly what it holds: x came in as 0 and comes back nonzero on
    # the rows held (cgs2: x_fill = NaN stands elsewhere), port_out came in as NaN
    for k, r in enumerate(rs):
        for name in ("cg", "tail", "gmres"):
            x = r[f"x_{name}"]
            assert np.all(x[~held[k]] == 0.0) and np.all(x[held[k]] != 0.0), (name, k)
            r[f"x_{name}"] = np.where(held[k], x, np.nan)
        assert np.array_equal(np.isnan(r["x_cgs2"]), ~held[k]), k
        for name in ("cg", "cgs2", "tail"):
            wrote = ~np.isnan(r[f"ports_{name}"])
            assert np.array_equal(wrote, np.tile(held[k][ports][:, None], W.NSTEPS + 1)), (name, k)
    assert all(held[k][ports[-1]] and held[k][ports[-2]] for k in range(P))     # separator ports: every rank
    for name in W.RUNS:
        g = got[name]
        x = merge(rs, f"x_{name}")                  # the separator's values agree on every rank
        assert int(rs[0][f"ret_{name}"]) == g["ret"], name
        assert np.array_equal(x, g["x"]), name
        if name == "gmres":
            assert g["ret"] == 0 and int(rs[0]["iters_gmres"]) == g["iters"]
            assert np.array_equal(rs[0]["hist_gmres"], g["hist"])
            continue
        pv = merge(rs, f"ports_{name}")
        o = ref[name]
        assert int(rs[0][f"iters_{name}"]) == g["iters_total"] == o["iters_total"], name
        assert g["ret"] == o["ret"], name
        assert np.array_equal(pv, g["ports"]) and np.array_equal(pv, o["ports"]), name
        assert np.array_equal(x, o["x"]), name
    assert ref["cg"]["ret"] == ref["cgs2"]["ret"] == 0
    assert min(i for _, i in ref["cg"]["steps"]) > T.K_CHUNK            # every hinted step crosses a chunk
    assert ref["tail"]["steps"] == [(1, T.K_CHUNK + 1)] * W.NSTEPS


@pytest.mark.parametrize("case", ["5pt_200x160_P2", "5pt_200x160_P4"])
def test_dd_transient_ipc_ranks_match_local_and_restatement(case, tmp_path, monkeypatch):
    P = int(case.split("_P")[1][0])
    monkeypatch.setattr(CR, "WORKER", WORKER)       # run_ranks' process handling, this file's worker
    check(CR.run_ranks(f"tr:{case}", P, tmp_path, timeout=240, env_extra={"GG_DD_XK": "0"}), case)
