"""The sharded CG solve across PROCESSES on one GPU (GG_DD_IPC), as
tests/test_gpu_dd_ranks.py does for GMRES: P fresh processes
(tests/dd_cg_rank_worker.py), one shard each.  Every rank must agree, and the
merged results must be bit-identical to the same decomposition in one process
(GG_DD_LOCAL) and to the restatement (tests/dd_cg_ref.py) in the sharded order.

Besides the values this checks the control flow a sharded CG solve adds: the
host enqueues chunks of iterations ahead of the state it has read and the
exchanges of an enqueued iteration are not gated, so a solve that ends inside
a chunk is followed by exchanges on every rank alike -- the GMRES solve that
each rank runs last would time out or diverge had the ranks' sequence counters
(or the fused SpMV's epochs) come apart.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import dd_cg_ref as D
import oracle as O
from conftest import REPO
from ggmres import host
from ggmres.dd import DD
from test_gpu_dd_ranks import _port, merge

pytestmark = pytest.mark.gpu
WORKER = os.path.join(REPO, "tests", "dd_cg_rank_worker.py")
sys.path.insert(0, os.path.join(REPO, "tests"))
import dd_cg_rank_worker as W  # noqa: E402


def run_ranks(mode, P, outdir, timeout=240, env_extra=None):
    """start P rank processes, wait for all; kill exactly those on failure; no retry"""
    port = _port()
    procs = []
    for r in range(P):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(P), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="2")
        env.update(env_extra or {})
        procs.append(subprocess.Popen([sys.executable, "-u", WORKER, mode, str(outdir)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=timeout)
            outs.append(o)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} exited {p.returncode}:\n{o[-3000:]}"
    return [dict(np.load(os.path.join(outdir, f"rank{r}.npz"))) for r in range(P)]


_LOCAL = {}


def local(case):
    """the same decomposition in one process and the restatement, once per case:
    (q, {run: GG_DD_LOCAL result}, {run: restatement (ret, x, iters, relres, hist)})"""
    if case not in _LOCAL:
        A, method = W.system(case)
        P = int(case.split("_P")[1][0])
        loc = DD(P, device=0)
        loc.set_system(A, method)
        pinv, q = loc.perm()
        segs, G = zip(*[loc.dot_layout(p) for p in range(P)])
        got = W.solves(loc, A)
        loc.close()
        B = host.permute(A, pinv, q)
        L, U = O.ilu0(B)
        from ggmres import matrices as M
        b = M.rhs_ones(A)[q]
        x0 = np.random.default_rng(9).standard_normal(A.shape[0])[q]
        ref = {
            "conv": D.solve(B, L, U, b, list(segs), G[0]),
            "warm": D.solve(B, L, U, b, list(segs), G[0], x0=x0, max_iter=40),
            "tail": D.solve(B, L, U, b, list(segs), G[0], max_iter=D.K_CHUNK + 1, tol=1e-300),
        }
        _LOCAL[case] = (q, got, ref)
    return _LOCAL[case]


def check(rs, case):
    P = len(rs)
    q, got, ref = local(case)
    for r in rs:                                    # every rank: the same plan, the same control flow
        assert np.array_equal(r["q"], q)
        assert r["info"][1] == P and r["info"][8] == 1
        for name in W.RUNS:
            assert np.array_equal(r[f"hist_{name}"], rs[0][f"hist_{name}"]), name
            for f in ("iters", "inner", "ret"):
                assert int(r[f"{f}_{name}"]) == int(rs[0][f"{f}_{name}"]), (f, name)
            assert float(r[f"relres_{name}"]) == float(rs[0][f"relres_{name}"]), name
    r0 = rs[0]
    for name in W.RUNS:
        g = got[name]
        x = merge(rs, f"x_{name}")                  # the separator replica agrees on every rank
        assert (int(r0[f"ret_{name}"]), int(r0[f"iters_{name}"]), int(r0[f"inner_{name}"])) == \
               (g["ret"], g["iters"], g["inner"]), name
        assert np.array_equal(r0[f"hist_{name}"], g["hist"]), name
        assert np.array_equal(x, g["x"]), name
        if name in ref:
            ret, xr, iters, relres, hist = ref[name]
            assert (g["ret"], g["iters"], g["relres"]) == (ret, iters, relres), name
            assert np.array_equal(g["hist"], hist) and np.array_equal(x[q], xr), name
    assert got["conv"]["ret"] == 0 and got["gmres"]["ret"] == 0
    assert got["warm"]["ret"] == 1 and got["warm"]["iters"] == 40
    assert got["tail"]["ret"] == 1 and got["tail"]["iters"] == D.K_CHUNK + 1


@pytest.mark.parametrize("xk", [0, 1])
@pytest.mark.parametrize("case", sorted(W.CASES))
def test_dd_cg_ipc_ranks_match_local_and_restatement(case, xk, tmp_path):
    """GG_DD_XK 0 and 1: CG takes no in-kernel orthogonalization exchange, but
    the exchange area and the sequence counter are the ones GMRES's use"""
    P = int(case.split("_P")[1][0])
    check(run_ranks(f"cg:{case}", P, tmp_path, env_extra={"GG_DD_XK": str(xk)}), case)


@pytest.mark.parametrize("form", ["second_stream", "separate_launches"])
def test_dd_cg_ipc_ranks_halo_forms(form, tmp_path):
    """the SpMV's interface exchange on the second stream (GG_DD_HALO_INLINE=0)
    and as a launch of its own (GG_DD_HALO_FUSED=0): the same bits"""
    case = "5pt_200x160_P4"
    env = {"GG_DD_HALO_INLINE": "0"} if form == "second_stream" else {"GG_DD_HALO_FUSED": "0"}
    env["GG_DD_XK"] = "0"
    check(run_ranks(f"cg:{case}", 4, tmp_path, env_extra=env), case)
