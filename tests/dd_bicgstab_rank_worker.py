"""One rank of a multi-process sharded BiCGStab run (tests/test_gpu_dd_bicgstab_ranks.py).

    python tests/dd_bicgstab_rank_worker.py bi:<case> OUTDIR     (RANK / WORLD_SIZE / MASTER_* set)

One shard per process over GG_DD_IPC, started and bounded as
tests/dd_cg_rank_worker.py's ranks are (2D band wavefronts only: safe with
several processes on one GPU); the handles are all-gathered over
torch.distributed "gloo" (CPU).  Every rank runs, on one object and in this
order (RUNS):
  conv      the converging BiCGStab solve, b = A 1, tol 1e-10
  tail      tol 1e-300 with max_iter = K_CHUNK + 1: the solve ends one iteration
            into a chunk, whose remaining exchanges -- not gated -- follow its end
  brk       NaN in b: rho at the start, on every rank alike
  tr        gg_dd_transient_bicgstab_src, NSTEPS steps (x and the ports preset to NaN
            where this rank writes nothing)
  gmres     GMRES(30) after them: the ranks' sequence counters still agree
Writes OUTDIR/rank<r>.npz.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "gpu-gmres_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402

import dd_bicgstab_ref as Q  # noqa: E402
import dd_transient_ref as T  # noqa: E402

CASES = {"5pt_200x160_P2": ("laplacian_5pt", (200, 160), dict(upwind=0.2), 2, "blocks"),
         "5pt_200x160_P4": ("laplacian_5pt", (200, 160), dict(upwind=0.2), 4, "blocks")}
RUNS = ("conv", "tail", "brk", "tr", "gmres")
NSTEPS = 3
NAN_ROW = 7


def system(case):
    """(A = G + C/h of the upwinded grid, cdiag, parts, partition method)"""
    from ggmres import matrices as M
    G, P, method = Q.system(CASES[case])
    A = M.transient(G, c=Q.C_CAP, h=Q.H_STEP)
    return A, np.full(A.shape[0], Q.C_CAP / Q.H_STEP), P, method


def inputs(A, q, nsep):
    """(b, b with the NaN, src_node, sources, ports): ports in the interiors and on the
    separator's first and last row (the separator closes the permuted order)"""
    from ggmres import matrices as M
    n = A.shape[0]
    b = M.rhs_ones(A)
    bn = b.copy()
    bn[NAN_ROW] = np.nan
    nodes, sources = T.mixed_sources(n)
    ports = np.concatenate([T.default_ports(n), [q[n - nsep], q[n - 1]]]).astype(np.int32)
    return b, bn, nodes, sources, ports


def runs(d, A, cdiag, fill=None):
    """the runs of RUNS on DD object d: name -> result dict"""
    import ggmres
    BI = ggmres.SOLVE_BICGSTAB
    n = A.shape[0]
    b, bn, nodes, sources, ports = inputs(A, d.perm()[1], d.info()["nsep"])
    kw = dict(restart=30, flags=BI)
    return {
        "conv": d.solve_bicgstab(b, max_iter=3000, tol=1e-10, **kw),
        "tail": d.solve_bicgstab(b, max_iter=Q.K_CHUNK + 1, tol=1e-300, **kw),
        "brk": d.solve_bicgstab(bn, max_iter=3000, tol=1e-10, **kw),
        "tr": d.transient_bicgstab_src(NSTEPS, Q.H_STEP, cdiag, nodes, sources, ports, np.zeros(n), tol=1e-7,
                                       x_fill=fill, port_fill=fill, **kw),
        "gmres": d.solve(b, restart=30, max_iter=1500, tol=1e-10),
    }


def main():
    mode, outdir = sys.argv[1], sys.argv[2]
    rank = int(os.environ["RANK"])
    world = int(os.environ["WORLD_SIZE"])
    import torch.distributed as dist
    from ggmres.dd import DD
    if not mode.startswith("bi:"):
        raise SystemExit(f"unknown mode {mode}")
    case = mode.split(":", 1)[1]
    dist.init_process_group("gloo", rank=rank, world_size=world)
    d = DD(world, device=0, rank=rank, comm="ipc")

    def allgather(b):
        lst = [None] * world
        dist.all_gather_object(lst, b)
        return lst

    d.connect_ipc(allgather)
    ranks, myrank = d.comm_ranks()
    assert (ranks, myrank) == (world, rank), (ranks, myrank)
    A, cdiag, P, method = system(case)
    assert P == world
    n = A.shape[0]
    d.set_system(A, method)
    out = {"q": d.perm()[1], "info": np.array(list(d.info().values()))}
    own = ~np.isnan(d.spmv(np.ones(n), np.full(n, np.nan)))        # the rows this process writes back
    out["own"] = own
    for name, g in runs(d, A, cdiag, fill=np.nan).items():
        out[f"ret_{name}"] = g["ret"]
        if name == "tr":
            out.update(x_tr=g["x"], ports_tr=g["ports"], iters_tr=g["iters_total"])
        else:
            out.update({f"x_{name}": np.where(own, g["x"], np.nan), f"hist_{name}": g["hist"],
                        f"iters_{name}": g["iters"], f"relres_{name}": g["relres"]})
    d.close()
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), **{k: np.asarray(v) for k, v in out.items()})
    dist.destroy_process_group()
    print(f"rank {rank}: ok ({mode})", flush=True)


if __name__ == "__main__":
    main()
