"""One rank of a multi-process sharded transient (tests/test_gpu_dd_transient_ranks.py).

    python tests/dd_transient_rank_worker.py tr:<case> OUTDIR     (RANK / WORLD_SIZE / MASTER_* set)

One shard per process over GG_DD_IPC, as tests/dd_cg_rank_worker.py; the cases are
tests/dd_rank_worker.py's (2D band wavefronts only, safe with several processes
on one GPU) with C/h added to the diagonal.  Every rank runs, on one object and
in this order (RUNS):
  cg        a GG_SOLVE_CG transient, tol 1e-7: hinted chunks, steps ending inside them
  cgs2      a GG_SOLVE_CGS2 transient
  tail      a GG_SOLVE_CG transient with max_iter = K_CHUNK + 1: every step ends one
            iteration into a chunk, whose remaining exchanges -- not gated -- follow it
  gmres     a GMRES(30) gg_dd_solve after them: the ranks' sequence counters still agree
x starts at 0 and port_out is preset to NaN.  Writes OUTDIR/rank<r>.npz: per run
the x array as the entry point left it (cg, tail: rows not held keep the 0 they
came in with; cgs2: x_fill = NaN there), the port matrix (NaN rows: not held),
return codes and iteration counts.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)                                # oracle (the restatements import it)
sys.path.insert(0, os.path.join(REPO, "gpu-gmres_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402

import dd_rank_worker as RW  # noqa: E402
import dd_transient_ref as T  # noqa: E402
from dd_rank_worker import CASES  # noqa: E402,F401

RUNS = ("cg", "cgs2", "tail", "gmres")
NSTEPS = 4


def system(case):
    """(A = G + C/h, cdiag, partition method) of a dd_rank_worker case"""
    from ggmres import matrices as M
    G, method = RW.system(case)
    A = M.transient(G, c=T.C_CAP, h=T.H_STEP)
    return A, np.full(A.shape[0], T.C_CAP / T.H_STEP), method


def inputs(A, q, nsep):
    """(src_node, sources, ports): the mixed sources; ports in the interiors and on
    the separator's first and last row (the separator closes the permuted order)"""
    n = A.shape[0]
    nodes, sources = T.mixed_sources(n)
    ports = np.concatenate([T.default_ports(n), [q[n - nsep], q[n - 1]]]).astype(np.int32)
    return nodes, sources, ports


def runs(d, A, cdiag, fill=None):
    """the four runs of RUNS on DD object d: name -> result dict"""
    from ggmres import matrices as M
    n = A.shape[0]
    nodes, sources, ports = inputs(A, d.perm()[1], d.info()["nsep"])
    kw = dict(restart=30, tol=1e-7, port_fill=fill)
    x0 = np.zeros(n)
    return {
        "cg": d.transient_src(NSTEPS, T.H_STEP, cdiag, nodes, sources, ports, x0, flags=T.SOLVE_CG, **kw),
        "cgs2": d.transient_src(NSTEPS, T.H_STEP, cdiag, nodes, sources, ports, x0, flags=T.SOLVE_CGS2,
                                x_fill=fill, **kw),
        "tail": d.transient_src(NSTEPS, T.H_STEP, cdiag, nodes, sources, ports, x0, flags=T.SOLVE_CG,
                                max_iter=T.K_CHUNK + 1, **kw),
        "gmres": d.solve(M.rhs_ones(A), restart=30, max_iter=1500, tol=1e-10),
    }


def main():
    mode, outdir = sys.argv[1], sys.argv[2]
    rank = int(os.environ["RANK"])
    world = int(os.environ["WORLD_SIZE"])
    import torch.distributed as dist
    from ggmres.dd import DD
    if not mode.startswith("tr:"):
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
    A, cdiag, method = system(case)
    d.set_system(A, method)
    out = {"q": d.perm()[1], "info": np.array(list(d.info().values()))}
    for name, g in runs(d, A, cdiag, fill=np.nan).items():
        out.update({f"x_{name}": g["x"], f"ret_{name}": g["ret"]})
        if name == "gmres":
            out.update(hist_gmres=g["hist"], iters_gmres=g["iters"])
        else:
            out.update({f"ports_{name}": g["ports"], f"iters_{name}": g["iters_total"]})
    d.close()
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), **{k: np.asarray(v) for k, v in out.items()})
    dist.destroy_process_group()
    print(f"rank {rank}: ok ({mode})", flush=True)


if __name__ == "__main__":
    main()
