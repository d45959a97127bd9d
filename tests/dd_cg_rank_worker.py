"""One rank of a multi-process sharded CG solve (tests/test_gpu_dd_cg_ranks.py).

    python tests/dd_cg_rank_worker.py cg:<case> OUTDIR     (RANK / WORLD_SIZE / MASTER_* set)

One shard per process over GG_DD_IPC, as tests/dd_rank_worker.py (whose CASES
these are: 2D band wavefronts only, safe with several processes on one GPU);
the handles are all-gathered over torch.distributed "gloo" (CPU).  Every rank
runs, on one object and in this order (RUNS):
  conv      the converging CG solve, b = A 1, tol 1e-10
  warm      a warm-started one cut short: x0 random, max_iter 40
  tail      tol 1e-300 with max_iter = K_CHUNK + 1: the solve ends one iteration
            into a chunk, whose remaining exchanges -- not gated -- follow its end
  gmres     GMRES(30) after them: the ranks' sequence counters still agree
Writes OUTDIR/rank<r>.npz: natural-order solutions with NaN in the rows this
rank does not own, histories, iteration counts, return codes.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)                                # oracle (dd_cg_ref's restatement imports it)
sys.path.insert(0, os.path.join(REPO, "gpu-gmres_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402

import dd_cg_ref as D  # noqa: E402
from dd_rank_worker import CASES, system  # noqa: E402,F401

RUNS = ("conv", "warm", "tail", "gmres")


def solves(d, A):
    """the four solves of RUNS on DD object d: name -> result dict"""
    import ggmres
    from ggmres import matrices as M
    n = A.shape[0]
    b = M.rhs_ones(A)
    x0 = np.random.default_rng(9).standard_normal(n)
    CG = ggmres.SOLVE_CG
    return {
        "conv": d.solve(b, restart=30, max_iter=3000, tol=1e-10, flags=CG),
        "warm": d.solve(b, x0=x0, restart=30, max_iter=40, tol=1e-10, flags=CG),
        "tail": d.solve(b, restart=30, max_iter=D.K_CHUNK + 1, tol=1e-300, flags=CG),
        "gmres": d.solve(b, restart=30, max_iter=1500, tol=1e-10),
    }


def main():
    mode, outdir = sys.argv[1], sys.argv[2]
    rank = int(os.environ["RANK"])
    world = int(os.environ["WORLD_SIZE"])
    import torch.distributed as dist
    from ggmres.dd import DD
    if not mode.startswith("cg:"):
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
    A, method = system(case)
    n = A.shape[0]
    d.set_system(A, method)
    out = {"q": d.perm()[1], "info": np.array(list(d.info().values()))}
    own = ~np.isnan(d.spmv(np.ones(n), np.full(n, np.nan)))        # the rows this process writes back
    for name, g in solves(d, A).items():
        out.update({f"x_{name}": np.where(own, g["x"], np.nan), f"hist_{name}": g["hist"],
                    f"iters_{name}": g["iters"], f"inner_{name}": g["inner"], f"ret_{name}": g["ret"],
                    f"relres_{name}": g["relres"]})
    d.close()
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), **{k: np.asarray(v) for k, v in out.items()})
    dist.destroy_process_group()
    print(f"rank {rank}: ok ({mode})", flush=True)


if __name__ == "__main__":
    main()
