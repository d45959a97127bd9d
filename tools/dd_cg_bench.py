#!/usr/bin/env python3
"""The sharded solve's per-rank time per iteration: conjugate gradients
(GG_SOLVE_CG in gg_dd_solve) against GMRES(30) with MGS and with CGS2.  JSON
lines on stdout, nothing else.

One process, GG_DD_LOOPBACK: shard --rank of P = each of --parts alone on this
GPU, every exchange the in-process all-gather kernel over its own buffer -- the
per-rank kernel and exchange-launch time of a one-shard-per-GPU run.  The system
is bench.py's `--workload dd --dd-grid c2`: the --grid x --grid 5-point grid,
GG_PART_GRID | GG_PART_COLOR_SEP, --division.  Loopback values are not the
system's, so every run is a FIXED iteration count (--iters, tol 1e-300); a run
that ends early (a breakdown on the loopback values) is reported as such and
carries no time.

Per P, after one warm-up of every method, the three methods are timed --reps
times in interleaved order (cg mgs cgs2, cg mgs cgs2, ...) by the solve's own
device events (gg_result.solve_ms: from the first launch to the last, staging
excluded) and the median is reported as microseconds per iteration per rank.
The GMRES figures are the yardstick: code paths older than the sharded CG.
Then one profiled run per method (gg_dd_profile_*: event pairs around every
family, which cost time -- kept out of the timed runs): microseconds per
iteration of each family; for CG "orthogonalization" is its four launches and
two all-gathers (two marks per iteration, summed here per iteration).

--count-grid N (0: skip): the real iteration counts on an N x N grid, where one
GPU holds every shard -- GG_DD_LOCAL at P = the largest of --parts, CG and
GMRES(30)/CGS2 to --tol, beside the single solver's CG on the same grid in the
natural order; the arrow order's ILU(0) is another preconditioner, so the
count differs.

--bicgstab [--upwind U]: the same measurement with sharded BiCGStab
(gg_dd_solve_bicgstab) in CG's place, on the grid made nonsymmetric
(M.laplacian_5pt(grid, upwind=U), default 0.2) -- BiCGStab against GMRES(30)
with MGS and with CGS2.  A BiCGStab iteration is two SpMVs, two applies and
three all-gathers of dot partials; "orthogonalization" is its five launches with
those (three marks per iteration).  --count-grid then reports BiCGStab's and
GMRES(30)/CGS2's real iteration counts and solve times at P = the largest of
--parts in one process (GG_DD_LOCAL, --reps solves each, interleaved, the median),
and the single solver's BiCGStab count in the natural order.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpu-gmres_amd"))

import ggmres                          # noqa: E402
from ggmres import host, matrices as M  # noqa: E402
from ggmres.dd import DD, PROF_NAMES    # noqa: E402

DIV = {"exact": ggmres.DIV_EXACT, "rcp": ggmres.DIV_RCP, "fma": ggmres.DIV_FMA}
METHODS = (("cg", ggmres.SOLVE_CG), ("mgs", 0), ("cgs2", ggmres.SOLVE_CGS2))
METHODS_BI = (("bicgstab", ggmres.SOLVE_BICGSTAB), ("mgs", 0), ("cgs2", ggmres.SOLVE_CGS2))


def solve(d, name, b, **kw):
    """DD.solve, or DD.solve_bicgstab for the method that has a door of its own"""
    return (d.solve_bicgstab if name == "bicgstab" else d.solve)(b, **kw)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--grid", type=int, default=1000)
    p.add_argument("--parts", type=int, nargs="+", default=[2, 4, 8])
    p.add_argument("--rank", type=int, default=0)
    p.add_argument("--iters", type=int, default=300)
    p.add_argument("--restart", type=int, default=30)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--division", choices=sorted(DIV), default="fma")
    p.add_argument("--count-grid", type=int, default=0)
    p.add_argument("--tol", type=float, default=1e-8)
    p.add_argument("--bicgstab", action="store_true")
    p.add_argument("--upwind", type=float, default=0.2)
    a = p.parse_args()

    methods = METHODS_BI if a.bicgstab else METHODS
    upwind = a.upwind if a.bicgstab else 0.0
    method = host.PART_GRID | host.PART_COLOR_SEP
    A = M.laplacian_5pt(a.grid, upwind=upwind)
    b = M.rhs_ones(A)
    for P in a.parts:
        d = DD(P, device=0, rank=a.rank, comm="loopback")
        d.set_system(A, method)
        d.set_division(DIV[a.division])

        def run(name, flags):
            return solve(d, name, b, restart=a.restart, max_iter=a.iters, tol=1e-300, flags=flags)

        ms = {name: [] for name, _ in methods}
        short = {}
        for name, f in methods:                         # warm-up
            g = run(name, f)
            if g["inner"] != a.iters:
                short[name] = (g["ret"], g["inner"])
        for _ in range(a.reps):
            for name, f in methods:
                if name not in short:
                    ms[name].append(run(name, f)["solve_ms"])
        info = d.info()
        for name, f in methods:
            if name in short:
                emit(kind="time", grid=a.grid, upwind=upwind, parts=P, rank=a.rank, method=name,
                     ended_early=short[name], us_per_iteration=None)
                continue
            med = statistics.median(ms[name])
            emit(kind="time", grid=a.grid, upwind=upwind, parts=P, rank=a.rank, method=name, iterations=a.iters,
                 reps=a.reps,
                 division=a.division, solve_ms_median=round(med, 4), solve_ms_min=round(min(ms[name]), 4),
                 solve_ms_max=round(max(ms[name]), 4), us_per_iteration=round(med * 1e3 / a.iters, 3),
                 local_len=info["local_len"], halo_doubles=info["halo_doubles"])
        for name, f in methods:                         # the families, in runs of their own
            if name in short:
                continue
            d.profile(True)
            g = run(name, f)
            fam = {}
            for k, fname in enumerate(PROF_NAMES):
                cnt, tot = d.profile_get(k)
                if cnt:
                    fam[fname] = {"marks": cnt, "us_per_iteration": round(tot * 1e3 / g["inner"], 3)}
            d.profile(False)
            emit(kind="families", grid=a.grid, upwind=upwind, parts=P, rank=a.rank, method=name, iterations=g["inner"],
                 families=fam)
        d.close()

    if a.count_grid and a.bicgstab:
        P = max(a.parts)
        Ac = M.laplacian_5pt(a.count_grid, upwind=upwind)
        bc = M.rhs_ones(Ac)
        d = DD(P, device=0)
        d.set_system(Ac, method)
        d.set_division(DIV[a.division])
        pair = (("bicgstab", ggmres.SOLVE_BICGSTAB), ("cgs2", ggmres.SOLVE_CGS2))
        kw = dict(restart=a.restart, max_iter=20000, tol=a.tol)
        last = {name: solve(d, name, bc, flags=f, **kw) for name, f in pair}      # warm-up
        ms = {name: [] for name, _ in pair}
        for _ in range(a.reps):
            for name, f in pair:
                last[name] = solve(d, name, bc, flags=f, **kw)
                ms[name].append(last[name]["solve_ms"])
        for name, _ in pair:
            g = last[name]
            emit(kind="count", grid=a.count_grid, upwind=upwind, parts=P, comm="local", method=name, ret=g["ret"],
                 iterations=g["inner"], relres=g["relres"], reps=a.reps,
                 solve_ms_all_shards_one_gpu=round(statistics.median(ms[name]), 3),
                 solve_ms_min=round(min(ms[name]), 3), solve_ms_max=round(max(ms[name]), 3))
        d.close()
        s = ggmres.Solver(0)
        s.set_matrix(Ac)
        s.set_precond_ilu0()
        s.set_division(DIV[a.division])
        g = s.solve(bc, restart=a.restart, max_iter=20000, tol=a.tol, flags=ggmres.SOLVE_BICGSTAB)
        emit(kind="count", grid=a.count_grid, upwind=upwind, parts=1, comm="single solver, natural order",
             method="bicgstab", ret=g["ret"], iterations=g["inner"], relres=g["relres"],
             solve_ms=round(g["solve_ms"], 3))
        s.close()
    elif a.count_grid:
        P = max(a.parts)
        Ac = M.laplacian_5pt(a.count_grid)
        bc = M.rhs_ones(Ac)
        d = DD(P, device=0)
        d.set_system(Ac, method)
        d.set_division(DIV[a.division])
        for name, f in (("cg", ggmres.SOLVE_CG), ("cgs2", ggmres.SOLVE_CGS2)):
            g = d.solve(bc, restart=a.restart, max_iter=20000, tol=a.tol, flags=f)
            emit(kind="count", grid=a.count_grid, parts=P, comm="local", method=name, ret=g["ret"],
                 iterations=g["inner"], relres=g["relres"], solve_ms_all_shards_one_gpu=round(g["solve_ms"], 3))
        d.close()
        s = ggmres.Solver(0)
        s.set_matrix(Ac)
        s.set_precond_ilu0()
        s.set_division(DIV[a.division])
        g = s.solve(bc, restart=a.restart, max_iter=20000, tol=a.tol, flags=ggmres.SOLVE_CG)
        emit(kind="count", grid=a.count_grid, parts=1, comm="single solver, natural order", method="cg",
             ret=g["ret"], iterations=g["inner"], relres=g["relres"], solve_ms=round(g["solve_ms"], 3))
        s.close()


if __name__ == "__main__":
    main()
