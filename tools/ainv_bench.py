#!/usr/bin/env python3
"""Time to solution of the built-in left preconditioners on the bench's system.

The grid side, restart, tolerance, iteration limit and division mode are
bench.py's own argument defaults, imported (bench.parse()); the system and the
right-hand side are formed by the two calls bench.py's main() makes inline
(laplacian_5pt(grid), rhs_ones(A)), which cannot be imported and are repeated
here.  One JSON line per preconditioner -- ILU(0) under the bench's
division mode, AINV at the reference's drop tolerance 0.1, DIAG, NONE -- with
  setup_s       wall seconds of the gg_set_precond_* call
  status, iters the solve's return code and iteration count
  solve_ms      device time of one solve (median of --solves)
  apply_us      one preconditioner application (gg_time_precond)
  hbm_frac      gg_bytes_precond / apply time / the HBM peak bench.py uses
  AINV only: nnz_z, nnz_wt, fused (a one-launch kernel served the apply)

--cg: GMRES(restart) and preconditioned CG (GG_SOLVE_CG; the system is SPD)
side by side instead -- per preconditioner one warm-up solve of each, then
--solves (default 5 here) timed solves of each, alternating in this process;
one JSON line with, for "gmres" and "cg": status, iters, relres, solve_ms (the
median of the device-event times), us_per_iter, solves; and cg_speedup =
gmres solve_ms / cg solve_ms.  A method that does not converge within the
iteration limit is timed once.

--bicgstab [--upwind U]: GMRES(restart) and BiCGStab (GG_SOLVE_BICGSTAB) side by
side in the same way, on laplacian_5pt(grid, upwind=U) (nonsymmetric for U != 0);
with U = 0 the system is SPD and CG is the third method of the alternation.  The
line holds "gmres", "bicgstab" (and "cg"), bicgstab_speedup = gmres solve_ms /
bicgstab solve_ms and, with CG, bicgstab_over_cg_us_per_iter.

  python tools/ainv_bench.py [--grid 1000] [--solves 3] [--cg | --bicgstab [--upwind U]] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def bench_defaults():
    """bench.py's argument defaults (grid, restart, tol, max_iter, division)"""
    import bench
    argv, sys.argv = sys.argv, [sys.argv[0]]
    try:
        return bench, bench.parse()
    finally:
        sys.argv = argv


def side_by_side(s, flags, b, kind, n, grid, d, setup, solves, upwind=None):
    """the methods of `flags` (name -> gg_options.flags) alternating on solver s
    after one warm-up of each"""
    ms = {k: [] for k in flags}
    last = {}
    for k, f in flags.items():                 # warm-up: code objects, work space, the fallbacks
        last[k] = s.solve(b, restart=d.restart, max_iter=d.max_iter, tol=d.tol, flags=f)
    for _ in range(solves):
        for k, f in flags.items():
            if last[k]["ret"] != 0 and ms[k]:
                continue                       # not converged: one timed run of the iteration limit is enough
            last[k] = s.solve(b, restart=d.restart, max_iter=d.max_iter, tol=d.tol, flags=f)
            ms[k].append(last[k]["solve_ms"])
    rec = {"precond": kind, "n": n, "grid": grid, "restart": d.restart, "tol": d.tol, "max_iter": d.max_iter,
           "setup_s": round(setup, 4)}
    if upwind is not None:
        rec["upwind"] = upwind
    if kind == "ilu0":
        rec["division"] = d.division
    for k in flags:
        g, med = last[k], statistics.median(ms[k])
        rec[k] = {"status": g["ret"], "iters": g["iters"], "relres": g["relres"], "solve_ms": round(med, 4),
                  "us_per_iter": round(med * 1e3 / max(g["inner"], 1), 3), "solves": len(ms[k])}
    for k in ("cg", "bicgstab"):
        if k in flags:
            rec[k + "_speedup"] = round(rec["gmres"]["solve_ms"] / rec[k]["solve_ms"], 3)
    if "cg" in flags and "bicgstab" in flags:
        rec["bicgstab_over_cg_us_per_iter"] = round(rec["bicgstab"]["us_per_iter"] / rec["cg"]["us_per_iter"], 3)
    return rec


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--grid", type=int, default=None, help="grid side (default: bench.py's)")
    p.add_argument("--solves", type=int, default=None,
                   help="timed solves (default 3; 5 of each method with --cg or --bicgstab)")
    p.add_argument("--cg", action="store_true", help="GMRES(restart) and CG (GG_SOLVE_CG) side by side")
    p.add_argument("--bicgstab", action="store_true",
                   help="GMRES(restart) and BiCGStab (GG_SOLVE_BICGSTAB) side by side, and CG when --upwind is 0")
    p.add_argument("--upwind", type=float, default=0.0,
                   help="with --bicgstab: west entries times 1 + U, east entries times 1 - U (nonsymmetric)")
    p.add_argument("--reps", type=int, default=50, help="applications per gg_time_precond call")
    p.add_argument("--drop-tol", type=float, default=0.1)
    p.add_argument("--only", default="ilu0,ainv,diag,none")
    p.add_argument("--out", default=None, help="also append the lines to this file")
    a = p.parse_args()
    if a.cg and a.bicgstab:
        p.error("--cg and --bicgstab exclude each other (--bicgstab --upwind 0 runs CG as well)")
    if a.upwind != 0.0 and not a.bicgstab:
        p.error("--upwind needs --bicgstab (GMRES alone and CG are measured on the bench's own system)")
    if a.solves is None:
        a.solves = 5 if (a.cg or a.bicgstab) else 3
    bench, d = bench_defaults()
    import ggmres
    from ggmres import matrices as M

    grid = a.grid or d.grid
    # bench.py main(): the C2 system (--upwind 0 passes nothing on: the same matrix)
    A = M.laplacian_5pt(grid, upwind=a.upwind) if a.upwind != 0.0 else M.laplacian_5pt(grid)
    b = M.rhs_ones(A)
    n = A.shape[0]
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    s = ggmres.Solver(0)
    s.set_matrix(A)
    setters = {
        "ilu0": lambda: (s.set_precond_ilu0(), s.set_division(bench.DIV_MODES[d.division])),
        "ainv": lambda: s.set_precond_ainv(a.drop_tol),
        "diag": s.set_precond_diag,
        "none": s.set_precond_none,
    }
    for kind in [k for k in a.only.split(",") if k]:
        t0 = time.perf_counter()
        setters[kind]()
        setup = time.perf_counter() - t0
        if a.cg:
            flags = {"gmres": 0, "cg": ggmres.SOLVE_CG}
            emit(side_by_side(s, flags, b, kind, n, grid, d, setup, max(1, a.solves)))
            continue
        if a.bicgstab:
            flags = {"gmres": 0, "bicgstab": ggmres.SOLVE_BICGSTAB}
            if a.upwind == 0.0:
                flags["cg"] = ggmres.SOLVE_CG
            emit(side_by_side(s, flags, b, kind, n, grid, d, setup, max(1, a.solves), upwind=a.upwind))
            continue
        ms, g = [], None
        for _ in range(max(1, a.solves)):
            g = s.solve(b, restart=d.restart, max_iter=d.max_iter, tol=d.tol)
            ms.append(g["solve_ms"])
            if g["ret"] != 0:
                break                      # not converged: one run of the iteration limit is enough
        rec = {"precond": kind, "n": n, "grid": grid, "restart": d.restart, "tol": d.tol, "max_iter": d.max_iter,
               "setup_s": round(setup, 4), "status": g["ret"], "iters": g["iters"], "relres": g["relres"],
               "solve_ms": round(statistics.median(ms), 4), "solves": len(ms)}
        if kind != "none":
            us = s.time_precond(a.reps) * 1e3
            rec["apply_us"] = round(us, 3)
            rec["hbm_frac"] = round(s.bytes_precond() / (us * 1e-6) / (bench.HBM_PEAK_GBS * 1e9), 4)
        if kind == "ilu0":
            rec["division"] = d.division
        if kind == "ainv":
            rec["drop_tol"] = a.drop_tol
            rec["nnz_z"], rec["nnz_wt"] = s.ainv_nnz()
            rec["fused"] = s.ainv_fused
        emit(rec)
    s.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
