#!/usr/bin/env python3
"""The C5 many-RHS transient by conjugate gradients, measured against what the
library had before the CG batch: JSON lines on stdout, nothing else.

The system and the scenarios are bench.py's `--workload c5 --c5-scenarios S`:
the --grid x --grid 5-point grid, A = G + C/h (c 1e-3, h 1e-2), scenario k's
1 % PULSE sources from M.pulse_sources(seed 20261015 + k), cdiag = c/h, ports
[0, n/2, n-1], ILU(0), --tol, --division, --steps backward-Euler steps from
x = 0.  In one process, after one warm-up of every run:

  a   gg_transient_batch, S scenarios          GMRES(--restart): the batch before this tool
  b   S x gg_transient(GG_SOLVE_CG), in turn    CG, one scenario at a time
  c   gg_transient_cg_batch, S scenarios       the CG batch
  b1, c1: b and c with one scenario

a, b and b1 run only code older than the CG batch: they are the baseline, c
and c1 are never compared with themselves.  Each run is timed --reps times in
interleaved order (a b c b1 c1, a b c b1 c1, ...) with a host clock around the
call -- every call ends in a stream synchronization -- and the median is
reported: seconds per run, total iterations, microseconds per
scenario-iteration.  --profile RUN executes that one run --profile-reps times
after a warm-up and nothing else (for rocprofv3 --kernel-trace --stats around
this tool, or one run under another GG_CG_BATCH_CHUNK).

--bicgstab [--upwind U] measures the BiCGStab batch the same way on the
upwinded (nonsymmetric) grid M.laplacian_5pt(grid, upwind=U), U = 0.2 unless
given: b, c, b1 and c1 are gg_transient(GG_SOLVE_BICGSTAB) in turn and
gg_transient_bicgstab_batch, a stays the GMRES batch on the same system.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpu-gmres_amd"))

import ggmres                          # noqa: E402
from ggmres import matrices as M       # noqa: E402

DIV = {"exact": ggmres.DIV_EXACT, "rcp": ggmres.DIV_RCP, "fma": ggmres.DIV_FMA}


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--grid", type=int, default=1000)
    p.add_argument("--scenarios", type=int, default=8)
    p.add_argument("--steps", type=int, default=1000, help="backward-Euler steps per run (bench.py --c5-steps)")
    p.add_argument("--restart", type=int, default=30)
    p.add_argument("--tol", type=float, default=1e-8)
    p.add_argument("--max-iter", type=int, default=20000)
    p.add_argument("--division", choices=sorted(DIV), default="fma")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--bicgstab", action="store_true", help="BiCGStab on the upwinded grid instead of CG")
    p.add_argument("--upwind", type=float, default=None,
                   help="upwind weight of the grid (default 0.2 with --bicgstab, else 0: CG needs symmetry)")
    p.add_argument("--profile", choices=["a", "b", "c", "b1", "c1"], default=None)
    p.add_argument("--profile-reps", type=int, default=1, help="timed executions of the --profile run")
    a = p.parse_args()

    h = 1e-2
    upwind = a.upwind if a.upwind is not None else (0.2 if a.bicgstab else 0.0)
    if upwind != 0.0 and not a.bicgstab:
        raise SystemExit("--upwind makes the grid nonsymmetric: conjugate gradients do not apply (use --bicgstab)")
    flag, name, tag = (ggmres.SOLVE_BICGSTAB, "BICGSTAB", "bicgstab") if a.bicgstab else (ggmres.SOLVE_CG, "CG", "cg")
    A = M.transient(M.laplacian_5pt(a.grid, upwind=upwind), c=1e-3, h=h)
    n = A.shape[0]
    S = max(1, a.scenarios)
    scen = [M.pulse_sources(n, frac=0.01, h=h, seed=20261015 + k) for k in range(S)]
    cdiag = np.full(n, 1e-3 / h)
    ports = np.array([0, n // 2, n - 1], np.int32)
    s = ggmres.Solver(0)
    s.set_matrix(A)
    s.set_precond_ilu0()
    s.set_division(DIV[a.division])
    if not s.batch_engine:
        raise SystemExit("this configuration takes no batched launches")
    kw = dict(restart=a.restart, max_iter=a.max_iter, tol=a.tol)

    def gmres_batch(k):
        r = s.transient_batch(a.steps, h, cdiag, scen[:k], ports, np.zeros((k, n)), **kw)
        return r["ret"], sum(r["iters_total"]), r["x"]

    def cg_each(k):
        ret, tot, xs = 0, 0, []
        for nodes, pulses in scen[:k]:
            r = s.transient(a.steps, h, cdiag, nodes, pulses, ports, np.zeros(n), flags=flag, **kw)
            ret = max(ret, r["ret"])
            tot += r["iters_total"]
            xs.append(r["x"])
        return ret, tot, np.stack(xs)

    def cg_batch(k):
        fn = s.transient_bicgstab_batch if a.bicgstab else s.transient_cg_batch
        r = fn(a.steps, h, cdiag, scen[:k], ports, np.zeros((k, n)), **kw)
        return r["ret"], sum(r["iters_total"]), r["x"]

    runs = {"a": (gmres_batch, S, "gg_transient_batch (GMRES)"),
            "b": (cg_each, S, f"gg_transient(GG_SOLVE_{name}) per scenario, in turn"),
            "c": (cg_batch, S, f"gg_transient_{tag}_batch"),
            "b1": (cg_each, 1, f"gg_transient(GG_SOLVE_{name}), one scenario"),
            "c1": (cg_batch, 1, f"gg_transient_{tag}_batch, one scenario")}
    order = [a.profile] if a.profile else list(runs)
    out = {}
    for run in order:                                   # warm-up: every shape the timed window uses
        fn, k, _ = runs[run]
        out[run] = fn(k)
        if out[run][0] != 0:
            raise SystemExit(f"run {run}: status {out[run][0]}")
    if a.profile:
        fn, k, what = runs[a.profile]
        ts = []
        for _ in range(a.profile_reps):
            t0 = time.perf_counter()
            ret, tot, _ = fn(k)
            ts.append(time.perf_counter() - t0)
        print(json.dumps(dict(run=a.profile, what=what, scenarios=k, steps=a.steps, seconds=statistics.median(ts),
                              seconds_all=ts, iterations=int(tot), status=int(ret),
                              chunk=os.environ.get("GG_CG_BATCH_CHUNK"))), flush=True)
        s.close()
        return
    # the batch computes what the single transients of its method compute
    same = bool(np.array_equal(out["b"][2], out["c"][2]) and out["b"][1] == out["c"][1])
    times = {run: [] for run in runs}
    for _ in range(a.reps):
        for run in order:
            fn, k, _ = runs[run]
            t0 = time.perf_counter()
            fn(k)
            times[run].append(time.perf_counter() - t0)
    s.close()
    print(json.dumps(dict(config=dict(grid=a.grid, n=int(n), scenarios=S, steps=a.steps, restart=a.restart,
                                      tol=a.tol, max_iter=a.max_iter, division=a.division, reps=a.reps,
                                      method=tag, upwind=upwind),
                          **{f"{tag}_batch_equals_single_{tag}_bits": same})), flush=True)
    for run in order:
        _, k, what = runs[run]
        tot = int(out[run][1])
        med = statistics.median(times[run])
        print(json.dumps(dict(run=run, what=what, scenarios=k, seconds=med, seconds_all=times[run],
                              iterations=tot, us_per_scenario_iteration=1e6 * med / max(tot, 1))), flush=True)


if __name__ == "__main__":
    main()
