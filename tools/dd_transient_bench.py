#!/usr/bin/env python3
"""The sharded transient loop (gg_dd_transient_src) against the host loop a user
writes around gg_dd_solve.  JSON lines on stdout, nothing else.

System: C5 -- M.transient(M.laplacian_5pt(--grid)) with M.pulse_sources, --steps
backward-Euler steps from x = 0 to --tol, two ports.  Setting: GG_DD_LOCAL at
P = --parts in ONE process on ONE GPU (every shard's launches on one stream): the
numbers say what the loop saves the host and the device per step there; nothing
multi-GPU is measured by this tool.

Three runs per method:
  host      per step, NumPy w = B u + (C/h) x on the host, then DD.solve(w, x0=x)
            (upload of w and x, two gathers per shard, the solve, a scatter, the
            download of x), the ports read on the host.  The sources' values are
            evaluated before the timed window (oracle.pulse, one value per step:
            every C5 source carries the same waveform).
  loop      DD.transient_src with GG_DD_TRANSIENT_HINT=0
  loop+hint DD.transient_src with the hint (GG_SOLVE_CG only: the GMRES steps
            take no hint)
Methods: GG_SOLVE_CG (all three), GG_SOLVE_CGS2 (host, loop).  After one warm-up
of every run, --reps repetitions in interleaved order; each is timed by the host
clock around the whole call(s) -- every one ends in a device synchronise -- and the
median is reported as seconds per run and microseconds per iteration.  Before
any time is printed the runs of a method must agree bit for bit in x, the ports
and the iteration total.

--bicgstab: the same three runs for BiCGStab steps alone, on the grid made
nonsymmetric (M.laplacian_5pt(grid, upwind=--upwind)): the host loop around
DD.solve_bicgstab against DD.transient_bicgstab_src without and with the hint.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "gpu-gmres_amd"))

import numpy as np                      # noqa: E402

import ggmres                           # noqa: E402
import oracle as O                      # noqa: E402
from ggmres import host, matrices as M  # noqa: E402
from ggmres.dd import DD                # noqa: E402


def emit(**kw):
    print(json.dumps(kw), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--grid", type=int, default=1000)
    p.add_argument("--parts", type=int, default=4)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--restart", type=int, default=32)
    p.add_argument("--tol", type=float, default=1e-7)
    p.add_argument("--bicgstab", action="store_true")
    p.add_argument("--upwind", type=float, default=0.2)
    a = p.parse_args()

    c, h = 1e-3, 1e-2
    A = M.transient(M.laplacian_5pt(a.grid, upwind=a.upwind if a.bicgstab else 0.0), c=c, h=h)
    n = A.shape[0]
    cdiag = np.full(n, c / h)
    nodes, pulses = M.pulse_sources(n, h=h)
    assert np.all(pulses == pulses[0]) and len(set(nodes.tolist())) == len(nodes)
    sources = [(ggmres.SRC_PULSE, q) for q in pulses]
    ports = np.array([nodes[0], n // 2], np.int32)
    uval = [O.pulse(pulses[0], it, h) for it in range(a.steps + 1)]      # outside the timed window
    d = DD(a.parts, device=0)
    d.set_system(A, host.PART_BLOCKS)
    kw = dict(restart=a.restart, max_iter=10000, tol=a.tol)

    def host_loop(flags):
        x = np.zeros(n)
        pv = np.zeros((len(ports), a.steps + 1))
        pv[:, 0] = x[ports]
        total, ret = 0, 0
        for it in range(1, a.steps + 1):
            w = 0.0 + cdiag * x                     # xnr = 0; xnr += (C/h) x
            w[nodes] = uval[it] + w[nodes]          # one source per row: bu + xnr
            r = (d.solve_bicgstab if a.bicgstab else d.solve)(w, x0=x, flags=flags, **kw)
            x = r["x"]
            total += r["iters"]
            ret = r["ret"] or ret
            pv[:, it] = x[ports]
        return dict(ret=ret, x=x, ports=pv, iters_total=total)

    def loop(flags, hint):
        if hint:
            os.environ.pop("GG_DD_TRANSIENT_HINT", None)
        else:
            os.environ["GG_DD_TRANSIENT_HINT"] = "0"
        try:
            fn = d.transient_bicgstab_src if a.bicgstab else d.transient_src
            return fn(a.steps, h, cdiag, nodes, sources, ports, np.zeros(n), flags=flags, **kw)
        finally:
            os.environ.pop("GG_DD_TRANSIENT_HINT", None)

    methods = (("cg", ggmres.SOLVE_CG), ("cgs2", ggmres.SOLVE_CGS2))
    if a.bicgstab:
        methods = (("bicgstab", ggmres.SOLVE_BICGSTAB),)
    for mname, flags in methods:
        runs = [("host", lambda f=flags: host_loop(f)), ("loop", lambda f=flags: loop(f, False))]
        if mname != "cgs2":
            runs.append(("loop+hint", lambda f=flags: loop(f, True)))
        first = {name: fn() for name, fn in runs}                       # warm-up, and the bits
        ref = first["host"]
        for name, g in first.items():
            assert g["ret"] == ref["ret"] == 0 and g["iters_total"] == ref["iters_total"], (mname, name)
            assert np.array_equal(g["x"], ref["x"]) and np.array_equal(g["ports"], ref["ports"]), (mname, name)
        secs = {name: [] for name, _ in runs}
        for _ in range(a.reps):
            for name, fn in runs:
                t0 = time.perf_counter()
                g = fn()
                secs[name].append(time.perf_counter() - t0)
                assert g["iters_total"] == ref["iters_total"]
        its = ref["iters_total"]
        for name, _ in runs:
            med = statistics.median(secs[name])
            emit(kind="time", grid=a.grid, parts=a.parts, comm="local, one process, one GPU", method=mname,
                 run=name, steps=a.steps, tol=a.tol, reps=a.reps, iters_total=its,
                 iterations_per_step=round(its / max(a.steps, 1), 2), seconds_median=round(med, 4),
                 seconds_min=round(min(secs[name]), 4), seconds_max=round(max(secs[name]), 4),
                 us_per_iteration=round(med * 1e6 / max(its, 1), 2),
                 ratio_to_host=round(med / statistics.median(secs["host"]), 4), bits="identical to host")
    d.close()


if __name__ == "__main__":
    main()
