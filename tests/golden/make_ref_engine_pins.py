"""Generate tests/golden/ref_engine_pins.npz: what the reference's OWN host GMRES
engines compute on the cases of ref_engine_cases.py.

    python tests/golden/make_ref_engine_pins.py

Needs oracle/_ref/libgg_ref.so built with the engines (oracle/Makefile cuts
GMRES_leftILU0, the GMRES without a preconditioner, GMRESilu and
MyILUPP::HostPrecond_* out of the reference checkout's src/gmres.cu and
src/preconditioner.cu; float widened to double, contraction off).  Recorded:

  <engine>/<case>/ret, iters, relres   the return value, *max_iter and *tol as
                                       the engine left them
  <engine>/<case>/tol                  the tolerance the case ran with
  <engine>/<case>/x                    the solution: whole for the cases the GPU
                                       test reads, else a sha256 above
                                       ref_pin_cases.WHOLE_MAX elements
  splitmap/<system>/<scale>/<map>      MyILUPP::HostPrecond_left / _right /
                                       _starting_value / _rhs on their own
  deviation/max_iter_inside_cycle      1: on ref_engine_cases.DEVIATION the
                                       reference's output differs from the
                                       oracle's and the oracle's is finite
  deviation/cut_to_budget/relres, x    the reference on the same system with the
                                       restart length cut to that max_iter (a
                                       whole cycle, defined): what the oracle
                                       returns on DEVIATION, bit for bit
  relres_order_dev                     the largest relative deviation, over the
                                       gpu cases, of the ORDER-MATCHED oracle's
                                       relres (CPU, the device's summation
                                       order) from the reference's
  cases, sources                       the keys above; the sha256 of every
                                       reference file that was compiled or cut

Outputs only: names and numbers, nothing of the reference's text.  A case whose
reference output is not finite is dropped and named; every engine must keep
MIN_CASES.  For every gpu case the serial oracle, the order-matched oracle and
the reference must agree on ret and iters (else it is no gpu case: choose
another seed or tolerance).  The file is written with fixed member order and
time stamps: a rerun rewrites the same bytes."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _p in (REPO, os.path.join(REPO, "gpu-gmres_amd"), os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import oracle as O                              # noqa: E402
from oracle import ref as R                     # noqa: E402
from golden import ref_pin_cases as C           # noqa: E402
from golden import ref_engine_cases as E        # noqa: E402


def finite(r):
    return bool(np.isfinite(r["relres"]) and np.all(np.isfinite(r["x"])))


def build_store(report=None):
    """-> (keys, store, sources); report: a list that receives the lines main() prints"""
    say = (lambda s: None) if report is None else report.append
    store, keys, kept = {}, [], {e: 0 for e in E.ENGINES}
    order_dev = 0.0

    def put(key, a, whole=False):
        E.put(store, key, a, whole)
        keys.append(key)

    for case in E.CASES:
        r = E.run(R, case)
        if not finite(r):
            assert not case.gpu, f"{E.key(case)}: a gpu case must have a finite reference"
            say(f"dropped {E.key(case)}: the reference's output is not finite")
            continue
        if case.gpu:
            o, t = E.run(O, case), E.run_order_matched(case)
            got = [(q["ret"], q["iters"]) for q in (r, o, t)]
            assert got[0] == got[1] == got[2], f"{E.key(case)}: (ret, iters) reference / serial / order-matched {got}"
            if r["relres"] != 0.0:
                order_dev = max(order_dev, abs(t["relres"] - r["relres"]) / r["relres"])
            else:
                assert t["relres"] == 0.0
        k = E.key(case)
        put(k + "/ret", np.array([r["ret"]], np.int32))
        put(k + "/iters", np.array([r["iters"]], np.int32))
        put(k + "/relres", np.array([r["relres"]]))
        put(k + "/tol", np.array([E.tolerance(case)]))
        put(k + "/x", r["x"], whole=case.gpu)
        kept[case.engine] += 1

    for name, scale in E.split_map_keys():
        v = E.split_map_vector(name, scale)
        for which in E.SPLIT_MAPS:
            out = R.split_apply(E.split(name), which, v)
            assert np.all(np.isfinite(out)), (name, scale, which)
            put(f"splitmap/{name}/{scale}/{which}", out)

    ref, orc = E.deviation_run(R.gmres_left_ilu0), E.deviation_run(O.gmres_left)
    differs = not (ref["relres"] == orc["relres"] and np.array_equal(ref["x"], orc["x"]))
    assert differs and finite(orc), "max_iter inside a cycle: the oracle no longer deviates from the reference"
    assert (ref["ret"], ref["iters"]) == (orc["ret"], orc["iters"]) == (1, E.DEVIATION.max_iter)
    put("deviation/max_iter_inside_cycle", np.array([1], np.int32))
    cut = E.deviation_run(R.gmres_left_ilu0, m=E.DEVIATION.max_iter)     # a whole cycle: defined
    assert finite(cut) and (cut["ret"], cut["iters"]) == (1, E.DEVIATION.max_iter)
    put(E.DEVIATION_KEY + "/relres", np.array([cut["relres"]]))
    put(E.DEVIATION_KEY + "/x", cut["x"])
    put("relres_order_dev", np.array([order_dev]))

    for e in E.ENGINES:
        say(f"{e}: {kept[e]} cases")
        assert kept[e] >= E.MIN_CASES, (e, kept[e])
    say(f"relres_order_dev = {order_dev:.3e}")
    return keys, store, [f"{name} {h}" for name, h in sorted(R.source_hashes(engines=True).items())]


def main():
    if not R.engines_available():
        raise SystemExit("oracle/_ref/libgg_ref.so is missing or has no engines: run make -C oracle with the "
                         "reference checked out")
    report = []
    keys, store, sources = build_store(report)
    C.write_npz(E.PINS, keys, store, sources)
    print("\n".join(report))
    print(f"wrote {len(keys)} arrays, {os.path.getsize(E.PINS)} bytes, to tests/golden/ref_engine_pins.npz")


if __name__ == "__main__":
    main()
