"""Generate tests/golden/ref_pins.npz: what the reference's OWN host routines
compute on the cases of ref_pin_cases.py.

    python tests/golden/make_ref_pins.py

Needs oracle/_ref/libgg_ref.so (oracle/Makefile builds it from the reference
checkout: src/SpMV_compute.cpp, src/iluk.cpp, src/itsol.cpp and
src/formatConvert.cpp, float widened to double, contraction off).  Recorded:

  spmv/<case>/<x>                   computeSpMV
  iluk/<case>/k<k>/...              lofC + ilukC: the strict L rows (l_rp, l_ci,
                                    l_v) and U rows (u_rp, u_ci, u_v) in the
                                    order lofC left them, d = D (the reciprocals);
                                    us_ci, us_v = the same U rows by ascending
                                    column (a permutation, for the sorted layout
                                    the solver takes)
  iluk/zero_pivot/k<k>/status       ilukC's return value (-2) only
  lusolve/<case>/k<k>/<rhs>         LUSolve_ignoreZero on those factors
  lusolve/skip_pivot/<rhs>          ... with 40 negligible U diagonals
  format/<routine>/n<n>/...         coo2csrDouble_in, sortDouble, LDcsc2csr,
                                    LDcsc2csrMySpMatrixDouble
  cases, sources                    the keys above; the sha256 of every
                                    reference file that was compiled

Outputs only: names and numbers, nothing of the reference's text.  Arrays above
ref_pin_cases.WHOLE_MAX elements are stored as a sha256 (see there).  The file
is written with fixed member order and time stamps: a rerun rewrites the same
bytes.  tests/test_ref_pins.py holds the oracle and the product's host code to
it, tests/test_gpu_ref_pins.py the HIP kernels."""
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

ILUK_FIELDS = ("l_rp", "l_ci", "l_v", "d", "u_rp", "u_ci", "u_v")


def reference_factors(A, k, r):
    """ilukC's output r as the (L, U) LUSolve_ignoreZero takes.  ilukC keeps only
    the reciprocal pivots D; the un-inverted ones are taken from the oracle's
    factorization after checking that 1.0 / pivot is D bit for bit."""
    _, Uo = O.iluk(A, k)
    diag = Uo.v[Uo.rp[:-1]]
    if not np.array_equal(Uo.ci[Uo.rp[:-1]], np.arange(Uo.n)) or not np.array_equal(1.0 / diag, r["d"]):
        raise SystemExit(f"ILU({k}): the oracle's pivots are not the reference's; fix oracle.c first")
    return C.to_factors(Uo.n, r, diag)


def build_store():
    store, cases = {}, []

    def put(key, a):
        C.put(store, key, a)
        cases.append(key)

    for name in C.SPMV:
        A = C.SPMV[name]()
        for kind in C.SPMV_X:
            put(f"spmv/{name}/{kind}", R.spmv(A, C.spmv_x(name, kind, A.shape[0])))

    for k in (0, 1, 2):
        put(f"iluk/zero_pivot/k{k}/status", np.array([R.iluk(C.ZERO_PIVOT(), k)["status"]], np.int32))

    for name, k in C.iluk_keys():
        A = C.ILUK[name][0]()
        r = R.iluk(A, k)
        assert r["status"] == 0, (name, k, r["status"])
        pat = R.iluk(A, k, numeric=False)               # lofC alone: the pattern ilukC fills
        assert pat["status"] == 0 and all(np.array_equal(pat[f], r[f]) for f in ("l_rp", "l_ci", "u_rp", "u_ci"))
        for f in ILUK_FIELDS:
            put(f"iluk/{name}/k{k}/{f}", r[f])
        L, U = reference_factors(A, k, r)
        _, us_ci, us_v, _ = C.strict(U, True)            # the same U rows by ascending column
        put(f"iluk/{name}/k{k}/us_ci", us_ci)
        put(f"iluk/{name}/k{k}/us_v", us_v)
        for kind in C.RHS:
            put(f"lusolve/{name}/k{k}/{kind}", R.lusolve(L, U, C.rhs(kind, L.n)))
        if (name, k) == C.SKIP_PIVOT:
            U2, _ = C.skip_pivot(U)
            for kind in C.RHS:
                put(f"lusolve/skip_pivot/{kind}", R.lusolve(L, U2, C.rhs(kind, L.n)))

    for n in C.FORMAT_N:
        r_, c_, v_ = C.coo_input(n)
        for f, a in zip(("rp", "ci", "v"), R.coo2csr_double(n, v_, r_, c_)):
            put(f"format/coo2csrDouble_in/n{n}/{f}", a)
        for f, a in zip(("ci", "v"), R.sort_double(*C.sort_input(n))):
            put(f"format/sortDouble/n{n}/{f}", a)
        p, i, x = C.csc_input(n)
        for routine, fn in (("LDcsc2csr", R.ldcsc2csr), ("LDcsc2csrMySpMatrixDouble", R.ldcsc2csr_double)):
            for f, a in zip(("rp", "ci", "v"), fn(n, n, p, i, x)):
                put(f"format/{routine}/n{n}/{f}", a)

    return cases, store, [f"{name} {h}" for name, h in sorted(R.source_hashes().items())]


def main():
    if not R.available():
        raise SystemExit("oracle/_ref/libgg_ref.so is missing: run make -C oracle with the reference checked out")
    cases, store, sources = build_store()
    C.write_npz(C.PINS, cases, store, sources)
    print(f"wrote {len(cases)} arrays, {os.path.getsize(C.PINS)} bytes, to tests/golden/ref_pins.npz")


if __name__ == "__main__":
    main()
