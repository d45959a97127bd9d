"""The oracle and the product's host code against what the reference's OWN host
routines compute (tests/golden/ref_pins.npz, recorded by golden/make_ref_pins.py
from computeSpMV, lofC + ilukC, LUSolve_ignoreZero and the COO/CSC -> CSR
conversions built from the reference checkout in double, contraction off).

Every bar is bit equality (a sha256 for the large arrays).  Only the live rerun
needs oracle/_ref; everything else reads the committed fixture.  The negative
control recomputes each family in NumPy with the order of operations reversed
and requires the result to differ from the fixture in at least 3 of 4 cases, so
the pins cannot pass on inputs where the order does not matter."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle as O
from conftest import PKG, REPO
from golden import ref_pin_cases as C
from oracle import format as OF
from oracle import ref as R

PI = ctypes.POINTER(ctypes.c_int)
PD = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def fix():
    return C.fixture()[1]


pinned_factors = C.pinned_factors


# ------------------------------------------------------------ live reference
@pytest.mark.skipif(not R.available(), reason="oracle/_ref/libgg_ref.so not built (no reference checkout)")
def test_live_reference_reproduces_fixture():
    from golden import make_ref_pins as G
    keys, store, sources = C.fixture()
    lkeys, lstore, lsources = G.build_store()
    assert lsources == sources                      # the same reference text went in
    assert lkeys == keys and set(lstore) == set(store)
    for key in store:
        assert lstore[key].dtype == store[key].dtype and lstore[key].tobytes() == store[key].tobytes(), key


def test_fixture_size_and_contents():
    keys, store, sources = C.fixture()
    assert os.path.getsize(C.PINS) < 256 * 1024
    assert sorted(s.split()[0] for s in sources) == sorted(
        ["SpMV_compute.cpp", "iluk.cpp", "itsol.cpp", "formatConvert.cpp", "SpMV.h", "defs.h", "gpuData.h", "config.h"])
    assert all(len(s.split()[1]) == 64 for s in sources)
    want = [f"spmv/{n}/{x}" for n in C.SPMV for x in C.SPMV_X]
    want += [f"lusolve/{n}/k{k}/{r}" for n, k in C.iluk_keys() for r in C.RHS]
    want += [f"lusolve/skip_pivot/{r}" for r in C.RHS]
    assert set(want) <= set(keys)
    assert all(a.size <= C.WHOLE_MAX for k, a in store.items() if "#" not in k)


# ------------------------------------------------------------ oracle
@pytest.mark.parametrize("name", sorted(C.SPMV))
def test_oracle_spmv(fix, name):
    A = C.SPMV[name]()
    for kind in C.SPMV_X:
        assert C.same(fix, f"spmv/{name}/{kind}", O.spmv(A, C.spmv_x(name, kind, A.shape[0]))) == ""


@pytest.mark.parametrize("name,k", C.iluk_keys())
def test_oracle_iluk(fix, name, k):
    """pattern, values at each (row, col), and D = 1.0 / the oracle's pivot"""
    A = C.ILUK[name][0]()
    L, U = O.iluk(A, k)
    assert C.iluk_mismatch(fix, name, k, L, U) == ""
    # the rows as lofC left them are a reordering of the sorted ones
    key = f"iluk/{name}/k{k}/"
    if key + "u_ci" in fix:
        rp, raw, srt = fix[key + "u_rp"], fix[key + "u_ci"], fix[key + "us_ci"]
        for i in range(A.shape[0]):
            assert np.array_equal(np.sort(raw[rp[i]:rp[i + 1]]), srt[rp[i]:rp[i + 1]])
        o = np.concatenate([rp[i] + np.argsort(raw[rp[i]:rp[i + 1]], kind="stable") for i in range(A.shape[0])]
                           + [np.zeros(0, np.int64)]).astype(np.int64)
        assert np.array_equal(fix[key + "u_v"][o], fix[key + "us_v"])


@pytest.mark.parametrize("k", [0, 1, 2])
def test_oracle_iluk_zero_pivot(fix, k):
    assert fix[f"iluk/zero_pivot/k{k}/status"][0] == -2
    with pytest.raises(ZeroDivisionError):
        O.iluk(C.ZERO_PIVOT(), k)


@pytest.mark.parametrize("name,k", C.iluk_keys())
def test_oracle_lusolve(fix, name, k):
    """division mode 0 (the reference's x / d)"""
    _, L, U = pinned_factors(name, k)
    for kind in C.RHS:
        assert C.same(fix, f"lusolve/{name}/k{k}/{kind}", O.lusolve(L, U, C.rhs(kind, L.n))) == ""


def test_oracle_lusolve_skipped_pivots(fix):
    _, L, U = pinned_factors(*C.SKIP_PIVOT)
    U2, rows = C.skip_pivot(U)
    assert len(rows) == 40 and np.all(np.abs(U2.v[U2.rp[rows]]) < 1e-9)
    for kind in C.RHS:
        x = O.lusolve(L, U2, C.rhs(kind, L.n))
        assert C.same(fix, f"lusolve/skip_pivot/{kind}", x) == ""
        assert C.same(fix, f"lusolve/{C.SKIP_PIVOT[0]}/k{C.SKIP_PIVOT[1]}/{kind}", x) != ""


@pytest.mark.parametrize("n", C.FORMAT_N)
def test_oracle_format(fix, n):
    r, c, v = C.coo_input(n)
    assert n == 1 or (len(set(zip(r, c))) < len(r) and len(set(r)) < n and np.any(np.diff(r) < 0))
    for f, a in zip(("rp", "ci", "v"), OF.coo2csr_in(n, v, r, c)):
        assert C.same(fix, f"format/coo2csrDouble_in/n{n}/{f}", a) == ""
    col, a, lo, hi = C.sort_input(n)
    col, a = list(col), list(a)
    OF.sort(col, a, lo, hi)
    assert C.same(fix, f"format/sortDouble/n{n}/ci", np.array(col)) == ""
    assert C.same(fix, f"format/sortDouble/n{n}/v", np.array(a)) == ""
    p, i, x = C.csc_input(n)
    for routine in ("LDcsc2csr", "LDcsc2csrMySpMatrixDouble"):
        for f, a in zip(("rp", "ci", "v"), OF.csc2csr(n, p, i, x)):
            assert C.same(fix, f"format/{routine}/n{n}/{f}", a) == ""


# ------------------------------------------------------------ product host code
def host_iluk(lib, A, level):
    A = O.csr(A)
    n = A.n
    lrp = np.zeros(n + 1, np.int32)
    urp = np.zeros(n + 1, np.int32)
    lci, lv, uci, uv = PI(), PD(), PI(), PD()
    rc = lib.gg_host_iluk(ctypes.c_int(level), ctypes.c_int(n), A.rp.ctypes.data_as(PI), A.ci.ctypes.data_as(PI),
                          A.v.ctypes.data_as(PD), lrp.ctypes.data_as(PI), ctypes.byref(lci), ctypes.byref(lv),
                          urp.ctypes.data_as(PI), ctypes.byref(uci), ctypes.byref(uv))
    if rc != 0:
        return rc, None, None

    def take(rp, ci, v):
        nnz = int(rp[n])
        out = O.CSR(n, rp, np.ctypeslib.as_array(ci, (max(nnz, 1),))[:nnz].copy(),
                    np.ctypeslib.as_array(v, (max(nnz, 1),))[:nnz].copy())
        lib.gg_host_free(ctypes.cast(ci, ctypes.c_void_p))
        lib.gg_host_free(ctypes.cast(v, ctypes.c_void_p))
        return out
    return 0, take(lrp, lci, lv), take(urp, uci, uv)


@pytest.mark.parametrize("name,k", C.iluk_keys())
def test_host_iluk(ggmres_lib, fix, name, k):
    """iluk_symbolic + the numeric phase of csrc/host/factor.cpp (gg_host_iluk)"""
    rc, L, U = host_iluk(ggmres_lib, C.ILUK[name][0](), k)
    assert rc == 0
    assert C.iluk_mismatch(fix, name, k, L, U) == ""


@pytest.mark.parametrize("k", [0, 1, 2])
def test_host_iluk_zero_pivot(ggmres_lib, k):
    assert host_iluk(ggmres_lib, C.ZERO_PIVOT(), k)[0] == -3      # GG_EZEROPIVOT


DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "format_convert.h"
template <class T> static void rd(FILE *f, T *p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) exit(2); }
template <class T> static void wr(FILE *f, const T *p, size_t n) { if (n && fwrite(p, sizeof(T), n, f) != n) exit(3); }
int main(int argc, char **argv) {
    int n = atoi(argv[1]);
    long nz = atol(argv[2]);
    FILE *f = fopen(argv[3], "rb"), *o = fopen(argv[4], "wb");
    if (!f || !o) return 1;
    size_t cap = nz > n + 1 ? nz : n + 1;
    std::vector<int> r(cap), c(nz + 1);
    std::vector<double> v(nz + 1), x(nz + 1);
    std::vector<long> p(n + 1), i(nz + 1);
    rd(f, r.data(), nz); rd(f, c.data(), nz); rd(f, v.data(), nz);
    rd(f, p.data(), n + 1); rd(f, i.data(), nz); rd(f, x.data(), nz);
    coo2csrDouble_in(n, (int)nz, v.data(), r.data(), c.data());
    wr(o, r.data(), n + 1); wr(o, c.data(), nz); wr(o, v.data(), nz);
    ucr_cs_dl M;
    M.shallowCpy(nz, n, n, p.data(), i.data(), x.data(), -1);
    MySpMatrixDouble D;
    LDcsc2csrMySpMatrixDouble(&D, &M);
    wr(o, D.rowIndices, n + 1); wr(o, D.indices, nz); wr(o, D.val, nz);
    MySpMatrix F;
    LDcsc2csrMySpMatrix(&F, &M);
    wr(o, F.rowIndices, n + 1); wr(o, F.indices, nz); wr(o, F.val, nz);
    fclose(o);
    return 0;
}
"""


@pytest.fixture(scope="module")
def convert_driver(tmp_path_factory, ggmres_lib):
    d = tmp_path_factory.mktemp("ref_pins")
    (d / "conv.cpp").write_text(DRIVER)
    lib = os.path.join(PKG, "lib")
    subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(REPO, "include", "compat"),
                           "-I", os.path.join(REPO, "include"), str(d / "conv.cpp"), "-o", str(d / "conv"),
                           "-L", lib, "-Wl,-rpath," + lib, "-lggmres"])
    return d


@pytest.mark.parametrize("n", C.FORMAT_N)
def test_product_format_symbols(convert_driver, fix, n):
    """coo2csrDouble_in, LDcsc2csrMySpMatrixDouble and LDcsc2csrMySpMatrix as
    csrc/compat/format_convert.cpp exports them (the reference's C++ names)"""
    r, c, v = C.coo_input(n)
    p, i, x = C.csc_input(n)
    nz = len(v)
    inp, out = convert_driver / f"in{n}.bin", convert_driver / f"out{n}.bin"
    with open(inp, "wb") as f:
        for a in (r.astype("<i4"), c.astype("<i4"), v, p.astype("<i8"), i.astype("<i8"), x):
            f.write(np.ascontiguousarray(a).tobytes())
    subprocess.check_call([str(convert_driver / "conv"), str(n), str(nz), str(inp), str(out)])
    with open(out, "rb") as f:
        take = lambda dt, cnt: np.frombuffer(f.read(np.dtype(dt).itemsize * cnt), dt)
        for routine in ("coo2csrDouble_in", "LDcsc2csrMySpMatrixDouble"):
            for fld, a in (("rp", take("<i4", n + 1)), ("ci", take("<i4", nz)), ("v", take("<f8", nz))):
                assert C.same(fix, f"format/{routine}/n{n}/{fld}", a) == ""
        # the float variant: the same moves, values narrowed once to fp32
        rp, ci, vf = take("<i4", n + 1), take("<i4", nz), take("<f4", nz)
        assert C.same(fix, f"format/LDcsc2csr/n{n}/rp", rp) == "" and C.same(fix, f"format/LDcsc2csr/n{n}/ci", ci) == ""
        _, _, vd = OF.csc2csr(n, p, i, x)
        assert C.same(fix, f"format/LDcsc2csr/n{n}/v", vd) == "" and np.array_equal(vf, vd.astype(np.float32))


# ------------------------------------------------------------ negative control
def spmv_reversed(A, x):
    """rows summed right to left"""
    y = np.zeros(A.shape[0])
    rp, ci, v = A.indptr, A.indices, A.data
    for i in range(A.shape[0]):
        t = 0.0
        for j in range(rp[i + 1] - 1, rp[i] - 1, -1):
            t += v[j] * x[ci[j]]
        y[i] = t
    return y


def lusolve_nearest_first(L, U, Y):
    """LUSolve_ignoreZero on the columns of Y with every U row accumulated from
    its nearest column outwards (the reference starts at the farthest)"""
    W = np.array(Y, copy=True)
    for i in range(L.n):
        for j in range(L.rp[i], L.rp[i + 1] - 1):
            W[i] -= L.v[j] * W[L.ci[j]]
    X = W
    for i in range(U.n - 1, -1, -1):
        for j in range(U.rp[i] + 1, U.rp[i + 1]):
            X[i] -= U.v[j] * X[U.ci[j]]
        d = U.v[U.rp[i]]
        if not abs(d) < 1e-9:
            X[i] /= d
    return X


def iluk_descending(A, l_rp, l_ci, u_rp, u_ci):
    """ilukC's numeric phase on the given pattern with the L multipliers of a
    row applied in descending column order -> (l_v, d, u_v)"""
    A = O.csr(A)
    n = A.n
    l_v, u_v, d = np.zeros(len(l_ci)), np.zeros(len(u_ci)), np.zeros(n)
    l_rp, l_ci, u_rp, u_ci = (t.tolist() for t in (l_rp, l_ci, u_rp, u_ci))
    lv, uv, dd = l_v.tolist(), u_v.tolist(), d.tolist()
    arp, aci, av = A.rp.tolist(), A.ci.tolist(), A.v.tolist()
    for i in range(n):
        pos = {l_ci[p]: p for p in range(l_rp[i], l_rp[i + 1])}
        pos.update({u_ci[p]: p for p in range(u_rp[i], u_rp[i + 1])})
        di = 0.0
        for p in range(arp[i], arp[i + 1]):
            col = aci[p]
            if col < i:
                lv[pos[col]] = av[p]
            elif col == i:
                di = av[p]
            else:
                uv[pos[col]] = av[p]
        for p in sorted(range(l_rp[i], l_rp[i + 1]), key=lambda q: -l_ci[q]):
            jrow = l_ci[p]
            lv[p] *= dd[jrow]
            m = lv[p]
            for q in range(u_rp[jrow], u_rp[jrow + 1]):
                col = u_ci[q]
                if col == i:
                    di -= m * uv[q]
                elif col in pos:
                    if col < i:
                        lv[pos[col]] -= m * uv[q]
                    else:
                        uv[pos[col]] -= m * uv[q]
        dd[i] = 1.0 / di
    return np.array(lv), np.array(dd), np.array(uv)


def test_negative_control_spmv(fix):
    """A case is a matrix (it runs with both x); it differs where either run
    does.  20 of the 22 matrices with two or more terms in a row differ (the
    two that do not are cusp's 8- and 10-entry pattern matrices, all ones).
    Run by run it is 29 of 44: x = 0.5 on the integer-valued stencils and
    pattern matrices is exact in any order, which is why those runs alone
    would pin nothing and every such matrix also runs with a random x."""
    counted = differ = runs = 0
    for name in C.SPMV:
        A = C.SPMV[name]()
        if A.nnz == 0 or np.diff(A.indptr).max() < 2:
            continue
        hits = [C.same(fix, f"spmv/{name}/{kind}", spmv_reversed(A, C.spmv_x(name, kind, A.shape[0]))) != ""
                for kind in C.SPMV_X]
        counted += 1
        differ += any(hits)
        runs += sum(hits)
    print(f"spmv: {differ} of {counted} matrices, {runs} of {2 * counted} runs differ")
    assert counted >= 20 and 4 * differ >= 3 * counted, (differ, counted)


def test_negative_control_lusolve(fix):
    counted = differ = 0
    for name, k in C.iluk_keys():
        _, L, U = pinned_factors(name, k)
        if np.diff(U.rp).max() < 3:             # diagonal + fewer than two terms
            continue
        X = lusolve_nearest_first(L, U, np.stack([C.rhs(kind, L.n) for kind in C.RHS], axis=1))
        for c, kind in enumerate(C.RHS):
            counted += 1
            differ += C.same(fix, f"lusolve/{name}/k{k}/{kind}", X[:, c]) != ""
    assert counted >= 100 and 4 * differ >= 3 * counted, (differ, counted)


def test_negative_control_iluk(fix):
    counted = differ = 0
    for name, k in C.iluk_keys():
        A, L, U = pinned_factors(name, k)
        l_rp, l_ci, _, _ = C.strict(L, False)
        u_rp, u_ci, _, _ = C.strict(U, True)
        if np.diff(l_rp).max() < 2:
            continue
        l_v, d, u_v = iluk_descending(A, l_rp, l_ci, u_rp, u_ci)
        key = f"iluk/{name}/k{k}/"
        counted += 1
        differ += any(C.same(fix, key + f, a) != "" for f, a in (("l_v", l_v), ("d", d), ("us_v", u_v)))
    assert counted >= 25 and 4 * differ >= 3 * counted, (differ, counted)
