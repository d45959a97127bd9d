"""ctypes binding of oracle/_ref/libgg_ref.so: the reference's own host routines
(src/SpMV_compute.cpp, src/iluk.cpp, src/itsol.cpp, src/formatConvert.cpp built
by oracle/Makefile with float = double) behind oracle/ref_shim.cpp.

TEST INFRASTRUCTURE ONLY: tests/golden/make_ref_pins.py records what these
routines compute, tests/test_ref_pins.py reruns them where the library exists.
Never imported by the product package, smoke() or bench.py.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_DIR = os.path.join(_HERE, "_ref")
_LIB = os.path.join(_DIR, "libgg_ref.so")
_HASHES = os.path.join(_DIR, "sources.sha256")
_lib = None

_i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_VP = ctypes.c_void_p


def available():
    return os.path.exists(_LIB) and os.path.exists(_HASHES)


def source_hashes():
    """{file name: sha256} of the reference files the library was compiled from"""
    out = {}
    with open(_HASHES) as f:
        for line in f:
            if line.strip():
                digest, name = line.split()
                out[name] = digest
    return out


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(_LIB)
        assert L.ref_sizeof_real() == 8, "the reference was not built with float = double"
        L.ref_spmv.argtypes = [ctypes.c_int, _i32p, _i32p, _f64p, _f64p, _f64p]
        L.ref_lusolve.argtypes = [ctypes.c_int, _i32p, _i32p, _f64p, _i32p, _i32p, _f64p, _f64p, _f64p]
        L.ref_iluk.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, _i32p, _i32p, _f64p,
                               ctypes.POINTER(ctypes.c_int)]
        L.ref_iluk.restype = _VP
        L.ref_iluk_counts.argtypes = [_VP, _i32p, _i32p]
        L.ref_iluk_get.argtypes = [_VP, _i32p, _VP, _VP, _i32p, _VP]
        L.ref_iluk_free.argtypes = [_VP]
        L.ref_coo2csr_double.argtypes = [ctypes.c_int, ctypes.c_int, _f64p, _i32p, _i32p]
        L.ref_sort_double.argtypes = [_i32p, _f64p, ctypes.c_int, ctypes.c_int]
        for f in (L.ref_ldcsc2csr, L.ref_ldcsc2csr_double):
            f.argtypes = [ctypes.c_long, ctypes.c_long, ctypes.c_long, _i64p, _i64p, _f64p,
                          _i32p, _i32p, _f64p]
        _lib = L
    return _lib


def _csr(A):
    import oracle as O
    return O.csr(A)


def spmv(A, x):
    """computeSpMV (src/SpMV_compute.cpp:19-37)"""
    A = _csr(A)
    y = np.zeros(A.n)
    lib().ref_spmv(A.n, A.rp, A.ci, A.v, np.ascontiguousarray(x, np.float64), y)
    return y


def lusolve(L, U, y):
    """LUSolve_ignoreZero (src/SpMV_compute.cpp:92-136); L, U: oracle CSR tuples
    (L unit diagonal last, U diagonal first)"""
    x = np.zeros(L.n)
    lib().ref_lusolve(L.n, L.rp, L.ci, L.v, U.rp, U.ci, U.v, np.ascontiguousarray(y, np.float64), x)
    return x


def iluk(A, k, numeric=True):
    """ilukC (src/iluk.cpp:56-191), or lofC alone (:193-334) with numeric=False.
    Returns dict(status, l_rp, l_ci, l_v, d, u_rp, u_ci, u_v): the strict
    triangles row by row in the order the reference left them (no diagonals),
    d = its D (the reciprocals); values None after lofC; only status where it
    is not 0."""
    A = _csr(A)
    n = A.n
    st = ctypes.c_int()
    h = lib().ref_iluk(int(bool(numeric)), int(k), n, A.rp, A.ci, A.v, ctypes.byref(st))
    out = dict(status=st.value)
    if st.value == 0:
        lnz = np.zeros(n, np.int32)
        unz = np.zeros(n, np.int32)
        lib().ref_iluk_counts(h, lnz, unz)
        l_rp = np.concatenate([[0], np.cumsum(lnz)]).astype(np.int32)
        u_rp = np.concatenate([[0], np.cumsum(unz)]).astype(np.int32)
        l_ci = np.zeros(max(int(l_rp[-1]), 1), np.int32)
        u_ci = np.zeros(max(int(u_rp[-1]), 1), np.int32)
        l_v = np.zeros(len(l_ci)) if numeric else None
        u_v = np.zeros(len(u_ci)) if numeric else None
        d = np.zeros(n) if numeric else None
        p = lambda a: a.ctypes.data if a is not None else None
        lib().ref_iluk_get(h, l_ci, p(l_v), p(d), u_ci, p(u_v))
        nl, nu = int(l_rp[-1]), int(u_rp[-1])
        out.update(l_rp=l_rp, l_ci=l_ci[:nl], u_rp=u_rp, u_ci=u_ci[:nu], d=d,
                   l_v=l_v[:nl] if numeric else None, u_v=u_v[:nu] if numeric else None)
    lib().ref_iluk_free(h)
    return out


def coo2csr_double(nrows, a, i_idx, j_idx):
    """coo2csrDouble_in (src/formatConvert.cpp:165-216) -> (row_ptr, col, val)"""
    nz = len(a)
    a = np.array(a, np.float64)
    ii = np.zeros(max(nz, nrows + 1), np.int32)
    ii[:nz] = i_idx
    jj = np.array(j_idx, np.int32)
    if nz == 0:
        jj = np.zeros(1, np.int32)
        a = np.zeros(1)
    lib().ref_coo2csr_double(int(nrows), nz, a, ii, jj)
    return ii[:nrows + 1].copy(), jj[:nz].copy(), a[:nz].copy()


def sort_double(col, a, start, end):
    """sortDouble (src/formatConvert.cpp:87-106) on copies -> (col, a)"""
    col = np.array(col, np.int32)
    a = np.array(a, np.float64)
    lib().ref_sort_double(col, a, int(start), int(end))
    return col, a


def _csc(fn, m, n, p, i, x):
    p = np.ascontiguousarray(p, np.int64)
    i = np.ascontiguousarray(i, np.int64)
    x = np.ascontiguousarray(x, np.float64)
    nnz = len(x)
    rp = np.zeros(max(nnz, m + 1), np.int32)
    ci = np.zeros(max(nnz, 1), np.int32)
    v = np.zeros(max(nnz, 1))
    fn(nnz, int(m), int(n), p, i if nnz else np.zeros(1, np.int64), x if nnz else np.zeros(1), rp, ci, v)
    return rp[:m + 1].copy(), ci[:nnz].copy(), v[:nnz].copy()


def ldcsc2csr(m, n, p, i, x):
    """LDcsc2csr (src/formatConvert.cpp:248-297; its float output is double in
    this build) -> (row_ptr, col, val)"""
    return _csc(lib().ref_ldcsc2csr, m, n, p, i, x)


def ldcsc2csr_double(m, n, p, i, x):
    """LDcsc2csrMySpMatrixDouble (src/formatConvert.cpp:368-398) -> (row_ptr, col, val)"""
    return _csc(lib().ref_ldcsc2csr_double, m, n, p, i, x)
