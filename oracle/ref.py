"""ctypes binding of oracle/_ref/libgg_ref.so: the reference's own host routines
(src/SpMV_compute.cpp, src/iluk.cpp, src/itsol.cpp, src/formatConvert.cpp, and
the host GMRES engines cut out of src/gmres.cu and src/preconditioner.cu by
oracle/slice_ref.py, built by oracle/Makefile with float = double) behind
oracle/ref_shim.cpp.

TEST INFRASTRUCTURE ONLY: tests/golden/make_ref_pins.py and
make_ref_engine_pins.py record what these routines compute,
tests/test_ref_pins.py and test_ref_engine_pins.py rerun them where the
library exists.
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
# the files the engines are cut from; every other name in sources.sha256 is
# compiled whole (the routines of tests/golden/ref_pins.npz)
ENGINE_FILES = ("gmres.cu", "preconditioner.cu")

_i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_VP = ctypes.c_void_p


def available():
    return os.path.exists(_LIB) and os.path.exists(_HASHES)


def source_hashes(engines=False):
    """{file name: sha256} of the reference files the library was compiled
    from: the files compiled whole, with engines=True also ENGINE_FILES"""
    out = {}
    with open(_HASHES) as f:
        for line in f:
            if line.strip():
                digest, name = line.split()
                if engines or name not in ENGINE_FILES:
                    out[name] = digest
    return out


def engines_available():
    """the library holds the host GMRES engines (built with the slice)"""
    return available() and hasattr(lib(), "ref_split_apply")


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
        if hasattr(L, "ref_split_apply"):
            tail = [_f64p, _f64p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)]
            mat = [ctypes.c_int, _i32p, _i32p, _f64p]
            tri = [_i32p, _i32p, _f64p]
            L.ref_gmres_left_ilu0.argtypes = mat + tri + tri + tail
            L.ref_gmres_plain.argtypes = mat + tail
            L.ref_gmres_split.argtypes = mat + tri + tri + [_f64p, _i32p, _i32p, _f64p, _f64p] + tail
            L.ref_split_apply.argtypes = ([ctypes.c_int, ctypes.c_int] + tri + tri +
                                          [_f64p, _i32p, _i32p, _f64p, _f64p, _f64p, _f64p])
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


def _engine(fn, args, b, x0, n, m, max_iter, tol):
    x = np.zeros(n) if x0 is None else np.array(x0, np.float64, copy=True)
    mi, tl = ctypes.c_int(int(max_iter)), ctypes.c_double(float(tol))
    ret = fn(*args, np.ascontiguousarray(b, np.float64), x, int(m), ctypes.byref(mi), ctypes.byref(tl))
    return dict(ret=int(ret), x=x, iters=mi.value, relres=tl.value)


def gmres_left_ilu0(A, L, U, b, x0=None, m=30, max_iter=3000, tol=1e-10):
    """GMRES_leftILU0 (src/gmres.cu:566-717) -> dict(ret, x, iters = *max_iter,
    relres = *tol as the engine left them)"""
    A = _csr(A)
    return _engine(lib().ref_gmres_left_ilu0, (A.n, A.rp, A.ci, A.v, L.rp, L.ci, L.v, U.rp, U.ci, U.v),
                   b, x0, A.n, m, max_iter, tol)


def gmres_plain(A, b, x0=None, m=30, max_iter=3000, tol=1e-10):
    """the host GMRES without a preconditioner (src/gmres.cu:721-850)"""
    A = _csr(A)
    return _engine(lib().ref_gmres_plain, (A.n, A.rp, A.ci, A.v), b, x0, A.n, m, max_iter, tol)


def gmres_split(A, P, b, x0=None, m=32, max_iter=10000, tol=1e-7):
    """GMRESilu (src/gmres.cu:2069-2252) over MyILUPP::HostPrecond_rhs /
    _starting_value / _left / _right (src/preconditioner.cu:1055-1137);
    P: an oracle.Split (its arrays are only read)"""
    A = _csr(A)
    return _engine(lib().ref_gmres_split,
                   (A.n, A.rp, A.ci, A.v, P.L.rp, P.L.ci, P.L.v, P.U.rp, P.U.ci, P.U.v, P.middle,
                    P.perm_row, P.perm_col, P.lscale, P.rscale), b, x0, A.n, m, max_iter, tol)


SPLIT_MAPS = ("left", "right", "start", "rhs")


def split_apply(P, which, v):
    """MyILUPP::HostPrecond_left / _right / _starting_value / _rhs
    (src/preconditioner.cu:1055-1137) on v; which: a name in SPLIT_MAPS"""
    out = np.zeros(P.L.n)
    lib().ref_split_apply(SPLIT_MAPS.index(which), P.L.n, P.L.rp, P.L.ci, P.L.v, P.U.rp, P.U.ci, P.U.v, P.middle,
                          P.perm_row, P.perm_col, P.lscale, P.rscale, np.ascontiguousarray(v, np.float64), out)
    return out
