"""The cases of tests/golden/ref_pins.npz: what the reference's own host routines
(oracle/_ref/libgg_ref.so, see oracle/Makefile) were run on.  Shared by the
generator (make_ref_pins.py) and the tests (test_ref_pins.py, test_gpu_ref_pins.py):
the fixture holds outputs only, the inputs are rebuilt here from the committed
fixture matrices and seeded generators.

Values are non-dyadic (standard_normal / uniform, or quotients of the
factorization) so that the order of operations changes bits; the exceptions are
the integer stencils with x = 0.5, which the reference's driver uses.
"""
import glob
import hashlib
import io
import os
import zipfile

import numpy as np
import scipy.sparse as sp

import oracle as O
from ggmres import matrices as M

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "fixtures")
PINS = os.path.join(HERE, "ref_pins.npz")
# arrays up to this many elements are stored whole; larger ones as the sha256
# of their little-endian bytes plus their first and last 8 values.  512 is the
# largest power of two that keeps the fixture under 256 KB (4,096 would make
# it 1.5 MB, 1,024 still 0.5 MB: most of it incompressible fp64 mantissas).  A
# digest pins the same bits as the array itself; only the report of WHERE a
# mismatch sits is lost for the large arrays.
WHOLE_MAX = 512


def _mtx(name):
    return lambda: M.read_mtx(os.path.join(FIX, name))


def _rua(name):
    return lambda: M.read_rua(os.path.join(FIX, name))


def _random_rows(n, per_row, seed):
    """n x n, about per_row standard_normal entries per row and a diagonal"""
    rng = np.random.default_rng(seed)
    k = min(per_row, n)
    rows = np.repeat(np.arange(n), k)
    cols = rng.integers(0, n, n * k)
    A = sp.coo_matrix((rng.standard_normal(n * k), (rows, cols)), shape=(n, n)).tocsr()
    A = A + sp.diags(rng.uniform(1.0, 2.0, n))
    return M._finish(A)


def _empty_rows():
    B = M.power_law(2000, 16000, seed=8).tolil()
    for r in range(0, 2000, 13):
        B.rows[r] = []
        B.data[r] = []
    return M._finish(B.tocsr())


def _long_rows():
    """one row of 1,500 entries, one of 257, the rest about 4"""
    n = 1600
    rng = np.random.default_rng(31)
    B = _random_rows(n, 3, 30).tolil()
    for r, ln in ((5, 1500), (900, 257)):
        c = np.sort(rng.choice(n, ln, replace=False))
        B.rows[r] = [int(t) for t in c]
        B.data[r] = [float(t) for t in rng.standard_normal(ln)]
    return M._finish(B.tocsr())


RANDOMS = sorted(os.path.basename(f) for f in glob.glob(os.path.join(FIX, "random_10x10", "*.mtx")))

SPMV = {
    "3pt_100": _mtx("3pt_100.mtx"),
    "5pt_10x10": _mtx("5pt_10x10.mtx"),
    "7pt_10x10x10": _mtx("7pt_10x10x10.mtx"),
    "9pt_10x10": _mtx("9pt_10x10.mtx"),
    "sherman1": _rua("sherman1.rua"),
    "test1": _rua("test1.rua"),
    "5pt_37x64": lambda: M.laplacian_5pt(37, 64),
    "powerlaw_3000": lambda: M.power_law(3000, 33000, seed=7),
    "empty_rows": _empty_rows,
    "long_rows": _long_rows,
}
for _r in RANDOMS:
    SPMV["random_10x10_" + _r[:3]] = _mtx(os.path.join("random_10x10", _r))
for _n in (1, 63, 64, 65, 513):
    SPMV[f"n{_n}"] = (lambda n: lambda: _random_rows(n, 5, 100 + n))(_n)
# cases the GPU test repeats under the column-panel switches
SPMV_PANEL_CASES = ("powerlaw_3000", "long_rows", "empty_rows")


def spmv_x(name, kind, n):
    if kind == "half":
        return np.full(n, 0.5)
    return np.random.default_rng(1000 + sorted(SPMV).index(name)).standard_normal(n)


SPMV_X = ("random", "half")


# ---------------------------------------------------------------- ILU(k)
def _nonsym_16():
    """laplacian_5pt(16) with every off-diagonal scaled by 1 + U(-0.3, 0.3) and
    the diagonal raised by U(0, 0.5): nonsymmetric values, the grid's pattern"""
    A = M.laplacian_5pt(16).tocoo()
    rng = np.random.default_rng(16)
    off = A.row != A.col
    v = A.data.copy()
    v[off] *= 1.0 + rng.uniform(-0.3, 0.3, int(off.sum()))
    v[~off] += rng.uniform(0.0, 0.5, int((~off).sum()))
    return M._finish(sp.coo_matrix((v, (A.row, A.col)), shape=A.shape))


def _zero_pivot():
    """the (1, 1) pivot is stored and becomes exactly 0: 2 - (1/0.5) * 1"""
    rp = np.array([0, 2, 4, 6, 7], np.int32)
    ci = np.array([0, 1, 0, 1, 2, 3, 3], np.int32)
    v = np.array([0.5, 1.0, 1.0, 2.0, 3.0, 1.0, 1.0])
    return sp.csr_matrix((v, ci, rp), shape=(4, 4))


# name -> (maker, levels, (nx, ny) of a grid or None)
ILUK = {
    "5pt_10x10": (_mtx("5pt_10x10.mtx"), (0, 1, 2), (10, None)),
    "9pt_10x10": (_mtx("9pt_10x10.mtx"), (0, 1, 2), None),
    "7pt_10x10x10": (_mtx("7pt_10x10x10.mtx"), (0, 1, 2), (10, 10)),
    "5pt_37x64": (lambda: M.laplacian_5pt(37, 64), (0, 1, 2), (37, None)),
    "5pt_5x200": (lambda: M.laplacian_5pt(5, 200), (0, 1, 2), (5, None)),
    "5pt_100x100": (lambda: M.laplacian_5pt(100, 100), (0, 1, 2), (100, None)),
    "sherman1": (_rua("sherman1.rua"), (0, 1, 2), (10, 10)),
    "nonsym_16": (_nonsym_16, (0, 1, 2), (16, None)),
    # the matrices test_iluk_device_factors_bitexact runs its long-row path on
    "powerlaw_3000": (lambda: M.power_law(3000, 33000, seed=7), (0, 1), None),
    "thermal_7pt_12": (lambda: M.grid_7pt(12), (0, 1, 2), (12, 12)),
    # 3D grids at the tile and wave3d kernels' edges (ILU(k = 0) factors)
    "7pt_9x5x3": (lambda: M.grid_7pt(9, 5, 3, upwind=0.2), (0,), (9, 5)),
    "7pt_17x9x8": (lambda: M.grid_7pt(17, 9, 8, upwind=0.2), (0,), (17, 9)),
    "7pt_2x40x40": (lambda: M.grid_7pt(2, 40, 40, upwind=0.2), (0,), (2, 40)),
    "7pt_20x30x7": (lambda: M.grid_7pt(20, 30, 7, upwind=0.1), (0,), (20, 30)),
}
ZERO_PIVOT = _zero_pivot
# GG_ILUK_LONG values of test_iluk_device_factors_bitexact's long-row cases
ILUK_LONG = {("powerlaw_3000", 1): 12, ("sherman1", 1): 6, ("9pt_10x10", 2): 0, ("thermal_7pt_12", 1): 9}


def iluk_keys():
    return [(name, k) for name in ILUK for k in ILUK[name][1]]


def to_factors(n, r, diag):
    """The reference's ilukC output r (oracle.ref.iluk) in the layout the
    reference's callers hand LUSolve_ignoreZero: L with a unit diagonal last,
    U with its diagonal first, then the strict upper part by ascending column
    (what orc_iluk emits).  diag: the un-inverted pivots."""
    l_rp = r["l_rp"] + np.arange(n + 1, dtype=np.int32)
    u_rp = r["u_rp"] + np.arange(n + 1, dtype=np.int32)
    l_ci = np.zeros(int(l_rp[-1]), np.int32)
    l_v = np.zeros(int(l_rp[-1]))
    u_ci = np.zeros(int(u_rp[-1]), np.int32)
    u_v = np.zeros(int(u_rp[-1]))
    for i in range(n):
        a, b = int(r["l_rp"][i]), int(r["l_rp"][i + 1])
        p = int(l_rp[i])
        l_ci[p:p + b - a] = r["l_ci"][a:b]
        l_v[p:p + b - a] = r["l_v"][a:b]
        l_ci[p + b - a] = i
        l_v[p + b - a] = 1.0
        a, b = int(r["u_rp"][i]), int(r["u_rp"][i + 1])
        p = int(u_rp[i])
        u_ci[p] = i
        u_v[p] = diag[i]
        o = np.argsort(r["u_ci"][a:b], kind="stable")
        u_ci[p + 1:p + 1 + b - a] = r["u_ci"][a:b][o]
        u_v[p + 1:p + 1 + b - a] = r["u_v"][a:b][o]
    return O.CSR(n, l_rp.astype(np.int32), l_ci, l_v), O.CSR(n, u_rp.astype(np.int32), u_ci, u_v)


def strict(T, diag_first):
    """(row lengths -> row_ptr, cols, vals, diag) of a triangle in the solver's
    layout (U: diagonal first; L: unit diagonal last) without its diagonal"""
    at = T.rp[:-1] if diag_first else T.rp[1:] - 1
    assert np.array_equal(T.ci[at], np.arange(T.n))
    keep = np.ones(len(T.ci), bool)
    keep[at] = False
    return (T.rp - np.arange(T.n + 1, dtype=T.rp.dtype)).astype(np.int32), T.ci[keep], T.v[keep], T.v[at]


def iluk_mismatch(fix, name, k, L, U):
    """'' where (L, U), in the solver's layout, are the factors the reference
    computed for ILUK case (name, k): pattern first, then values (U against
    the reference's rows sorted by column), then 1.0 / diagonal against D"""
    key = f"iluk/{name}/k{k}/"
    l_rp, l_ci, l_v, l_d = strict(L, False)
    u_rp, u_ci, u_v, u_d = strict(U, True)
    if not np.array_equal(l_d, np.ones(L.n)):
        return key + ": L's diagonal is not 1"
    for f, a in (("l_rp", l_rp), ("l_ci", l_ci), ("u_rp", u_rp), ("us_ci", u_ci),
                 ("l_v", l_v), ("us_v", u_v), ("d", 1.0 / u_d)):
        msg = same(fix, key + f, a)
        if msg:
            return msg
    return ""


_factors = {}


def pinned_factors(name, k):
    """(A, L, U): the oracle's ILU(k) factors of ILUK case name after holding
    them to the reference's.  The fixture records the large factors as digests
    only, so the solve cases rebuild them here; nothing the reference did not
    compute bit for bit gets through."""
    if (name, k) not in _factors:
        A = ILUK[name][0]()
        L, U = O.iluk(A, k)
        msg = iluk_mismatch(fixture()[1], name, k, L, U)
        assert msg == "", msg
        _factors[(name, k)] = (A, L, U)
    return _factors[(name, k)]


# ------------------------------------------------------------ LUSolve
RHS =("random", "ones", "big", "small")


def rhs(kind, n):
    if kind == "ones":
        return np.ones(n)
    y = np.random.default_rng(2000 + n).standard_normal(n)
    return y * {"random": 1.0, "big": 1e250, "small": 1e-250}[kind]


SKIP_PIVOT = ("5pt_37x64", 0)      # the factor whose U diagonals are made negligible


def skip_pivot(U):
    """40 U diagonals set to 1e-12 * (1 + u): LUSolve_ignoreZero skips the
    division there (Equal(u, 0), src/SpMV_compute.cpp:132)"""
    rng = np.random.default_rng(40)
    v = U.v.copy()
    rows = np.sort(rng.choice(U.n, 40, replace=False))
    v[U.rp[rows]] = 1e-12 * (1.0 + rng.random(40))
    return O.CSR(U.n, U.rp, U.ci, v), rows


# ------------------------------------------------------------ format conversion
FORMAT_N = (1, 7, 200)


def coo_input(n):
    """(rows, cols, vals): unsorted, repeated (row, col) pairs, an empty row (n > 1)"""
    rng = np.random.default_rng(300 + n)
    nz = max(1, 6 * n)
    r = rng.integers(0, n, nz)
    c = rng.integers(0, n, nz)
    dup = rng.integers(0, nz, nz // 5)
    r[:len(dup)] = r[dup]
    c[:len(dup)] = c[dup]
    if n > 1:
        empty = n // 2
        r[r == empty] = empty - 1
    return r.astype(np.int32), c.astype(np.int32), rng.standard_normal(nz)


def csc_input(n):
    """(col_ptr, row_idx, vals) of an n x n CSC matrix: rows unsorted inside a
    column, repeated (row, col) pairs, an empty row (n > 1)"""
    r, c, v = coo_input(n)
    o = np.argsort(c, kind="stable")
    p = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=n))]).astype(np.int64)
    return p, r[o].astype(np.int64), v[o]


def sort_input(n):
    """(cols, vals, start, end): an unsorted segment inside a longer array"""
    rng = np.random.default_rng(400 + n)
    ln = 3 * n + 2
    return rng.integers(0, n, ln).astype(np.int32), rng.standard_normal(ln), 1, ln - 1



# ------------------------------------------------------------ the fixture
# In memory: {key: whole array} and, for a large array, {key#sha256, key#ends,
# key#size}.  On disk the many small arrays share a few npz members (a zip
# member costs more bytes than most of them hold): keys, kind, size, the whole
# float and integer arrays back to back, the digests and ends as tables.
def _norm(a):
    """float64 or int32, little-endian, contiguous: what the fixture stores"""
    a = np.asarray(a)
    if a.dtype.kind == "f":
        return np.ascontiguousarray(a, "<f8")
    assert a.dtype.kind in "iu" and (a.size == 0 or np.abs(a).max() < 2 ** 31)
    return np.ascontiguousarray(a, "<i4")


def digest(a):
    return hashlib.sha256(_norm(a).tobytes()).hexdigest()


def _ends(a):
    return np.concatenate([a.ravel()[:8], a.ravel()[-8:]]).astype(np.float64)


def put(store, key, a):
    a = _norm(a).ravel()
    if a.size <= WHOLE_MAX:
        store[key] = a
    else:
        store[key + "#sha256"] = np.frombuffer(bytes.fromhex(digest(a)), np.uint8)
        store[key + "#ends"] = _ends(a)
        store[key + "#size"] = np.array([a.size, a.dtype.kind == "f"], np.int32)


def same(fix, key, a):
    """'' where a equals, bit for bit, what the fixture recorded under key; else
    what differs"""
    a = _norm(a).ravel()
    if key in fix:
        w = fix[key]
        if w.shape != a.shape or w.dtype != a.dtype:
            return f"{key}: {a.dtype}{a.shape}, recorded {w.dtype}{w.shape}"
        bits = "<u8" if a.dtype.kind == "f" else "<u4"
        bad = np.flatnonzero(a.view(bits) != w.view(bits))
        if bad.size:
            return (f"{key}: {bad.size} of {a.size} entries differ, first at {bad[0]}: "
                    f"{a[bad[0]]!r} vs recorded {w[bad[0]]!r}")
        return ""
    if key + "#sha256" not in fix:
        return f"{key}: not in the fixture"
    size, is_f = (int(t) for t in fix[key + "#size"])
    if size != a.size or is_f != (a.dtype.kind == "f"):
        return f"{key}: {a.dtype} size {a.size}, recorded size {size} (float: {is_f})"
    if bytes(fix[key + "#sha256"]).hex() != digest(a):
        return f"{key}: sha256 differs; ends {_ends(a)!r} vs recorded {fix[key + '#ends']!r}"
    return ""


def text(a):
    return bytes(a).decode().split("\n")


def as_text(lines):
    return np.frombuffer("\n".join(lines).encode(), np.uint8)


W_F64, W_I32, H_F64, H_I32 = range(4)


def write_npz(path, keys, store, sources):
    """keys: the recorded arrays in order; sources: text lines.  numpy.savez_compressed's
    format with fixed member order and time stamps, so that regenerating the
    fixture rewrites the same bytes."""
    kind, size, wf, wi, sha, ends = [], [], [], [], [], []
    for key in keys:
        if key in store:
            a = store[key]
            kind.append(W_F64 if a.dtype.kind == "f" else W_I32)
            size.append(a.size)
            (wf if a.dtype.kind == "f" else wi).append(a)
        else:
            n, is_f = store[key + "#size"]
            kind.append(H_F64 if is_f else H_I32)
            size.append(int(n))
            sha.append(store[key + "#sha256"])
            ends.append(store[key + "#ends"])
    members = {
        "keys": as_text(keys), "sources": as_text(sources),
        "kind": np.array(kind, np.uint8), "size": np.array(size, "<i4"),
        "whole_f64": np.concatenate(wf + [np.zeros(0, "<f8")]),
        "whole_i32": np.concatenate(wi + [np.zeros(0, "<i4")]),
        "sha256": np.array(sha, np.uint8).reshape(-1, 32),
        "ends": np.array(ends, "<f8").reshape(-1, 16),
    }
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(members):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(members[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def read_npz(path):
    """-> (keys, store as put() builds it, sources)"""
    with np.load(path) as z:
        m = {k: z[k] for k in z.files}
    keys = text(m["keys"])
    store, pf, pi, ph = {}, 0, 0, 0
    for key, kind, size in zip(keys, m["kind"], m["size"]):
        size = int(size)
        if kind == W_F64:
            store[key] = m["whole_f64"][pf:pf + size]
            pf += size
        elif kind == W_I32:
            store[key] = m["whole_i32"][pi:pi + size]
            pi += size
        else:
            store[key + "#sha256"] = m["sha256"][ph]
            store[key + "#ends"] = m["ends"][ph]
            store[key + "#size"] = np.array([size, kind == H_F64], np.int32)
            ph += 1
    assert pf == m["whole_f64"].size and pi == m["whole_i32"].size and ph == len(m["sha256"])
    return keys, store, text(m["sources"])


_fix = None


def fixture():
    """(keys, store, sources) of the committed fixture, read once"""
    global _fix
    if _fix is None:
        _fix = read_npz(PINS)
    return _fix
