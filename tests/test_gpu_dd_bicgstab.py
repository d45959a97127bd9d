"""GPU: the sharded BiCGStab solve (gg_dd_solve_bicgstab, csrc/dd.hip) in one
process (GG_DD_LOCAL) against its restatement tests/dd_bicgstab_ref.py:
bicgstab_ref.bicgstab on B = P A P^T with the ILU(0) of B and the dots in the
sharded order (dd_cg_ref.shard_dot over DD.dot_layout).

Bar: return code, iteration count, the whole history, relres and x[q] are
bit-identical (np.array_equal, NaN equal to NaN) to the restatement.  b = A 1
and tol 1e-10 unless a test says otherwise.  CPU iteration counts in the natural
block layout: tests/test_dd_bicgstab_ref.py.
"""
import numpy as np
import pytest

import dd_bicgstab_ref as Q
import ggmres
import oracle as O
from ggmres import host, matrices as M
from ggmres.dd import DD, PROF_NAMES, PROF_ORTH

pytestmark = pytest.mark.gpu
BI = ggmres.SOLVE_BICGSTAB
K = Q.K_CHUNK
EINVAL, ESTATE = -1, -5

_cache = {}


def build(A, P, method):
    d = DD(P, device=0)
    d.set_system(A, method)
    pinv, q = d.perm()
    B = host.permute(A, pinv, q)
    L, U = O.ilu0(B)
    segs, G = zip(*[d.dot_layout(p) for p in range(P)])
    return A, d, q, B, L, U, list(segs), G[0]


def setup(key):
    """(A, d, q, B, L, U, segments, G) of a LAYOUT_CASES name, "small" or "mixed", once"""
    if key not in _cache:
        _cache[key] = build(*Q.system(Q.named(key)))
    return _cache[key]


_REF = {}


def reference(key, b, x0=None, max_iter=3000, tol=1e-10, tag=None):
    """the restatement in the sharded order (b, x0 natural order); a tagged solve
    is computed once and never modified"""
    A, d, q, B, L, U, segs, G = setup(key)
    k = (key, tag, max_iter, tol) if tag is not None else None
    if k in _REF:
        return _REF[k]
    out = Q.solve(B, L, U, b[q], segs, G, None if x0 is None else x0[q], max_iter, tol)
    if k:
        _REF[k] = out
    return out


def same_bits(g, o, q, what):
    ret, x, iters, relres, hist = o
    print(f"{what}: device ret {g['ret']} iters {g['iters']} relres {g['relres']!r}; "
          f"restatement ret {ret} iters {iters} relres {relres!r}")
    assert g["ret"] == ret, what
    assert g["iters"] == g["inner"] == iters and g["restarts"] == 0, what
    assert g["hist"].shape == hist.shape, what
    if not np.array_equal(g["hist"], hist, equal_nan=True):
        k = int(np.flatnonzero(g["hist"] != hist)[0])
        raise AssertionError(f"{what}: history differs first at entry {k}: {g['hist'][k]!r} vs {hist[k]!r}")
    assert g["relres"] == relres or (np.isnan(relres) and np.isnan(g["relres"])), what
    assert np.array_equal(g["x"][q], x, equal_nan=True), what


def run(d, b, **kw):
    kw.setdefault("restart", 30)
    kw.setdefault("max_iter", 3000)
    kw.setdefault("tol", 1e-10)
    return d.solve_bicgstab(b, **kw)


@pytest.mark.parametrize("key", sorted(Q.LAYOUT_CASES))
def test_dd_bicgstab_bit_identical_to_the_restatement(key):
    A, d, q, B, L, U, segs, G = setup(key)
    b = M.rhs_ones(A)
    o = reference(key, b, tag="ones")
    assert o[0] == 0 and o[2] > 2 * K + 2
    g = run(d, b, flags=BI)
    assert g["ret"] == 0
    same_bits(g, o, q, f"sharded BiCGStab {key}")
    assert np.linalg.norm(g["x"] - 1.0) < 1e-6 * np.sqrt(len(b))


def test_dd_bicgstab_flags_zero_and_warm_start():
    """flags 0 means BiCGStab too; a warm start that exhausts max_iter"""
    A, d, q, B, L, U, segs, G = setup("7pt_16_P4_bisect")
    b = M.rhs_ones(A)
    same_bits(run(d, b, flags=0), reference("7pt_16_P4_bisect", b, tag="ones"), q, "flags 0")
    x0 = np.random.default_rng(9).standard_normal(A.shape[0])
    o = reference("7pt_16_P4_bisect", b, x0=x0, max_iter=20)
    assert o[0] == 1 and o[2] == 20
    g = run(d, b, x0=x0, max_iter=20, flags=BI)
    assert g["ret"] == 1 and g["iters"] == 20 and g["hist"].size == 21
    same_bits(g, o, q, "warm start, max_iter 20")


def full_small():
    A, d, q, B, L, U, segs, G = setup("small")
    b = M.rhs_ones(A)
    full = reference("small", b, tag="ones")
    assert full[0] == 0 and full[2] > 2 * K + 2
    return A, d, q, b, full


@pytest.mark.parametrize("which", ["0", "1", "K", "2K", "end", "end-1"])
def test_dd_bicgstab_chunk_boundaries_max_iter(which):
    A, d, q, b, full = full_small()
    end = full[2]
    max_iter = {"0": 0, "1": 1, "K": K, "2K": 2 * K, "end": end, "end-1": end - 1}[which]
    o = reference("small", b, max_iter=max_iter)
    if which == "end":
        assert o[0] == 0 and o[2] == end
    else:
        assert o[0] == 1 and o[2] == max_iter
    assert np.array_equal(o[4], full[4][:max_iter + 1])
    g = run(d, b, max_iter=max_iter, flags=BI)
    same_bits(g, o, q, f"sharded BiCGStab max_iter {max_iter}")


@pytest.mark.parametrize("end", [K, K + 1, 3 * K, 3 * K + 1])
def test_dd_bicgstab_converges_at_a_chunk_boundary(end):
    """a tolerance met at a chunk's last iteration and at the next chunk's first,
    from the restatement's history: the launches and exchanges of up to two
    chunks run behind the end and change nothing (the first and the third
    chunk's boundaries: the history is a record low there, tests/test_dd_bicgstab_ref.py)"""
    A, d, q, b, full = full_small()
    tol = Q.tol_ending_at(full[4], end)
    o = reference("small", b, tol=tol)
    assert o[0] == 0 and o[2] == end
    g = run(d, b, tol=tol, flags=BI)
    same_bits(g, o, q, f"sharded BiCGStab ending at iteration {end}")


def test_dd_bicgstab_start_exits():
    A, d, q, b, full = full_small()
    n = A.shape[0]
    z = run(d, np.zeros(n), flags=BI)                                       # b = 0: normb -> 1
    assert z["ret"] == 0 and z["iters"] == 0 and z["hist"].tolist() == [0.0]
    assert np.array_equal(z["x"], np.zeros(n))
    xs = run(d, b, flags=BI)["x"]                                            # the converged solution
    o = reference("small", b, x0=xs, tol=1e-8)
    assert o[0] == 0 and o[2] == 0
    e = run(d, b, x0=xs, tol=1e-8, flags=BI)
    assert e["ret"] == 0 and e["iters"] == 0 and np.array_equal(e["x"], xs)
    same_bits(e, o, q, "sharded BiCGStab from the converged solution")


def last_error():
    return ggmres.lib().gg_last_error().decode()


def test_dd_bicgstab_nan_in_b_breaks_down_at_the_start_and_leaves_the_object_clean():
    """NaN in b: normb, the initial residual and rho are NaN -- rho at the start,
    iteration 0, x untouched.  The next solve on the object gives the clean bits,
    so the re-zeroing reached every vector and partial the NaN had reached"""
    A, d0, q0, b, full = full_small()
    _, d, q, B, L, U, segs, G = build(*Q.system(Q.SMALL))
    try:
        assert np.array_equal(q, q0)
        bn = b.copy()
        bn[7] = np.nan
        o = Q.solve(B, L, U, bn[q], segs, G)
        assert o[0] == Q.BREAKDOWN and o[2] == 0 and np.isnan(o[3])
        g = run(d, bn, flags=BI)
        assert g["ret"] == ggmres.EBREAKDOWN
        # (the sign bit of a NaN is not specified: printf's %g gives "nan" or "-nan")
        assert last_error().replace("-nan", "nan") == (
            "gg_dd_solve_bicgstab: BiCGStab broke down at iteration 0: rho = nan (zero or not finite)"), last_error()
        same_bits(g, o, q, "NaN in b")
        assert np.array_equal(g["x"], np.zeros(A.shape[0]))
        same_bits(run(d, b, flags=BI), full, q, "after the NaN breakdown")
    finally:
        d.close()


@pytest.mark.parametrize("name", sorted(Q.EXACT_BLOCKS))
def test_dd_bicgstab_exact_breakdowns(name):
    """rt.v, omega (and the next rho where a construction exists) exact zeros under
    ILU(0) on a two-part system: dd_bicgstab_ref.EXACT_BLOCKS"""
    why, its = Q.EXACT_BLOCKS[name][2:]
    A, b = Q.exact_system(name)
    _, d, q, B, L, U, segs, G = build(A, 2, host.PART_BLOCKS)
    try:
        assert d.info()["nsep"] == 2
        info = {}
        o = Q.solve(B, L, U, b[q], segs, G, info=info)
        assert o[0] == Q.BREAKDOWN and info["why"] == why and o[2] == its and info["bad"] == 0.0
        g = run(d, b, flags=BI)
        assert g["ret"] == ggmres.EBREAKDOWN
        word = {"rtv": "rt.v", "omega": "omega", "rho": "rho"}[why]
        assert last_error() == (f"gg_dd_solve_bicgstab: BiCGStab broke down at iteration {its}: {word} = 0 "
                                "(zero or not finite)"), last_error()
        same_bits(g, o, q, f"exact breakdown {name}")
        same_bits(run(d, b, flags=BI), o, q, f"exact breakdown {name}, again")
    finally:
        d.close()


def test_dd_bicgstab_interleaved_with_gmres_and_cg():
    """BiCGStab, GMRES(30), CG, BiCGStab, CGS2-GMRES on one object: each gives the
    bits of the same solve on an object that ran nothing else (CG on this
    nonsymmetric system ends as it ends -- the same way on both objects)"""
    A, d, q, B, L, U, segs, G = setup("mixed")
    _, P, method = Q.system(Q.MIXED)
    b = M.rhs_ones(A)
    assert d.info()["wave_separator"] == 1                  # the fused separator step
    kw = dict(restart=30, max_iter=1500, tol=1e-10)
    calls = {"bi": lambda e: e.solve_bicgstab(b, flags=BI, **kw), "mgs": lambda e: e.solve(b, flags=0, **kw),
             "cg": lambda e: e.solve(b, flags=ggmres.SOLVE_CG, **dict(kw, max_iter=60)),
             "cgs2": lambda e: e.solve(b, flags=ggmres.SOLVE_CGS2, **kw)}
    order = ["bi", "mgs", "cg", "bi", "cgs2"]
    got = [calls[name](d) for name in order]
    fresh = {}
    for name in calls:
        e = DD(P, device=0)
        try:
            e.set_system(A, method)
            fresh[name] = calls[name](e)
        finally:
            e.close()
    for name, g in zip(order, got):
        w = fresh[name]
        assert (g["ret"], g["iters"], g["inner"], g["restarts"]) == (w["ret"], w["iters"], w["inner"], w["restarts"])
        assert np.array_equal(g["hist"], w["hist"], equal_nan=True), name
        assert np.array_equal(g["x"], w["x"], equal_nan=True), name
        if name != "cg":
            assert g["ret"] == 0, name
    same_bits(got[0], reference("mixed", b, max_iter=1500, tag="ones"), q, "sharded BiCGStab, mixed")


@pytest.mark.parametrize("flags", [ggmres.SOLVE_CG, ggmres.SOLVE_CGS2, 0x10, BI | 0x10])
def test_dd_bicgstab_refusals(flags):
    A, d, q, b, full = full_small()
    with pytest.raises(ggmres.GGError) as e:
        run(d, b, max_iter=10, flags=flags)
    assert e.value.code == EINVAL
    with pytest.raises(ggmres.GGError) as e:
        run(d, b, restart=0, max_iter=10, flags=BI)                          # restart is validated
    assert e.value.code == EINVAL
    with pytest.raises(ggmres.GGError) as e:
        run(d, b, max_iter=-1, flags=BI)
    assert e.value.code == EINVAL
    same_bits(run(d, b, flags=BI), full, q, "after the refusals")


def test_dd_bicgstab_before_set_system():
    e = DD(2, device=0)
    try:
        e.n = 4
        with pytest.raises(ggmres.GGError) as err:
            e.solve_bicgstab(np.ones(4), flags=BI)
        assert err.value.code == ESTATE
    finally:
        e.close()


@pytest.mark.parametrize("key,max_iter,tol", [("small", 2 * K + 3, 1e-300), ("5pt_200x160_P4_color", 3000, 1e-10)])
def test_dd_bicgstab_profile_counts(key, max_iter, tol):
    """every family's launch count = the iterations performed x its marks per
    iteration: two for the SpMV and each of the apply's three, three for
    GG_DD_PROF_ORTH -- which pins three partial all-gathers per iteration"""
    A, d, q, B, L, U, segs, G = setup(key)
    b = M.rhs_ones(A)
    d.profile(True)
    try:
        g = run(d, b, max_iter=max_iter, tol=tol, flags=BI)
        counts = [d.profile_get(k) for k in range(len(PROF_NAMES))]
    finally:
        d.profile(False)
    its = g["iters"]
    assert its > 0 and (its == max_iter or g["ret"] == 0)
    for k, (n, ms) in enumerate(counts):
        assert n == its * (3 if k == PROF_ORTH else 2), (PROF_NAMES[k], n, its)
        assert ms > 0.0
    same_bits(g, reference(key, b, max_iter=max_iter, tol=tol, tag="ones"), q, "sharded BiCGStab, profiled")


def test_dd_bicgstab_device_vectors():
    """gg_dd_solve_bicgstab_device on device vectors: the bits of the host-vector form"""
    import ctypes
    from test_gpu_batch import _hip         # libggmres's own HIP runtime (not torch's in this process)
    A, d, q, b, full = full_small()
    hx = np.zeros(A.shape[0])
    hip = _hip()
    db, dx = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(db), b.nbytes) == 0 and hip.hipMalloc(ctypes.byref(dx), hx.nbytes) == 0
    try:
        assert hip.hipMemcpy(db, b.ctypes.data, b.nbytes, 1) == 0
        assert hip.hipMemcpy(dx, hx.ctypes.data, hx.nbytes, 1) == 0
        r = d.solve_bicgstab_device(db.value, dx.value, restart=30, max_iter=3000, tol=1e-10, flags=BI)
        assert hip.hipMemcpy(hx.ctypes.data, dx, hx.nbytes, 2) == 0
    finally:
        hip.hipFree(db)
        hip.hipFree(dx)
    same_bits(dict(r, x=hx, hist=d.history()), full, q, "device vectors")
