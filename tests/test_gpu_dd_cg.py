"""GPU: the sharded conjugate-gradient solve (GG_SOLVE_CG in gg_dd_solve,
csrc/dd.hip) in one process (GG_DD_LOCAL) against its restatement
tests/dd_cg_ref.py: cg_ref.pcg on B = P A P^T with the ILU(0) of B and the dots
in the sharded order (dd_cg_ref.shard_dot over DD.dot_layout).

Bar: return code, iteration count, the whole history, relres and x[q] are
bit-identical (np.array_equal) to the restatement; against the serial-order
cg_ref.pcg the history is within 1e-10 of its scale, with the one-iteration
straddle rule of tests/test_gpu_dd.py check_serial.  b = A 1 and tol 1e-10
unless a test says otherwise.  CPU iteration counts in the natural block layout
(tests/test_dd_cg_ref.py): 188 / 188 / 202 / 204 on the 200 x 160 grids, 93 and
81 on the 3D grids, 60 on 60 x 60, 44 on the small 40 x 30 system.
"""
import numpy as np
import pytest

import cg_ref as C
import dd_cg_ref as D
import ggmres
import oracle as O
from ggmres import host, matrices as M
from ggmres.dd import DD, PROF_NAMES, PROF_ORTH
from test_gpu_dd import check_serial

pytestmark = pytest.mark.gpu
CG = ggmres.SOLVE_CG
K = D.K_CHUNK

_cache = {}


def setup(key):
    """(A, d, q, B, L, U, segments, G) of a LAYOUT_CASES name, "small" or "mixed", once"""
    if key not in _cache:
        spec = D.LAYOUT_CASES[key] if key in D.LAYOUT_CASES else {"small": D.SMALL, "mixed": D.MIXED}[key]
        A, P, method = D.system(spec)
        _cache[key] = build(A, P, method)
    return _cache[key]


def build(A, P, method):
    d = DD(P, device=0)
    d.set_system(A, method)
    pinv, q = d.perm()
    B = host.permute(A, pinv, q)
    L, U = O.ilu0(B)
    segs, G = zip(*[d.dot_layout(p) for p in range(P)])
    return A, d, q, B, L, U, list(segs), G[0]


_REF = {}


def reference(key, b, x0=None, max_iter=3000, tol=1e-10, tag=None):
    """the restatement in the sharded order (b, x0 natural order); the default
    solve of a case is computed once and never modified"""
    A, d, q, B, L, U, segs, G = setup(key)
    k = (key, tag, max_iter, tol) if tag is not None else None
    if k in _REF:
        return _REF[k]
    out = D.solve(B, L, U, b[q], segs, G, None if x0 is None else x0[q], max_iter, tol)
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


@pytest.mark.parametrize("key", sorted(D.LAYOUT_CASES))
def test_dd_cg_bit_identical_to_the_restatement(key):
    A, d, q, B, L, U, segs, G = setup(key)
    b = M.rhs_ones(A)
    o = reference(key, b, tag="ones")
    assert o[0] == 0 and o[2] > 30
    g = d.solve(b, restart=30, max_iter=3000, tol=1e-10, flags=CG)
    assert g["ret"] == 0
    same_bits(g, o, q, f"sharded CG {key}")
    assert np.linalg.norm(g["x"] - 1.0) < 1e-7 * np.sqrt(len(b))
    ret, x, iters, relres, hist = C.pcg(B, lambda v: O.lusolve(L, U, v), b[q])       # serial-order dots
    check_serial(g, dict(hist=hist, iters=iters, x=x), x_g=g["x"][q], tol=1e-10)


@pytest.mark.parametrize("key", ["5pt_200x160_P4", "7pt_16_P4_bisect"])
def test_dd_cg_warm_start_and_exhaustion(key):
    A, d, q, B, L, U, segs, G = setup(key)
    b = M.rhs_ones(A)
    x0 = np.random.default_rng(9).standard_normal(A.shape[0])
    o = reference(key, b, x0=x0, max_iter=40)
    assert o[0] == 1 and o[2] == 40
    g = d.solve(b, x0=x0, restart=30, max_iter=40, tol=1e-10, flags=CG)
    assert g["ret"] == 1 and g["iters"] == 40 and g["hist"].size == 41
    same_bits(g, o, q, f"sharded CG {key} warm start, max_iter 40")


@pytest.mark.parametrize("max_iter", [0, 1, K - 1, K, K + 1, 2 * K])
def test_dd_cg_chunk_boundaries_max_iter(max_iter):
    A, d, q, B, L, U, segs, G = setup("small")
    b = M.rhs_ones(A)
    full = reference("small", b, tag="ones")
    assert full[0] == 0 and full[2] > 2 * K + 2
    o = reference("small", b, max_iter=max_iter, tol=1e-300)
    assert o[0] == 1 and o[2] == max_iter and np.array_equal(o[4], full[4][:max_iter + 1])
    g = d.solve(b, restart=30, max_iter=max_iter, tol=1e-300, flags=CG)
    same_bits(g, o, q, f"sharded CG max_iter {max_iter}")


@pytest.mark.parametrize("end", [K, K + 1])
def test_dd_cg_converges_at_a_chunk_boundary(end):
    """a tolerance met at a chunk's last iteration (K) and at the next chunk's
    first (K + 1), from the restatement's history: the launches and exchanges
    of up to two chunks run behind the end and change nothing"""
    A, d, q, B, L, U, segs, G = setup("small")
    b = M.rhs_ones(A)
    full = reference("small", b, tag="ones")
    tol = D.tol_ending_at(full[4], end)
    o = reference("small", b, tol=tol)
    assert o[0] == 0 and o[2] == end
    g = d.solve(b, restart=30, max_iter=3000, tol=tol, flags=CG)
    same_bits(g, o, q, f"sharded CG ending at iteration {end}")


def test_dd_cg_start_exits():
    A, d, q, B, L, U, segs, G = setup("small")
    n = A.shape[0]
    z = d.solve(np.zeros(n), restart=30, max_iter=3000, tol=1e-10, flags=CG)          # b = 0: normb -> 1
    assert z["ret"] == 0 and z["iters"] == 0 and z["hist"].tolist() == [0.0]
    assert np.array_equal(z["x"], np.zeros(n))
    b = M.rhs_ones(A)
    xs = d.solve(b, restart=30, max_iter=3000, tol=1e-10, flags=CG)["x"]              # the converged solution
    o = reference("small", b, x0=xs, tol=1e-8)
    assert o[0] == 0 and o[2] == 0
    e = d.solve(b, x0=xs, restart=30, max_iter=3000, tol=1e-8, flags=CG)
    assert e["ret"] == 0 and e["iters"] == 0 and np.array_equal(e["x"], xs)
    same_bits(e, o, q, "sharded CG from the converged solution")


@pytest.mark.parametrize("kind", sorted(D.BREAKDOWNS))
def test_dd_cg_breakdown(kind):
    why, its = D.BREAKDOWNS[kind]
    A, d0, q0, B0, L0, U0, segs0, G0 = setup("small")
    S = D.breakdown_matrix(kind)
    _, P, method = D.system(D.SMALL)
    _, d, q, B, L, U, segs, G = build(S, P, method)
    try:
        n = S.shape[0]
        b = np.ones(n)
        info = {}
        o = D.solve(B, L, U, b[q], segs, G, info=info)
        assert o[0] == C.BREAKDOWN and info["why"] == why and o[2] == its, info
        g = d.solve(b, restart=30, max_iter=3000, tol=1e-10, flags=CG)
        assert g["ret"] == ggmres.EBREAKDOWN
        msg = ggmres.lib().gg_last_error().decode()
        assert msg == (f"gg_dd_solve: conjugate gradients broke down at iteration {its} "
                       "(p.Ap or r.Mr not positive: A and M must be symmetric positive definite)"), msg
        same_bits(g, o, q, f"sharded CG breakdown {kind}")
        g2 = d.solve(b, restart=30, max_iter=3000, tol=1e-10, flags=CG)                # the object is clean
        same_bits(g2, o, q, f"sharded CG breakdown {kind}, again")
        # the same object then solves the SPD system with a fresh object's bits
        d.set_system(A, method)
        bs = M.rhs_ones(A)
        g3 = d.solve(bs, restart=30, max_iter=3000, tol=1e-10, flags=CG)
        f3 = d0.solve(bs, restart=30, max_iter=3000, tol=1e-10, flags=CG)
        assert np.array_equal(d.perm()[1], q0)
        same_bits(g3, reference("small", bs, tag="ones"), q0, "sharded CG after a breakdown")
        assert np.array_equal(g3["hist"], f3["hist"]) and np.array_equal(g3["x"], f3["x"])
    finally:
        d.close()


def test_dd_cg_interleaved_with_gmres():
    """CG, GMRES(30), CG, CGS2-GMRES, CG on one object: each bit-identical to the
    same solve on an object that ran nothing else, the GMRES ones to the oracle
    in the sharded order as tests/test_gpu_dd.py expects -- CG leaves the work
    space, the wave sentinels and the error words as GMRES needs them (and takes
    them as GMRES leaves them)"""
    A, d, q, B, L, U, segs, G = setup("mixed")
    _, P, method = D.system(D.MIXED)
    b = M.rhs_ones(A)
    assert d.info()["wave_separator"] == 1                  # the fused separator step
    runs = [("cg", CG), ("mgs", 0), ("cg", CG), ("cgs2", ggmres.SOLVE_CGS2), ("cg", CG)]
    got = [d.solve(b, restart=30, max_iter=1500, tol=1e-10, flags=f) for _, f in runs]
    fresh = {}
    for name, f in runs:
        if name in fresh:
            continue
        e = DD(P, device=0)
        e.set_system(A, method)
        fresh[name] = e.solve(b, restart=30, max_iter=1500, tol=1e-10, flags=f)
        e.close()
    for (name, f), g in zip(runs, got):
        w = fresh[name]
        assert (g["ret"], g["iters"], g["inner"], g["restarts"]) == (w["ret"], w["iters"], w["inner"], w["restarts"])
        assert g["ret"] == 0, name
        assert np.array_equal(g["hist"], w["hist"]) and np.array_equal(g["x"], w["x"]), name
    same_bits(got[0], reference("mixed", b, tag="ones"), q, "sharded CG, mixed")
    for k, cgs2 in ((1, False), (3, True)):
        O.set_dot_order_shards(segs, G)
        O.set_orth(cgs2)
        try:
            ref = O.gmres_left(B, L, U, b[q], m=30, max_iter=1500, tol=1e-10)
        finally:
            O.set_dot_order(None)
            O.set_orth()
        assert got[k]["iters"] == ref["iters"] and np.array_equal(got[k]["hist"], ref["hist"])
        assert np.array_equal(got[k]["x"][q], ref["x"])


@pytest.mark.parametrize("flags", [CG | ggmres.SOLVE_CGS2, ggmres.SOLVE_BICGSTAB, CG | 0x10])
def test_dd_cg_refusals(flags):
    A, d, q, B, L, U, segs, G = setup("small")
    with pytest.raises(ggmres.GGError) as e:
        d.solve(M.rhs_ones(A), restart=30, max_iter=10, flags=flags)
    assert e.value.code == -1                                                            # GG_EINVAL
    with pytest.raises(ggmres.GGError) as e:
        d.solve(M.rhs_ones(A), restart=0, max_iter=10, flags=CG)                         # restart is validated
    assert e.value.code == -1


@pytest.mark.parametrize("key,max_iter,tol", [("small", 2 * K + 3, 1e-300), ("5pt_200x160_P4_color", 3000, 1e-10)])
def test_dd_cg_profile_counts(key, max_iter, tol):
    """every family's launch count = the iterations performed x its marks per
    iteration: one for the SpMV and each of the apply's three, two for
    GG_DD_PROF_ORTH (p.q | all-gather | x, r update and r.z, z.z | all-gather | p
    update) -- which pins two partial all-gathers per iteration"""
    A, d, q, B, L, U, segs, G = setup(key)
    b = M.rhs_ones(A)
    d.profile(True)
    try:
        g = d.solve(b, restart=30, max_iter=max_iter, tol=tol, flags=CG)
        counts = [d.profile_get(k) for k in range(len(PROF_NAMES))]
    finally:
        d.profile(False)
    its = g["iters"]
    assert its > 0 and (its == max_iter or g["ret"] == 0)
    for k, (n, ms) in enumerate(counts):
        assert n == its * (2 if k == PROF_ORTH else 1), (PROF_NAMES[k], n, its)
        assert ms > 0.0
    same_bits(g, reference(key, b, max_iter=max_iter, tol=tol, tag="ones"), q, "sharded CG, profiled")
