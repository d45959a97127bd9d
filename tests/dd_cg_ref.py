"""NumPy restatement of the sharded conjugate-gradient solve (GG_SOLVE_CG in
gg_dd_solve, csrc/dd.hip "short-recurrence methods on shards") -- test code.

The method is cg_ref.pcg on B = P A P^T with M = the ILU(0) of B; what the
shards change is the order of the dots alone.  shard_dot(segments, G) restates
it: segments[p] = shard p's dot range, slot -> index into the (permuted) vector,
-1 = padding (DD.dot_layout(p)[0]: H0 slots on shard 0, which counts the
separator replica, S0 on the others).  Per shard, cg_ref.layout_dot's first
stage over that segment: G blocks of 256 threads, each thread summing its
grid-stride 16-byte units in order, the wave / block tree.  Then the P * G
partials, shard-major and each shard's in block order, through one more block:
256 lanes strided, the wave / block tree (sum_partials over the all-gathered
array).  The paired dot (r.z with z.z) moves both arrays in one all-gather and
sums each of them in this same order, so it needs no restatement of its own.

natural_segments(plan): the segments of the natural block layout from a host
DDPlan -- what the CPU tests use where no device is there to ask (interiors and
separator in B's order, each region padded to a multiple of 512 slots, the
interior region as long as the longest shard's); the device's wavefront
layouts differ from it in the order inside a segment only.
"""
import numpy as np

import cg_ref as C
import oracle as O
from ainv_ref import _wave_tree


def _stage1(seg, G):
    """seg's products -> G block partials: (scatter map, rounds, nthr)"""
    seg = np.asarray(seg, np.int64)
    assert seg.size % 512 == 0, seg.size
    real = np.flatnonzero(seg >= 0)
    units = seg.size // 2
    nthr = G * 256
    return real, seg[real], -(-units // nthr), nthr


def shard_dot(segments, G):
    G = int(G)
    stages = [_stage1(s, G) for s in segments]

    def dot(x, y):
        prod = np.asarray(x) * np.asarray(y)
        parts = []
        for real, rows, rounds, nthr in stages:
            p = np.zeros(rounds * nthr * 2)
            p[real] = prod[rows]
            p = p.reshape(rounds, nthr, 2)
            acc = np.zeros(nthr)
            for k in range(rounds):
                acc = acc + p[k, :, 0]
                acc = acc + p[k, :, 1]
            parts.append(_wave_tree(acc.reshape(G, 256)))
        part = np.concatenate(parts)                    # shard-major, block order inside
        v = np.zeros(256)
        for k0 in range(0, part.size, 256):
            q = part[k0:k0 + 256]
            v[:q.size] = v[:q.size] + q
        return float(_wave_tree(v))
    return dot


def _pad512(k):
    return (max(int(k), 1) + 511) // 512 * 512


def natural_segments(plan):
    """(segments, G) of the natural block layout of a host.DDPlan (module comment)"""
    P = plan.P
    beg = plan.begin
    S0 = max(_pad512(beg[p + 1] - beg[p]) for p in range(P))
    PS = _pad512(plan.nsep) if plan.nsep else 0
    H0 = S0 + PS
    segs = []
    for p in range(P):
        seg = np.full(H0 if p == 0 else S0, -1, np.int64)
        seg[: beg[p + 1] - beg[p]] = np.arange(beg[p], beg[p + 1])
        if p == 0 and plan.nsep:
            seg[S0: S0 + plan.nsep] = np.arange(beg[P], beg[P] + plan.nsep)
        segs.append(seg)
    G = min(1024, max(1, (H0 // 2 + 255) // 256))
    return segs, G


def solve(B, L, U, b, segments, G, x0=None, max_iter=3000, tol=1e-10, info=None):
    """the sharded CG solve restated: (ret, x, iters, relres, hist) of cg_ref.pcg
    on B with M = (LU)^-1 and the dots in the sharded order; b, x0, x in B's order"""
    return C.pcg(B, lambda v: O.lusolve(L, U, v), b, x0, max_iter, tol, dot=shard_dot(segments, G), info=info)


# ---- the systems of the sharded CG tests (tests/test_dd_cg_ref.py on the CPU,
# tests/test_gpu_dd_cg.py and tests/test_gpu_dd_cg_ranks.py on the device) ------
K_CHUNK = 8             # csrc/dd.hip DdCg::kChunk: iterations per enqueued chunk


def _method(name):
    from ggmres import host
    return {"blocks": host.PART_BLOCKS, "bisect": host.PART_BISECT,
            "blocks_color": host.PART_BLOCKS | host.PART_COLOR_SEP,
            "grid_color": host.PART_GRID | host.PART_COLOR_SEP}[name]


# name: (matrices function, its arguments, parts, partition) -- the smallest
# systems of tests/test_gpu_dd.py CASES, one per layout and separator form
LAYOUT_CASES = {
    "5pt_200x160_P2": ("laplacian_5pt", (200, 160), 2, "blocks"),
    "5pt_200x160_P4": ("laplacian_5pt", (200, 160), 4, "blocks"),
    "7pt_24_P4": ("grid_7pt", (24,), 4, "blocks"),
    "7pt_16_P4_bisect": ("grid_7pt", (16,), 4, "bisect"),
    "5pt_200x160_P4_color": ("laplacian_5pt", (200, 160), 4, "blocks_color"),
    "5pt_160x200_P8_grid": ("laplacian_5pt", (160, 200), 8, "grid_color"),
    "5pt_60x60_P1": ("laplacian_5pt", (60, 60), 1, "blocks"),
}
# the small system of the chunk-boundary, start-exit and breakdown tests, and
# the one of the interleaving test (the fused separator step)
SMALL = ("laplacian_5pt", (40, 30), 2, "blocks")
MIXED = ("laplacian_5pt", (96, 80), 4, "blocks_color")
# the breakdowns: SMALL's matrix negated or shifted, b = 1 -> (the exit of
# cg_ref.pcg, iterations performed)
BREAKDOWNS = {"negated": ("rz0", 0), "shift_0.05": ("pq", 1), "shift_2": ("rz", 1)}


def system(spec):
    """(A, parts, partition method) of a table entry above"""
    from ggmres import matrices as M
    fn, args, P, meth = spec
    return getattr(M, fn)(*args), P, _method(meth)


def breakdown_matrix(kind):
    import scipy.sparse as sp
    A = sp.csr_matrix(system(SMALL)[0])
    if kind == "negated":
        S = (-A).tocsr()
    else:
        S = (A - float(kind.split("_")[1]) * sp.identity(A.shape[0], format="csr")).tocsr()
    S.sort_indices()
    return S


def tol_ending_at(hist, k):
    """a tolerance that cg_ref.pcg's history `hist` first meets at iteration k"""
    lo, hi = hist[k], min(hist[:k])
    assert lo < hi, (k, lo, hi)
    return 0.5 * (lo + hi)
