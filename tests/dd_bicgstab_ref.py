"""NumPy restatement of the sharded BiCGStab solve (gg_dd_solve_bicgstab,
csrc/dd.hip "Sharded BiCGStab") -- test code.

No new arithmetic: the method is bicgstab_ref.bicgstab on B = P A P^T with M =
the ILU(0) of B, and what the shards change is the order of the dots alone,
which dd_cg_ref.shard_dot restates (the paired dots move two arrays in one
all-gather and sum each in that same order).  Below: the composition, and the
tables of systems the CPU test (tests/test_dd_bicgstab_ref.py) and the GPU tests
(tests/test_gpu_dd_bicgstab*.py) share.
"""
import numpy as np
import scipy.sparse as sp

import bicgstab_ref as R
import dd_cg_ref as D
import oracle as O
import sr_exit_cases as X

BREAKDOWN = R.BREAKDOWN
K_CHUNK = D.K_CHUNK // 2        # csrc/dd.hip DdBiCgStab::kChunk: iterations per enqueued chunk
tol_ending_at = D.tol_ending_at


def solve(B, L, U, b, segments, G, x0=None, max_iter=3000, tol=1e-10, info=None):
    """the sharded BiCGStab solve restated: (ret, x, iters, relres, hist); b, x0, x in B's order"""
    return R.bicgstab(B, lambda v: O.lusolve(L, U, v), b, x0, max_iter, tol, dot=D.shard_dot(segments, G),
                      info=info)


# name: (matrices function, its arguments, its keywords, parts, partition) -- one
# per interior and separator form, the smallest of tests/test_gpu_dd.py CASES /
# dd_cg_ref.LAYOUT_CASES, made nonsymmetric
LAYOUT_CASES = {
    "5pt_200x160_P2": ("laplacian_5pt", (200, 160), dict(upwind=0.2), 2, "blocks"),
    "5pt_200x160_P4": ("laplacian_5pt", (200, 160), dict(upwind=0.2), 4, "blocks"),
    "5pt_200x160_P4_color": ("laplacian_5pt", (200, 160), dict(upwind=0.2), 4, "blocks_color"),
    "5pt_160x200_P8_grid": ("laplacian_5pt", (160, 200), dict(upwind=0.2), 8, "grid_color"),
    "7pt_16x16x24_P4": ("grid_7pt", (16, 16, 24), dict(upwind=0.1), 4, "blocks"),
    "7pt_16_P4_bisect": ("grid_7pt", (16,), dict(upwind=0.1), 4, "bisect"),
    "sherman1_P4": ("read_rua", ("sherman1.rua",), {}, 4, "bisect"),
    "5pt_60x60_P1": ("laplacian_5pt", (60, 60), dict(upwind=0.2), 1, "blocks"),
}
# the small system of the chunk-boundary and start-exit tests, the one of the
# interleaving test (the fused separator step)
SMALL = ("laplacian_5pt", (40, 30), dict(upwind=0.2), 2, "blocks")
MIXED = ("laplacian_5pt", (96, 80), dict(upwind=0.2), 4, "blocks_color")


def system(spec):
    """(A, parts, partition method) of a table entry above"""
    from conftest import fixture_path
    from ggmres import matrices as M
    fn, args, kw, P, meth = spec
    if fn == "read_rua":
        return M.read_rua(fixture_path(args[0])), P, D._method(meth)
    return getattr(M, fn)(*args, **kw), P, D._method(meth)


def named(key):
    return LAYOUT_CASES[key] if key in LAYOUT_CASES else {"small": SMALL, "mixed": MIXED}[key]


# ---- the breakdowns -------------------------------------------------------------
# tests/sr_exit_cases.py's constructions re-derived for ILU(0) on a partitioned
# system.  Its exact cases are block-diagonal matrices of tiny integer blocks
# solved WITHOUT a preconditioner; the sharded solve always applies the ILU(0)
# of B.  EXACT_BLOCKS below are 3 x 3 integer blocks T whose ILU(0) drops fill
# (so M T is not the identity and the solve does not end at the half step) and
# has pivots +-1, +-2 or +-4: L, U, every triangular solve, every SpMV row and
# every product of every dot stay small dyadic numbers, exact in any summation
# order, and a true zero is a true zero on the device too.  The system is
# block_diag(T, count) around two 1 x 1 connector rows (diagonal 1, b = 0, an
# explicit 0.0 coupling them) at the cut of the two-part block partition: the
# connectors give the partition a separator without touching a block, so
# B = P A P^T keeps every block's rows in order and the ILU(0) of B is the
# blocks' own.  name: (block rows, b per block, exit, iterations performed);
# found by a search in rational arithmetic over blocks with entries in
# {-2..2}, confirmed in floating point by tests/test_dd_bicgstab_ref.py.  The
# search met no block whose next rho is an exact zero with every number
# dyadic, so that exit has no entry here.
EXACT_BLOCKS = {
    "rtv": ([[1, -1, 0], [0, 1, -1], [-1, 0, 1]], [0, 1, 0], "rtv", 0),
    "rtv_mid": ([[1, -1, 0], [0, 1, -1], [-1, 0, 1]], [1, 1, 1], "rtv", 1),
    "omega": ([[1, -1, -1], [0, 1, -1], [-2, 0, 1]], [0, 1, 0], "omega", 1),
}
EXACT_COUNT = 90                # blocks per part: n = 2 * (3 * 90 + 1)


def exact_system(name):
    """(A, b) of an EXACT_BLOCKS entry (natural order)"""
    rows, bb, why, its = EXACT_BLOCKS[name]
    T = X.block_diag(X._dense_rows(rows), EXACT_COUNT)
    m = T.shape[0]
    # [T, c0, c1, T]; the connectors' explicit zeros stay stored: they are what
    # couples the two parts
    rp = np.concatenate([T.indptr, T.nnz + np.array([2, 4]), T.nnz + 4 + T.indptr[1:]])
    ci = np.concatenate([T.indices, [m, m + 1, m, m + 1], m + 2 + T.indices])
    v = np.concatenate([T.data, [1.0, 0.0, 0.0, 1.0], T.data])
    A = sp.csr_matrix((v, ci.astype(np.int32), rp.astype(np.int32)), shape=(2 * m + 2,) * 2)
    b = np.concatenate([np.tile(np.asarray(bb, np.float64), EXACT_COUNT), [0.0, 0.0],
                        np.tile(np.asarray(bb, np.float64), EXACT_COUNT)])
    return A, b


# ---- the transient loop ---------------------------------------------------------
C_CAP, H_STEP = 1e-3, 1e-2               # A = G + (c / h) I, as tests/dd_transient_ref.py
# tests/dd_transient_ref.py's small system made nonsymmetric: (G's function,
# arguments, keywords, parts, partition, steps)
TRANSIENT_SMALL = ("laplacian_5pt", (40, 30), dict(upwind=0.2), 2, "blocks", 10)


def transient_system():
    """(A = G + C/h, cdiag, parts, partition method, steps) of TRANSIENT_SMALL"""
    from ggmres import matrices as M
    fn, args, kw, P, meth, nsteps = TRANSIENT_SMALL
    A = M.transient(getattr(M, fn)(*args, **kw), c=C_CAP, h=H_STEP)
    return A, np.full(A.shape[0], C_CAP / H_STEP), P, D._method(meth), nsteps


def transient(B, L, U, q, segs, G, nsteps, h, cdiag, src_node, sources, ports, x0, max_iter=10000, tol=1e-7):
    """dd_transient_ref.transient's step loop with solve() above as the step:
    dict(ret, x, ports [nport, nsteps+1], iters_total, steps [(ret, iters)], whys [the
    exit each step took, bicgstab_ref's info["why"]])"""
    x = np.array(x0, np.float64, copy=True)
    ports = np.asarray(ports, np.int64)
    pv = np.zeros((len(ports), nsteps + 1))
    pv[:, 0] = x[ports]
    status, steps, whys = 0, [], []
    for it in range(1, nsteps + 1):
        u = np.array([O.source_value(k, p, it, h) for k, p in sources], np.float64)
        w = O.transient_rhs(cdiag, src_node, u, x)
        info = {}
        ret, xs, iters, relres, hist = solve(B, L, U, w[q], segs, G, x[q], max_iter, tol, info=info)
        whys.append(info["why"])
        x = np.empty_like(x)
        x[q] = xs
        if ret != 0:
            status = ret
        steps.append((int(ret), int(iters)))
        pv[:, it] = x[ports]
    return dict(ret=status, x=x, ports=pv, iters_total=sum(i for _, i in steps), steps=steps, whys=whys)


def exact_transient(name):
    """an EXACT_BLOCKS system as a transient whose every right-hand side is the
    block's b: cdiag = 0, one DC source of value b[r] on every row with b[r] != 0.
    (A, cdiag, src_node, sources)"""
    A, b = exact_system(name)
    nodes = np.flatnonzero(b).astype(np.int32)
    return A, np.zeros(A.shape[0]), nodes, [(O.SRC_DC, np.array([b[r]])) for r in nodes]
