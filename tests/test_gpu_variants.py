"""Every alternate launch form against the default solve's bits.

About twenty-five GG_* switches in gpu-gmres_amd/csrc pick another kernel
instantiation or launch structure and promise "the same bits".  Several are
what the library falls back to by itself at sizes the other tests never reach
(the per-step batched orthogonalization, one persistent launch per scenario,
the tail's flow kernel), so each form runs here, per case:

  * the DEFAULT environment once, in a fresh child (tests/variant_worker.py:
    most switches are cached in a function-local static on first use, so they
    cannot be flipped inside this process), and that child's results compared
    with the order-matched oracle bit for bit (the reduction order of the
    child's own layout, which it reports): the anchor;
  * every VARIANT in a child of its own, every saved array and scalar
    bit-identical to the default child's -- and, where the library can say what
    it launched (gg_mgs_kernel, gg_batch_mgs_kernel, gg_division_active), the
    evidence that the variant really ran.  The fold / chunk / flow-tuning
    switches have no such getter: their children are compared, not identified,
    and the anchors assert instead the preconditions under which the library
    reads each switch (a fused forward solve for GG_SPLIT_DIVFOLD: case Cf; the
    sliced copy, the RCM layout and the persistent kernel for the other folds;
    more flow tasks than the CUs hold for GG_FLOW_BPC: case Bbpc; a tail within
    k_tail_small's bounds for GG_TAIL_SMALL).

Two kinds of variant change the arithmetic or the layout instead and are
compared with the oracle in their own terms: GG_FMA_TILE (case H: the
per-triangle division mix, oracle.set_div_mode) and GG_WAVE3D_PLANES /
GG_NO_WAVE3D (case W: the applies against the default child, the solve against
the oracle in the variant's own reduction order).

Case A's grids give (G reduction blocks, J units per thread) = G in 2..7, in
9..15 and >= 17 not a multiple of 8 on the 2D wavefront; G = 1 with J = 1, 2
and 4 in the natural layout (case A1 runs under GG_NO_WAVEFRONT=1: the
smallest 2D wavefront layout holds 4096 slots, G = 2).  test_case_a_grid_coverage
asserts the set on what the children report.  J = 8 needs more than 2.1 M slots
and is out of scope: case Apad reaches that many with 65,664 rows (a 3 x 21888
grid, 342 bands of padding), but its 1024 blocks of the J = 8 instantiation are
not co-resident on an MI355X, so the library runs the per-step kernels there
(gg_mgs_kernel ""), which is what that case then compares -- with and without
the padding skip, over 2 M padding slots.

Cases Epad and Eres are the batch's own fall-backs, with nothing forced in the
default child of Epad: on the padded grid no persistent grid fits, so the
library runs k_dot / k_mgs_step / k_arnoldi_finalize on a (G, nsc) grid by
itself (gg_batch_mgs_kernel ""); in Eres the test hook GG_PERSIST_TEST_LDS
leaves room for one block per CU, fewer than the 258 the grid has, so the first
two-scenario persistent launch gives its cycle up (a bounded wait inside the
kernel) and the batch reruns on the per-step kernels -- the same bits (one
batch per child; the single solves' same fall-back is test_gpu_residency's).

Children run one after the other under subprocess.run(timeout=120) (a safety
limit, not a measurement).  A child that dies by a signal or hits the limit
or ends with any other non-zero status (a HIP error or a GG_ETIMEOUT ends a
child with status 1) sets a module flag: every later test fails at once and
starts nothing.  No child is retried: a failed one is remembered and re-raised.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import cg_ref as C
import oracle as O
import variant_worker as W
from helpers import device_layout

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TIMEOUT = 120
FATAL = {-6, -11, 134, 139}

_GP = [("0/0", 0, 0), ("0/1", 0, 1), ("2/0", 2, 0), ("2/2", 2, 2), ("3/1", 3, 1),
       # settings the launch remaps (gg_mgs_kernel must name what runs)
       ("3/0", 3, 0), ("0/2", 0, 2)]
_A = {f"gather{n}": {"GG_MGS_GATHER": str(g), "GG_MGS_PREFETCH": str(p)} for n, g, p in _GP}
_A.update({"cycle_pipe0": {"GG_CYCLE_PIPE": "0"}, "no_padskip": {"GG_NO_PADSKIP": "1"},
           "no_padskip_no_persist": {"GG_NO_PADSKIP": "1", "GG_NO_PERSIST": "1"}, "no_persist": {"GG_NO_PERSIST": "1"}})
_FOLDS = {"GG_SPLIT_DIVFOLD": "0", "GG_SPLIT_MULFOLD": "0", "GG_SPMV_XDIV": "0", "GG_FLOW_FILLFOLD": "0"}
_E = {"batch_mgs0": {"GG_BATCH_MGS": "0"}, "batch_mgs2_0": {"GG_BATCH_MGS2": "0"}, "gather0": {"GG_MGS_GATHER": "0"},
      "gather3": {"GG_MGS_GATHER": "3"}, "prefetch0": {"GG_MGS_PREFETCH": "0"}, "chunk1": {"GG_BATCH_CHUNK": "1"},
      "chunk2": {"GG_BATCH_CHUNK": "2"}, "chunk50": {"GG_BATCH_CHUNK": "50"}, "zmap0": {"GG_BATCH_ZMAP": "0"},
      "s1_single": {"GG_BATCH_S1_SINGLE": "1"}}
# case -> (the case's own environment, {variant: switches})
CASES = {
    "A": ({}, _A),
    "A1": ({"GG_NO_WAVEFRONT": "1"}, _A),
    "Apad": ({}, {"no_padskip": {"GG_NO_PADSKIP": "1"}, "cycle_pipe0": {"GG_CYCLE_PIPE": "0"},
                  "prefetch2": {"GG_MGS_PREFETCH": "2"}}),
    "B": ({}, {"flow_long4": {"GG_FLOW_LONG": "4"}, "flow_long100000": {"GG_FLOW_LONG": "100000"}}),
    # every row with a term a task of its own: more tasks than 4 waves on each of the CUs, so
    # that the blocks-per-CU cap decides the grid (test_anchor_flow asserts the count)
    "Bbpc": ({"GG_NO_WAVEFRONT": "1", "GG_FLOW_LONG": "0"}, {"flow_bpc4": {"GG_FLOW_BPC": "4"}}),
    # (the four the issue sets; on these flow-kernel factors GG_SPLIT_DIVFOLD is not read --
    # nothing is fused -- so its own coverage is case Cf's)
    "C": ({}, dict({k.lower()[3:] + "0": {k: v} for k, v in _FOLDS.items()}, all_folds0=_FOLDS)),
    # the split engine where A' z is fused into the forward solve (GG_DIV_FMA, grid-shaped
    # factors): the only path on which GG_SPLIT_DIVFOLD is read
    "Cf": ({}, {"split_divfold0": {"GG_SPLIT_DIVFOLD": "0"}, "split_mulfold0": {"GG_SPLIT_MULFOLD": "0"},
                "div_mul_fold0": {"GG_SPLIT_DIVFOLD": "0", "GG_SPLIT_MULFOLD": "0"}}),
    "D": ({}, {"tail_small0": {"GG_TAIL_SMALL": "0"}}),
    "E": ({}, _E),
    "Efix": ({}, _E),
    "Epad": ({}, {"no_padskip": {"GG_NO_PADSKIP": "1"}, "chunk1": {"GG_BATCH_CHUNK": "1"}}),
    "Eres": ({}, {"resid_lds": {"GG_PERSIST_TEST_LDS": "98304"}}),
    "F": ({}, {"hint0": {"GG_TRANSIENT_HINT": "0"}, "chunk1": {"GG_BATCH_CHUNK": "1"}, "batch_mgs0": {"GG_BATCH_MGS": "0"}}),
    "G": ({}, {"chunk1": {"GG_CG_BATCH_CHUNK": "1"}, "chunk3": {"GG_CG_BATCH_CHUNK": "3"},
               "chunk1000": {"GG_CG_BATCH_CHUNK": "1000"}}),
}
# compared with the oracle, not with a default child
H_VARIANTS = {"fma_tile0": ("0", (0, 1)), "fma_tile1": ("1", (2, 1)), "fma_tile2": ("2", (0, 2))}
W_VARIANTS = {"planes": {"GG_WAVE3D_PLANES": "1"}, "no_wave3d": {"GG_NO_WAVE3D": "1"}}
PAIRS = [(c, v) for c, (_, vs) in CASES.items() for v in vs]


class Children:
    """runs and caches the children; dead: a child faulted or hung"""

    def __init__(self, tmp):
        self.tmp = tmp
        self.dead = None
        self.cache = {}
        self.failed = {}
        self.wall = {}

    def run(self, case, name, env_extra):
        key = (case, name)
        if key in self.cache:
            return self.cache[key]
        assert key not in self.failed, f"not run again: {self.failed.get(key)}"
        assert self.dead is None, f"not started: an earlier child faulted or hung ({self.dead})"
        path = os.path.join(self.tmp, f"{case}_{name.replace('/', '_')}.npz")
        env = {k: v for k, v in os.environ.items() if not k.startswith("GG_")}
        env.update(env_extra)
        t0 = time.perf_counter()
        try:
            p = subprocess.run([sys.executable, os.path.join(HERE, "variant_worker.py"), case, path], env=env,
                               capture_output=True, text=True, timeout=TIMEOUT)
        except subprocess.TimeoutExpired:
            self.dead = self.failed[key] = f"{key}: no end within {TIMEOUT} s"
            raise AssertionError(self.dead)
        self.wall[key] = time.perf_counter() - t0
        if p.returncode != 0:
            # a signal (FATAL) for certain, but a HIP error or a GG_ETIMEOUT also ends a
            # child with status 1: any failed child may have left the card faulted, so
            # none is started after it, and this one is never run again
            self.dead = self.failed[key] = f"{key}: exit status {p.returncode}" + \
                (" (a signal)" if p.returncode in FATAL or p.returncode < 0 else "")
        assert p.returncode == 0, f"{key}: exit status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
        with np.load(path) as z:
            out = {k: z[k] for k in z.files}
        print(f"child {case} / {name}: {self.wall[key]:.2f} s wall, {float(out['t_gpu']):.2f} s in the case")
        self.cache[key] = out
        return out

    def default(self, case):
        return self.run(case, "default", CASES[case][0] if case in CASES else {})

    def variant(self, case, name):
        base, vs = CASES[case]
        return self.run(case, name, dict(base, **vs[name]))


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    return Children(str(tmp_path_factory.mktemp("variants")))


# ---- comparisons ---------------------------------------------------------------
def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def evidence_key(k):
    return k == "t_gpu" or k.endswith("mgs_kernel")


def assert_same_child(v, d, what):
    assert set(v) == set(d), (what, set(v) ^ set(d))
    for k in sorted(d):
        if not evidence_key(k):
            assert same_bits(v[k], d[k]), (what, k)


def units_per_thread(G, Ppad):
    """kernels/arnoldi_persist.hip arnoldi_persist_units"""
    J = -(-(Ppad // 2) // (G * 256))
    return 1 if J <= 1 else 2 if J <= 2 else 4 if J <= 4 else 8 if J <= 8 else 0


def persist_name(env, J):
    """the instantiation GG_MGS_GATHER / GG_MGS_PREFETCH select (kernels/arnoldi_persist.hip
    persist_fn, stated on its own): prefetch 2 exists for the elected gather up
    to J = 4, the reducer-only blocks with a prefetch only"""
    g = int(env.get("GG_MGS_GATHER", 2))
    p = min(max(int(env.get("GG_MGS_PREFETCH", 1)), 0), 2)
    g = g if g in (2, 3) else 0
    if g == 2 and p == 2 and J <= 4:
        xg, pf = 2, 2
    elif g == 3 and p:
        xg, pf = 3, 1
    elif g >= 2:
        xg, pf = 2, int(p > 0)
    else:
        xg, pf = 0, int(p > 0)
    return f"k_arnoldi_persist<{J}, {xg}, {pf}>"


def with_order(lay, G, fn, div=None):
    O.set_dot_order(np.asarray(lay, np.int64), int(G))
    if div:
        O.set_div_mode(*div)
    try:
        return fn()
    finally:
        O.set_div_mode()
        O.set_dot_order(None)


def assert_solve(d, p, o, what):
    assert (int(d[f"{p}_status"]), int(d[f"{p}_iters"]), int(d[f"{p}_inner"])) == (o["ret"], o["iters"], o["inner"]), what
    assert same_bits(d[f"{p}_hist"], o["hist"]), what
    assert same_bits(d[f"{p}_x"], o["x"]), what


def assert_batch_is_singles(d, r, S, what):
    for q in range(S):
        s = f"{r}_single{q}"
        assert (int(d[f"{r}_status"][q]), int(d[f"{r}_iters"][q]), int(d[f"{r}_inner"][q]), int(d[f"{r}_restarts"][q])) == \
               (int(d[f"{s}_status"]), int(d[f"{s}_iters"]), int(d[f"{s}_inner"]), int(d[f"{s}_restarts"])), (what, q)
        assert same_bits(d[f"{r}_relres"][q], d[f"{s}_relres"]), (what, q)
        assert same_bits(d[f"{r}_hist{q}"], d[f"{s}_hist"]) and same_bits(d[f"{r}_x"][q], d[f"{s}_x"]), (what, q)


# ---- the anchors: each default child against the order-matched oracle -----------
@pytest.mark.parametrize("case", ["A", "A1", "Apad"])
def test_anchor_single_gmres(children, case):
    d = children.default(case)
    for nx, ny in W.A_GRIDS[case]:
        p = f"g{nx}x{ny}"
        A, b = W.grid_system(nx, ny)
        n = A.shape[0]
        wave = bool(d[f"{p}_uses_wavefront"])
        assert wave == (case != "A1")
        lay, G = device_layout(n, nx if wave else None)
        assert same_bits(d[f"{p}_lay2nat"], lay) and int(d[f"{p}_G"]) == G, p
        L, U = O.ilu0(A)
        for r, opt in W.A_RUNS.items():
            o = with_order(lay, G, lambda: O.gmres_left(A, L, U, b, m=opt["restart"], max_iter=opt["max_iter"],
                                                        tol=opt["tol"]))
            assert_solve(d, f"{p}_{r}", o, (p, r))
        # two full cycles and a partial third, max_iter exhausted; then to convergence
        assert (int(d[f"{p}_fix_status"]), int(d[f"{p}_fix_iters"]), int(d[f"{p}_fix_inner"])) == (1, 70, 70), p
        assert int(d[f"{p}_conv_status"]) == 0, p
        print(f"{p}: G {G}, J {units_per_thread(G, len(lay))}, {d[f'{p}_mgs_kernel']}, converged in "
              f"{int(d[f'{p}_conv_iters'])} ({int(d[f'{p}_conv_inner']) % 30} into its last cycle)")
    if case == "A":
        assert any(int(d[f"g{nx}x{ny}_conv_inner"]) % 30 for nx, ny in W.A_GRIDS[case])      # ends mid-cycle


def test_case_a_grid_coverage(children):
    """the (G, J) edges, on what the children report; every grid persistent"""
    seen = set()
    pad = children.default("Apad")
    assert (int(pad["g3x21888_G"]), units_per_thread(1024, int(pad["g3x21888_Ppad"]))) == (1024, 8)
    assert str(pad["g3x21888_mgs_kernel"]) == ""          # not co-resident: the per-step kernels
    for case in ("A", "A1"):
        d = children.default(case)
        for nx, ny in W.A_GRIDS[case]:
            p = f"g{nx}x{ny}"
            G, J = int(d[f"{p}_G"]), units_per_thread(int(d[f"{p}_G"]), int(d[f"{p}_Ppad"]))
            assert str(d[f"{p}_mgs_kernel"]) == f"k_arnoldi_persist<{J}, 2, 1>", p
            seen.add((G, J))
    print("case A (G, J):", sorted(seen))
    assert {(1, 1), (1, 2), (1, 4)} <= seen
    assert any(2 <= G <= 7 for G, _ in seen) and any(9 <= G <= 15 for G, _ in seen)
    assert any(G >= 17 and G % 8 for G, _ in seen)


@pytest.mark.parametrize("case", ["B", "Bbpc"])
def test_anchor_flow(children, case):
    d = children.default(case)
    A, b, v = W.flow_system(case)
    L, U = O.ilu0(A)
    for T in (L, U):
        off = np.diff(T.rp) - 1                          # (the stored diagonal is no term)
        if case == "B":
            assert off.min() < 32 < off.max()            # rows below and above the flow kernel's long-row bound
            continue
        # Bbpc (GG_FLOW_LONG=0): every row with a term is a task of its own, a wave each, 4
        # waves a block -- more blocks than 4 on each of 256 CUs, so GG_FLOW_BPC decides the
        # grid (kernels.hip launch_trsv_levels: min(occupancy, bpc * CUs, tasks / 4)) ...
        tasks = int(np.count_nonzero(off > 0))
        assert tasks // 4 > 4 * 256
        # ... and few enough a level that the default is one block per CU (at most 4 waves
        # on each CU a level), not already the larger grid
        lev = np.zeros(T.n, np.int64)
        for r in (range(T.n) if T is L else range(T.n - 1, -1, -1)):
            c = T.ci[T.rp[r]:T.rp[r + 1]]
            c = c[c != r]
            lev[r] = lev[c].max() + 1 if c.size else 0
        assert (tasks + T.n) / (int(lev.max()) + 1) <= 4 * 256
    assert not bool(d["d_uses_wavefront"]) and str(d["d_trsv_kernel0"]) == "k_trsv_flow"
    for k, scale in enumerate((1.0, 1e200)):
        assert same_bits(d[f"apply{k}"], O.lusolve(L, U, v * scale)), k
    o = with_order(d["d_lay2nat"], d["d_G"], lambda: O.gmres_left(A, L, U, b, m=30, max_iter=2000, tol=1e-10))
    assert_solve(d, "solve", o, case)


def _assert_split(d, A, P, b, x0, v, opt, what):
    assert same_bits(d["apply_left"], P.left(v)) and same_bits(d["apply_right"], P.right(v)), what
    assert same_bits(d["apply_start"], P.start(v)), what
    o = with_order(d["d_lay2nat"], d["d_G"],
                   lambda: O.gmres_split(A, P, b, x0=x0, m=opt["restart"], max_iter=opt["max_iter"], tol=opt["tol"]))
    assert_solve(d, "solve", o, what)


def test_anchor_split(children):
    d = children.default("C")
    A, P, b, x0, v = W.split_system()
    assert not bool(d["d_uses_wavefront"])
    # what makes case C's switches live (solver.hip enqueue_cycle): A' has its sliced copy and
    # the layout is the RCM one (the x-division path, GG_SPMV_XDIV), both triangles on the
    # flow kernel (its fills folded, GG_FLOW_FILLFOLD), the persistent orthogonalization
    # (GG_SPLIT_MULFOLD).  GG_SPLIT_DIVFOLD is read on the fused path only: case Cf
    n = A.shape[0]
    assert bool(d["d_spmv_sliced"]) and not np.array_equal(d["d_lay2nat"][:n], np.arange(n))
    assert str(d["d_trsv_kernel0"]) == str(d["d_trsv_kernel1"]) == "k_trsv_flow"
    assert str(d["d_mgs_kernel"]).startswith("k_arnoldi_persist<")
    _assert_split(d, A, P, b, x0, v, dict(restart=32, max_iter=2000, tol=1e-11), "C")


def test_anchor_fused_split(children):
    """the split engine with A' z inside the forward solve's launch, GG_DIV_FMA
    on both grid-shaped triangles: against oracle.gmres_split in that mode"""
    d = children.default("Cf")
    A, P, b, v = W.fused_split_system()
    n = A.shape[0]
    assert str(d["d_trsv_kernel0"]).startswith("k_trsv_wave2d_spmv<")          # fused: GG_SPLIT_DIVFOLD is live
    assert str(d["d_mgs_kernel"]).startswith("k_arnoldi_persist<")             # GG_SPLIT_MULFOLD is live
    assert (int(d["division0"]), int(d["division1"])) == (2, 2)
    lay, G = device_layout(n, W.CF_GRID[0])
    assert same_bits(d["d_lay2nat"], lay) and int(d["d_G"]) == G
    O.set_div_mode(2, 2)
    try:
        ops = P.left(v), P.right(v), P.start(v)
    finally:
        O.set_div_mode()
    for name, z in zip(("left", "right"), ops):
        assert same_bits(d[f"apply_{name}"], z), name
    o = with_order(lay, G, lambda: O.gmres_split(A, P, b, m=W.CF_OPT["restart"], max_iter=W.CF_OPT["max_iter"],
                                                 tol=W.CF_OPT["tol"]), div=(2, 2))
    assert_solve(d, "solve", o, "Cf")


def test_anchor_border(children, tmp_path):
    d = children.default("D")
    A, P, nt, b, v = W.border_system(str(tmp_path))
    assert bool(d["d_uses_wavefront"]) and int(d["d_trsv_levels0"]) > 60 + 60 - 1      # the tail's levels on top
    # within k_tail_small's bounds (gg_internal.h kTailSmallRows / kTailSmallLevels), so the
    # default child runs that kernel and GG_TAIL_SMALL=0 is the other one
    assert nt <= 16384 and int(d["d_trsv_levels0"]) - (60 + 60 - 1) <= 256
    lay, G = device_layout(A.shape[0], 60, border=nt)
    assert same_bits(d["d_lay2nat"], lay) and int(d["d_G"]) == G
    _assert_split(d, A, P, b, None, v, dict(restart=32, max_iter=600, tol=1e-10), "D")


@pytest.mark.parametrize("case", ["E", "Efix", "Epad", "Eres"])
def test_anchor_batch(children, case):
    d = children.default(case)
    A, B, X0 = W.batch_system(case)
    n = A.shape[0]
    lay, G = device_layout(n, W.E_GRIDS[case][0])
    assert same_bits(d["d_lay2nat"], lay) and int(d["d_G"]) == G and bool(d["d_batch_engine"])
    J = units_per_thread(G, len(lay))
    L, U = O.ilu0(A)
    for r, (S, opt) in W.E_RUNS[case].items():
        for q in range(S):
            o = with_order(lay, G, lambda: O.gmres_left(A, L, U, B[q], x0=X0[q], m=opt["restart"],
                                                        max_iter=opt["max_iter"], tol=opt["tol"]))
            assert (int(d[f"{r}_status"][q]), int(d[f"{r}_iters"][q]), int(d[f"{r}_inner"][q])) == \
                   (o["ret"], o["iters"], o["inner"]), (r, q)
            assert same_bits(d[f"{r}_hist{q}"], o["hist"]) and same_bits(d[f"{r}_x"][q], o["x"]), (r, q)
            if case != "Eres":                            # (Eres: the batch alone)
                assert_solve(d, f"{r}_single{q}", o, (r, q))
        if case != "Eres":
            assert_batch_is_singles(d, r, S, r)
        # a pair (and an odd last scenario) per launch; one scenario alone on the single kernel
        want = f"k_arnoldi_persist2<{J}>" if S > 1 else f"k_arnoldi_persist<{J}, 2, 1>"
        if case == "Epad":
            # no persistent grid fits: by itself the library runs k_dot, k_mgs_step and
            # k_arnoldi_finalize on a (G, nsc) grid
            assert (G, J) == (1024, 8) and str(d["d_mgs_kernel"]) == ""
            want = ""
        assert str(d[f"{r}_batch_mgs_kernel"]) == want, r
        print(f"{case} {r}: iters {list(d[f'{r}_iters'])} status {list(d[f'{r}_status'])} {d[f'{r}_batch_mgs_kernel']}")
    if case == "E":
        it = [int(x) for x in d["n9_iters"]]
        assert it[1] == 0 and int(d["n9_status"][1]) == 0                  # converged at the start
        assert 0 < it[2] and it[2] + 30 <= min(it[0], it[3])               # ends a cycle and more before the cold ones
        assert list(d["cap3_status"]) == [1, 0, 0] and int(d["cap3_iters"][0]) == 20      # max_iter caps one
    else:
        mi = W.E_RUNS[case]["fix3"][1]["max_iter"]
        assert list(d["fix3_status"]) == [1, 0, 1] and list(d["fix3_iters"]) == [mi, 0, mi]
    if case == "Eres":
        assert G > 256                        # more blocks than CUs: one block per CU cannot hold the grid


def _step_counts(run, nsteps):
    tot = [run(k)["iters_total"] for k in range(nsteps + 1)]
    return [b - a for a, b in zip(tot, tot[1:])]


def test_anchor_transient(children):
    d = children.default("F")
    A, cdiag, sc, ports, taps, X0 = W.transient_system()
    n = A.shape[0]
    lay, G = device_layout(n, 24)
    assert same_bits(d["d_lay2nat"], lay) and int(d["d_G"]) == G
    L, U = O.ilu0(A)

    def run(q, nsteps, tp=None):
        return with_order(lay, G, lambda: O.transient(A, L, U, nsteps, W.F_H, cdiag, sc[q][0], None, ports, X0[q],
                                                      m=32, max_iter=10000, tol=1e-7, sources=sc[q][1], taps=tp))
    o = run(0, W.F_STEPS, taps)
    assert int(d["src_iters_total"]) == o["iters_total"] and int(d["src_ret"]) == 0
    assert same_bits(d["src_ports"], o["ports"]) and same_bits(d["src_x"], o["x"])
    for k, t in enumerate(o["taps"]):
        assert same_bits(d[f"src_taps{k}"], t), k
    steps = _step_counts(lambda k: run(0, k), W.F_STEPS)
    print("F scenario 0, iterations per step:", steps)
    # the pulse's edge: a step that outruns the first chunk the previous step's count sizes
    assert any(b > a + 2 for a, b in zip(steps, steps[1:]))
    for q in range(3):
        oq = run(q, W.F_STEPS)
        assert int(d["tb_iters_total"][q]) == oq["iters_total"], q
        assert same_bits(d["tb_ports"][q], oq["ports"]) and same_bits(d["tb_x"][q], oq["x"]), q
    assert str(d["tb_batch_mgs_kernel"]) == f"k_arnoldi_persist2<{units_per_thread(G, len(lay))}>"


def _minv(A, kind):
    import ainv_ref as R
    if kind == "diag":
        inv = R.diag_nearest(A)
        return lambda v: v * inv
    L, U = O.ilu0(A)
    return lambda v: O.lusolve(L, U, v)


def test_anchor_cg_batch(children):
    d = children.default("G")
    A, B = W.cg_system()
    n = A.shape[0]
    for kind in ("diag", "ilu0"):
        dot = C.layout_dot(d[f"{kind}_lay2nat"], int(d[f"{kind}_G"]))
        minv = _minv(A, kind)
        for r, opt in W.G_RUNS.items():
            for q in range(3):
                ret, x, iters, relres, hist = C.pcg(A, minv, B[q], None, opt["max_iter"], opt["tol"], dot)
                p = f"{kind}_{r}"
                assert (int(d[f"{p}_status"][q]), int(d[f"{p}_iters"][q])) == (ret, iters), (p, q)
                assert same_bits(d[f"{p}_hist{q}"], hist) and same_bits(d[f"{p}_x"][q], x), (p, q)
                assert same_bits(d[f"{p}_relres"][q], np.float64(relres)), (p, q)
        # converged at the start; stopped by max_iter = 13 (no multiple of a chunk of 8, 3 or 1)
        assert list(d[f"{kind}_cap_status"]) == [0, 1, 1] and list(d[f"{kind}_cap_iters"]) == [0, 13, 13]
        assert list(d[f"{kind}_conv_status"]) == [0, 0, 0]
        print(f"G {kind}: converged in {list(d[f'{kind}_conv_iters'])}, batch engine {bool(d[f'{kind}_batch_engine'])}")
    Ab, Bb = W.cg_breakdown_system()
    mb = _minv(Ab, "ilu0")
    assert list(d["brk_status"]) == [C.BREAKDOWN, 0, C.BREAKDOWN] and int(d["brk_ret"]) == C.BREAKDOWN
    dotb = C.layout_dot(d["brk_lay2nat"], int(d["brk_G"]))
    for q in range(3):
        ret, x, iters, relres, hist = C.pcg(Ab, mb, Bb[q], None, 3000, 1e-10, dotb)
        assert (ret, iters) == (int(d["brk_status"][q]), int(d["brk_iters"][q])), q
        assert same_bits(d[f"brk_hist{q}"], hist) and same_bits(d["brk_x"][q], x), q
        assert same_bits(d["brk_relres"][q], np.float64(relres)), q
    # the transient: every step the restated CG on the restated right-hand side, warm start
    At, cdiag, sc, ports = W.cg_transient_system()
    nt = At.shape[0]
    for kind in ("diag", "ilu0"):
        dot = C.layout_dot(d[f"{kind}_lay2nat"], int(d[f"{kind}_G"]))      # (the same grid: the same layout)
        minv = _minv(At, kind)
        counts = []
        for q, (nodes, pulses) in enumerate(sc):
            x = np.zeros(nt)
            total, per = 0, []
            for it in range(1, W.F_STEPS + 1):
                u = np.array([O.pulse(p, it, W.F_H) for p in pulses])
                w = O.transient_rhs(cdiag, nodes, u, x)
                ret, x, iters, _, _ = C.pcg(At, minv, w, x, 3000, 1e-10, dot)
                assert ret == 0
                total += iters
                per.append(iters)
                assert same_bits(d[f"tcg_{kind}_ports"][q][:, it], x[ports]), (kind, q, it)
            assert int(d[f"tcg_{kind}_iters_total"][q]) == total and same_bits(d[f"tcg_{kind}_x"][q], x), (kind, q)
            counts.append(per)
        print(f"G transient {kind}: iterations per step and scenario {counts}")
        mx = [max(c[k] for c in counts) for k in range(W.F_STEPS)]
        # both ends of "first chunk = previous largest count + 2": a step beyond it, a step within it
        assert any(b > a + 2 for a, b in zip(mx, mx[1:])) and any(b <= a + 2 for a, b in zip(mx, mx[1:]))


# ---- the variants ------------------------------------------------------------
def _check_evidence(case, name, env, v, d):
    if case in ("A", "A1", "Apad"):
        for nx, ny in W.A_GRIDS[case]:
            p = f"g{nx}x{ny}"
            J = units_per_thread(int(d[f"{p}_G"]), int(d[f"{p}_Ppad"]))
            want = "" if env.get("GG_NO_PERSIST") == "1" or case == "Apad" else persist_name(env, J)
            assert str(v[f"{p}_mgs_kernel"]) == want, (case, name, p)
            print(f"{case} / {name} {p}: G {int(d[f'{p}_G'])} J {J} '{v[f'{p}_mgs_kernel']}'")
        if name in ("gather3/0", "gather0/2"):
            # the settings the launch remaps: not the environment's numbers
            assert all(f"{env.get('GG_MGS_GATHER', 2)}, {env.get('GG_MGS_PREFETCH', 1)}>" not in str(v[k])
                       for k in v if k.endswith("_mgs_kernel"))
    elif case in ("E", "Efix", "Epad", "Eres", "F"):
        J = units_per_thread(int(d["d_G"]), int(d["d_Ppad"]))
        none = case == "Epad" or "GG_PERSIST_TEST_LDS" in env      # fell back / aborted: the per-step kernels
        keys = [k for k in d if k.endswith("_batch_mgs_kernel")]
        assert keys
        for k in keys:
            if env.get("GG_BATCH_MGS") == "0" or none:
                want = ""
            elif name in ("batch_mgs2_0", "gather0", "gather3", "prefetch0") or k.startswith("n1_"):
                want = persist_name(env, J)
            else:
                want = f"k_arnoldi_persist2<{J}>"
            assert str(v[k]) == want, (case, name, k)
            print(f"{case} / {name} {k}: G {int(d['d_G'])} J {J} '{v[k]}'")
        single = [k for k in d if k.endswith("_mgs_kernel") and not k.endswith("_batch_mgs_kernel")]
        for k in single:      # the scenario solved alone after the batch
            assert str(v[k]) == ("" if none else persist_name(env, J)), (case, name, k)


@pytest.mark.parametrize("case,name", PAIRS, ids=[f"{c}-{v}" for c, v in PAIRS])
def test_variant_same_bits(children, case, name):
    d = children.default(case)
    v = children.variant(case, name)
    assert_same_child(v, d, (case, name))
    _check_evidence(case, name, dict(CASES[case][0], **CASES[case][1][name]), v, d)


@pytest.mark.parametrize("name", sorted(H_VARIANTS))
def test_fma_tile_mix(children, name):
    """GG_FMA_TILE under GG_DIV_FMA on the 3D tiles: bit 0 / 1 admits the fused
    rows on L / U; the other triangle keeps the division (unit L) or the
    multiply by RN(1/d) (U).  Another arithmetic, so against oracle.lusolve in
    that per-triangle mode, on test_tile3d_edges_and_ranges' smallest grid."""
    bits, (ml, mu) = H_VARIANTS[name]
    v = children.run("H", name, {"GG_FMA_TILE": bits})
    A, vs = W.tile_system()
    L, U = O.ilu0(A)
    mode = {0: 0, 1: 1, 2: 2}      # gg_div_mode -> oracle mode
    assert (mode[int(v["division0"])], mode[int(v["division1"])]) == (ml, mu)
    assert bool(v["d_uses_wavefront"]) and str(v["d_trsv_kernel0"]).startswith("k_trsv_tile3d<true")
    O.set_div_mode(ml, mu)
    try:
        ref = [O.lusolve(L, U, y) for y in vs]
    finally:
        O.set_div_mode()
    for k, z in enumerate(ref):
        assert same_bits(v[f"apply{k}"], z), (name, k)


def _assert_grid3d(d, lay, G, what):
    A, b, v = W.grid3d_system()
    L, U = O.ilu0(A)
    for k, scale in enumerate((1.0, 1e-250, 1e250)):
        assert same_bits(d[f"apply{k}"], O.lusolve(L, U, v * scale)), (what, k)
    o = with_order(lay, G, lambda: O.gmres_left(A, L, U, b, m=W.W_OPT["restart"], max_iter=W.W_OPT["max_iter"],
                                                tol=W.W_OPT["tol"]))
    assert_solve(d, "solve", o, what)


def test_anchor_grid3d(children):
    d = children.default("W")
    nx, ny, nz = W.W_DIMS
    lay, G = device_layout(nx * ny * nz, nx, ny)
    assert same_bits(d["d_lay2nat"], lay) and int(d["d_G"]) == G
    assert str(d["d_trsv_kernel0"]).startswith("k_trsv_tile3d<true")
    _assert_grid3d(d, lay, G, "W")


@pytest.mark.parametrize("name", sorted(W_VARIANTS))
def test_grid3d_other_layouts(children, name):
    """a 3D grid off the tiles: the (plane, band) pipeline (GG_WAVE3D_PLANES=1)
    and the flow kernel in the natural order (GG_NO_WAVE3D=1).  Another vector
    space, so another reduction order: the applies equal the default child's,
    the solve the oracle's in the layout this child reports."""
    d = children.default("W")
    v = children.run("W", name, W_VARIANTS[name])
    for k in range(3):
        assert same_bits(v[f"apply{k}"], d[f"apply{k}"]), (name, k)
    if name == "planes":
        assert bool(v["d_uses_wavefront"]) and str(v["d_trsv_kernel0"]).startswith("k_trsv_wave2d<true")
        assert ", true, 1," in str(v["d_trsv_kernel0"])
    else:
        assert not bool(v["d_uses_wavefront"]) and str(v["d_trsv_kernel0"]) == "k_trsv_flow"
    assert not same_bits(v["d_lay2nat"], d["d_lay2nat"])
    _assert_grid3d(v, v["d_lay2nat"], int(v["d_G"]), name)
