"""The cases of tests/golden/ref_engine_pins.npz: what the reference's own host
GMRES engines (GMRES_leftILU0, the GMRES without a preconditioner, GMRESilu
over MyILUPP::HostPrecond_*; cut out of src/gmres.cu and src/preconditioner.cu
into oracle/_ref/libgg_ref.so, see oracle/Makefile) were run on.  Shared by the
generator (make_ref_engine_pins.py) and the tests (test_ref_engine_pins.py,
test_gpu_ref_engine_pins.py).  The fixture holds outputs only: ret, iters
(*max_iter as the engine left it), relres (*tol as it left it) and x; the
inputs are rebuilt here from seeded generators, with no reference needed.

Per engine the cases are the smallest at which its branches differ: cold and
warm starts, b = 0 (normb -> 1), a start that already solves the system
(converged at the "<=" test before the loop), a tolerance EQUAL to the starting
residual (the same test, where "<" would go on), n = 1, convergence at the last
iteration of a cycle, convergence at the residual test after a restart (the
tolerance set to the cycle's last estimate, which "<" inside the loop refuses
and the smaller true residual passes), and exhaustion with max_iter a multiple
of m (ret 1).  No case ends its max_iter inside a cycle without converging:
the reference is undefined there (its closing Update(m-1) reads Hessenberg
columns the cycle never wrote), see DEVIATION below.

A case marked gpu is also run on the device (test_gpu_ref_engine_pins.py) and
stores x whole; the others store an x above WHOLE_MAX elements as a sha256.
"""
import ctypes
import os
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

import oracle as O
from ggmres import matrices as M
from golden import ref_pin_cases as C
from helpers import device_layout, make_split

HERE = os.path.dirname(os.path.abspath(__file__))
PINS = os.path.join(HERE, "ref_engine_pins.npz")
WHOLE_MAX = C.WHOLE_MAX
ENGINES = ("left", "plain", "split")
MIN_CASES = 8

# env: the orthogonalization form the GPU test runs the case with
#   None = the one-launch kernel, or (variable, value) set through monkeypatch
# tol: a number, "start" (the starting residual itself) or ("restart", cycles):
#   the last estimate of the first cycle, among `cycles`, whose true residual
#   after the restart is smaller
Case = namedtuple("Case", "engine name system m tol max_iter rhs x0 gpu env")


def _case(engine, name, system, m, tol, max_iter, rhs="ones", x0=None, gpu=False, env=None):
    return Case(engine, name, system, m, tol, max_iter, rhs, x0, gpu, env)


# ------------------------------------------------------------------ systems
def _perm_40x33():
    """a symmetric random permutation of the 40 x 33 grid: no grid left, the
    ILU(0) factors go to the dataflow kernel"""
    A = M.laplacian_5pt(40, 33)
    p = np.random.default_rng(4033).permutation(A.shape[0])
    return M._finish(A[p][:, p])


def _rand300():
    """test_abi.random_nonsym(300, 4, 11)"""
    rng = np.random.default_rng(11)
    rows = np.repeat(np.arange(300), 4)
    cols = rng.integers(0, 300, 1200)
    A = sp.csr_matrix((rng.standard_normal(1200), (rows, cols)), shape=(300, 300))
    A = A + sp.diags(np.abs(A).sum(axis=1).A1 + 1.0)
    return M._finish(A)


def _one():
    return sp.csr_matrix(np.array([[2.5]]))


# name -> (maker, (nx, ny) of the grid the device lays the vectors out by, or None)
SYSTEMS = {
    "5pt_40x40": (lambda: M.laplacian_5pt(40, 40), (40, None)),
    "5pt_37x23": (lambda: M.laplacian_5pt(37, 23), (37, None)),
    "perm_40x33": (_perm_40x33, None),
    "7pt_17x9x8": (lambda: M.grid_7pt(17, 9, 8, upwind=0.2), (17, 9)),
    "sherman1": (lambda: M.read_rua(os.path.join(C.FIX, "sherman1.rua")), (10, 10)),
    "rand300": (_rand300, None),
    "n1": (_one, None),
    "5pt_3x2": (lambda: M.laplacian_5pt(3, 2), None),
}
# the systems' numbers in the seeds of their vectors (a new system takes a new number)
SYSTEM_SEED = {"5pt_37x23": 0, "5pt_40x40": 1, "7pt_17x9x8": 2, "n1": 3, "perm_40x33": 4, "rand300": 5,
               "sherman1": 6, "5pt_3x2": 7}
# the kernel family of the triangular solves a gpu case is there for
# (Solver.uses_wavefront, a fragment of Solver.trsv_kernel(0))
KERNEL = {
    ("left", "5pt_40x40"): (True, "wave2d"), ("left", "5pt_37x23"): (True, "wave2d"),
    ("left", "perm_40x33"): (False, "flow"), ("left", "7pt_17x9x8"): (True, "tile3d"),
    ("left", "sherman1"): (True, None), ("left", "n1"): (False, None),
    ("split", "5pt_40x40"): (False, "flow"), ("split", "5pt_37x23"): (True, "wave2d"),
}
# split preconditioners: random permutations on 40 x 40 (the dataflow kernel),
# identity permutations on 37 x 23 (the 2D wavefront; `middle` rounded to fp32,
# so with the integer stencil and fp32 right-hand sides the boundary driver's
# float interface can carry the same system)
SPLIT_SEED = {"5pt_40x40": 9, "5pt_37x23": 23, "n1": 1, "5pt_3x2": 32}
SPLIT_IDENTITY = ("5pt_37x23", "n1", "5pt_3x2")

_cache = {}


def system(name):
    if ("A", name) not in _cache:
        _cache[("A", name)] = SYSTEMS[name][0]()
    return _cache[("A", name)]


def factors(name):
    if ("LU", name) not in _cache:
        _cache[("LU", name)] = O.ilu0(system(name))
    return _cache[("LU", name)]


def split(name):
    if ("P", name) not in _cache:
        P = make_split(system(name), seed=SPLIT_SEED[name], identity_perm=name in SPLIT_IDENTITY)
        if name in SPLIT_IDENTITY:
            P = O.Split(P.L, P.U, P.middle.astype(np.float32).astype(np.float64), P.perm_row, P.perm_col,
                        P.lscale, P.rscale)
        _cache[("P", name)] = P
    return _cache[("P", name)]


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def vectors(case):
    """(b, x0): the seeded vectors are fp32 values (on an integer stencil so
    are A 1 and A x0), so a case can also pass a float boundary"""
    A = system(case.system)
    n = A.shape[0]
    seed = 7000 + 13 * SYSTEM_SEED[case.system] + ENGINES.index(case.engine)
    rng = np.random.default_rng(seed)
    x0 = None
    if case.x0 == "random":
        x0 = _f32(rng.standard_normal(n) * 0.1)
    elif case.x0 == "solution":
        x0 = rng.integers(32, 97, n) / 64.0     # 7 bits: A x0 of an integer stencil is an fp32 value too
    if case.rhs == "ones":
        b = O.spmv(A, np.ones(n))
    elif case.rhs == "uniform":
        b = _f32(M.rhs_uniform(n, seed=seed))
    elif case.rhs == "zero":
        b = np.zeros(n)
    elif case.rhs == "exact":
        b = O.spmv(A, x0)                      # b - A x0 is 0 to the last bit
    else:
        raise ValueError(case.rhs)
    return b, x0


def _engine(mod, case, b, x0, tol, max_iter):
    """mod: oracle (the restatement) or oracle.ref (the reference itself)"""
    A = system(case.system)
    kw = dict(x0=x0, m=case.m, max_iter=max_iter, tol=tol)
    if case.engine == "left":
        L, U = factors(case.system)
        fn = mod.gmres_left if mod is O else mod.gmres_left_ilu0
        return fn(A, L, U, b, **kw)
    if case.engine == "plain":
        return mod.gmres_plain(A, b, **kw)
    return mod.gmres_split(A, split(case.system), b, **kw)


def tolerance(case):
    """The case's tolerance as a number.  The two derived ones come from the
    oracle's serial run -- a wrong oracle gives another tolerance and with it
    another result than the one recorded."""
    if ("tol", case) in _cache:
        return _cache[("tol", case)]
    b, x0 = vectors(case)
    if case.tol == "start":
        tol = _engine(O, case, b, x0, 1e-300, 0)["relres"]
    elif isinstance(case.tol, tuple):
        cycles = case.tol[1]
        h = _engine(O, case, b, x0, 1e-300, case.m * cycles)["hist"]
        tol = None
        for c in range(cycles):                 # hist: start, then m estimates + 1 true residual per cycle
            est, true = h[(case.m + 1) * (c + 1) - 1], h[(case.m + 1) * (c + 1)]
            if true < est < h[0] and np.all(h[:(case.m + 1) * (c + 1)] >= est):
                tol = est
                break
        assert tol is not None, f"{case.name}: no cycle whose true residual is below its last estimate"
    else:
        tol = float(case.tol)
    _cache[("tol", case)] = tol
    return tol


def run(mod, case):
    b, x0 = vectors(case)
    return _engine(mod, case, b, x0, tolerance(case), case.max_iter)


def split_layout(P):
    """(lay2nat, G) of the split engine's vector space off the wavefront: the
    dataflow kernel's RCM layout, from the product's host analysis
    (gg_host_split_layout; no device needed)"""
    import ggmres
    n = P.L.n
    PI, PD = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    slot = np.zeros(max(n, 1), np.int64)
    info = np.zeros(9, np.int32)
    ok = ggmres.lib().gg_host_split_layout(
        ctypes.c_int(n), P.L.rp.ctypes.data_as(PI), P.L.ci.ctypes.data_as(PI), P.L.v.ctypes.data_as(PD),
        P.U.rp.ctypes.data_as(PI), P.U.ci.ctypes.data_as(PI), P.U.v.ctypes.data_as(PD),
        slot.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), info.ctypes.data_as(PI))
    lay, G = device_layout(n)
    if ok == 1:
        assert info[0] == 6
        lay = np.full(len(lay), -1, np.int64)
        lay[slot[:n]] = np.arange(n)
    return lay, G


def layout(case):
    """(lay2nat, G) of the device's vector space for a gpu case; GG_WIDE_FORCE
    sums every dot in 512 block partials"""
    n = system(case.system).shape[0]
    grid = SYSTEMS[case.system][1]
    wave = KERNEL.get((case.engine, case.system), (False, None))[0]
    if case.engine == "split" and not wave:
        lay, G = split_layout(split(case.system))
    elif case.engine != "plain" and wave:
        lay, G = device_layout(n, *grid)
    else:
        lay, G = device_layout(n)                # natural order
    if case.env and case.env[0] == "GG_WIDE_FORCE":
        G = 512
    return lay, G


def run_order_matched(case, lay_G=None):
    lay, G = lay_G if lay_G is not None else layout(case)
    tolerance(case)                             # a derived one comes from the serial order
    O.set_dot_order(lay, G)
    try:
        return run(O, case)
    finally:
        O.set_dot_order(None)


# ------------------------------------------------------------------ the cases
def _edges(engine, sysname, m, tol, cyc_m, cyc_tol, restart_m):
    """the edge cases every engine gets, on one system; cyc_m / cyc_tol: a
    restart length and tolerance with which the cold start converges at
    iteration cyc_m, the last of the first cycle"""
    c = lambda name, **kw: _case(engine, f"{sysname}/{name}", sysname, **kw)
    return [
        c("zero_rhs", m=m, tol=tol, max_iter=100, rhs="zero", gpu=True),
        c("exact_start", m=m, tol=tol, max_iter=100, rhs="exact", x0="solution", gpu=True),
        c("tol_is_start", m=m, tol="start", max_iter=100, rhs="uniform", x0="random"),
        c("cycle_end", m=cyc_m, tol=cyc_tol, max_iter=1000, gpu=True),
        c("post_restart", m=restart_m, tol=("restart", 12), max_iter=1000, rhs="uniform"),
        c("exhausted", m=5, tol=1e-300, max_iter=15, rhs="uniform", gpu=True),
        _case(engine, "n1/cold", "n1", m=m, tol=tol, max_iter=100, rhs="uniform", gpu=engine != "split"),
        # m above n = 6: the Krylov space is exhausted inside the one cycle and
        # the engine goes on dividing by norms at rounding level
        _case(engine, "5pt_3x2/krylov_exhausted", "5pt_3x2", m=30, tol=1e-300, max_iter=30, rhs="uniform"),
    ]


CASES = (
    # ---- GMRES_leftILU0
    [_case("left", "5pt_40x40/cold_m30", "5pt_40x40", 30, 1e-10, 3000, gpu=True),
     _case("left", "5pt_40x40/warm_m33", "5pt_40x40", 33, 1e-10, 3000, "uniform", "random", gpu=True),
     _case("left", "5pt_40x40/cold_m5_wide", "5pt_40x40", 5, 1e-6, 3000, gpu=True, env=("GG_WIDE_FORCE", "1")),
     _case("left", "5pt_37x23/cold_m1", "5pt_37x23", 1, 1e-3, 3000, "uniform", gpu=True),
     _case("left", "5pt_37x23/warm_m5_per_step", "5pt_37x23", 5, 1e-6, 3000, "uniform", "random", gpu=True,
           env=("GG_NO_PERSIST", "1")),
     _case("left", "perm_40x33/cold_m30", "perm_40x33", 30, 1e-10, 3000, gpu=True),
     _case("left", "perm_40x33/warm_m33", "perm_40x33", 33, 1e-6, 3000, "uniform", "random"),
     _case("left", "7pt_17x9x8/warm_m33", "7pt_17x9x8", 33, 1e-8, 3000, "uniform", "random", gpu=True),
     _case("left", "7pt_17x9x8/cold_m30", "7pt_17x9x8", 30, 1e-6, 3000),
     _case("left", "sherman1/cold_m30", "sherman1", 30, 1e-10, 3000, "uniform", gpu=True),
     _case("left", "sherman1/warm_m33", "sherman1", 33, 1e-6, 3000, "uniform", "random")]
    + _edges("left", "5pt_37x23", 30, 1e-10, cyc_m=24, cyc_tol=1e-6, restart_m=5)
    # ---- GMRES (no preconditioner)
    + [_case("plain", "5pt_37x23/cold_m30", "5pt_37x23", 30, 1e-8, 3000, gpu=True),
       _case("plain", "5pt_37x23/warm_m33", "5pt_37x23", 33, 1e-6, 3000, "uniform", "random"),
       _case("plain", "rand300/cold_m30", "rand300", 30, 1e-10, 3000),
       _case("plain", "rand300/warm_m5", "rand300", 5, 1e-10, 3000, "uniform", "random", gpu=True),
       _case("plain", "rand300/cold_m1", "rand300", 1, 1e-3, 3000, "uniform")]
    + _edges("plain", "rand300", 30, 1e-10, cyc_m=20, cyc_tol=1e-6, restart_m=5)
    # ---- GMRESilu + MyILUPP::HostPrecond_*
    + [_case("split", "5pt_40x40/cold_pg", "5pt_40x40", 32, 1e-7, 10000, "uniform", gpu=True),
       _case("split", "5pt_40x40/warm_m7", "5pt_40x40", 7, 1e-9, 10000, "uniform", "random", gpu=True),
       _case("split", "5pt_37x23/cold_pg", "5pt_37x23", 32, 1e-7, 10000, gpu=True),
       _case("split", "5pt_37x23/warm_pg", "5pt_37x23", 32, 1e-7, 10000, "uniform", "random", gpu=True),
       _case("split", "5pt_37x23/warm_m7", "5pt_37x23", 7, 1e-9, 10000, "uniform", "random", gpu=True)]
    + _edges("split", "5pt_37x23", 32, 1e-7, cyc_m=24, cyc_tol=1e-6, restart_m=7)
)
# the split cases the boundary driver's gmresInterfacePG::GMRES_host_PG can
# carry: its fixed m = 32, tol 1e-7, max_iter 10000; A, middle, b, x0 in fp32
DRIVER_CASES = ("5pt_37x23/cold_pg", "5pt_37x23/warm_pg", "5pt_37x23/zero_rhs", "5pt_37x23/exact_start")
# b = 0, the start that solves the system, n = 1: nothing for a changed
# operation order to change
TRIVIAL = ("zero_rhs", "exact_start", "n1/cold")

# The one known deviation of the restatement: max_iter ending INSIDE a cycle
# without convergence.  The reference's closing Update(x, m-1, ...) then reads
# columns of H the cycle never wrote (uninitialised memory: NaN or garbage in x
# and *tol); the oracle and the product update with the last filled column.
# That is what the reference itself computes when the restart length is cut to
# the budget (m = max_iter = 17: a whole cycle, defined), so the fixture records
# that run under DEVIATION_KEY and the oracle's m = 30 run is held to it: the
# deviation is exactly "the last cycle as if m were the iterations left".
DEVIATION = _case("left", "5pt_37x64/max_iter_inside_cycle", None, 30, 1e-10, 17)
DEVIATION_KEY = "deviation/cut_to_budget"


def deviation_run(fn, m=None):
    """fn (oracle.gmres_left or oracle.ref.gmres_left_ilu0) on DEVIATION, or
    with the restart length m in its place"""
    A = M.laplacian_5pt(37, 64)
    L, U = O.ilu0(A)
    b = O.spmv(A, np.ones(A.shape[0]))
    return fn(A, L, U, b, m=DEVIATION.m if m is None else m, max_iter=DEVIATION.max_iter, tol=DEVIATION.tol)


# MyILUPP's four host maps on their own (GMRESilu's building blocks), on both
# split preconditioners; 1e250 / 1e-250 leave the device's fast-division range
SPLIT_MAP_SCALES = {"unit": 1.0, "big": 1e250, "small": 1e-250}
SPLIT_MAPS = ("left", "right", "start", "rhs")


def split_map_keys():
    return [(name, scale) for name in ("5pt_40x40", "5pt_37x23") for scale in SPLIT_MAP_SCALES]


def split_map_vector(name, scale):
    n = system(name).shape[0]
    return np.random.default_rng(8000 + n).standard_normal(n) * SPLIT_MAP_SCALES[scale]


def oracle_split_map(P, which, v):
    """HostPrecond_rhs is HostPrecond_left (src/preconditioner.cu:1055-1057)"""
    return {"left": P.left, "right": P.right, "start": P.start, "rhs": P.left}[which](v)


def trivial(case):
    return case.name.endswith(TRIVIAL)


def no_iteration(case):
    """ends at the test before the loop: nothing for another orthogonalization to change"""
    return trivial(case) and not case.name.startswith("n1") or case.tol == "start"


def key(case):
    return f"{case.engine}/{case.name}"


def by_key():
    return {key(c): c for c in CASES}


def put(store, k, a, whole):
    """ref_pin_cases.put, with x of a gpu case stored whole at any size"""
    a = C._norm(a).ravel()
    if whole and a.size > WHOLE_MAX:
        store[k] = a
    else:
        C.put(store, k, a)


_fix = None


def fixture():
    """(keys, store, sources) of the committed fixture, read once"""
    global _fix
    if _fix is None:
        _fix = C.read_npz(PINS)
    return _fix
