"""The oracle's GMRES engines and the product's host engine against what the
reference's OWN host engines compute (tests/golden/ref_engine_pins.npz, recorded
by golden/make_ref_engine_pins.py from GMRES_leftILU0, the GMRES without a
preconditioner and GMRESilu over MyILUPP::HostPrecond_*, cut out of the
reference checkout's src/gmres.cu and src/preconditioner.cu and built in
double, contraction off).

Every bar is bit equality of ret, iters (*max_iter), relres (*tol) and x (a
sha256 for the large x of the cases no GPU test reads).  Only the live rerun
needs oracle/_ref; everything else reads the committed fixture.  The negative
controls rerun the oracle with another orthogonalization (CGS2) and with the
split preconditioner's two scales swapped and require at least 3 of 4
non-trivial cases to leave the fixture, so the pins are shown able to fail."""
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle as O
from conftest import REPO
from golden import ref_engine_cases as E
from golden import ref_pin_cases as C
from oracle import ref as R

BOUNDARY = os.path.join(REPO, "tests", "boundary")
KEYS = [E.key(c) for c in E.CASES]


@pytest.fixture(scope="module")
def fix():
    return E.fixture()[1]


def mismatch(fix, case, o):
    """'' where the run o reproduces what the reference left for the case"""
    k = E.key(case)
    for f, a in (("ret", [o["ret"]]), ("iters", [o["iters"]]), ("relres", [o["relres"]]), ("x", o["x"])):
        a = np.asarray(a, np.float64 if f in ("relres", "x") else np.int32)
        msg = C.same(fix, f"{k}/{f}", a)
        if msg:
            return msg
    return ""


# ------------------------------------------------------------ live reference
@pytest.mark.skipif(not R.engines_available(),
                    reason="oracle/_ref/libgg_ref.so not built with the engines (no reference checkout)")
def test_live_reference_reproduces_fixture():
    from golden import make_ref_engine_pins as G
    keys, store, sources = E.fixture()
    report = []
    lkeys, lstore, lsources = G.build_store(report)
    assert lsources == sources                      # the same reference text went in
    assert lkeys == keys and set(lstore) == set(store)
    for key in store:
        assert lstore[key].dtype == store[key].dtype and lstore[key].tobytes() == store[key].tobytes(), key
    assert not [line for line in report if line.startswith("dropped")]


def test_fixture_size_and_contents():
    keys, store, sources = E.fixture()
    assert os.path.getsize(E.PINS) < 256 * 1024
    assert sorted(s.split()[0] for s in sources) == sorted(
        ["SpMV_compute.cpp", "iluk.cpp", "itsol.cpp", "formatConvert.cpp", "SpMV.h", "defs.h", "gpuData.h",
         "config.h", "gmres.cu", "preconditioner.cu"])
    assert all(len(s.split()[1]) == 64 for s in sources)
    for e in E.ENGINES:
        assert sum(c.engine == e and E.key(c) + "/ret" in store for c in E.CASES) >= E.MIN_CASES
    for c in E.CASES:                               # no case was dropped
        k = E.key(c)
        assert all(f"{k}/{f}" in store for f in ("ret", "iters", "relres", "tol"))
        n = E.system(c.system).shape[0]
        if c.gpu or n <= C.WHOLE_MAX:               # whole where a GPU test reads it
            assert store[k + "/x"].size == n and np.all(np.isfinite(store[k + "/x"]))
        else:
            assert k + "/x#sha256" in store and int(store[k + "/x#size"][0]) == n
        assert np.isfinite(store[k + "/relres"][0])
    assert store["deviation/max_iter_inside_cycle"][0] == 1
    dev = store["relres_order_dev"][0]
    assert 0.0 < dev < 1e-3                         # rounding's reach into a residual near 1e-10, not a method's
    # the branches the cases are there for
    got = lambda k: (int(store[k + "/ret"][0]), int(store[k + "/iters"][0]))
    for c in E.CASES:
        k = E.key(c)
        if c.name.endswith(("zero_rhs", "exact_start", "tol_is_start")):
            assert got(k) == (0, 0)
        if c.name.endswith("tol_is_start"):
            assert store[k + "/relres"][0] == store[k + "/tol"][0] > 0
        if c.name.endswith("cycle_end"):
            assert got(k) == (0, c.m)               # the inner test at i = m - 1
        if c.name.endswith("post_restart"):         # j already counts the next iteration there
            assert got(k)[0] == 0 and got(k)[1] % c.m == 1 and store[k + "/relres"][0] < store[k + "/tol"][0]
        if c.name.endswith("exhausted"):
            assert got(k) == (1, c.max_iter) and c.max_iter % c.m == 0
    assert {c.m for c in E.CASES if c.engine == "left"} >= {30, 5, 1, 33}


# ------------------------------------------------------------ oracle
@pytest.mark.parametrize("k", KEYS)
def test_oracle_engine(fix, k):
    """oracle.gmres_left / gmres_plain / gmres_split, serial order"""
    case = E.by_key()[k]
    assert np.array([E.tolerance(case)]).tobytes() == fix[k + "/tol"].tobytes()
    assert mismatch(fix, case, E.run(O, case)) == ""


def test_plain_is_left_with_identity_factors(fix):
    """what test_gpu_ainv.py compares set_precond_none with -- the left engine
    with L = U = I -- is the reference's unpreconditioned GMRES bit for bit"""
    import scipy.sparse as sp
    for case in (c for c in E.CASES if c.engine == "plain"):
        A = E.system(case.system)
        I = O.csr(sp.identity(A.shape[0], format="csr"))
        b, x0 = E.vectors(case)
        o = O.gmres_left(A, I, I, b, x0=x0, m=case.m, max_iter=case.max_iter, tol=E.tolerance(case))
        assert mismatch(fix, case, o) == "", E.key(case)


@pytest.mark.parametrize("name,scale", E.split_map_keys())
def test_oracle_split_maps(fix, name, scale):
    """orc_split_left / _right / _start against MyILUPP::HostPrecond_* on their own"""
    P, v = E.split(name), E.split_map_vector(name, scale)
    for which in E.SPLIT_MAPS:
        assert C.same(fix, f"splitmap/{name}/{scale}/{which}", E.oracle_split_map(P, which, v)) == ""
    # swapping the two scales leaves the fixture: the maps are able to fail
    Q = O.Split(P.L, P.U, P.middle, P.perm_row, P.perm_col, P.rscale, P.lscale)
    for which in E.SPLIT_MAPS:
        assert C.same(fix, f"splitmap/{name}/{scale}/{which}", E.oracle_split_map(Q, which, v)) != ""


def test_max_iter_inside_a_cycle(fix):
    """The one deviation: where max_iter ends inside a cycle without
    convergence the reference's closing Update(m-1) reads columns of H the
    cycle never wrote; the oracle updates with the last filled column.  That is
    the reference's own result with the restart length cut to the iterations
    left (a whole cycle, defined), recorded in the fixture."""
    o = E.deviation_run(O.gmres_left)
    assert (o["ret"], o["iters"], o["inner"]) == (1, E.DEVIATION.max_iter, E.DEVIATION.max_iter)
    assert C.same(fix, E.DEVIATION_KEY + "/relres", np.array([o["relres"]])) == ""
    assert C.same(fix, E.DEVIATION_KEY + "/x", o["x"]) == ""
    if R.engines_available():
        r = E.deviation_run(R.gmres_left_ilu0)
        assert not (r["relres"] == o["relres"] and np.array_equal(r["x"], o["x"]))


# ------------------------------------------------------------ product host engine
def _driver():
    exe = os.path.join(BOUNDARY, "pg_driver")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", BOUNDARY, "pg_driver"], check=True, capture_output=True)
    return exe


@pytest.mark.parametrize("name", E.DRIVER_CASES)
def test_host_engine_through_boundary_driver(fix, tmp_path, name):
    """gmresInterfacePG::GMRES_host_PG (csrc/host/gmres_host.cpp behind the
    reference's C++ boundary, tests/boundary/pg_driver.cpp mode 2) on the split
    cases whose A, middle, b and x0 are fp32 values: x is the reference's x
    rounded once to fp32, max_it its iteration count, tol its relres in fp32"""
    case = E.by_key()["split/" + name]
    assert (case.m, E.tolerance(case)) == (32, 1e-7)          # the interface's fixed settings
    A, P = E.system(case.system), E.split(case.system)
    n = A.shape[0]
    b, x0 = E.vectors(case)
    x0 = np.zeros(n) if x0 is None else x0
    f32 = lambda a: np.asarray(a, np.float32)
    for a in (A.data, P.middle, b, x0):
        assert np.array_equal(f32(a).astype(np.float64), a)
    cb = lambda rp, ci, v, dt: (np.asarray(rp, np.int32).tobytes() + np.asarray(ci, np.int32).tobytes() +
                                np.asarray(v, dt).tobytes())
    payload = (struct.pack("<6i", 2, n, A.nnz, P.L.rp[n], P.U.rp[n], 1) +
               cb(A.indptr, A.indices, A.data, np.float32) + cb(P.L.rp, P.L.ci, P.L.v, np.float64) +
               cb(P.U.rp, P.U.ci, P.U.v, np.float64) + f32(P.middle).tobytes() +
               P.perm_row.astype(np.int32).tobytes() + P.perm_col.astype(np.int32).tobytes() +
               P.lscale.tobytes() + P.rscale.tobytes() + f32(x0).tobytes() + f32(b).tobytes())
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(payload)
    p = subprocess.run([_driver(), str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    data = fout.read_bytes()
    assert len(data) == 12 + 4 * n
    rc, max_it, tol = struct.unpack_from("<iif", data, 0)
    x = np.frombuffer(data, np.float32, n, 12)
    k = E.key(case)
    assert rc == fix[k + "/ret"][0] == 0
    assert max_it == fix[k + "/iters"][0]
    assert tol == np.float32(fix[k + "/relres"][0])
    assert np.array_equal(x, fix[k + "/x"].astype(np.float32))


# ------------------------------------------------------------ negative control
def test_negative_control_cgs2(fix):
    """every engine with CGS2 in place of modified Gram-Schmidt: the cases that
    iterate at all (not b = 0, not a start that already passes the test before
    the loop) and have more than one unknown must leave the fixture"""
    counted = differ = 0
    O.set_orth(cgs2=True)
    try:
        for case in E.CASES:
            if E.trivial(case) or E.no_iteration(case):
                continue
            counted += 1
            differ += mismatch(fix, case, E.run(O, case)) != ""
    finally:
        O.set_orth()
    print(f"cgs2: {differ} of {counted} cases differ")
    assert counted >= 24 and 4 * differ >= 3 * counted, (differ, counted)


def test_negative_control_swapped_scales(fix):
    """GMRESilu with lscale and rscale swapped"""
    counted = differ = 0
    for case in (c for c in E.CASES if c.engine == "split" and not E.trivial(c)):
        P = E.split(case.system)
        Q = O.Split(P.L, P.U, P.middle, P.perm_row, P.perm_col, P.rscale, P.lscale)
        b, x0 = E.vectors(case)
        o = O.gmres_split(E.system(case.system), Q, b, x0=x0, m=case.m, max_iter=case.max_iter,
                          tol=E.tolerance(case))
        counted += 1
        differ += mismatch(fix, case, o) != ""
    print(f"swapped scales: {differ} of {counted} cases differ")
    assert counted >= 8 and 4 * differ >= 3 * counted, (differ, counted)
