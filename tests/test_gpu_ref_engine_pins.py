"""The device's GMRES solves against what the reference's OWN host engines
computed (tests/golden/ref_engine_pins.npz: GMRES_leftILU0, the GMRES without a
preconditioner, GMRESilu over MyILUPP::HostPrecond_*, built from the reference
checkout in double).  Reads only the fixture, never oracle/_ref.

Two links on the same bits in one test:
  * device against the reference: ret and iters equal; x within 1e-10 relative
    (the project's bar for the device against the serial summation order);
    relres within 10 x relres_order_dev relative -- the fixture's largest
    deviation of the CPU oracle in the DEVICE's summation order from the
    reference, measured without a device;
  * device against the order-matched oracle: bit for bit, as test_gpu_parity.
The one-launch orthogonalization by default; the cases named *_per_step and
*_wide run the per-step kernels (GG_NO_PERSIST=1) and k_arnoldi_wide
(GG_WIDE_FORCE=1) on a solver of their own."""
import numpy as np
import pytest

import ggmres
from golden import ref_engine_cases as E
from golden import ref_pin_cases as C
from helpers import hist_close, rel_err

pytestmark = pytest.mark.gpu
GPU_KEYS = [E.key(c) for c in E.CASES if c.gpu]
X_RTOL = 1e-10
RELRES_FACTOR = 10.0


@pytest.fixture(scope="module")
def fix():
    return E.fixture()[1]


@pytest.fixture(scope="module")
def solver():
    s = ggmres.Solver(0)
    yield s
    s.close()


def test_gpu_cases_cover_every_form():
    cases = [c for c in E.CASES if c.gpu]
    assert {c.env[0] for c in cases if c.env} == {"GG_NO_PERSIST", "GG_WIDE_FORCE"}
    assert {(c.engine, c.system) for c in cases} >= {
        ("left", "5pt_40x40"), ("left", "perm_40x33"), ("left", "7pt_17x9x8"), ("left", "sherman1"),
        ("plain", "5pt_37x23"), ("plain", "rand300"), ("split", "5pt_40x40"), ("split", "5pt_37x23")}
    for e in E.ENGINES:
        assert {c.name.split("/")[-1] for c in cases if c.engine == e} >= {"zero_rhs", "exact_start", "cycle_end",
                                                                           "exhausted"}


def setup(s, case):
    A = E.system(case.system)
    s.set_matrix(A)
    if case.engine == "left":
        s.set_precond_ilu0()
    elif case.engine == "plain":
        s.set_precond_none()
    else:
        P = E.split(case.system)
        s.set_precond_split(P.L, P.U, P.middle, P.perm_row, P.perm_col, P.lscale, P.rscale)
    if case.engine == "plain":
        assert not s.uses_wavefront and s.trsv_kernel(0) == "" and s.trsv_kernel(1) == ""
    else:
        wave, family = E.KERNEL[(case.engine, case.system)]
        assert s.uses_wavefront == wave
        if family:
            assert family in s.trsv_kernel(0) and family in s.trsv_kernel(1), (s.trsv_kernel(0), s.trsv_kernel(1))


@pytest.mark.parametrize("name,scale", E.split_map_keys())
def test_device_split_maps(solver, fix, name, scale):
    """gg_precond_apply's four split maps against MyILUPP::HostPrecond_* on
    their own, bit for bit: the dataflow kernel (random permutations) and the
    2D wavefront (identity permutations), 1e250 / 1e-250 through the range
    guard of the fast division"""
    P, v = E.split(name), E.split_map_vector(name, scale)
    solver.set_matrix(E.system(name))
    solver.set_precond_split(P.L, P.U, P.middle, P.perm_row, P.perm_col, P.lscale, P.rscale)
    assert solver.uses_wavefront == E.KERNEL[("split", name)][0]
    ops = {"left": ggmres.APPLY_LEFT, "right": ggmres.APPLY_RIGHT, "start": ggmres.APPLY_START,
           "rhs": ggmres.APPLY_RHS}
    for _ in range(2):                  # the second apply runs after any fallback demotion
        for which in E.SPLIT_MAPS:
            out = solver.precond_apply(ops[which], v)
            assert C.same(fix, f"splitmap/{name}/{scale}/{which}", out) == "", which


@pytest.mark.parametrize("k", GPU_KEYS)
def test_device_engine(solver, fix, k, monkeypatch):
    case = E.by_key()[k]
    s = solver
    if case.env:                        # read when the space and the workspace are built
        monkeypatch.setenv(*case.env)
        s = ggmres.Solver(0)
    try:
        setup(s, case)
        n = E.system(case.system).shape[0]
        b, x0 = E.vectors(case)
        tol = E.tolerance(case)
        assert np.array([tol]).tobytes() == fix[k + "/tol"].tobytes()
        lay, G = s.layout()
        play, pG = E.layout(case)       # the order relres_order_dev was measured in
        assert G == pG and np.array_equal(lay, play)
        g = s.solve(b, x0=x0, restart=case.m, max_iter=case.max_iter, tol=tol)
        if n >= 512:
            want = {None: "k_arnoldi_persist", "GG_NO_PERSIST": "", "GG_WIDE_FORCE": "k_arnoldi_wide"}
            name = want[case.env[0] if case.env else None]
            if g["inner"] > 0:
                assert s.mgs_kernel().startswith(name) and (name or s.mgs_kernel() == ""), s.mgs_kernel()

        # ---- against the reference
        ret, iters = int(fix[k + "/ret"][0]), int(fix[k + "/iters"][0])
        relres, x = float(fix[k + "/relres"][0]), fix[k + "/x"]
        margin = RELRES_FACTOR * float(fix["relres_order_dev"][0])
        dev = abs(g["relres"] - relres) / relres if relres else abs(g["relres"])
        print(f"{k}: ret {g['ret']} iters {g['iters']} relres {g['relres']:.17e} reference {relres:.17e} "
              f"relative deviation {dev:.3e} (margin {margin:.3e}) x rel_err {rel_err(g['x'], x):.3e}")
        assert (g["ret"], g["iters"]) == (ret, iters)
        assert rel_err(g["x"], x) <= X_RTOL
        assert dev <= margin

        # ---- against the order-matched oracle
        ot = E.run_order_matched(case, (lay, G))
        assert (g["ret"], g["iters"], g["inner"]) == (ot["ret"], ot["iters"], ot["inner"])
        ok, msg = hist_close(g["hist"], ot["hist"], 0.0)
        assert ok, msg
        assert g["relres"] == ot["relres"]
        assert np.array_equal(g["x"], ot["x"]), rel_err(g["x"], ot["x"])
    finally:
        if s is not solver:
            s.close()
