"""The HIP kernels against what the reference's OWN host routines computed
(tests/golden/ref_pins.npz; see golden/make_ref_pins.py and test_ref_pins.py):
computeSpMV for the SpMV kernels, LUSolve_ignoreZero for the triangular-solve
kernels, lofC + ilukC for the device ILU(k).  Only the committed fixture and the
seeded generators are read.  Every bar is bit equality (a sha256 for the large
arrays), except GG_DIV_FMA, a tolerance mode by design, which keeps
test_gpu_fastdiv.test_fma_apply's 1e-12 with the reference's output in the
oracle's place."""
import numpy as np
import pytest

import ggmres
import oracle as O
from golden import ref_pin_cases as C
from helpers import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    s = ggmres.Solver(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def fsolver():
    s = ggmres.Solver(0)
    s.set_division(ggmres.DIV_FMA)
    yield s
    s.close()


@pytest.fixture(scope="module")
def fix():
    return C.fixture()[1]


# ------------------------------------------------------------------ SpMV
# the matrices test_gpu_parity.test_spmv_bitexact also factors, and which of
# them the ILU(0) setup moves into the wavefront layout
ILU0_LAYOUT = {"3pt_100": False, "5pt_10x10": False, "7pt_10x10x10": True, "9pt_10x10": False,
               "sherman1": True, "5pt_37x64": True, "powerlaw_3000": False}


@pytest.mark.parametrize("name", sorted(C.SPMV))
def test_spmv(solver, fix, name):
    A = C.SPMV[name]()
    xs = {kind: C.spmv_x(name, kind, A.shape[0]) for kind in C.SPMV_X}
    solver.set_matrix(A)
    solver.set_precond_none()
    for kind, x in xs.items():
        assert C.same(fix, f"spmv/{name}/{kind}", solver.spmv(x)) == ""
    if name in ILU0_LAYOUT:
        solver.set_precond_ilu0()
        assert solver.uses_wavefront == ILU0_LAYOUT[name]
        for kind, x in xs.items():
            assert C.same(fix, f"spmv/{name}/{kind}", solver.spmv(x)) == ""


@pytest.mark.parametrize("layout", ["rtile", "rtile7", "panel_major"])
@pytest.mark.parametrize("name", C.SPMV_PANEL_CASES)
def test_spmv_panels(solver, fix, name, layout, monkeypatch):
    """the column-panel launches of test_gpu_parity.test_spmv_panels_bitexact"""
    A = C.SPMV[name]()
    monkeypatch.setenv("GG_SPMV_PANEL_MIN", "1000")
    monkeypatch.setenv("GG_SPMV_PANEL", str(A.shape[0] // 4 + 1))
    monkeypatch.setenv("GG_SPMV_RTILE", {"rtile": "1024", "rtile7": "7", "panel_major": "0"}[layout])
    solver.set_matrix(A)
    solver.set_precond_none()
    assert solver.spmv_panels >= 2
    assert (solver.spmv_rtile > 0) == (layout != "panel_major")
    for kind in C.SPMV_X:
        assert C.same(fix, f"spmv/{name}/{kind}", solver.spmv(C.spmv_x(name, kind, A.shape[0]))) == ""


# ------------------------------------------------------- triangular solves
GRID2D = ("5pt_37x64", "5pt_5x200", "5pt_100x100")
GRID3D = ("7pt_9x5x3", "7pt_17x9x8", "7pt_2x40x40", "7pt_20x30x7", "thermal_7pt_12", "7pt_10x10x10")
FLOW = ("powerlaw_3000",)


def expected_kernel(name, k):
    """what gg_trsv_kernel must name for the U solve of ILUK case (name, k) in
    the default setup, or None where the case pins no kernel"""
    if name in GRID2D:
        return f"k_trsv_wave2d<false, *, false, false, {k + 1}, "      # 2D band; skew k + 1
    if name in GRID3D and k == 0:
        return "k_trsv_tile3d<false, "
    if name in FLOW:
        return "k_trsv_flow"
    return None


def kernel_matches(got, want):
    head, _, tail = want.partition("*")
    return got.startswith(head) and (not tail or tail in got[len(head):])


def check_applies(s, fix, key, n):
    for kind in C.RHS:
        z = s.precond_apply(ggmres.APPLY_MINV, C.rhs(kind, n))
        msg = C.same(fix, f"{key}/{kind}", z)
        assert msg == "", msg


FORCED = {"flow": {"GG_NO_WAVEFRONT": "1"}, "csr": {"GG_NO_WAVEFRONT": "1", "GG_FLOW_ELL": "0"},
          "per_level": {"GG_NO_WAVEFRONT": "1", "GG_TRSV_LEVELS": "1"}}


@pytest.mark.parametrize("path", ["default"] + sorted(FORCED))
@pytest.mark.parametrize("name,k", C.iluk_keys())
def test_lusolve_exact(solver, fix, name, k, path, monkeypatch):
    """GG_DIV_EXACT: the reference's factors through the user-factor entry; the
    2D band and skewed wavefronts, the 3D tile kernel and the dataflow kernel
    where the case takes them, and the forced dataflow (sliced and CSR term
    copies) and per-level kernels: LUSolve_ignoreZero's bits, scaled
    right-hand sides included"""
    for var, val in FORCED.get(path, {}).items():
        monkeypatch.setenv(var, val)
    A, L, U = C.pinned_factors(name, k)
    solver.set_matrix(A)
    solver.set_precond_lu(L, U)
    assert solver.division_active(0) == solver.division_active(1) == ggmres.DIV_EXACT
    if path == "default":
        want = expected_kernel(name, k)
        if want is not None:
            assert solver.uses_wavefront == (want != "k_trsv_flow")
            assert kernel_matches(solver.trsv_kernel(1), want), (solver.trsv_kernel(1), want)
    else:
        assert not solver.uses_wavefront
        assert solver.trsv_kernel(1) == ("k_trsv_level" if path == "per_level" else "k_trsv_flow")
    check_applies(solver, fix, f"lusolve/{name}/k{k}", L.n)


def test_lusolve_wave3d_planes(solver, fix, monkeypatch):
    """the (plane, band) pipeline on the 3D shape test_wave3d_apply_and_gmres singles out"""
    monkeypatch.setenv("GG_WAVE3D_PLANES", "1")
    A, L, U = C.pinned_factors("7pt_20x30x7", 0)
    solver.set_matrix(A)
    solver.set_precond_lu(L, U)
    assert solver.uses_wavefront
    assert kernel_matches(solver.trsv_kernel(1), "k_trsv_wave2d<false, *, false, true, 1, ")
    check_applies(solver, fix, "lusolve/7pt_20x30x7/k0", L.n)


@pytest.mark.parametrize("path", ["default"] + sorted(FORCED))
def test_lusolve_skipped_pivots(solver, fix, path, monkeypatch):
    """40 U diagonals below 1e-9: the reference leaves those rows undivided"""
    for var, val in FORCED.get(path, {}).items():
        monkeypatch.setenv(var, val)
    A, L, U = C.pinned_factors(*C.SKIP_PIVOT)
    U2, _ = C.skip_pivot(U)
    solver.set_matrix(A)
    solver.set_precond_lu(L, U2)
    assert solver.uses_wavefront == (path == "default")
    check_applies(solver, fix, "lusolve/skip_pivot", L.n)


FMA_CASES = [(n, k) for n in GRID2D for k in (0, 1, 2)] + [(n, 0) for n in GRID3D]
SCALE = {"random": 1.0, "ones": 1.0, "big": 1e250, "small": 1e-250}


@pytest.mark.parametrize("name,k", FMA_CASES)
def test_lusolve_fma(fsolver, fix, name, k):
    """GG_DIV_FMA (fused rows, U pre-scaled by the reciprocal): within 1e-12 of
    the reference's solve, test_fma_apply's bar.  The reference's output is
    what the serial oracle returns once the fixture confirms its bits."""
    A, L, U = C.pinned_factors(name, k)
    fsolver.set_matrix(A)
    fsolver.set_precond_lu(L, U)
    assert fsolver.uses_wavefront
    assert fsolver.division_active(1) == ggmres.DIV_FMA
    for kind in C.RHS:
        y = C.rhs(kind, L.n)
        ref = O.lusolve(L, U, y)
        assert C.same(fix, f"lusolve/{name}/k{k}/{kind}", ref) == ""
        z = fsolver.precond_apply(ggmres.APPLY_MINV, y)
        err = rel_err(z / SCALE[kind], ref / SCALE[kind])
        print(f"{name} k={k} {kind}: {err:.3e}")
        assert err <= 1e-12


# ------------------------------------------------------- device factorization
def device_factors(s, k):
    (lrp, lci, lv), (urp, uci, uv), ms = s.iluk_device_factors(k)
    assert ms > 0
    n = len(lrp) - 1
    return O.CSR(n, lrp, lci, lv), O.CSR(n, urp, uci, uv)


@pytest.mark.parametrize("name,k", C.iluk_keys())
def test_iluk_device(solver, fix, name, k):
    """the device ILU(k) (levels 1 and 2: k_iluk_wave's LDS path; level 0 too):
    lofC's pattern, ilukC's L, D and U"""
    solver.set_matrix(C.ILUK[name][0]())
    L, U = device_factors(solver, k)
    msg = C.iluk_mismatch(fix, name, k, L, U)
    assert msg == "", msg


@pytest.mark.parametrize("name,k", sorted(C.ILUK_LONG))
def test_iluk_device_long_rows(solver, fix, name, k, monkeypatch):
    """rows above GG_ILUK_LONG entries on the kernel's long-row path (HBM values,
    dense position map): test_iluk_device_factors_bitexact's settings"""
    monkeypatch.setenv("GG_ILUK_LONG", str(C.ILUK_LONG[(name, k)]))
    solver.set_matrix(C.ILUK[name][0]())
    L, U = device_factors(solver, k)
    msg = C.iluk_mismatch(fix, name, k, L, U)
    assert msg == "", msg


@pytest.mark.parametrize("k", [0, 1, 2])
def test_iluk_device_zero_pivot(solver, fix, k):
    """ilukC returns -2; the device path reports it as test_iluk_device_zero_pivot expects"""
    assert fix[f"iluk/zero_pivot/k{k}/status"][0] == -2
    solver.set_matrix(C.ZERO_PIVOT())
    with pytest.raises(ggmres.GGError) as e:
        solver.set_precond_iluk_device(k)
    assert e.value.code == -3                       # GG_EZEROPIVOT
