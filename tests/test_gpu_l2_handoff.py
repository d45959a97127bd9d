"""The 2D wavefront solves' band hand-off through the XCD's own L2.

A band's writer wave publishes its edge values with plain stores when the
consumer band's workgroup runs on the same XCD (each band names its XCD in a
word tagged with the launch's number), and with write-through (sc1) stores in
every other case; bands are dealt to candidate workgroups in contiguous groups
so that neighbours share an XCD (kernels/trsv_wave.hip).  Whatever
the placement, the results are those of the serial rows, bit for bit.

Grids: 24 x 200 -- 4 bands, the last of 8 lines, 6 batches each -- and 17 x 260
-- 5 bands, the last of 4 lines: with contiguous groups the smallest shapes
that hold a local hand-off, a crossing and a ragged last band.
"""
import numpy as np
import pytest

import ggmres
import oracle as O
from ggmres import matrices as M
from helpers import device_layout

GRIDS = {"24x200": (24, 200), "17x260": (17, 260)}
DIVS = {"exact": ggmres.DIV_EXACT, "rcp": ggmres.DIV_RCP, "fma": ggmres.DIV_FMA}
MODE = {ggmres.DIV_EXACT: 0, ggmres.DIV_RCP: 1, ggmres.DIV_FMA: 2}


@pytest.fixture(scope="module")
def solver():
    s = ggmres.Solver(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def cases():
    """per grid: A, its ILU(0) factors and a right-hand side -- computed once"""
    out = {}
    for name, (nx, ny) in GRIDS.items():
        A = M.laplacian_5pt(nx, ny)
        L, U = O.ilu0(A)
        out[name] = (A, L, U, np.random.default_rng(11).standard_normal(A.shape[0]))
    return out


def setup(solver, A, div):
    solver.set_division(DIVS[div])
    solver.set_matrix(A)
    solver.set_precond_ilu0()
    assert solver.uses_wavefront
    return MODE[solver.division_active(0)], MODE[solver.division_active(1)]


@pytest.mark.gpu
@pytest.mark.parametrize("div", sorted(DIVS))
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_apply_bitexact_twice(solver, cases, grid, div):
    """two applies in a row: the second runs on granules the first re-armed and on
    XCD words that carry the first launch's tag"""
    A, L, U, y = cases[grid]
    md = setup(solver, A, div)
    O.set_div_mode(*md)
    try:
        zm = O.lusolve(L, U, y)
    finally:
        O.set_div_mode()
    for _ in range(2):
        assert np.array_equal(solver.precond_apply(ggmres.APPLY_MINV, y), zm)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_fused_launch_gmres_bitexact(solver, cases, grid):
    """GMRES(5), three cycles, fused rows (the forward solve with the SpMV in its
    launch where the grid admits it): the order-matched oracle's bits"""
    A, L, U, _ = cases[grid]
    nx, ny = GRIDS[grid]
    b = M.rhs_ones(A)
    md = setup(solver, A, "fma")
    assert md == (2, 2)
    O.set_dot_order(*device_layout(A.shape[0], nx, ny))
    O.set_div_mode(*md)
    try:
        o = O.gmres_left(A, L, U, b, m=5, max_iter=15, tol=1e-300)
    finally:
        O.set_dot_order(None)
        O.set_div_mode()
    g = solver.solve(b, restart=5, max_iter=15, tol=1e-300)
    assert g["ret"] == o["ret"] and g["iters"] == o["iters"] and g["inner"] == o["inner"]
    assert np.array_equal(g["hist"], o["hist"])
    assert np.array_equal(g["x"], o["x"])


def placement(raw):
    """(xcd per band or -1, groups compiled in, batches published locally per band)"""
    nbt = (raw.shape[1] - 8) // 3
    w = raw[:, nbt + 7]
    return (w & 15) - 1, int((w[0] >> 4) & 15), w >> 8


@pytest.mark.gpu
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_mode_is_sound(solver, cases, grid):
    """a hand-off published with plain stores has producer and consumer on one
    XCD; a direction built with fewer band groups than the 4-band grid has bands
    has at least one such hand-off there (else the placement its speed rests
    on did not happen), a direction built without groups has none"""
    A, _, _, y = cases[grid]
    setup(solver, A, "fma")
    solver.precond_apply(ggmres.APPLY_MINV, y)
    for which in (0, 1):
        xcd, ng, nlocal = placement(solver.trace_precond(which))
        nb = len(xcd)
        assert np.all((xcd >= 0) & (xcd < 8)), xcd
        step = 1 if which == 0 else -1          # the consumer of band k: k + 1 (L), k - 1 (U)
        print(f"{'LU'[which]} {grid}: groups {ng}, xcd {xcd.tolist()}, local batches {nlocal.tolist()}")
        for k in range(nb):
            c = k + step
            if 0 <= c < nb:
                if nlocal[k]:
                    assert xcd[k] == xcd[c], (which, k, xcd.tolist(), nlocal.tolist())
            else:
                assert nlocal[k] == 0           # the last band of the chain publishes nothing
        if ng == 0:
            assert not nlocal.any(), (which, nlocal.tolist())
        elif grid == "24x200" and ng < nb:      # (as many groups as bands: every hand-off crosses)
            assert nlocal.any(), (f"{'LU'[which]}: built with {ng} band group(s), yet no hand-off stayed in "
                                  f"one XCD: xcd per band {xcd.tolist()}")


@pytest.mark.parametrize("ng", [1, 2, 4])
@pytest.mark.parametrize("nbands", [1, 2, 3, 16, 17])
def test_band_candidate_map(ggmres_lib, nbands, ng):
    """host side: band -> candidate workgroup is monotone (groups contiguous),
    covers every band, uses candidates below the group count and splits the
    bands as evenly as the counts allow"""
    f = ggmres_lib.gg_wave_band_candidate
    c = [f(nbands, ng, k) for k in range(nbands)]
    assert all(0 <= v < ng for v in c), c
    assert c[0] == 0 and all(0 <= b - a <= 1 or ng > nbands for a, b in zip(c, c[1:])), c
    assert all(a <= b for a, b in zip(c, c[1:])), c
    sizes = [c.count(v) for v in sorted(set(c))]
    assert sum(sizes) == nbands and max(sizes) - min(sizes) <= 1, sizes
    if nbands >= ng:
        assert sorted(set(c)) == list(range(ng)), c
    assert f(nbands, ng, nbands) == -1 and f(nbands, ng, -1) == -1 and f(nbands, 0, 0) == -1
