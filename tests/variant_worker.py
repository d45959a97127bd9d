"""One fresh process per launch form (tests/test_gpu_variants.py).

    python tests/variant_worker.py CASE OUT.npz

The GG_* switches of the variant arrive in this process's environment (most are
read once into a function-local static, so they cannot be flipped inside the
pytest process).  The worker builds the case's system with fixed seeds, runs
it, and saves everything observable to OUT.npz: per solve / scenario the
status, iteration counts, relres, the full history and x; for transients the
ports, iteration totals and taps; and the diagnostics (kernel names, reduction
blocks, layout).  It computes no oracle: the parent compares a variant with the
default child bit for bit and the default child with the order-matched oracle,
for which it rebuilds the same systems through the functions below.

Keys: "<run>_<field>"; "t_gpu" (seconds from the first solver to the last
result, not compared); "*mgs_kernel" keys name the orthogonalization that ran
(checked against what the variant should launch, not compared).
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "tests"), os.path.join(REPO, "gpu-gmres_amd"), REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

# ---- the systems (also imported by the parent for its oracles) ---------------
# A: 2D wavefront grids; A1: grids in the natural layout (GG_NO_WAVEFRONT=1 in
# the case's own environment: the smallest 2D wavefront layout is 4096 slots,
# G = 2, so G = 1 is reachable in the natural layout only)
# Apad: 342 bands of 3-point lines pad to 2.1 M slots (1024 reduction blocks)
A_GRIDS = {"A": [(22, 22), (100, 100), (130, 130)], "A1": [(16, 16), (30, 30), (40, 40)], "Apad": [(3, 21888)]}
W_DIMS = (20, 30, 7)
W_OPT = dict(restart=30, max_iter=120, tol=1e-10)
A_RUNS = {"fix": dict(restart=30, max_iter=70, tol=1e-300), "conv": dict(restart=30, max_iter=3000, tol=1e-10)}
# Epad: the padded 3 x 21888 grid, where the library itself takes the per-step
# kernels with every scenario in each launch (1024 blocks at 8 units per thread
# are not co-resident); Eres: 3 x 5504, 258 reduction blocks -- with
# GG_PERSIST_TEST_LDS=98304 one block per CU fits, the first persistent launch
# aborts its cycle and the batch reruns on the per-step kernels
E_GRIDS = {"E": (40, 30), "Efix": (40, 30), "Epad": (3, 21888), "Eres": (3, 5504)}
E_RUNS = {"E": {"n3": (3, dict(restart=30, max_iter=3000, tol=1e-10)),
                "n9": (9, dict(restart=30, max_iter=3000, tol=1e-10)),
                "cap3": (3, dict(restart=30, max_iter=20, tol=1e-10)),      # max_iter caps the cold scenario
                "n1": (1, dict(restart=30, max_iter=3000, tol=1e-10))},
          "Efix": {"fix3": (3, dict(restart=30, max_iter=70, tol=1e-300))},
          "Epad": {"fix3": (3, dict(restart=10, max_iter=25, tol=1e-300))},
          "Eres": {"fix3": (3, dict(restart=10, max_iter=25, tol=1e-300))}}
F_STEPS, F_H, F_C = 6, 1e-2, 1e-5
F_OPT = dict(restart=32, max_iter=10000, tol=1e-7)
G_RUNS = {"cap": dict(max_iter=13, tol=1e-300), "conv": dict(max_iter=3000, tol=1e-10)}
H_DIMS = (9, 5, 3)
CF_GRID = (600, 128)
CF_OPT = dict(restart=30, max_iter=70, tol=1e-300)


def grid_system(nx, ny):
    from ggmres import matrices as M
    A = M.laplacian_5pt(nx, ny)
    return A, M.rhs_uniform(A.shape[0])


def flow_system(case="B"):
    """B: power-law rows (C3 stand-in, small): ILU(0) factors in the natural order
    on the flow kernel, rows from 0 to far above 32 terms.  Bbpc: a 70 x 70 grid
    kept off the wavefront (GG_NO_WAVEFRONT=1, GG_FLOW_LONG=0 in the case's
    environment): some 4,800 one-row flow tasks in 139 levels"""
    from ggmres import matrices as M
    A = M.power_law(3000, 33000, seed=7) if case == "B" else M.laplacian_5pt(70, 70)
    n = A.shape[0]
    return A, M.rhs_uniform(n), np.random.default_rng(2).standard_normal(n)


def fused_split_system():
    """test_fused_spmv_same_bits' smaller split: grid-shaped factors (identity
    permutations), large enough for A' to have its sliced copy, so that under
    GG_DIV_FMA A' z runs inside the forward solve's launch (k_trsv_wave2d_spmv)"""
    from ggmres import matrices as M
    from helpers import make_split
    A = M.laplacian_5pt(*CF_GRID)
    n = A.shape[0]
    return A, make_split(A, seed=9, identity_perm=True), M.rhs_uniform(n), np.random.default_rng(6).standard_normal(n)


def split_system():
    """test_gmres_split_parity's: randomly permuted split factors (flow kernel)"""
    from ggmres import matrices as M
    from helpers import make_split
    A = M.laplacian_5pt(40)
    n = A.shape[0]
    return (A, make_split(A, seed=9), M.rhs_uniform(n), np.random.default_rng(3).random(n) * 0.1,
            np.random.default_rng(6).standard_normal(n))


def border_system(tmpdir):
    """test_gpu_border.py's smallest: the 60 x 60 netlist, pads every 20"""
    from helpers import make_split, netlist_system
    A, prow, pcol, nt = netlist_system(os.path.join(tmpdir, "pg60.sp"), 60, 20)
    n = A.shape[0]
    return (A, make_split(A, seed=3, perm=(prow, pcol)), nt, np.random.default_rng(1).random(n),
            np.random.default_rng(6).standard_normal(n))


def batch_system(case="E"):
    """9 right-hand sides on the case's grid (40 x 30): b = A 1 cold; zero (converged at
    the start); b = A 1 from a start 1e-7 off the solution (ends cycles before
    the cold ones); then random / scaled / warm ones"""
    from ggmres import matrices as M
    A = M.laplacian_5pt(*E_GRIDS[case])
    n = A.shape[0]
    rng = np.random.default_rng(3)
    ones = M.rhs_ones(A)
    B = np.array([ones, np.zeros(n), ones, rng.standard_normal(n), 1e3 * rng.uniform(-1, 1, n), M.rhs_uniform(n),
                  rng.standard_normal(n), ones, 1e-3 * rng.standard_normal(n)])
    X0 = np.zeros((9, n))
    X0[2] = 1.0 + 1e-7 * rng.standard_normal(n)
    X0[6] = 1e-2 * rng.standard_normal(n)
    X0[7] = 1.0 + 1e-4 * rng.standard_normal(n)
    return A, B, X0


def transient_system():
    """24 x 24, A = G + C/h; scenario 0: DC / PULSE / PWL sources as
    test_transient_mixed_sources (two on one node); C/h small, so steps 2 and 3
    (DC alone) need fewer and fewer iterations, then the PULSE and PWL edges
    after 3 h, 500 x the DC level: step 4 needs far more than step 3's count + 2;
    scenario 1: PULSE sources from t = 0; scenario 2: two DC sources, warm start"""
    import oracle as O
    from ggmres import matrices as M
    h = F_H
    A = M.transient(M.laplacian_5pt(24, 24), c=F_C, h=h)
    n = A.shape[0]
    cdiag = np.full(n, F_C / h)
    rng = np.random.default_rng(21)
    nodes = np.sort(rng.choice(n, size=12, replace=False)).astype(np.int32)
    nodes[5] = nodes[4]
    srcs = []
    for k in range(len(nodes)):
        if k % 3 == 0:
            srcs.append((O.SRC_DC, [1e-3 * (1 + k)]))
        elif k % 3 == 1:
            srcs.append((O.SRC_PULSE, [0.0, 0.5, 3 * h, 1 * h, 1 * h, 2 * h, 20 * h]))
        else:
            srcs.append((O.SRC_PWL, [0.0, 0.0, 3 * h, 0.0, 4.5 * h, 1e-3, 12 * h, -5e-4]))
    n1, p1 = M.pulse_sources(n, frac=0.01, h=h, seed=101)
    sc = [(nodes, srcs), (n1, [(O.SRC_PULSE, q) for q in p1]),
          (np.array([7, n - 9], np.int32), [(O.SRC_DC, [2e-3]), (O.SRC_DC, [-1e-3])])]
    ports = np.array([nodes[0], nodes[1], nodes[2], n - 1], np.int32)
    taps = np.concatenate([nodes[:6], [0, n // 2, n - 1]]).astype(np.int32)
    X0 = np.zeros((3, n))
    X0[2] = 1e-4
    return A, cdiag, sc, ports, taps, X0


def cg_system():
    """24 x 24 SPD: zero (converged at the start), b = A 1, random"""
    from ggmres import matrices as M
    A = M.laplacian_5pt(24, 24)
    n = A.shape[0]
    B = np.array([np.zeros(n), A @ np.ones(n), np.random.default_rng(6).standard_normal(n)])
    return A, B


def cg_breakdown_system():
    """test_cg_batch_breakdown_stays_in_its_scenario's: a negative definite A"""
    import scipy.sparse as sp
    from ggmres import matrices as M
    A = -sp.csr_matrix(M.laplacian_5pt(16, 17))
    A.sort_indices()
    A = A.tocsr()
    n = A.shape[0]
    return A, np.array([A @ np.ones(n), np.zeros(n), np.random.default_rng(6).standard_normal(n)])


def cg_transient_system():
    from ggmres import matrices as M
    h = F_H
    A = M.transient(M.laplacian_5pt(24, 24), c=F_C, h=h)
    n = A.shape[0]
    cdiag = np.full(n, F_C / h)
    sc = []
    for q in range(3):
        nodes, p = M.pulse_sources(n, frac=0.01, h=h, seed=200 + q)
        p = p.copy()
        p[:, 2] = q * 2 * h                      # the edges start at steps 0, 2, 4
        p[:, 3] = h
        sc.append((nodes, p))
    ports = np.array([0, n // 3, n - 1], np.int32)
    return A, cdiag, sc, ports


def grid3d_system():
    """test_wave3d_apply_and_gmres' first grid"""
    from ggmres import matrices as M
    A = M.grid_7pt(*W_DIMS, upwind=0.1)
    n = A.shape[0]
    return A, M.rhs_uniform(n), np.random.default_rng(8).standard_normal(n)


def tile_system():
    from ggmres import matrices as M
    A = M.grid_7pt(*H_DIMS, upwind=0.2)
    n = A.shape[0]
    rng = np.random.default_rng(11)
    return A, [rng.standard_normal(n) * s for s in (1.0, 1e-250, 1e250)]


# ---- what a run leaves ---------------------------------------------------------
def put_solve(out, p, g):
    out.update({f"{p}_status": g["ret"], f"{p}_iters": g["iters"], f"{p}_inner": g["inner"],
                f"{p}_restarts": g["restarts"], f"{p}_relres": g["relres"], f"{p}_hist": g["hist"], f"{p}_x": g["x"]})


def put_batch(out, p, g, s, gmres=True):
    out.update({f"{p}_ret": g["ret"], f"{p}_status": g["status"], f"{p}_iters": g["iters"], f"{p}_inner": g["inner"],
                f"{p}_restarts": g["restarts"], f"{p}_relres": g["relres"], f"{p}_x": g["x"]})
    for q, hq in enumerate(g["hist"]):
        out[f"{p}_hist{q}"] = hq
    if gmres:
        out[f"{p}_batch_mgs_kernel"] = s.batch_mgs_kernel()


def put_diag(out, p, s, solved=True):
    lay, G = s.layout()
    out.update({f"{p}_trsv_kernel0": s.trsv_kernel(0), f"{p}_trsv_kernel1": s.trsv_kernel(1), f"{p}_G": G,
                f"{p}_batch_engine": s.batch_engine, f"{p}_uses_wavefront": s.uses_wavefront, f"{p}_Ppad": len(lay),
                f"{p}_spmv_sliced": s.spmv_sliced,
                f"{p}_lay2nat": lay})
    if solved:
        out[f"{p}_mgs_kernel"] = s.mgs_kernel()


def split_solver(A, P):
    import ggmres
    s = ggmres.Solver(0)
    s.set_matrix(A)
    s.set_precond_split(P.L, P.U, P.middle, P.perm_row, P.perm_col, P.lscale, P.rscale)
    return s


def put_split(out, s, v, b, x0, opt):
    import ggmres
    for name, op in (("left", ggmres.APPLY_LEFT), ("right", ggmres.APPLY_RIGHT), ("start", ggmres.APPLY_START)):
        out[f"apply_{name}"] = s.precond_apply(op, v)
    put_solve(out, "solve", s.solve(b, x0=x0, **opt))
    put_diag(out, "d", s)


def run(case, out, tmpdir):
    import ggmres
    if case in A_GRIDS:
        for nx, ny in A_GRIDS[case]:
            A, b = grid_system(nx, ny)
            s = ggmres.Solver(0)
            s.set_matrix(A)
            s.set_precond_ilu0()
            for r, opt in A_RUNS.items():
                put_solve(out, f"g{nx}x{ny}_{r}", s.solve(b, **opt))
            put_diag(out, f"g{nx}x{ny}", s)
            s.close()
    elif case in ("B", "Bbpc"):
        A, b, v = flow_system(case)
        s = ggmres.Solver(0)
        s.set_matrix(A)
        s.set_precond_ilu0()
        for k, scale in enumerate((1.0, 1e200)):
            out[f"apply{k}"] = s.precond_apply(ggmres.APPLY_MINV, v * scale)
        put_solve(out, "solve", s.solve(b, restart=30, max_iter=2000, tol=1e-10))
        put_diag(out, "d", s)
        s.close()
    elif case == "C":
        A, P, b, x0, v = split_system()
        s = split_solver(A, P)
        put_split(out, s, v, b, x0, dict(restart=32, max_iter=2000, tol=1e-11))
        s.close()
    elif case == "Cf":
        A, P, b, v = fused_split_system()
        s = split_solver(A, P)
        s.set_division(ggmres.DIV_FMA)
        out.update(division0=s.division_active(0), division1=s.division_active(1))
        put_split(out, s, v, b, None, CF_OPT)
        s.close()
    elif case == "D":
        A, P, nt, b, v = border_system(tmpdir)
        s = split_solver(A, P)
        put_split(out, s, v, b, None, dict(restart=32, max_iter=600, tol=1e-10))
        out["d_trsv_levels0"] = s.trsv_levels(0)
        s.close()
    elif case in E_RUNS:
        A, B, X0 = batch_system(case)
        s = ggmres.Solver(0)
        s.set_matrix(A)
        s.set_precond_ilu0()
        for r, (S, opt) in E_RUNS[case].items():
            put_batch(out, r, s.solve_batch(B[:S], X0[:S], **opt), s)
            for q in range(S if case != "Eres" else 0):       # every scenario alone (gg_solve)
                put_solve(out, f"{r}_single{q}", s.solve(B[q], x0=X0[q], **opt))
        put_diag(out, "d", s)
        s.close()
    elif case == "F":
        A, cdiag, sc, ports, taps, X0 = transient_system()
        s = ggmres.Solver(0)
        s.set_matrix(A)
        s.set_precond_ilu0()
        s.set_taps(taps)
        g = s.transient_src(F_STEPS, F_H, cdiag, sc[0][0], sc[0][1], ports, X0[0], **F_OPT)
        out.update(src_x=g["x"], src_ports=g["ports"], src_iters_total=g["iters_total"], src_ret=g["ret"])
        for k, t in enumerate(s.get_taps()):
            out[f"src_taps{k}"] = t
        s.set_taps([])
        g = s.transient_batch(F_STEPS, F_H, cdiag, sc, ports, X0, **F_OPT)
        out.update(tb_x=g["x"], tb_ports=g["ports"], tb_iters_total=g["iters_total"], tb_ret=g["ret"],
                   tb_batch_mgs_kernel=s.batch_mgs_kernel())
        put_diag(out, "d", s)
        s.close()
    elif case == "G":
        A, B = cg_system()
        X0 = np.zeros_like(B)
        for kind in ("diag", "ilu0"):
            s = ggmres.Solver(0)
            s.set_matrix(A)
            getattr(s, "set_precond_" + kind)()
            for r, opt in G_RUNS.items():
                put_batch(out, f"{kind}_{r}", s.solve_cg_batch(B, X0, **opt), s, gmres=False)
            put_diag(out, f"{kind}", s)
            s.close()
        A, B = cg_breakdown_system()
        s = ggmres.Solver(0)
        s.set_matrix(A)
        s.set_precond_ilu0()
        put_batch(out, "brk", s.solve_cg_batch(B, np.zeros_like(B), max_iter=3000, tol=1e-10), s, gmres=False)
        put_diag(out, "brk", s)
        s.close()
        A, cdiag, sc, ports = cg_transient_system()
        n = A.shape[0]
        for kind in ("diag", "ilu0"):
            s = ggmres.Solver(0)
            s.set_matrix(A)
            getattr(s, "set_precond_" + kind)()
            g = s.transient_cg_batch(F_STEPS, F_H, cdiag, sc, ports, np.zeros((3, n)), restart=30, max_iter=3000,
                                     tol=1e-10)
            out.update({f"tcg_{kind}_x": g["x"], f"tcg_{kind}_ports": g["ports"],
                        f"tcg_{kind}_iters_total": g["iters_total"], f"tcg_{kind}_ret": g["ret"]})
            s.close()
    elif case == "W":
        A, b, v = grid3d_system()
        s = ggmres.Solver(0)
        s.set_matrix(A)
        s.set_precond_ilu0()
        for k, scale in enumerate((1.0, 1e-250, 1e250)):
            out[f"apply{k}"] = s.precond_apply(ggmres.APPLY_MINV, v * scale)
        put_solve(out, "solve", s.solve(b, **W_OPT))
        put_diag(out, "d", s)
        s.close()
    elif case == "H":
        A, vs = tile_system()
        s = ggmres.Solver(0)
        s.set_division(ggmres.DIV_FMA)
        s.set_matrix(A)
        s.set_precond_ilu0()
        out.update(division0=s.division_active(0), division1=s.division_active(1))
        for k, v in enumerate(vs):
            out[f"apply{k}"] = s.precond_apply(ggmres.APPLY_MINV, v)
        put_diag(out, "d", s, solved=False)
        s.close()
    else:
        raise SystemExit(f"unknown case {case}")


def main():
    case, path = sys.argv[1], sys.argv[2]
    out = {}
    t0 = time.perf_counter()
    run(case, out, os.path.dirname(os.path.abspath(path)))
    out["t_gpu"] = time.perf_counter() - t0
    np.savez(path, **{k: np.asarray(v) for k, v in out.items()})
    print(f"variant_worker {case}: ok, {out['t_gpu']:.2f} s", flush=True)


if __name__ == "__main__":
    main()
