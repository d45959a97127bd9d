"""NumPy restatement of the sharded transient loop (gg_dd_transient_src,
csrc/dd.hip "Sharded transient") -- test code.

Per step it = 1..nsteps, as solver.hip's transient_loop: u = the sources at time
index it (oracle.source_value), w = B u + (C/h) x in the reference's order
(oracle.transient_rhs, natural order), then the sharded solve of B = P A P^T
with w[q] from the warm start x[q]:
  GG_SOLVE_CG          dd_cg_ref.solve (the dots in the sharded order);
  0 / GG_SOLVE_CGS2    oracle.gmres_left under oracle.set_dot_order_shards
                       (segments, G), with oracle.set_orth(True) for CGS2.
The status is GG_OK or that of the last step that was not; a step that exhausts
max_iter or breaks down does not stop the loop (x keeps its last iterate).

The systems, sources and ports of tests/test_dd_transient_ref.py (CPU, natural
block layout) and tests/test_gpu_dd_transient*.py (the device's own layout).
"""
import numpy as np

import dd_cg_ref as D
import oracle as O

K_CHUNK = D.K_CHUNK
SOLVE_CGS2, SOLVE_CG = 0x2, 0x4          # ggmres.h gg_options.flags
C_CAP, H_STEP = 1e-3, 1e-2               # A = G + (c / h) I

# name: (matrices function of G, its arguments, parts, partition, steps)
SYSTEMS = {
    "small": ("laplacian_5pt", (40, 30), 2, "blocks", 10),
    "mixed": ("laplacian_5pt", (96, 80), 4, "blocks_color", 6),
    "7pt_16_bisect": ("grid_7pt", (16,), 4, "bisect", 6),
}


def system(name):
    """(A = G + C/h, cdiag, parts, partition method, steps) of a SYSTEMS entry"""
    from ggmres import matrices as M
    fn, args, P, meth, nsteps = SYSTEMS[name]
    A = M.transient(getattr(M, fn)(*args), c=C_CAP, h=H_STEP)
    return A, np.full(A.shape[0], C_CAP / H_STEP), P, D._method(meth), nsteps


def mixed_sources(n, h=H_STEP):
    """(src_node, sources): pulse_sources(n, 0.02)'s nodes, the kinds cycling by k % 3 --
    its PULSE row, DC {5e-4}, PWL {0,0, 3h,1e-3, 6h,2e-4}"""
    from ggmres import matrices as M
    nodes, pulses = M.pulse_sources(n, frac=0.02, h=h)
    sources = []
    for k in range(len(nodes)):
        if k % 3 == 0:
            sources.append((O.SRC_PULSE, pulses[k].copy()))
        elif k % 3 == 1:
            sources.append((O.SRC_DC, np.array([5e-4])))
        else:
            sources.append((O.SRC_PWL, np.array([0.0, 0.0, 3 * h, 1e-3, 6 * h, 2e-4])))
    return nodes, sources


def default_ports(n):
    return np.array([0, n // 3, n // 2 + 1, n - 1], np.int32)


def step_solve(B, L, U, segs, G, w, x, flags, restart, max_iter, tol):
    """one step's sharded solve in B's order: (ret, x, iters)"""
    if flags & SOLVE_CG:
        ret, xs, iters, relres, hist = D.solve(B, L, U, w, segs, G, x, max_iter, tol)
        return ret, xs, iters
    O.set_dot_order_shards(list(segs), G)
    O.set_orth(bool(flags & SOLVE_CGS2))
    try:
        o = O.gmres_left(B, L, U, w, x0=x, m=restart, max_iter=max_iter, tol=tol)
    finally:
        O.set_dot_order(None)
        O.set_orth()
    return o["ret"], o["x"], o["iters"]


def transient(B, L, U, q, segs, G, nsteps, h, cdiag, src_node, sources, ports, x0, flags=0, restart=32,
              max_iter=10000, tol=1e-7):
    """dict(ret, x, ports [nport, nsteps+1], iters_total, steps [(ret, iters)]); x0, x,
    cdiag, src_node and ports in natural order, B = P A P^T with q its row order"""
    x = np.array(x0, np.float64, copy=True)
    ports = np.asarray(ports, np.int64)
    pv = np.zeros((len(ports), nsteps + 1))
    pv[:, 0] = x[ports]
    status, steps = 0, []
    for it in range(1, nsteps + 1):
        u = np.array([O.source_value(k, p, it, h) for k, p in sources], np.float64)
        w = O.transient_rhs(cdiag, src_node, u, x)
        ret, xs, iters = step_solve(B, L, U, segs, G, w[q], x[q], flags, restart, max_iter, tol)
        x = np.empty_like(x)
        x[q] = xs
        if ret != 0:
            status = ret
        steps.append((int(ret), int(iters)))
        pv[:, it] = x[ports]
    return dict(ret=status, x=x, ports=pv, iters_total=sum(i for _, i in steps), steps=steps)
