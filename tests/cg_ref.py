"""Plain NumPy fp64 restatement of the solver's preconditioned conjugate
gradients (GG_SOLVE_CG, csrc/cg.hip; DESIGN.md "CG") -- test code, in the style
of ainv_ref.gmres_left.

pcg(A, minv, b, x0, max_iter, tol, dot): left-preconditioned CG on A x = b with
M = the callable minv, stopping on ||M r|| / ||M b||:

    bb = M b; normb = sqrt(dot(bb, bb)) (0 -> 1);  r = b - A x;  z = M r
    res0 = sqrt(dot(z, z)) / normb;  p = z;  rz = dot(r, z)
    repeat:  q = A p;  pq = dot(p, q);  alpha = rz / pq
             x = alpha p + x;  r = (-alpha) q + r
             z = M r;  rzn = dot(r, z);  zz = dot(z, z);  res = sqrt(zz) / normb
             beta = rzn / rz;  p = beta p + z;  rz = rzn

"<=" on the initial residual, "<" afterwards (the GMRES engine's comparisons);
BREAKDOWN when p.q is not > 0, or r.z is not > 0 while the solve has not
converged (NaN counts as not > 0).  Every product and sum is one rounding (NumPy
does not contract), the SpMV rows are the oracle's serial sums.

layout_dot(lay2nat, G): the solver's dot product in any of its vector spaces
(Solver.layout()): ainv_ref.device_dot generalised from the natural order to
the wavefront layouts -- the operands scattered into their Ppad slots (padding
+0), G blocks of 256 threads, each thread summing its grid-stride 16-byte units
in order, the wave / block tree, then the G partials summed by one more block.
"""
import math

import numpy as np

import oracle as O
from ainv_ref import _wave_tree

BREAKDOWN = -8          # ggmres.h GG_EBREAKDOWN


def layout_dot(lay2nat, G):
    lay2nat = np.asarray(lay2nat, np.int64)
    ppad = lay2nat.size
    assert ppad % 512 == 0
    real = np.flatnonzero(lay2nat >= 0)
    rows = lay2nat[real]
    units = ppad // 2
    nthr = G * 256
    rounds = -(-units // nthr)

    def dot(x, y):
        p = np.zeros(rounds * nthr * 2)
        p[real] = (np.asarray(x) * np.asarray(y))[rows]
        p = p.reshape(rounds, nthr, 2)
        acc = np.zeros(nthr)
        for k in range(rounds):
            acc = acc + p[k, :, 0]
            acc = acc + p[k, :, 1]
        part = _wave_tree(acc.reshape(G, 256))
        v = np.zeros(256)
        for k0 in range(0, G, 256):
            q = part[k0:k0 + 256]
            v[:q.size] = v[:q.size] + q
        return float(_wave_tree(v))
    return dot


def pcg(A, minv, b, x0=None, max_iter=3000, tol=1e-10, dot=None, info=None):
    """(ret, x, iters, relres, hist): ret 0 converged, 1 max_iter exhausted,
    BREAKDOWN; hist = [res0, res after each iteration]; x the last iterate.
    info: a dict that receives the exit taken -- info["why"] one of "conv0",
    "conv", "exhausted", "rz0" (r.z not > 0 at the start), "pq", "rz", and
    info["bad"] the offending scalar (None where nothing broke down)"""
    if dot is None:
        dot = lambda u, v: float(np.dot(u, v))      # noqa: E731

    def out(ret, why, bad=None):
        if info is not None:
            info["why"] = why
            info["bad"] = bad
        return ret, x, it, res, np.array(hist)
    A = O.csr(A)
    b = np.asarray(b, np.float64)
    x = np.zeros(A.n) if x0 is None else np.array(x0, np.float64, copy=True)
    it = 0
    with np.errstate(over="ignore", invalid="ignore"):
        bb = minv(b)
        normb = math.sqrt(dot(bb, bb))
        if normb == 0.0:
            normb = 1.0
        r = O.residual(A, x, b)
        z = minv(r)
        zz = dot(z, z)
        res = math.sqrt(zz) / normb if zz >= 0.0 else float("nan")
        hist = [res]
        rz = dot(r, z)
        if res <= tol:
            return out(0, "conv0")
        if not rz > 0.0:
            return out(BREAKDOWN, "rz0", rz)
        p = z.copy()
        while it < max_iter:
            q = O.spmv(A, p)
            pq = dot(p, q)
            if not pq > 0.0:
                return out(BREAKDOWN, "pq", pq)
            alpha = rz / pq
            x = alpha * p + x
            r = (-alpha) * q + r
            z = minv(r)
            rzn = dot(r, z)
            zz = dot(z, z)
            res = math.sqrt(zz) / normb if zz >= 0.0 else float("nan")
            it += 1
            hist.append(res)
            if res < tol:
                return out(0, "conv")
            if not rzn > 0.0:
                return out(BREAKDOWN, "rz", rzn)
            beta = rzn / rz
            p = beta * p + z
            rz = rzn
    return out(1, "exhausted")
