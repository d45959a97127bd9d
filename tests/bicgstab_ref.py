"""Plain NumPy fp64 restatement of the solver's preconditioned BiCGStab
(GG_SOLVE_BICGSTAB, csrc/bicgstab.hip; DESIGN.md "BiCGStab") -- test code, in
the style of cg_ref.pcg.

bicgstab(A, minv, b, x0, max_iter, tol, dot): left-preconditioned BiCGStab,
i.e. BiCGStab on (M A) x = M b with M = the callable minv, stopping on
||M r|| / ||M b||:

    bb = M b; normb = sqrt(dot(bb, bb)) (0 -> 1)
    r = M (b - A x); res0 = sqrt(dot(r, r)) / normb;  rt = r; rho = dot(rt, r); p = r
    repeat:  v = M (A p);  rtv = dot(rt, v);  alpha = rho / rtv;  s = (-alpha) v + r
             t = M (A s);  ts = dot(t, s);  tt = dot(t, t);  omega = tt > 0 ? ts / tt : 0
             x = omega s + (alpha p + x);  r = (-omega) t + s
             rr = dot(r, r);  rhon = dot(rt, r);  res = sqrt(rr) / normb
             beta = (rhon / rho) (alpha / omega);  p = beta ((-omega) v + p) + r;  rho = rhon

"<=" on the initial residual, "<" afterwards; no exit at the half step.
BREAKDOWN when rho or rt.v is zero or not finite (nothing has moved in that
iteration), or when omega or the next rho is while the solve has not converged.
Every product and sum is one rounding (NumPy does not contract), the SpMV rows
are the oracle's serial sums; `dot` is cg_ref.layout_dot for the solver's order.
"""
import math

import numpy as np

import oracle as O
from cg_ref import BREAKDOWN, layout_dot      # noqa: F401  (re-exported)


def _bad(v):
    return not math.isfinite(v) or v == 0.0


def bicgstab(A, minv, b, x0=None, max_iter=3000, tol=1e-10, dot=None, info=None):
    """(ret, x, iters, relres, hist): ret 0 converged, 1 max_iter exhausted,
    BREAKDOWN; hist = [res0, res after each iteration]; x the last iterate.
    info: a dict that receives the exit taken -- info["why"] one of "conv0",
    "conv", "exhausted", "rho0" (rho at the start), "rtv", "omega", "rho"
    (omega named first when both are bad, as k_bi_p does), and info["bad"] the
    offending scalar (None where nothing broke down)"""
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
        r = minv(O.residual(A, x, b))
        rr = dot(r, r)
        res = math.sqrt(rr) / normb if rr >= 0.0 else float("nan")
        hist = [res]
        if res <= tol:
            return out(0, "conv0")
        rt = r.copy()
        rho = dot(rt, r)
        if _bad(rho):
            return out(BREAKDOWN, "rho0", rho)
        p = r.copy()
        while it < max_iter:
            v = minv(O.spmv(A, p))
            rtv = dot(rt, v)
            if _bad(rtv):
                return out(BREAKDOWN, "rtv", rtv)
            alpha = rho / rtv
            s = (-alpha) * v + r
            t = minv(O.spmv(A, s))
            ts = dot(t, s)
            tt = dot(t, t)
            omega = ts / tt if tt > 0.0 else 0.0
            x = omega * s + (alpha * p + x)
            r = (-omega) * t + s
            rr = dot(r, r)
            rhon = dot(rt, r)
            res = math.sqrt(rr) / normb if rr >= 0.0 else float("nan")
            it += 1
            hist.append(res)
            if res < tol:
                return out(0, "conv")
            if _bad(omega):
                return out(BREAKDOWN, "omega", omega)
            if _bad(rhon):
                return out(BREAKDOWN, "rho", rhon)
            beta = (rhon / rho) * (alpha / omega)
            p = beta * ((-omega) * v + p) + r
            rho = rhon
    return out(1, "exhausted")
