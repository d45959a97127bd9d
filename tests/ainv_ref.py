"""Plain-Python fp64 restatements for the AINV / DIAG preconditioners (test code).

ainv(A, tol): cusp's nonsym_bridson_ainv as the reference calls it (MyAINV::
Initilize, src/preconditioner.cu:166; the algorithm of include/cusp-v0.3.1/cusp/
precond/detail/ainv.inl), no bound on a row's entries, rows as dicts walked in
sorted order.  What fixes the bits:
  z_j, w_j start as e_j; for j = 0 .. n-1
    u = A^T w_j, l = A z_j: over the vector's entries in ascending index and the
      matrix row's entries in stored order, the first product assigned, later
      ones added (named by the matrix cusp hands its matrix_vector_product,
      A^T for u and A for l; it forms b[col] += M[row][col] x[row])
    p = w_j . l as an ascending merge from 0; dinv[j] = 1 / p
    z_i += (-u_i / p) z_j for each i > j with u_i != 0, ascending; each term is
      mult * value, skipped when |term| < tol; the same for w_i from l
  Z row i = z_i; Wt = the transpose of the matrix whose row i is w_i.

gmres_left(op_A, op_M, b, ...): NumPy left-preconditioned GMRES(m) with callable
operators, following oracle/oracle.c's gmres_core (orc_gmres_left) in its
recurrence, convergence tests and history format (the oracle's own gmres_left
takes only L and U factors).
"""
import math

import numpy as np
import scipy.sparse as sp

import oracle as O


class ZeroPivot(ArithmeticError):
    pass


def _matvec(rp, ci, v, x):
    """sparse M x for a dict x (matrix_vector_product): dict in first-touch order"""
    b = {}
    for r in sorted(x):
        xr = x[r]
        for k in range(rp[r], rp[r + 1]):
            c = ci[k]
            prod = v[k] * xr
            if c in b:
                b[c] += prod
            else:
                b[c] = prod
    return b


def _add_drop(res, mult, op, tol):
    for c in sorted(op):
        term = mult * op[c]
        if abs(term) < tol:
            continue
        if c in res:
            res[c] += term
        else:
            res[c] = term


def ainv(A, tol=0.1):
    """(Z, Wt, dinv): scipy CSR factors with ascending columns, M = Wt diag(dinv) Z."""
    if not tol >= 0.0:
        raise ValueError("drop tolerance must be >= 0")
    A = O.csr(A)
    n = A.n
    rp, ci, v = (a.tolist() for a in (A.rp, A.ci, A.v))
    # stable transpose: column c's entries in ascending row order
    tr = [[] for _ in range(n)]
    for r in range(n):
        for k in range(rp[r], rp[r + 1]):
            tr[ci[k]].append((r, v[k]))
    trp, tci, tv = [0], [], []
    for c in range(n):
        for r, a in tr[c]:
            tci.append(r)
            tv.append(a)
        trp.append(len(tci))
    z = [{i: 1.0} for i in range(n)]
    w = [{i: 1.0} for i in range(n)]
    dinv = np.zeros(n)
    for j in range(n):
        u = _matvec(trp, tci, tv, w[j])
        l = _matvec(rp, ci, v, z[j])
        p = 0.0
        for c in sorted(w[j]):
            if c in l:
                p += w[j][c] * l[c]
        if p == 0.0 or not math.isfinite(p):
            raise ZeroPivot(f"pivot {j}")
        dinv[j] = 1.0 / p
        for i in sorted(c for c in u if c > j and u[c] != 0.0):
            _add_drop(z[i], -u[i] / p, z[j], tol)
        for i in sorted(c for c in l if c > j and l[c] != 0.0):
            _add_drop(w[i], -l[i] / p, w[j], tol)

    def rows_csr(rows):
        indptr, idx, val = [0], [], []
        for row in rows:
            for c in sorted(row):
                idx.append(c)
                val.append(row[c])
            indptr.append(len(idx))
        return sp.csr_matrix((np.array(val, np.float64), np.array(idx, np.int32), np.array(indptr, np.int32)),
                             shape=(n, n))

    Z = rows_csr(z)
    wt = [{} for _ in range(n)]
    for i in range(n):
        for c, a in w[i].items():
            wt[c][i] = a
    return Z, rows_csr(wt), dinv


def ainv_apply(Z, Wt, dinv, x):
    """MyAINV::HostPrecond: out = Wt (dinv o (Z x)), rows summed serially in column order"""
    return O.spmv(Wt, dinv * O.spmv(Z, x))


def diag_nearest(A):
    """MyDIAG::Initilize: 1 / the entry of each row nearest the diagonal (first wins)"""
    A = O.csr(A)
    inv = np.zeros(A.n)
    for i in range(A.n):
        d, dist = 0.0, 2 * A.n
        for k in range(A.rp[i], A.rp[i + 1]):
            if abs(int(A.ci[k]) - i) < dist:
                dist = abs(int(A.ci[k]) - i)
                d = float(A.v[k])
        if d == 0.0:
            raise ZeroPivot(f"row {i}")
        inv[i] = 1.0 / d
    return inv


def _wave_tree(v):
    """64-lane xor butterflies over the last axis (4 waves of 64), then (w0+w1)+(w2+w3)"""
    lanes = np.arange(64)
    v = v.reshape(v.shape[:-1] + (4, 64))
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return (v[..., 0, 0] + v[..., 1, 0]) + (v[..., 2, 0] + v[..., 3, 0])


def device_dot(n):
    """The solver's dot product in the natural-order vector space, restated as
    oracle.c's dot_blocked restates it (DESIGN.md "Reduction order"): the vector
    padded to a multiple of 512 slots, G blocks of 256 threads, each thread
    summing its grid-stride pairs in order, the wave / block tree above, then the
    G partials summed by one more block."""
    from helpers import device_layout
    ppad = max((max(n, 1) + 511) // 512 * 512, 512)
    units = ppad // 2
    G = device_layout(n)[1]
    nthr = G * 256
    rounds = -(-units // nthr)

    def dot(x, y):
        p = np.zeros(rounds * nthr * 2)
        p[:n] = np.asarray(x) * np.asarray(y)
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


def _update(x, k, H, s, V):
    y = s[:k + 1].copy()
    for i in range(k, -1, -1):
        y[i] /= H[i, i]
        for j in range(i - 1, -1, -1):
            y[j] -= H[j, i] * y[i]
    for j in range(k + 1):
        x += V[j] * y[j]


def gmres_left(A, minv, b, x0=None, m=30, max_iter=3000, tol=1e-10, dot=None):
    """oracle.c gmres_core, kind 0, with M^-1 = the callable minv: dict(ret, x,
    iters, relres, hist, inner).  History: [beta0/normb, |s[i+1]|/normb per inner
    iteration, beta/normb after each restart ...].  dot: the inner product
    (default NumPy's; device_dot(n) sums in the solver's order)."""
    if dot is None:
        dot = lambda p, q: float(np.dot(p, q))      # noqa: E731
    A = O.csr(A)
    n = A.n
    b = np.asarray(b, np.float64)
    x = np.zeros(n) if x0 is None else np.array(x0, np.float64, copy=True)
    hist = []
    bb = minv(b)
    normb = math.sqrt(dot(bb, bb))
    if normb == 0.0:
        normb = 1.0
    r = minv(O.residual(A, x, b))
    beta = math.sqrt(dot(r, r))
    resid = beta / normb
    hist.append(resid)
    if resid <= tol:
        return dict(ret=0, x=x, iters=0, relres=resid, hist=np.array(hist), inner=0)
    j, inner = 1, 0
    H = np.zeros((m + 1, m))
    V = np.zeros((m + 1, n))
    cs, sn = np.zeros(m + 1), np.zeros(m + 1)
    while j <= max_iter:
        V[0] = (1.0 / beta) * r
        s = np.zeros(m + 1)
        s[0] = beta
        i = 0
        while i < m and j <= max_iter:
            w = minv(O.spmv(A, V[i]))
            for k in range(i + 1):
                h = dot(w, V[k])
                H[k, i] = h
                w = (-h) * V[k] + w
            hn = math.sqrt(dot(w, w))
            H[i + 1, i] = hn
            V[i + 1] = (1.0 / hn) * w if hn != 0.0 else 0.0
            for k in range(i):
                t = cs[k] * H[k, i] + sn[k] * H[k + 1, i]
                H[k + 1, i] = -sn[k] * H[k, i] + cs[k] * H[k + 1, i]
                H[k, i] = t
            cs[i], sn[i] = O.gen_rot(H[i, i], H[i + 1, i])
            t = cs[i] * H[i, i] + sn[i] * H[i + 1, i]
            H[i + 1, i] = -sn[i] * H[i, i] + cs[i] * H[i + 1, i]
            H[i, i] = t
            t = cs[i] * s[i] + sn[i] * s[i + 1]
            s[i + 1] = -sn[i] * s[i] + cs[i] * s[i + 1]
            s[i] = t
            inner += 1
            resid = abs(s[i + 1]) / normb
            hist.append(resid)
            if resid < tol:
                _update(x, i, H, s, V)
                return dict(ret=0, x=x, iters=j, relres=resid, hist=np.array(hist), inner=inner)
            i += 1
            j += 1
        _update(x, i - 1, H, s, V)
        r = minv(O.residual(A, x, b))
        beta = math.sqrt(dot(r, r))
        resid = beta / normb
        hist.append(resid)
        if resid < tol:
            return dict(ret=0, x=x, iters=j, relres=resid, hist=np.array(hist), inner=inner)
    return dict(ret=1, x=x, iters=max_iter, relres=resid, hist=np.array(hist), inner=inner)


def pert(nx, ny=None):
    """laplacian_5pt(nx, ny) plus a uniform(-0.3, 0.3) perturbation of every entry
    (default_rng(21)): nonsymmetric, the matrix of test_engine_abi_preconditioner_plugin"""
    from ggmres import matrices as M
    A = sp.csr_matrix(M.laplacian_5pt(nx, ny if ny is not None else nx)).copy()
    A.sort_indices()
    A.data = A.data + np.random.default_rng(21).uniform(-0.3, 0.3, A.nnz)
    return A


def two_dense_rows(n):
    """4 I plus a dense first row and a dense last row: row n-1 of Z and row 0
    of Wt then hold n entries each (every term is about 0.2 >= the tolerance) --
    above the SpMV's block capacity of 2048, the long-row path"""
    rng = np.random.default_rng(8)
    r = np.arange(n)
    rows = np.concatenate([r, np.zeros(n - 1, int), np.full(n - 1, n - 1)])
    cols = np.concatenate([r, r[1:], r[:-1]])
    vals = np.concatenate([np.full(n, 4.0), rng.uniform(0.8, 1.2, n - 1), rng.uniform(0.8, 1.2, n - 1)])
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    A.sort_indices()
    return A
