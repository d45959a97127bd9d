"""Input builders of the BiCGStab batch's tests (tests/test_gpu_bicgstab_batch.py
on the device, tests/test_bicgstab_batch_cases.py holds the restatement
tests/bicgstab_ref.py to the conditions the device tests rely on).  A plain
module: matrices, right-hand sides and warm starts, nothing solved here.

Every matrix is the upwinded 5-point grid M.laplacian_5pt(..., upwind=0.2):
nonsymmetric, ILU(0) on the 2D wavefront."""
import numpy as np

from ggmres import matrices as M

UPWIND = 0.2
# `tiny`: b = 10**e * N(0, 1).  The scalars underflow, so the solve breaks down
# after x and r have moved; with plain dots e = -162: rt.v at iteration 0,
# -161 / -159 / -157 / -155 / -154: omega at 2 / 6 / 8 / 10 / 12, -160 / -158 /
# -156 / -153 converge
TINY_EXPONENTS = (-162, -161, -160, -159, -158, -157, -156, -155, -154, -153)


def rhs_set(A, S, seed):
    """test_gpu_cg_batch.rhs_set's pattern: b = A 1, random normal, zeros, 1e3 * uniform, repeated"""
    n = A.shape[0]
    rng = np.random.default_rng(seed)
    out = []
    for q in range(S):
        k = q % 4
        if k == 0:
            out.append(A @ np.ones(n))
        elif k == 1:
            out.append(rng.standard_normal(n))
        elif k == 2:
            out.append(np.zeros(n))
        else:
            out.append(1e3 * rng.uniform(-1, 1, n))
    return np.array(out)


def band():
    """60 x 52 upwinded: one 64-line band with padded steps; 9 scenarios (the
    batched SpMV carries 8 per launch: groups of 8 + 1), three of them warm
    starts.  Plain-dot counts at tol 1e-10: 34, 33, 0, 33, 21, 34, 0, 31, 11"""
    A = M.laplacian_5pt(60, 52, upwind=UPWIND)
    n = A.shape[0]
    S = 9
    B = rhs_set(A, S, seed=3)
    rng = np.random.default_rng(9)
    X0 = np.zeros((S, n))
    X0[1] = 1e-2 * rng.standard_normal(n)
    X0[4] = 1.0 + 1e-5 * rng.standard_normal(n)
    X0[8] = 1.0 + 1e-7 * rng.standard_normal(n)
    return A, B, X0


def nat():
    """37 x 64 upwinded, 4 scenarios, scenario 1 a warm start.  Counts: 27, 28, 0, 28"""
    A = M.laplacian_5pt(37, 64, upwind=UPWIND)
    n = A.shape[0]
    S = 4
    B = rhs_set(A, S, seed=5)
    X0 = np.zeros((S, n))
    X0[1] = 1e-2 * np.random.default_rng(9).standard_normal(n)
    return A, B, X0


def small_matrix():
    return M.laplacian_5pt(16, 17, upwind=UPWIND)


def small():
    """272 rows, x0 = 0: b = A 1 (14 iterations), 1e200 * 1 (rho overflows at
    the start: breakdown at iteration 0, relres NaN, x untouched), 0 (converged
    at the start), random normal (14)"""
    A = small_matrix()
    n = A.shape[0]
    B = np.array([A @ np.ones(n), 1e200 * np.ones(n), np.zeros(n), np.random.default_rng(6).standard_normal(n)])
    return A, B, np.zeros((4, n))


def tiny(exponents=TINY_EXPONENTS):
    """the small matrix with b = 10**e * N(0, 1) for each exponent, then A 1 and zeros"""
    A = small_matrix()
    n = A.shape[0]
    g = np.random.default_rng(6).standard_normal(n)
    B = np.array([10.0 ** e * g for e in exponents] + [A @ np.ones(n), np.zeros(n)])
    return A, B, np.zeros((B.shape[0], n))


def diverse(counts):
    """the `band` condition: scenarios end several chunks of the read-back apart"""
    pos = [c for c in counts if c > 0]
    return len(set(counts)) >= 4 and 0 in counts and max(counts) > 2 * min(pos)
