"""CPU: every case of tests/sr_exit_cases.py reaches the exit it is named for.

The GPU tests hold the device to the restatement's bits but cannot see which
kernel set the done bit; this file is the proof that each case's restatement
leaves through the intended branch -- once with plain NumPy dots and once with
the products of every dot summed in a seeded random permutation.  For the exact
cases (integer or dyadic data) the two orders give identical histories, relres
and x, equal to the hand-computed values of the table; for the rounded cases
the iteration stays inside the case's window in both orders.
"""
import numpy as np
import pytest

import sr_exit_cases as X


def shuffled_dot(seed):
    """a dot whose products are summed one by one in a random order, a new one per call"""
    rng = np.random.default_rng(seed)

    def dot(u, v):
        with np.errstate(over="ignore", invalid="ignore"):
            p = np.asarray(u) * np.asarray(v)
            acc = 0.0
            for k in rng.permutation(p.size):
                acc = acc + p[k]
        return float(acc)
    return dot


def same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


@pytest.mark.parametrize("name", X.names())
def test_case_reaches_its_exit_in_two_orders(name):
    c = X.cases()[name]
    runs = []
    for what, dot in (("plain", None), ("shuffled", shuffled_dot(20261021))):
        info = {}
        ret, x, iters, relres, hist = X.reference(c, dot, info=info)
        print(f"{name} {what}: ret {ret} iters {iters} why {info['why']} bad {info['bad']!r} relres {relres!r}")
        assert info["why"] == c.why, what
        assert ret == c.ret and c.iters_ok(iters), what
        assert hist.size == iters + 1 and same(hist[-1], relres), what
        if ret == X.BREAKDOWN:
            assert info["bad"] is not None, what
        else:
            assert info["bad"] is None, what
        if iters == 0:
            assert np.array_equal(x, c.x0), what        # nothing has moved
        else:
            assert not same(x, c.x0), what              # x and r moved before the exit
        runs.append((x, relres, hist))
    if c.x is not None:                                 # the exact cases: one answer in any order
        (xa, ra, ha), (xb, rb, hb) = runs
        assert same(ha, hb) and same(ra, rb) and same(xa, xb)
        assert same(ha, c.hist) and same(ra, c.relres) and same(xa, c.x)


def test_the_named_scalars():
    """the scalars the issue's table names: which one is bad, and its value where exact"""
    got = {}
    for name in X.names():
        info = {}
        X.reference(X.cases()[name], info=info)
        got[name] = info["bad"]
    assert got["omega"] == 0.0 and got["rho_mid"] == 0.0 and got["rtv_mid"] == 0.0 and got["rtv0"] == 0.0
    assert got["rho0_inf"] == np.inf
    assert got["lucky"] is None and got["lucky_oblique"] is None
    assert got["pq_zero"] == 0.0
    assert got["pq0"] < 0.0 and got["pq_mid"] < 0.0 and got["pq_late"] < 0.0
    assert got["rz_mid"] < 0.0 and got["rz0"] < 0.0
    assert np.isnan(got["nan"])


def test_omega_takes_precedence_over_rho():
    """in the `omega` case the next rho is 0 as well: the restatement names omega, as k_bi_p does"""
    c = X.cases()["omega"]
    seen = {}

    def spy(u, v):
        d = float(np.dot(u, v))
        seen.setdefault("dots", []).append(d)
        return d
    info = {}
    X.reference(c, spy, info=info)
    # bb.bb, r.r, rho | rt.v, t.s, t.t, r.r, rt.r
    assert seen["dots"][-1] == 0.0 and seen["dots"][-3] == 0.0
    assert info["why"] == "omega"


def test_pcg_and_bicgstab_return_tuples_are_unchanged():
    """info is optional: the five-tuple is the same with and without it"""
    for name in ("pq_mid", "rho_mid", "lucky"):
        c = X.cases()[name]
        a = X.reference(c)
        b = X.reference(c, info={})
        assert len(a) == len(b) == 5 and a[0] == b[0] and a[2] == b[2]
        assert same(a[1], b[1]) and same(a[3], b[3]) and same(a[4], b[4])
        assert X.reference(c, max_iter=0, info=(i := {}))[0] == 1 and i["why"] == "exhausted"
    z = X.cases()["lucky"]._replace(b=np.zeros(272))
    assert X.reference(z, info=(i := {}))[:1] == (0,) and i["why"] == "conv0"
