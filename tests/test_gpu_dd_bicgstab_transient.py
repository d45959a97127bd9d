"""GPU: the sharded transient loop with BiCGStab steps (gg_dd_transient_bicgstab_src,
csrc/dd.hip "Sharded transient") in one process (GG_DD_LOCAL): the new loop, the
host loop a user writes around gg_dd_solve_bicgstab, and the restatement
(dd_bicgstab_ref.transient: dd_transient_ref's step loop with
dd_bicgstab_ref.solve in the sharded order) agree bit for bit on the status, the
iteration total, the final x and every port column.

tests/test_gpu_dd_transient.py's small system with upwind = 0.2 (c = 1e-3,
h = 1e-2, 10 steps from x = 0); sources of the three kinds on a separator row
and in both interiors beside dd_transient_ref.mixed_sources', ports likewise.
Per-step counts on the CPU (natural layout): 10 to 13 at tol 1e-7, 14 to 17 at 1e-10.
"""
import numpy as np
import pytest

import dd_bicgstab_ref as Q
import dd_transient_ref as T
import ggmres
import oracle as O
from ggmres import host
from ggmres.dd import DD
from test_gpu_dd_bicgstab import build

pytestmark = pytest.mark.gpu
BI = ggmres.SOLVE_BICGSTAB
K = Q.K_CHUNK
H = Q.H_STEP
EINVAL, ESTATE = -1, -5

_cache = {}


def setup():
    if "s" not in _cache:
        A, cdiag, P, method, nsteps = Q.transient_system()
        A_, d, q, B, L, U, segs, G = build(A, P, method)
        n = A.shape[0]
        plan = host.DDPlan(A, P, method)
        assert np.array_equal(plan.q, q) and plan.nsep > 0
        beg = plan.begin
        sep = [int(q[beg[P]]), int(q[beg[P] + plan.nsep - 1])]
        inner = [int(q[beg[p] + (beg[p + 1] - beg[p]) // 2]) for p in range(P)]
        nodes, sources = T.mixed_sources(n)
        nodes = np.concatenate([nodes, np.array(sep + inner, np.int32)]).astype(np.int32)
        sources = list(sources) + [(O.SRC_DC, np.array([3e-4])),
                                   (O.SRC_PWL, np.array([0.0, 0.0, 3 * H, 1e-3, 6 * H, 2e-4])),
                                   (O.SRC_DC, np.array([-2e-4])), (O.SRC_DC, np.array([7e-4]))]
        ports = np.array(sep + inner + [0, n - 1], np.int32)
        _cache["s"] = dict(A=A, d=d, q=q, B=B, L=L, U=U, segs=segs, G=G, n=n, P=P, method=method, cdiag=cdiag,
                           nsteps=nsteps, nodes=nodes, sources=sources, ports=ports)
    return _cache["s"]


def device(s, d=None, **kw):
    d = s["d"] if d is None else d
    kw.setdefault("restart", 30)
    kw.setdefault("flags", BI)
    kw.setdefault("tol", 1e-7)
    x0 = kw.pop("x0", np.zeros(s["n"]))
    return d.transient_bicgstab_src(kw.pop("nsteps", s["nsteps"]), H, s["cdiag"], s["nodes"], s["sources"],
                                    s["ports"], x0, **kw)


_REF = {}


def restate(s, tol=1e-7, max_iter=10000, nsteps=None, x0=None, cache=None):
    k = (cache, tol, max_iter)
    if cache is None or k not in _REF:
        o = Q.transient(s["B"], s["L"], s["U"], s["q"], s["segs"], s["G"], s["nsteps"] if nsteps is None else nsteps,
                        H, s["cdiag"], s["nodes"], s["sources"], s["ports"],
                        np.zeros(s["n"]) if x0 is None else x0, max_iter=max_iter, tol=tol)
        if cache is None:
            return o
        _REF[k] = o
    return _REF[k]


def host_loop(s, d=None, tol=1e-7, max_iter=10000, nsteps=None, x0=None):
    """B u + (C/h) x on the host and gg_dd_solve_bicgstab per step, warm-started"""
    d = s["d"] if d is None else d
    nsteps = s["nsteps"] if nsteps is None else nsteps
    x = np.zeros(s["n"]) if x0 is None else x0.copy()
    pv = np.zeros((len(s["ports"]), nsteps + 1))
    pv[:, 0] = x[s["ports"]]
    total, ret = 0, 0
    for it in range(1, nsteps + 1):
        u = np.array([O.source_value(k, p, it, H) for k, p in s["sources"]])
        w = O.transient_rhs(s["cdiag"], s["nodes"], u, x)
        r = d.solve_bicgstab(w, x0=x, restart=30, max_iter=max_iter, tol=tol, flags=BI)
        x = r["x"]
        total += r["iters"]
        ret = r["ret"] or ret
        pv[:, it] = x[s["ports"]]
    return dict(ret=ret, x=x, ports=pv, iters_total=total)


def same_bits(g, o, what):
    print(f"{what}: device ret {g['ret']} iters_total {g['iters_total']}; other ret {o['ret']} "
          f"iters_total {o['iters_total']} steps {o.get('steps')}")
    assert g["ret"] == o["ret"], what
    assert g["iters_total"] == o["iters_total"], what
    assert g["ports"].shape == o["ports"].shape, what
    assert np.array_equal(g["x"], o["x"]), what
    assert np.array_equal(g["ports"], o["ports"]), what


@pytest.mark.parametrize("tol", [1e-7, 1e-10])
def test_dd_bicgstab_transient_hint_on_and_off(tol, monkeypatch):
    """the loop, hint on (a step's first chunk = the previous count + 2) and off
    (GG_DD_TRANSIENT_HINT=0: kChunk), the host loop and the restatement"""
    s = setup()
    o = restate(s, tol=tol, cache="default")
    counts = [i for _, i in o["steps"]]
    assert o["ret"] == 0 and min(counts) > K and len(set(counts)) > 1
    monkeypatch.delenv("GG_DD_TRANSIENT_HINT", raising=False)
    on = device(s, tol=tol)
    monkeypatch.setenv("GG_DD_TRANSIENT_HINT", "0")
    off = device(s, tol=tol)
    monkeypatch.delenv("GG_DD_TRANSIENT_HINT")
    same_bits(on, o, f"hint on, tol {tol:g}")
    same_bits(off, o, f"hint off, tol {tol:g}")
    same_bits(on, host_loop(s, tol=tol), f"host loop, tol {tol:g}")
    assert np.all(on["ports"][:, 0] == 0.0) and np.any(on["ports"][:, -1] != 0.0)
    assert s["d"].history().size == counts[-1] + 1                      # the last step's history
    flags0 = device(s, tol=tol, flags=0)                                 # flags 0 means BiCGStab too
    same_bits(flags0, o, "flags 0")


def test_dd_bicgstab_transient_exhausted_steps():
    s = setup()
    o = restate(s, max_iter=3, cache="default")
    assert o["steps"] == [(1, 3)] * s["nsteps"]
    g = device(s, max_iter=3)
    assert g["ret"] == 1 and g["iters_total"] == 3 * s["nsteps"]
    same_bits(g, o, "max_iter 3")
    same_bits(g, host_loop(s, max_iter=3), "max_iter 3, host loop")


def test_dd_bicgstab_transient_breakdown_keeps_the_state():
    """dd_bicgstab_ref.EXACT_BLOCKS "omega" as a transient (every right-hand side
    the block's b): step 1 breaks down after one iteration and x keeps that
    iterate (omega = 0), the later steps break down before their first from it
    (rt.v = 0).  The object
    then runs the default transient with the cached object's bits"""
    s0 = setup()
    A, cdiag, nodes, sources = Q.exact_transient("omega")
    A_, d, q, B, L, U, segs, G = build(A, 2, host.PART_BLOCKS)
    n = A.shape[0]
    m = 3 * Q.EXACT_COUNT
    s = dict(d=d, q=q, B=B, L=L, U=U, segs=segs, G=G, n=n, cdiag=cdiag, nsteps=4, nodes=nodes, sources=sources,
             ports=np.array([0, 1, 2, m, m + 1, n - 1], np.int32))
    try:
        o = restate(s)
        assert o["steps"] == [(Q.BREAKDOWN, 1)] + [(Q.BREAKDOWN, 0)] * 3 and np.any(o["x"] != 0.0)
        g = device(s)
        assert g["ret"] == ggmres.EBREAKDOWN and g["iters_total"] == 1
        # gg_last_error: the last step's text
        assert o["whys"] == ["omega", "rtv", "rtv", "rtv"]
        assert ggmres.lib().gg_last_error().decode() == (
            "gg_dd_solve_bicgstab: BiCGStab broke down at iteration 0: rt.v = 0 (zero or not finite)")
        same_bits(g, o, "breakdown inside the loop")
        assert np.array_equal(g["ports"][:, 1], g["ports"][:, 4])       # the state is kept
        same_bits(g, host_loop(s), "breakdown, host loop")
        d.set_system(s0["A"], s0["method"])
        assert np.array_equal(d.perm()[1], s0["q"])
        same_bits(device(s0, d=d), restate(s0, cache="default"), "after the breakdowns")
    finally:
        d.close()


def test_dd_bicgstab_transient_pulse_form_and_refusals():
    s = setup()
    n = s["n"]
    from ggmres import matrices as M
    nodes, pulses = M.pulse_sources(n, frac=0.02, h=H)
    g = s["d"].transient_bicgstab(4, H, s["cdiag"], nodes, pulses, s["ports"], np.zeros(n), restart=30, tol=1e-7,
                                  flags=BI)
    w = s["d"].transient_bicgstab_src(4, H, s["cdiag"], nodes, [(O.SRC_PULSE, p) for p in pulses], s["ports"],
                                      np.zeros(n), restart=30, tol=1e-7, flags=BI)
    assert g["ret"] == 0 and g["iters_total"] > 0
    same_bits(g, w, "PULSE form")
    for kw in (dict(flags=ggmres.SOLVE_CG), dict(flags=ggmres.SOLVE_CGS2), dict(flags=0x10), dict(restart=0),
               dict(nsteps=-1)):
        with pytest.raises(ggmres.GGError) as e:
            device(s, **kw)
        assert e.value.code == EINVAL, kw
    e = DD(s["P"], device=0)
    try:
        with pytest.raises(ggmres.GGError) as err:
            e.transient_bicgstab_src(2, H, np.zeros(1), np.zeros(0, np.int32), [], np.zeros(0, np.int32),
                                     np.zeros(1))
        assert err.value.code == ESTATE
    finally:
        e.close()
    same_bits(device(s), restate(s, cache="default"), "after the refusals")
