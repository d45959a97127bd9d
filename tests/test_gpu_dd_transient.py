"""GPU: the sharded transient loop (gg_dd_transient_src, csrc/dd.hip "Sharded
transient") in one process (GG_DD_LOCAL) against its restatement
tests/dd_transient_ref.py in the sharded order (DD.dot_layout), and against the
host loop a user writes around gg_dd_solve.

Bar: the return code, iters_total, the final x and the whole port matrix are
bit-identical (np.array_equal).  c = 1e-3, h = 1e-2, GMRES(30), sources of the
three kinds cycling over pulse_sources(n, 0.02)'s nodes, from x = 0 unless a test
says otherwise; per-step counts on the CPU in tests/test_dd_transient_ref.py.
"""
import numpy as np
import pytest

import dd_cg_ref as D
import dd_transient_ref as T
import ggmres
import oracle as O
from ggmres import host, matrices as M
from ggmres.dd import DD

pytestmark = pytest.mark.gpu
CG, CGS2 = ggmres.SOLVE_CG, ggmres.SOLVE_CGS2
assert (CG, CGS2) == (T.SOLVE_CG, T.SOLVE_CGS2)
K = T.K_CHUNK
H = T.H_STEP
EINVAL, ESTATE = -1, -5

_cache = {}


def build(A, P, method):
    d = DD(P, device=0)
    d.set_system(A, method)
    pinv, q = d.perm()
    B = host.permute(A, pinv, q)
    L, U = O.ilu0(B)
    segs, G = zip(*[d.dot_layout(p) for p in range(P)])
    return dict(d=d, q=q, B=B, L=L, U=U, segs=list(segs), G=G[0])


def setup(name):
    """the system, its cached DD object, the restatement's pieces, the default sources and ports"""
    if name not in _cache:
        A, cdiag, P, method, nsteps = T.system(name)
        s = build(A, P, method)
        n = A.shape[0]
        nodes, sources = T.mixed_sources(n)
        s.update(A=A, cdiag=cdiag, P=P, method=method, nsteps=nsteps, n=n, nodes=nodes, sources=sources,
                 ports=T.default_ports(n))
        _cache[name] = s
    return _cache[name]


def device(s, d=None, nsteps=None, nodes=None, sources=None, ports=None, x0=None, **kw):
    d = s["d"] if d is None else d
    kw.setdefault("restart", 30)
    return d.transient_src(s["nsteps"] if nsteps is None else nsteps, H, s["cdiag"],
                           s["nodes"] if nodes is None else nodes, s["sources"] if sources is None else sources,
                           s["ports"] if ports is None else ports, np.zeros(s["n"]) if x0 is None else x0, **kw)


_REF = {}


def reference(name, flags=0, tol=1e-7, max_iter=10000):
    """the restatement of the default run of a system, once per option set, never modified"""
    k = (name, flags, tol, max_iter)
    if k not in _REF:
        _REF[k] = restate(setup(name), flags=flags, tol=tol, max_iter=max_iter)
    return _REF[k]


def restate(s, nsteps=None, nodes=None, sources=None, ports=None, x0=None, **kw):
    return T.transient(s["B"], s["L"], s["U"], s["q"], s["segs"], s["G"], s["nsteps"] if nsteps is None else nsteps,
                       H, s["cdiag"], s["nodes"] if nodes is None else nodes,
                       s["sources"] if sources is None else sources, s["ports"] if ports is None else ports,
                       np.zeros(s["n"]) if x0 is None else x0, restart=30, **kw)


def same_bits(g, o, what):
    print(f"{what}: device ret {g['ret']} iters_total {g['iters_total']}; restatement ret {o['ret']} "
          f"iters_total {o['iters_total']} steps {o.get('steps')}")
    assert g["ret"] == o["ret"], what
    assert g["iters_total"] == o["iters_total"], what
    assert g["ports"].shape == o["ports"].shape, what
    assert np.array_equal(g["x"], o["x"]), what
    assert np.array_equal(g["ports"], o["ports"]), what


@pytest.mark.parametrize("flags", [0, CGS2, CG])
@pytest.mark.parametrize("name", sorted(T.SYSTEMS))
def test_dd_transient_bit_identical_to_the_restatement(name, flags):
    s = setup(name)
    o = reference(name, flags)
    assert o["ret"] == 0 and all(i > 0 for _, i in o["steps"])
    g = device(s, flags=flags, tol=1e-7)
    same_bits(g, o, f"sharded transient {name} flags {flags}")
    assert np.all(g["ports"][:, 0] == 0.0) and np.any(g["ports"][:, -1] != 0.0)
    if flags == CG and name == "small":
        assert s["d"].history().size == o["steps"][-1][1] + 1          # the last step's history


@pytest.mark.parametrize("name,flags", [("small", 0), ("small", CGS2), ("small", CG), ("mixed", CG)])
def test_dd_transient_bit_identical_to_the_host_loop(name, flags):
    """B u + (C/h) x on the host and gg_dd_solve per step, warm-started: keeping x in
    the slots and assembling on the device changes nothing"""
    s = setup(name)
    d = s["d"]
    x = np.zeros(s["n"])
    pv = np.zeros((len(s["ports"]), s["nsteps"] + 1))
    pv[:, 0] = x[s["ports"]]
    total, ret = 0, 0
    for it in range(1, s["nsteps"] + 1):
        u = np.array([O.source_value(k, p, it, H) for k, p in s["sources"]])
        w = O.transient_rhs(s["cdiag"], s["nodes"], u, x)
        r = d.solve(w, x0=x, restart=30, max_iter=10000, tol=1e-7, flags=flags)
        x = r["x"]
        total += r["iters"]
        ret = r["ret"] or ret
        pv[:, it] = x[s["ports"]]
    g = device(s, flags=flags, tol=1e-7)
    same_bits(g, dict(ret=ret, x=x, ports=pv, iters_total=total), f"host loop {name} flags {flags}")


def test_dd_transient_placement():
    """sources and ports on a separator row and in every interior, three sources on one
    row (their sum in ascending k: two would commute), a port listed twice"""
    s = setup("mixed")
    d, q, P = s["d"], s["q"], s["P"]
    plan = host.DDPlan(s["A"], P, s["method"])
    assert np.array_equal(plan.q, q) and d.info()["nsep"] == plan.nsep > 0
    beg = plan.begin
    sep = [int(q[beg[P]]), int(q[beg[P] + plan.nsep - 1])]
    inner = [int(q[beg[p] + (beg[p + 1] - beg[p]) // 2]) for p in range(P)]
    assert len(set(sep + inner)) == P + 2
    nodes = np.array([sep[0]] + inner + [inner[1], sep[0], inner[1], sep[1]], np.int32)
    vals = [0.1, 0.2, 0.3, 0.4, 0.5, 0.7, 1e-17, -0.7, 0.6]
    assert (vals[2] + vals[5]) + vals[7] != vals[2] + (vals[5] + vals[7])     # inner[1]: the order is visible
    sources = [(O.SRC_DC, np.array([1e-3 * v])) for v in vals]
    sources[3] = (O.SRC_PWL, np.array([0.0, 0.0, 3 * H, 1e-3, 6 * H, 2e-4]))
    ports = np.array([sep[0], inner[0], inner[1], sep[1], inner[2], inner[3], sep[0], inner[1]], np.int32)
    x0 = 1e-3 * np.linspace(0.5, 1.5, s["n"])
    kw = dict(nodes=nodes, sources=sources, ports=ports, x0=x0, flags=CG, tol=1e-7)
    g = device(s, **kw)
    o = restate(s, **kw)
    assert o["ret"] == 0
    same_bits(g, o, "placement")
    assert np.array_equal(g["ports"][:, 0], x0[ports])
    assert np.array_equal(g["ports"][0], g["ports"][6]) and np.array_equal(g["ports"][2], g["ports"][7])


def test_dd_transient_empty_arguments():
    s = setup("small")
    x0 = 1e-3 * np.linspace(0.5, 1.5, s["n"])
    none = np.zeros(0, np.int32)
    for kw in (dict(nodes=none, sources=[]), dict(ports=none), dict(nodes=none, sources=[], ports=none)):
        kw.update(x0=x0, flags=CG, tol=1e-7, nsteps=3)
        g = device(s, **kw)                                             # nport = 0: port_out is NULL
        same_bits(g, restate(s, **kw), f"empty {sorted(kw)}")
    g = device(s, nsteps=0, x0=x0, flags=CG)
    assert g["ret"] == 0 and g["iters_total"] == 0 and np.array_equal(g["x"], x0)
    assert g["ports"].shape == (len(s["ports"]), 1) and np.array_equal(g["ports"][:, 0], x0[s["ports"]])


@pytest.mark.parametrize("tol", [1e-7, 1e-10])
def test_dd_transient_hint_changes_no_bits(tol, monkeypatch):
    """GG_DD_TRANSIENT_HINT=0 and unset: a step's first chunk is 8 iterations or the
    previous step's count + 2 -- step ends before, at and after chunk boundaries;
    also max_iter = a step's own count and one short of it"""
    s = setup("small")
    o = reference("small", CG, tol)
    counts = [i for _, i in o["steps"]]
    assert min(counts) > K and len(set(counts)) > 1
    # (the first step's count: later steps start from what the earlier ones left)
    for max_iter in (10000, counts[0], counts[0] - 1):
        oo = o if max_iter == 10000 else reference("small", CG, tol, max_iter)
        if max_iter == counts[0]:
            assert oo["steps"] == o["steps"] and oo["steps"][0] == (0, max_iter)
        if max_iter == counts[0] - 1:
            assert oo["steps"][0] == (1, max_iter) and oo["ret"] in (0, 1)
        monkeypatch.delenv("GG_DD_TRANSIENT_HINT", raising=False)
        on = device(s, flags=CG, tol=tol, max_iter=max_iter)
        monkeypatch.setenv("GG_DD_TRANSIENT_HINT", "0")
        off = device(s, flags=CG, tol=tol, max_iter=max_iter)
        monkeypatch.delenv("GG_DD_TRANSIENT_HINT")
        same_bits(on, oo, f"hint on, tol {tol:g}, max_iter {max_iter}")
        same_bits(off, oo, f"hint off, tol {tol:g}, max_iter {max_iter}")


@pytest.mark.parametrize("flags", [0, CGS2, CG])
def test_dd_transient_exhausted_steps(flags):
    s = setup("small")
    o = reference("small", flags, 1e-7, 5)
    assert o["steps"] == [(1, 5)] * s["nsteps"]
    g = device(s, flags=flags, tol=1e-7, max_iter=5)
    assert g["ret"] == 1 and g["iters_total"] == 5 * s["nsteps"]
    same_bits(g, o, f"max_iter 5, flags {flags}")


def test_dd_transient_cg_breakdown_inside_the_loop():
    """the negated matrix: every step breaks down before its first iteration; x and
    every port column keep the initial values (finite inputs only), and the same
    object then runs the SPD system's transient with a fresh object's bits"""
    s0 = setup("small")
    S = D.breakdown_matrix("negated")
    b = build(S, s0["P"], s0["method"])
    d = b["d"]
    try:
        x0 = np.linspace(0.5, 1.5, s0["n"])
        g = device(s0, d=d, nsteps=3, x0=x0, flags=CG, tol=1e-7)
        assert g["ret"] == ggmres.EBREAKDOWN and g["iters_total"] == 0
        assert np.array_equal(g["x"], x0)
        assert np.array_equal(g["ports"], np.tile(x0[s0["ports"]][:, None], 4))
        s = dict(s0, **{k: b[k] for k in ("q", "B", "L", "U", "segs", "G")})
        same_bits(g, restate(s, nsteps=3, x0=x0, flags=CG, tol=1e-7), "breakdown")
        d.set_system(s0["A"], s0["method"])
        assert np.array_equal(d.perm()[1], s0["q"])
        g2 = device(s0, d=d, flags=CG, tol=1e-7)
        same_bits(g2, reference("small", CG), "after a breakdown")
        same_bits(g2, device(s0, flags=CG, tol=1e-7), "after a breakdown, the cached object")
    finally:
        d.close()


def test_dd_transient_interleaved_with_solves():
    """transient, gg_dd_solve (GMRES, then CG), transient on one object: each
    bit-identical to the same call on a fresh object"""
    s = setup("small")
    b = M.rhs_ones(s["A"])

    def calls(d):
        return [lambda: device(s, d=d, flags=CG, tol=1e-7),
                lambda: d.solve(b, restart=30, max_iter=1500, tol=1e-10),
                lambda: d.solve(b, restart=30, max_iter=1500, tol=1e-10, flags=CG),
                lambda: device(s, d=d, flags=0, tol=1e-7)]
    got = [f() for f in calls(s["d"])]
    for k, g in enumerate(got):
        e = DD(s["P"], device=0)
        try:
            e.set_system(s["A"], s["method"])
            w = calls(e)[k]()
        finally:
            e.close()
        assert g["ret"] == w["ret"] == 0 and np.array_equal(g["x"], w["x"]), k
        if "ports" in g:
            assert g["iters_total"] == w["iters_total"] and np.array_equal(g["ports"], w["ports"]), k
        else:
            assert g["iters"] == w["iters"] and np.array_equal(g["hist"], w["hist"]), k
    same_bits(got[0], reference("small", CG), "interleaved, first")
    same_bits(got[3], reference("small", 0), "interleaved, last")


def test_dd_transient_refusals():
    s = setup("small")
    n = s["n"]

    def refused(code, **kw):
        with pytest.raises(ggmres.GGError) as e:
            device(s, **kw)
        assert e.value.code == code, (kw, e.value)

    refused(EINVAL, flags=ggmres.SOLVE_BICGSTAB)
    refused(EINVAL, flags=CG | CGS2)
    refused(EINVAL, flags=CG | 0x10)
    refused(EINVAL, flags=CG, restart=0)
    bad = s["nodes"].copy()
    bad[-1] = n
    refused(EINVAL, nodes=bad, flags=CG)
    refused(EINVAL, ports=np.array([0, n], np.int32), flags=CG)
    refused(EINVAL, ports=np.array([-1], np.int32), flags=CG)
    short = list(s["sources"])
    assert short[0][0] == O.SRC_PULSE
    short[0] = (O.SRC_PULSE, short[0][1][:6])
    refused(EINVAL, sources=short, flags=CG)
    refused(EINVAL, nsteps=-1, flags=CG)
    e = DD(s["P"], device=0)
    try:
        with pytest.raises(ggmres.GGError) as err:
            e.transient_src(2, H, np.zeros(1), np.zeros(0, np.int32), [], np.zeros(0, np.int32), np.zeros(1))
        assert err.value.code == ESTATE
    finally:
        e.close()
    same_bits(device(s, flags=CG, tol=1e-7), reference("small", CG), "after the refusals")


def test_dd_transient_pulse_form():
    """gg_dd_transient: the all-PULSE form is gg_dd_transient_src with PULSE rows"""
    s = setup("small")
    nodes, pulses = M.pulse_sources(s["n"], frac=0.02, h=H)
    g = s["d"].transient(4, H, s["cdiag"], nodes, pulses, s["ports"], np.zeros(s["n"]), restart=30, tol=1e-7,
                         flags=CG)
    w = device(s, nsteps=4, nodes=nodes, sources=[(O.SRC_PULSE, p) for p in pulses], flags=CG, tol=1e-7)
    assert g["ret"] == 0 and g["iters_total"] > 0
    same_bits(g, w, "PULSE form")
