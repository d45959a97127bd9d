"""bench.py's plain / --full split and --dump-outputs.

CPU: a plain run asks for no event brackets and no CPU baseline whatever the
other options say, --full keeps them as given; dump_outputs writes float64
arrays within its byte cap, a larger array as the same seeded sample every time.
GPU (C1, 100 x 100 grid): a plain run prints the headline fields and leaves the
extra measurements null, and its dumped solution solves the system; --full
fills the extra fields and, run on the same arguments, dumps the same bits.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")


def _parse(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_plain_run_measures_nothing_extra(monkeypatch):
    a = _parse(monkeypatch, ["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert not a.full and a.no_profile and a.cpu_iters == 0 and a.dump_outputs is None
    assert (a.steps, a.warmup) == (5, 2)
    a = _parse(monkeypatch, ["--cpu-iters", "50"])            # --full's options do nothing without it
    assert a.no_profile and a.cpu_iters == 0


def test_full_keeps_the_extra_measurements(monkeypatch):
    a = _parse(monkeypatch, ["--full"])
    assert a.full and not a.no_profile and a.cpu_iters == 120
    a = _parse(monkeypatch, ["--full", "--no-profile", "--cpu-iters", "0", "--dump-outputs", "d"])
    assert a.no_profile and a.cpu_iters == 0 and a.dump_outputs == "d"


def test_dump_outputs_whole_arrays(tmp_path):
    x = np.linspace(0.0, 1.0, 1001)
    bench.dump_outputs(str(tmp_path / "o"), {"x": x, "ports": np.arange(12, dtype=np.float32).reshape(3, 4),
                                             "iters_total": [3, 4]})
    assert sorted(os.listdir(tmp_path / "o")) == ["iters_total.npy", "ports.npy", "x.npy"]
    got = np.load(tmp_path / "o" / "x.npy")
    assert got.dtype == np.float64 and np.array_equal(got, x)
    p = np.load(tmp_path / "o" / "ports.npy")
    assert p.dtype == np.float64 and p.shape == (3, 4)
    assert np.array_equal(np.load(tmp_path / "o" / "iters_total.npy"), [3.0, 4.0])


def test_dump_outputs_samples_within_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CAP", 8 * 1000)
    big = np.arange(5000, dtype=np.float64)
    small = np.arange(10, dtype=np.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert np.array_equal(a, b)                                # the same positions every time
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small)
    assert a.size == 1000 - 10 and a.nbytes + small.nbytes <= 8 * 1000
    assert np.all(np.diff(a) > 0) and set(a) <= set(big)       # ascending, distinct, its own values


def _bench(args):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-u", os.path.join(REPO, "bench.py"), "--gpus", "1", "--grid", "100",
                        "--tol", "1e-10"] + args, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("plain")
    return _bench(["--steps", "2", "--warmup", "1", "--dump-outputs", str(d)]), d


@pytest.fixture(scope="module")
def full(tmp_path_factory):
    d = tmp_path_factory.mktemp("full")
    return _bench(["--full", "--steps", "2", "--warmup", "1", "--cpu-iters", "30", "--dump-outputs", str(d)]), d


@pytest.mark.gpu
def test_plain_run_line(plain):
    r, _ = plain
    for k in HEADLINE:
        assert r[k] is not None, k
    assert (r["steps"], r["warmup"], r["unit"], r["dtype"]) == (2, 1, "iterations/s", "f64")
    assert r["value"] > 0 and r["ms_per_step"] > 0 and r["higher_is_better"] is True
    # value = iterations of the timed steps / their time (both rounded to 3 decimals)
    assert r["value"] == pytest.approx(r["config"]["iters_per_solve"] / (r["ms_per_step"] * 1e-3), rel=1e-2)
    assert r["kernels"] == {} and r["rooflines"] == {} and r["roofline"] is None
    assert r["spmv_isolated"] is None and r["cpu_baseline"] is None and r["cpu_baseline_mt"] is None


@pytest.mark.gpu
def test_dumped_solution_is_the_systems(plain):
    from ggmres import matrices as M
    r, d = plain
    x = np.load(d / "x.npy")
    res = np.load(d / "result.npy")
    assert x.dtype == np.float64 and x.shape == (100 * 100,)
    assert res[0] == 0 and res[2] == r["config"]["iters_per_solve"] and res[4] == r["config"]["relres"]
    # the solve stops on the left-preconditioned residual, M^-1 (b - A x) with M = LU
    # of ILU(0), at 1e-10 of M^-1 b: the true residual is within cond(M) of that, and
    # cond(M) stays below cond(A) = cot^2(pi / 202) = 4.1e3 for this Laplacian
    A = M.laplacian_5pt(100)
    b = M.rhs_ones(A)
    assert np.linalg.norm(b - A @ x) <= 4.2e3 * 1e-10 * np.linalg.norm(b)


@pytest.mark.gpu
def test_full_run_fills_the_extra_fields_and_computes_the_same(plain, full):
    r, d = full
    for k in HEADLINE:
        assert r[k] is not None, k
    assert r["kernels"] and r["rooflines"] and r["roofline"]["kernel"]
    assert r["spmv_isolated"]["avg_us"] > 0
    assert r["cpu_baseline"]["value"] > 0 and r["cpu_baseline_mt"]["value"] > 0
    # the same seeded inputs, the same arithmetic: the two runs' outputs are the same bits
    for name in ("x", "result"):
        assert np.array_equal(np.load(d / (name + ".npy")), np.load(plain[1] / (name + ".npy"))), name
