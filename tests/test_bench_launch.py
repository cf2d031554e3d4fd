"""bench.py --gpus N launches its own ranks (CPU; no GPU touched).

The driver runs `python bench.py --gpus N` for the N=1 line and, for the scaling curve, either the same
command or a torch.distributed.run launch of it.  Run directly with N > 1, bench.py starts N gloo ranks
itself (torch.distributed.run child, rendezvous on 127.0.0.1); `--dry-run` stops every rank right after
the rendezvous, so the plumbing is checked without a device.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args, env=None, timeout=240):
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                          timeout=timeout, env=e, cwd=ROOT)


def _json_line(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def test_gpus2_spawns_two_gloo_ranks():
    r = _bench("--gpus", "2", "--dry-run")
    assert r.returncode == 0, r.stderr[-2000:]
    line = _json_line(r.stdout)
    assert line["ranks"] == 2 and line["rank_ids"] == [0, 1]
    assert line["processes"] == 2 and line["backend"] == "gloo" and line["gpus"] == 2


def test_gpus3_pipeline_mode_spawns_three_ranks():
    r = _bench("--gpus", "3", "--mode", "pipeline", "--dry-run")
    assert r.returncode == 0, r.stderr[-2000:]
    assert _json_line(r.stdout)["rank_ids"] == [0, 1, 2]


def test_gpus1_dry_run_single_process():
    r = _bench("--dry-run")
    assert r.returncode == 0, r.stderr[-2000:]
    line = _json_line(r.stdout)
    assert line["ranks"] == 1 and line["backend"] is None


def test_refuses_more_ranks_than_gpus():
    # this container has no GPU: asking for 2 must fail loudly, not run one rank and report it as 2
    r = _bench("--gpus", "2", "--steps", "1", "--warmup", "0")
    assert r.returncode == 2
    assert "refusing" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_launcher_world_mismatch_is_an_error():
    r = _bench("--gpus", "4", "--dry-run", env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "launcher started 1" in r.stderr


def test_abandoned_extra_exits_nonzero():
    """A guarded extra abandoned at its deadline (a hung first RCCL run) prints the line with the error and
    then exits non-zero on every rank, so the driver does not read the hang as success."""
    r = _bench("--gpus", "2", "--dry-run", env={"ACMMP_BENCH_SELFTEST_ABANDON": "1"})
    assert r.returncode != 0, r.stderr[-2000:]
    line = _json_line(r.stdout)
    assert line["ranks"] == 2 and "abandoned" in line["extra"]["error"]
    r1 = _bench("--dry-run", env={"ACMMP_BENCH_SELFTEST_ABANDON": "1"})
    assert r1.returncode == 3


def test_visible_gpus_counts_without_hip():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n = bench.visible_gpus()
    assert n >= 0
    os.environ["HIP_VISIBLE_DEVICES"] = ""
    try:
        assert bench.visible_gpus() == 0
    finally:
        del os.environ["HIP_VISIBLE_DEVICES"]
    assert "torch" not in bench.visible_gpus.__code__.co_names


def _bench_mod():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_plain_run_has_no_side_measurements(monkeypatch):
    """Without --full every leg that takes runs of its own is off; --full turns them on, and the --no-* options
    and --timed-only still switch them off there."""
    bench = _bench_mod()
    legs = ("no_other_mode", "no_cpu_baseline", "no_variant", "no_pipeline", "no_clock")

    def parse(*argv):
        monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
        return bench.parse()
    a = parse("--gpus", "1", "--steps", "3", "--warmup", "1")
    assert a.steps == 3 and a.warmup == 1 and not a.full and not a.extras and a.dump_outputs is None
    assert all(getattr(a, k) for k in legs)
    a = parse("--full")
    assert a.extras and not any(getattr(a, k) for k in legs)
    a = parse("--full", "--no-variant", "--no-clock")
    assert a.extras and a.no_variant and a.no_clock and not a.no_other_mode and not a.no_cpu_baseline
    a = parse("--full", "--timed-only")
    assert not a.extras and all(getattr(a, k) for k in legs[:4]) and not a.no_clock


def test_dump_outputs_files_and_budget(tmp_path):
    """--dump-outputs writes float32 planes / costs; above the byte budget a fixed pixel sample of both."""
    import numpy as np
    bench = _bench_mod()
    rng = np.random.default_rng(3)
    planes = rng.standard_normal((30, 50, 4)).astype(np.float32)
    costs = rng.standard_normal((30, 50)).astype(np.float32)
    costs[3, 7], costs[4, 8], planes[5, 6, 3] = np.nan, np.inf, np.nan
    bench.dump_outputs(str(tmp_path / "a"), planes, costs, 0, 1)
    assert sorted(os.listdir(tmp_path / "a")) == ["costs.npy", "planes.npy"]
    p, c = np.load(tmp_path / "a" / "planes.npy"), np.load(tmp_path / "a" / "costs.npy")
    assert p.dtype == np.float32 and c.dtype == np.float32
    # finite numbers only: a non-finite cost is written as -1, a non-finite plane component as 0
    assert np.isfinite(p).all() and np.isfinite(c).all()
    assert c[3, 7] == -1.0 and c[4, 8] == -1.0 and p[5, 6, 3] == 0.0
    ok_p, ok_c = np.isfinite(planes), np.isfinite(costs)
    assert np.array_equal(p[ok_p], planes[ok_p]) and np.array_equal(c[ok_c], costs[ok_c])
    # over budget: 400 pixels of 20 bytes each fit 8000 bytes; the same pixels in both files and in every run
    costs = np.arange(1500, dtype=np.float32).reshape(30, 50)      # a pixel's cost = its flat index
    planes[5, 6, 3] = 0.0
    old = bench.DUMP_BUDGET_BYTES
    bench.DUMP_BUDGET_BYTES = 8000
    try:
        bench.dump_outputs(str(tmp_path / "b"), planes, costs, 0, 1)
        bench.dump_outputs(str(tmp_path / "c"), planes, costs, 0, 1)
        bench.dump_outputs(str(tmp_path / "d"), planes, costs, 1, 2)
    finally:
        bench.DUMP_BUDGET_BYTES = old
    p, c = np.load(tmp_path / "b" / "planes.npy"), np.load(tmp_path / "b" / "costs.npy")
    assert p.shape == (400, 4) and c.shape == (400,) and p.nbytes + c.nbytes <= 8000
    idx = c.astype(np.int64)
    assert np.all(np.diff(idx) > 0) and np.array_equal(p, planes.reshape(-1, 4)[idx])
    assert np.array_equal(p, np.load(tmp_path / "c" / "planes.npy"))
    assert sorted(os.listdir(tmp_path / "d")) == ["costs_rank1.npy", "planes_rank1.npy"]
    assert np.load(tmp_path / "d" / "costs_rank1.npy").shape == (200,)


def test_multi_rank_extras_are_guarded():
    """The first runs of the RCCL extras (depth_exchange, band_split) cannot cost the headline line: an
    exception is reported in the line, and a hang is abandoned at the deadline."""
    import importlib.util
    import time
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)

    def boom():
        raise RuntimeError("rccl said no")
    r, abandoned = bench.guarded(boom, 5)
    assert not abandoned and "rccl said no" in r["error"]
    r, abandoned = bench.guarded(lambda x: {"ok": x}, 5, 7)
    assert r == {"ok": 7} and not abandoned
    t0 = time.perf_counter()
    r, abandoned = bench.guarded(time.sleep, 0.5, 30)
    assert abandoned and "abandoned" in r["error"] and time.perf_counter() - t0 < 5
