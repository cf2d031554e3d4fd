"""The strip schedule of RunPatchMatch (ACMMP_STRIPS strips of rows over ACMMP_STRIP_STREAMS
streams, each strip's half-sweep behind the previous half-sweep of its neighbours) changes no result: planes,
costs, selected views and the work counters of a run with strips equal the single-strip run's bit for bit, and
a second run with the same settings equals the first (a missing wait shows as a difference between runs).

One context per case runs the same uploaded views and seed with ACMMP_STRIPS=1 and then with the strip setting
(both knobs are read per run).  Tolerance: none; the bits are compared through view(np.uint32)."""
import numpy as np
import pytest

from acmmp import capi, scene, types

pytestmark = pytest.mark.gpu


def _params(sc, **kw):
    c0 = sc.cameras[0]
    return types.default_params(num_images=len(sc.images), depth_min=float(c0["depth_min"]) * 0.6,
                                depth_max=float(c0["depth_max"]) * 1.2, **kw)


def _scene(kind, W, H, V, seed):
    if kind == "pinhole":
        return scene.pinhole_scene(W, H, n_src=V, seed=seed)
    return scene.sphere_scene(W, H, n_src=V, seed=seed)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _run(ctx, monkeypatch, strips, streams, seed, n_half_sweeps=-1):
    monkeypatch.setenv("ACMMP_STRIPS", str(strips))
    if streams is None:
        monkeypatch.delenv("ACMMP_STRIP_STREAMS", raising=False)
    else:
        monkeypatch.setenv("ACMMP_STRIP_STREAMS", str(streams))
    ctx.run_patchmatch(seed, n_half_sweeps=n_half_sweeps)
    planes, costs = ctx.download()
    sel, _ = ctx.download_aux()
    return {"planes": planes, "costs": costs, "selected_views": sel, "work": np.array(ctx.last_work(), np.uint64)}


def _same(got, want, what):
    for name in want:
        g, w = _bits(got[name]), _bits(want[name])
        assert g.shape == w.shape, (what, name)
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: {name}: {len(bad)} of {g.size} words differ, first at {bad[:5].tolist()}"


def _compare(monkeypatch, kind, W, H, V, math, settings, seed=2024, n_half_sweeps=-1, env=None):
    sc = _scene(kind, W, H, V, seed=W + H + V)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    with capi.Context(0) as ctx:
        ctx.set_math(math)
        ctx.set_params(_params(sc))
        ctx.upload_views(sc.images, sc.cameras)
        want = _run(ctx, monkeypatch, 1, None, seed, n_half_sweeps)
        assert np.isfinite(want["costs"]).any()
        for strips, streams in settings:
            first = _run(ctx, monkeypatch, strips, streams, seed, n_half_sweeps)
            _same(first, want, f"strips {strips} / streams {streams} against one strip")
            again = _run(ctx, monkeypatch, strips, streams, seed, n_half_sweeps)
            _same(again, first, f"strips {strips} / streams {streams}, second run against the first")


@pytest.mark.parametrize("math", ["fast", "exact"])
def test_basic_schedule(monkeypatch, math):
    """128x96: 96 checkerboard rows, 4 strips of 24 rows (the minimum height) on 4 streams, 2 of 48 on 2, and
    4 on 2 streams: strips 0 and 2 (1 and 3) share a stream, which orders them in place of an event wait."""
    assert capi.strip_plan(96, 4)[0] == [0, 24, 48, 72, 96]
    _compare(monkeypatch, "sphere", 128, 96, 4, math, [(4, 4), (2, 2), (4, 2)])


def test_uneven_strips(monkeypatch):
    """128x100: 100 rows in 3 strips of 36, 32 and 32 rows (25 units of 4 rows do not divide by 3)."""
    assert capi.strip_plan(100, 3)[0] == [0, 36, 68, 100]
    _compare(monkeypatch, "sphere", 128, 100, 4, "fast", [(3, None)])


def test_five_views_spread_off(monkeypatch):
    """V = 5 takes the wide-view kernels (k_select's 8-view instance, 2-view refinement chunks), with
    ACMMP_SPREAD_MAX=-1 in force.  (A view of this size does not interpolate sample coordinates -- that starts
    at 2000x1000 -- so its fallback queue stays empty; test_fallback_queue_slices runs one that does.  A view that
    interpolates with V > 4 runs as one strip whatever the knob says)"""
    _compare(monkeypatch, "sphere", 128, 96, 5, "fast", [(4, None)], env={"ACMMP_SPREAD_MAX": "-1"})


@pytest.mark.parametrize("math", ["fast", "exact"])
def test_pinhole(monkeypatch, math):
    """The pinhole path.  Fast pinhole runs stay one strip whatever the knob says (their low bits depend on
    which pixels share a wave): the fast case pins that the knob is harmless there, and the exact
    mode is the one that runs pinhole kernels on strips."""
    _compare(monkeypatch, "pinhole", 128, 96, 2, math, [(4, None)])


def test_strip_count_is_clamped(monkeypatch):
    """64 strips asked of 96 rows: clamped to 4; the run succeeds and equals the single-strip run."""
    assert len(capi.strip_plan(96, 64)[0]) == 5
    _compare(monkeypatch, "sphere", 128, 96, 4, "fast", [(64, None)])


def test_fallback_queue_slices(monkeypatch):
    """The smallest view whose fast SPHERE kernels interpolate sample coordinates (2000x1000), V = 4 and
    ACMMP_SPREAD_MAX=-1: every entry of k_eval_nb is deferred to the fallback queue, so each strip's queue slice
    and its capacity are used to the full (an overflow fails the run).  Three half-sweeps: every kind of
    cross-strip wait occurs once.  (The refinement's own fallbacks need V > 4, which runs as one strip.)"""
    _compare(monkeypatch, "sphere", 2000, 1000, 4, "fast", [(4, None)], n_half_sweeps=3,
             env={"ACMMP_SPREAD_MAX": "-1"})


@pytest.mark.parametrize("V", [3, 4])
def test_interpolated_views_default_spread(monkeypatch, V):
    """Fast SPHERE at 2000x1000 with the default spread threshold, every half-sweep: k_eval_nb's interpolated
    costs and its per-sample fallbacks both reach the result, and the refinement's tail evaluates the union of a
    wave's selected views while the grouping into waves and 51-pixel blocks shifts with every strip start -- up
    to V = 4 every cost the refinement caches is per-sample arithmetic whichever kernel forms it, so no bit moves.
    2 strips (the default from 2 Mpixel), 4, and 8 on 4 streams (two strips per stream)."""
    _compare(monkeypatch, "sphere", 2000, 1000, V, "fast", [(2, None), (4, None), (8, 4)])


def test_kernel_timing_with_strips(monkeypatch):
    """ACMMP_KERNEL_TIMING=all with 4 strips: each bucket sums the strips' intervals, its launch count stays
    the number of half-sweeps, and the results are unchanged."""
    sc = _scene("sphere", 128, 96, 4, seed=5)
    p = _params(sc)
    n = 2 * int(p["max_iterations"])
    with capi.Context(0) as ctx:
        ctx.set_math("fast")
        ctx.set_params(p)
        ctx.upload_views(sc.images, sc.cameras)
        monkeypatch.delenv("ACMMP_KERNEL_TIMING", raising=False)
        want = _run(ctx, monkeypatch, 1, None, 11)
        monkeypatch.setenv("ACMMP_KERNEL_TIMING", "all")
        got = _run(ctx, monkeypatch, 4, 4, 11)
        kt = ctx.last_kernel_timing()
    for k, (ms, launches) in kt.items():
        assert launches == n and ms > 0.0, (k, ms, launches)
    _same(got, want, "4 strips with every bucket timed against one strip")
