"""One engine context reused across problems gives what a fresh context gives -- bit for bit.

The context owns every device and pinned buffer it uses (csrc/devbuf.h): the maps sized by the view are
released and reallocated when the size changes, the buffers refilled per call only grow, and a whole-view run
and a band run share one prologue and one epilogue.  None of that may show in a result: every step below is
compared with acmmp_create -> the same step -> acmmp_destroy.  Sizes are the golden fixtures' (SPHERE 80x40,
pinhole 64x48, two source views).  Tolerance: none (NaNs compared as NaN).

The allocation-failure path of upload_views (a resize that runs out of memory partway) is not exercised: it
would take exhausting the device's memory."""
import math

import numpy as np
import pytest

from acmmp import capi, scene, types
from conftest import assert_bitwise_equal

pytestmark = pytest.mark.gpu

SEED = 4321
KEYS = ("planes", "costs", "selected_views", "pre_costs")


def _scene(kind, W, H):
    if kind == "pinhole":
        return scene.pinhole_scene(W, H, n_src=2, seed=W + 2)
    return scene.sphere_scene(W, H, n_src=2, seed=W + 2)


def _params(sc, **kw):
    c0 = sc.cameras[0]
    return types.default_params(num_images=len(sc.images), depth_min=float(c0["depth_min"]) * 0.6,
                                depth_max=float(c0["depth_max"]) * 1.2, **kw)


def _outputs(ctx):
    planes, costs = ctx.download()
    sel, pre = ctx.download_aux()
    return dict(zip(KEYS, (planes, costs, sel, pre)))


def _run(ctx, kind, W, H, upload=True, **kw):
    sc = _scene(kind, W, H)
    ctx.set_params(_params(sc, **kw))
    if upload:
        ctx.upload_views(sc.images, sc.cameras)
    ctx.run_patchmatch(SEED)
    return _outputs(ctx)


def _same(got, want, what):
    for k in KEYS:
        assert_bitwise_equal(got[k], want[k], f"{what}: {k}")


_fresh_runs = {}


def _fresh(kind, W, H, **kw):
    """The step on a context of its own, computed once per module and left unchanged."""
    key = (kind, W, H, tuple(sorted(kw.items())))
    if key not in _fresh_runs:
        with capi.Context(0) as ctx:
            _fresh_runs[key] = _run(ctx, kind, W, H, **kw)
    return _fresh_runs[key]


def test_reuse_equals_fresh():
    """Size and model change, back to a size whose maps and scratch were released, then another patch radius
    (the ray tables are rebuilt)."""
    steps = [("sphere", 80, 40, {}), ("pinhole", 64, 48, {}), ("sphere", 80, 40, {}),
             ("sphere", 80, 40, {"patch_size": 7})]
    with capi.Context(0) as ctx:
        for i, (kind, W, H, kw) in enumerate(steps):
            _same(_run(ctx, kind, W, H, **kw), _fresh(kind, W, H, **kw), f"step {i} ({kind} {W}x{H} {kw})")
    assert not np.array_equal(_fresh("sphere", 80, 40)["planes"], _fresh("sphere", 80, 40, patch_size=7)["planes"])


def test_growth_policies():
    """The grow-only buffers (images, staging, spatial table, scratch) serve a smaller problem after a larger
    one: stale contents beyond the smaller problem's share do not matter."""
    with capi.Context(0) as ctx:
        first = _run(ctx, "sphere", 80, 40)
        second = _run(ctx, "sphere", 160, 80)
        third = _run(ctx, "sphere", 80, 40)
    _same(third, first, "80x40 after 160x80 vs before")
    _same(first, _fresh("sphere", 80, 40), "80x40 vs fresh")
    _same(second, _fresh("sphere", 160, 80), "160x80 vs fresh")


def _planar(ctx, kind, W, H):
    sc = _scene(kind, W, H)
    p = _params(sc)
    ctx.set_params(p)
    ctx.upload_views(sc.images, sc.cameras)
    ctx.run_patchmatch(SEED)
    n = ctx.set_planar_prior_from_state(float(p["depth_min"]), float(p["depth_max"]))
    prior, masks = ctx.download_planar_prior()
    return n, prior, masks


def test_planar_prior_twice():
    """set_planar_prior_from_state at 80x40, then after a new upload_views at 64x48: the triangle tables, their
    pinned staging and its event are reused, the second call waiting for the first one's copy."""
    sizes = [("sphere", 80, 40), ("pinhole", 64, 48)]
    with capi.Context(0) as ctx:
        got = [_planar(ctx, *s) for s in sizes]
    for s, (n, prior, masks) in zip(sizes, got):
        with capi.Context(0) as fresh:
            n_f, prior_f, masks_f = _planar(fresh, *s)
        assert n == n_f and n > 0, (s, n, n_f)
        assert_bitwise_equal(masks, masks_f, f"{s}: masks")
        assert_bitwise_equal(prior, prior_f, f"{s}: prior planes")


def _timing_ok(ctx):
    t = ctx.last_timing()
    assert len(t) == 3 and all(math.isfinite(v) and v >= 0.0 for v in t.values()), t


def test_band_run_after_whole_view_run():
    """A whole-view run, a one-band run over all rows and a whole-view run again, same seed: the shared prologue
    and epilogue leave the double buffers in the same state either way."""
    sc = _scene("sphere", 80, 40)
    with capi.Context(0) as ctx:
        ctx.set_params(_params(sc))
        ctx.upload_views(sc.images, sc.cameras)
        results = []
        for band in (False, True, False):
            if band:
                ctx.band_begin(SEED, 0, 40)
                while ctx.band_sweeps_left():
                    ctx.band_sweep()
                ctx.band_end()
            else:
                ctx.run_patchmatch(SEED)
            _timing_ok(ctx)
            results.append(_outputs(ctx))
    _same(results[1], results[0], "band run vs the whole-view run before it")
    _same(results[2], results[0], "whole-view run after the band run vs before it")
    _same(results[0], _fresh("sphere", 80, 40), "whole-view run vs fresh")


def test_rejected_upload_leaves_a_usable_context():
    sc = _scene("sphere", 80, 40)
    bad = sc.cameras.copy()
    bad["model"][1] = types.PINHOLE
    with capi.Context(0) as ctx:
        first = _run(ctx, "sphere", 80, 40)
        with pytest.raises(capi.AcmmpError, match="mixed camera models"):
            ctx.upload_views(sc.images, bad)
        again = _run(ctx, "sphere", 80, 40)
    _same(again, first, "run after the rejected upload vs before it")
    _same(first, _fresh("sphere", 80, 40), "vs fresh")
