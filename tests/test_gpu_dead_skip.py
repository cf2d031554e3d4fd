"""The SPHERE dead mask (pixels whose bilateral weight sum is below 1e-6 skip the half-sweep
kernels' long paths) changes no result: planes, costs, selected views and the work counters of a run with the
mask equal those of the same run with ACMMP_DEAD_SKIP=0 bit for bit, NaN payloads included.  (The Philox
counters are not exposed, and a dead pixel's counter shows in no result: none of its draws is ever used.)

The shape is SPHERE 128x512, seed 5: about 62% of its pixels are dead, with all-dead rows, all-live rows and
rows that mix both, so all-dead blocks, all-live blocks and mixed waves occur.  Every case first asserts from
the work counters that the dead fraction lies strictly between 0.3 and 0.9.  One context per case runs the
same state with the knob off and then on (it is read per run).  Tolerance: none."""
import functools

import numpy as np
import pytest

from acmmp import capi, scene, types
from conftest import assert_bitwise_equal

pytestmark = pytest.mark.gpu

W, H = 128, 512


@functools.lru_cache(maxsize=None)
def _scene(kind, w, h, V, seed=5):
    if kind == "pinhole":
        return scene.pinhole_scene(w, h, n_src=V, seed=seed)
    return scene.sphere_scene(w, h, n_src=V, seed=seed)


def _params(sc, **kw):
    c0 = sc.cameras[0]
    return types.default_params(num_images=len(sc.images), depth_min=float(c0["depth_min"]) * 0.6,
                                depth_max=float(c0["depth_max"]) * 1.2, **kw)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _run(ctx, monkeypatch, skip, seed, strips=1, n_half_sweeps=-1, prepare=None):
    monkeypatch.setenv("ACMMP_DEAD_SKIP", "1" if skip else "0")
    monkeypatch.setenv("ACMMP_STRIPS", str(strips))
    if prepare:
        prepare()
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


def _dead_fraction(res):
    evaluated, total = (int(x) for x in res["work"])
    return 1.0 - evaluated / total


def _ab(ctx, monkeypatch, seed, strips=(1,), band=True, **kw):
    """Knob off against knob on for every strip count; returns the knob-off result."""
    want = _run(ctx, monkeypatch, False, seed, **kw)
    frac = _dead_fraction(want)
    print(f"dead fraction {frac:.3f}")
    if band:
        assert 0.3 < frac < 0.9, frac
        assert np.isfinite(want["costs"]).any() and np.isnan(want["costs"]).any()
    else:
        assert frac == 0.0, frac
    for ns in strips:
        got = _run(ctx, monkeypatch, True, seed, strips=ns, **kw)
        _same(got, want, f"mask on, {ns} strip(s), against ACMMP_DEAD_SKIP=0")
    return want


def _ctx(sc, math, **kw):
    ctx = capi.Context(0)
    ctx.set_math(math)
    ctx.set_params(_params(sc, **kw))
    ctx.upload_views(sc.images, sc.cameras)
    return ctx


@pytest.mark.parametrize("math", ["fast", "exact"])
def test_band_view(monkeypatch, math):
    """128x512, V = 4, every half-sweep, one strip and two (the cut at row 256 lies inside the band)."""
    sc = _scene("sphere", W, H, 4)
    with _ctx(sc, math) as ctx:
        _ab(ctx, monkeypatch, 2024, strips=(1, 2))


def test_band_view_against_oracle(monkeypatch, oracle_mod):
    """Exact mode with the mask on against the oracle, bit for bit (NaNs canonicalised: x86 and gfx950 differ in
    their payloads)."""
    sc = _scene("sphere", W, H, 4)
    p = _params(sc)
    with _ctx(sc, "exact") as ctx:
        got = _run(ctx, monkeypatch, True, 4321)
    assert 0.3 < _dead_fraction(got) < 0.9
    ref = oracle_mod.run_patchmatch(oracle_mod.Problem(sc.images, sc.cameras, p), seed=4321)
    for k in ("planes", "costs", "selected_views"):
        assert_bitwise_equal(got[k], ref[k], k)


def test_five_views_spread_off(monkeypatch):
    """V = 5 takes the wide-view instances (k_select's 8-view one, 2-view refinement chunks), with
    ACMMP_SPREAD_MAX=-1 in force."""
    monkeypatch.setenv("ACMMP_SPREAD_MAX", "-1")
    sc = _scene("sphere", W, H, 5)
    with _ctx(sc, "fast") as ctx:
        _ab(ctx, monkeypatch, 7)


@pytest.fixture(scope="module")
def first_pass():
    """A plain pass of the V = 2 view: the state the geom and prior passes start from."""
    sc = _scene("sphere", W, H, 2)
    with _ctx(sc, "fast") as ctx:
        ctx.run_patchmatch(1)
        planes, costs = ctx.download()
    return sc, planes, costs


def test_geom_pass(monkeypatch, first_pass):
    sc, planes, costs = first_pass
    rng = np.random.default_rng(0)
    depths = [planes[..., 3]] + [planes[..., 3] * rng.uniform(0.97, 1.03, (H, W)).astype(np.float32) for _ in range(2)]
    with _ctx(sc, "fast", geom_consistency=1, max_iterations=2) as ctx:
        ctx.upload_depths(depths)
        _ab(ctx, monkeypatch, 2, prepare=lambda: ctx.set_state(planes, costs))


def test_planar_prior_pass(monkeypatch, first_pass):
    """Prior-restricted propagation with the prior's label set over the band (every seventh column keeps the
    plain branch)."""
    sc, planes, costs = first_pass
    rng = np.random.default_rng(2)
    prior = np.zeros((H, W, 4), np.float32)
    prior[..., 2] = -1.0
    prior[..., 3] = rng.uniform(4.0, 6.0, (H, W)).astype(np.float32)
    prior[..., :3] += rng.normal(0, 0.1, (H, W, 3)).astype(np.float32)
    mask = np.ones((H, W), np.uint32)
    mask[:, ::7] = 0
    with _ctx(sc, "fast", planar_prior=1) as ctx:
        ctx.set_planar_prior(prior, mask)
        want = _ab(ctx, monkeypatch, 6, prepare=lambda: ctx.set_state(planes, costs))
    dead = np.isnan(want["costs"])
    assert (mask[dead] > 0).any() and (mask[dead] == 0).any()


def test_hierarchy_pass(monkeypatch):
    """The upsample branch of the initialisation and the hierarchy gate."""
    sc = _scene("sphere", W, H, 2)
    h, w = H // 2, W // 2
    rng = np.random.default_rng(4)
    coarse = np.zeros((h, w, 4), np.float32)
    coarse[..., :3] = rng.normal(0, 0.2, (h, w, 3))
    coarse[..., 2] -= 1.0
    coarse[..., :3] /= np.linalg.norm(coarse[..., :3], axis=-1, keepdims=True)
    coarse[..., 3] = rng.uniform(0.05, 1.5, (h, w))
    cur = np.zeros((H, W, 4), np.float32)
    cur[..., 3] = (sc.gt_depth * rng.uniform(0.95, 1.05, (H, W))).astype(np.float32)
    with _ctx(sc, "fast", hierarchy=1, upsample=1, scaled_cols=w, scaled_rows=h) as ctx:
        ctx.set_scaled_state(coarse)
        _ab(ctx, monkeypatch, 9, prepare=lambda: ctx.set_state(cur))


def test_view_without_band(monkeypatch):
    """128x96 SPHERE has no dead pixel: the mask is all zero (every pixel counted as evaluated), same result."""
    sc = _scene("sphere", 128, 96, 4)
    with _ctx(sc, "fast") as ctx:
        _ab(ctx, monkeypatch, 3, strips=(1, 2), band=False)


def test_pinhole(monkeypatch):
    """Pinhole runs keep no mask."""
    sc = _scene("pinhole", 128, 96, 2)
    with _ctx(sc, "fast") as ctx:
        _ab(ctx, monkeypatch, 3, band=False)


def test_kernel_timing_with_mask(monkeypatch):
    """ACMMP_KERNEL_TIMING=all with the mask on: every bucket is timed and the results are unchanged."""
    sc = _scene("sphere", W, H, 4)
    p = _params(sc)
    n = 2 * int(p["max_iterations"])
    with _ctx(sc, "fast") as ctx:
        monkeypatch.delenv("ACMMP_KERNEL_TIMING", raising=False)
        want = _run(ctx, monkeypatch, False, 11)
        monkeypatch.setenv("ACMMP_KERNEL_TIMING", "all")
        got = _run(ctx, monkeypatch, True, 11, strips=2)
        kt = ctx.last_kernel_timing()
    assert 0.3 < _dead_fraction(want) < 0.9
    for k, (ms, launches) in kt.items():
        assert launches == n and ms > 0.0, (k, ms, launches)
    _same(got, want, "mask on with every bucket timed against ACMMP_DEAD_SKIP=0")
