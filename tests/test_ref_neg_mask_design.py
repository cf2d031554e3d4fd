"""The design behind the per-pixel negligible-sample mask of the fast SPHERE refinement, CPU, float64.

A pixel drops the samples with w_k <= tau * sbw, so at most 36 tau of its weight sum; tau = 2^-35 makes that 2^-29.8,
1/57 of one binary32 rounding of a sum (test_neg_skip_design.py holds the arithmetic of that).  Here, on the pole,
seam and random query sets and on rows at the edges of the dead band, at 2000x1000 V = 2 and 2000x1500 V = 4 (the
shapes of tests/test_gpu_ref_neg_skip.py): every pixel's dropped share is at most 36 tau; every query's masked
per-sample NCC lies within the bound propagated from its own dropped share (np_neg_skip.on_off_bound with binary64's
spacing per operation) of the unmasked one; and the cost class is the same.  The sets hold at least MIN_LIVE live queries each.

The per-query sets the GPU test runs (np_ref_neg_skip.hook_queries, the entries of float64_study) are held here too:
they have at least MIN_HOOK_LIVE live entries per shape, the large threshold (test_gpu_neg_skip.BIG_TAU) moves at least a
tenth of them by more than 1e-3, and the share the restatement itself excludes from the on / off bound -- a cost of 2.0,
or a source variance too small for the bound's first-order form -- is printed; the second is at most 2%.
"""
import numpy as np
import pytest

import np_interp as ni
import np_neg_skip as ns
import np_ref_neg_skip as rn
from acmmp import scene, types

MIN_LIVE = 40                   # live (cost below 2.0) queries per shape the study must see
MIN_HOOK_LIVE = 100             # live entries of the GPU test's sets per shape (test_gpu_ref_neg_skip.py needs 100)


def test_pixel_mask_rule():
    rng = np.random.default_rng(7)
    for trial in range(200):
        w = np.exp(-rng.uniform(0, 60, 36))
        m = rn.pixel_mask(w)
        assert (w * m).sum() <= 36 * rn.TAU * w.sum()
        assert not np.any(m & (w > rn.TAU * w.sum()))
    assert not rn.pixel_mask(w * 1e-12).any()                   # below the patch-sum floor: no mask (nothing evaluated)
    assert not rn.pixel_mask(w, tau=-1.0).any()
    assert rn.pixel_mask(w, tau=1.0).all()


@pytest.mark.parametrize("W,H,n_src,seed", [(2000, 1000, 2, 77), (2000, 1500, 4, 1234)])
def test_masked_per_sample_ncc_within_its_bound(W, H, n_src, seed):
    sc = scene.sphere_scene(W, H, n_src=n_src, seed=seed, n_waves=16)
    c0 = sc.cameras[0]
    p = types.default_params(num_images=len(sc.images), depth_min=float(c0["depth_min"]) * 0.6,
                             depth_max=float(c0["depth_max"]) * 1.2)
    rng = np.random.default_rng(seed + 1)
    xs, ys = [], []
    for kind in ("pole", "seam", "random"):
        px, py, _ = ni.special_pixels(sc, kind, 10, seed=seed + 2)
        xs.append(px)
        ys.append(py)
    # rows around the dead band's edges (|latitude| 38 .. 50 degrees)
    for s in (-1, 1):
        for d in (38, 41, 44, 47, 50):
            xs.append(rng.integers(8, W - 8, 2))
            ys.append(np.full(2, int(H * (0.5 + s * d / 180.0))))
    px, py = np.concatenate(xs).astype(int), np.concatenate(ys).astype(int)
    planes = ni.near_surface_planes(sc, px, py, 1, seed=seed + 3)
    none = np.zeros(36, bool)
    n = n_live = n_small = n_masked = 0
    worst = worst_ratio = 0.0
    for q in range(len(px)):
        x, y = int(px[q]), int(py[q])
        w = ns.weights(sc.images, sc.cameras, p, x, y)
        mask = rn.pixel_mask(w)
        own = float((w * mask).sum() / w.sum())
        assert own <= 36 * rn.TAU
        for v in range(1, n_src + 1):
            a = (sc.images, sc.cameras, p, v, x, y, planes[q, 0].astype(np.float64))
            f = rn.masked_ncc(*a, mask)
            g, t = rn.masked_ncc(*a, none, terms=True)
            n += 1
            assert (f >= 2.0) == (g >= 2.0), (x, y, v, f, g)
            if t is None:
                continue
            n_live += 1
            n_masked += int(mask.sum())
            # the restatement's own arithmetic is binary64: one binary64 spacing (2^-52 = 2^-29 binary32 spacings) per
            # operation beside the dropped share, which at 1500 rows is often smaller than that (4e-13 of a cost)
            bound = ns.on_off_bound(t, spacings=2.0 ** -29, drop=own)
            if bound is None:
                n_small += 1
                continue
            worst = max(worst, abs(f - g))
            worst_ratio = max(worst_ratio, abs(f - g) / bound)
            assert abs(f - g) <= bound, (x, y, v, abs(f - g), bound)
    print(f"{W}x{H}: {n} queries, {n_live} live, {n_masked / max(n_live, 1):.1f} of 36 samples masked on average, worst "
          f"|masked - unmasked| {worst:.3g} ({worst_ratio:.3g} of its bound); {n_small} with too small a variance for it")
    assert n_live >= MIN_LIVE, n_live
    assert n_masked > 0 and n_small <= 0.02 * n_live


@pytest.mark.parametrize("name", ["2000x1000-v2", "2000x1500-v4"])
def test_gpu_query_sets_have_enough_live_queries(name):
    from test_gpu_neg_skip import BIG_TAU, SHAPES, _params
    W, H, V, seed = SHAPES[name]
    sc = scene.sphere_scene(W, H, n_src=V, seed=seed, n_waves=16)
    p = _params(sc)
    px, py, planes = rn.hook_queries(sc, W, H)
    study = rn.float64_study(sc, p, px, py, planes, BIG_TAU[H])
    n = len(study)
    live = [e for e in study if e[4] is not None]
    n_small = sum(ns.on_off_bound(e[4], drop=e[7]) is None for e in live)
    moves = np.mean([abs(e[6] - e[3]) > 1e-3 for e in live])
    print(f"{name}: {n} entries, {len(live)} live ({1 - len(live) / n:.3f} excluded as cost 2.0), {n_small / n:.4f} with "
          f"too small a variance for the bound; the large threshold moves {moves:.3f} of the live ones by more than 1e-3")
    assert len(live) >= MIN_HOOK_LIVE, len(live)
    assert n_small / n <= 0.02
    assert moves >= 0.1, moves
    for e in live:                                              # the class and the dropped share, on these sets too
        assert e[7] <= 36 * rn.TAU and e[5] < 2.0
