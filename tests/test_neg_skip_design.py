"""The design behind the fast SPHERE k_eval_nb's negligible-sample mask, CPU, float64.

The threshold.  A masked sample has w_k <= tau * sbw in every live pixel of its wave, so a pixel drops at most
36 tau of its weight sum.  Texels are at most 255, so the drop moves m_src = sum w s / sbw by at most 255 * 36 tau
and e_ss, e_rs by at most 255^2 * 36 tau -- in units of the sums' own scale (255, 255^2) that is 36 tau.  One
binary32 rounding of such a sum moves it by up to 2^-24 of its scale, and the fast mode's sums carry 36 of them.
tau = 2^-35 makes 36 tau = 2^-29.8: 1/57 of a single rounding.  The study below holds the interpolated-and-masked
NCC (np_neg_skip.masked_ncc) against the projected one (np_interp.ncc, every sample projected) on the pole, seam
and random query sets of test_interp_design.py at 2000x1000, 2000x1500 and 3200x1600: inside the 1e-4 the
existing gates are built on, and within the 36 tau bound propagated through the NCC (np_neg_skip.on_off_bound
without rounding) of the unmasked interpolated NCC, query by query.
"""
import numpy as np
import pytest

import np_interp as ni
import np_neg_skip as ns
import np_reference as npr
from acmmp import scene, types

TAU = ns.TAU


def test_tau_is_below_one_binary32_rounding_with_margin():
    assert 36 * TAU * 32 <= 2.0 ** -24          # the dropped mass: at least 32 times below one rounding of a sum
    assert 255 * 36 * TAU < 255 * 2.0 ** -24 / 32 and 255 ** 2 * 36 * TAU < 255 ** 2 * 2.0 ** -24 / 32


def test_mask_rule_properties():
    rng = np.random.default_rng(5)
    for trial in range(200):
        # weights spanning many binary orders, as the sigma-in-radians spatial term makes them
        w = np.exp(-rng.uniform(0, 60, (8, 36)))
        w[rng.integers(0, 8)] *= 1e-12 if trial % 3 == 0 else 1.0        # a pixel below the 1e-6 patch sum
        dead = rng.random(8) < 0.25
        m = ns.wave_mask(w, dead)
        sbw = w.sum(-1)
        live = ~dead & ~(sbw < 1e-6)
        # the dropped mass of every live pixel is at most 36 tau of its patch sum
        assert np.all((w * m).sum(-1)[live] <= 36 * TAU * sbw[live])
        # dead pixels (and ones below the patch-sum floor) never enter: their weights may be anything
        w2 = w.copy()
        w2[~live] = rng.random((int((~live).sum()), 36)) * (1e-9 if trial % 2 else 1.0)
        dead2 = dead | ~live
        assert np.array_equal(ns.wave_mask(w2, dead2), ns.wave_mask(w, dead2))
        # a sample that matters in one live pixel is kept for the whole wave
        if live.any():
            big = (w[live] > TAU * sbw[live, None]).any(0)
            assert not np.any(m & big)
    assert not ns.wave_mask(w, dead, tau=-1.0).any()


def _study(W, H, n_src, seed, n_each):
    sc = scene.sphere_scene(W, H, n_src=n_src, seed=seed)
    c0 = sc.cameras[0]
    p = types.default_params(num_images=len(sc.images), depth_min=float(c0["depth_min"]) * 0.6,
                             depth_max=float(c0["depth_max"]) * 1.2)
    assert ni.interp_enabled(W, H, p)
    rng = np.random.default_rng(seed + 1)
    worst_proj = worst_unmasked = worst_ratio = 0.0
    n = n_masked = n_small = 0
    for kind in ("pole", "seam", "random"):
        px, py, src = ni.special_pixels(sc, kind, n_each, seed=seed + 2)
        assert len(px) >= n_each // 2, kind
        planes = ni.near_surface_planes(sc, px, py, 1, seed=seed + 3)
        for q in range(len(px)):
            x, y, v = int(px[q]), int(py[q]), int(src[q])
            wave = ns.wave_pixels(x, y)
            wts = np.stack([ns.weights(sc.images, sc.cameras, p, min(max(a, 0), W - 1), b) for a, b in wave])
            mask = ns.wave_mask(wts)
            d = npr.pixel_to_dir(c0, x, y)
            nrm = rng.normal(0, 1, 3)
            nrm = -nrm if nrm @ d > 0 else nrm
            nrm /= np.linalg.norm(nrm)
            depth = 1.0 / rng.uniform(1.0 / float(p["depth_max"]), 1.0 / float(p["depth_min"]))
            for plane in (planes[q, 0].astype(np.float64), np.array([*nrm, -float(nrm @ (d * depth))])):
                e = ni.ncc(sc.images, sc.cameras, p, v, x, y, plane, False)[0]
                f, _ = ns.masked_ncc(sc.images, sc.cameras, p, v, x, y, plane, mask)
                g, _, t = ns.masked_ncc(sc.images, sc.cameras, p, v, x, y, plane, np.zeros(36, bool), terms=True)
                # an all-clear mask is the unmasked interpolated NCC of np_interp
                u = ni.ncc(sc.images, sc.cameras, p, v, x, y, plane, True, nodes=ni.nodes_for(p), span_max=ni.SPREAD_MAX)[0]
                assert g == pytest.approx(u, abs=1e-12)
                assert (e >= 2.0) == (f >= 2.0)
                if e < 2.0:
                    worst_proj = max(worst_proj, abs(f - e))
                    worst_unmasked = max(worst_unmasked, abs(f - g))
                    # no rounding here: the masked NCC lies within the 36 tau bound propagated through the NCC
                    # -- with the patch's own dropped share of the weight sum in place of its cap, 36 tau
                    own = float((wts[wave.index((x, y))] * mask).sum() / wts[wave.index((x, y))].sum())
                    assert own <= 36 * TAU
                    bound = ns.on_off_bound(t, spacings=0, drop=own)
                    if bound is None:
                        n_small += 1
                    else:
                        worst_ratio = max(worst_ratio, abs(f - g) / bound)
                        assert abs(f - g) <= bound, (W, H, kind, q, abs(f - g), bound)
                    n += 1
                    n_masked += int(mask.sum())
    return worst_proj, worst_unmasked, n, n_masked, worst_ratio, n_small


@pytest.mark.parametrize("W,H,n_src", [(2000, 1000, 2), (2000, 1500, 3), (3200, 1600, 2)])
def test_masked_interpolated_ncc_within_noise_floor(W, H, n_src):
    worst_proj, worst_unmasked, n, n_masked, worst_ratio, n_small = _study(W, H, n_src, seed=5, n_each=12)
    print(f"{W}x{H}: {n} live queries, {n_masked / max(n, 1):.1f} of 36 samples masked on average, "
          f"worst |masked - projected| {worst_proj:.3g}, worst |masked - unmasked| {worst_unmasked:.3g} "
          f"({worst_ratio:.3g} of the bound from its own dropped mass; {n_small} queries with too small a variance for it)")
    assert n >= 20 and n_masked > 0 and n_small <= 0.02 * n
    assert worst_proj < 1e-4, worst_proj
