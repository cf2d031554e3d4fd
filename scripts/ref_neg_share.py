#!/usr/bin/env python3
"""Share of the sample steps the per-pixel negligible-sample mask of the fast SPHERE refinement skips on a bench
scene (ncc_chunk's PNEG instances).  Bit s of a live pixel's mask is set iff w_s <= tau x its patch
sum; a wave skips a sample's body when every live pixel it holds has the bit set.  In float64, over every pixel of
the reference view (every colour pixel is a refinement candidate's; which of them survive to the tail depends on
the run, so the tail's figure is the per-pixel upper bound):
  * k_eval_ref's grouping: blocks of kRefPix = 51 consecutive colour pixels x kRefLanes = 5 lanes, 64-lane waves
    (lane t of a block holds pixel t // 5);
  * 64 consecutive pixels of a row (one lane per pixel);
  * per pixel (the upper bound: a wave of pixels with equal masks).
CPU only.

  python scripts/ref_neg_share.py [--width 2000 --height 1500 --n-src 4 --seed 1234] [--json OUT]
"""
import argparse
import json

import numpy as np

import neg_skip_share as nss
from neg_skip_share import ns, scene, types

K_REF_PIX, K_REF_LANES = 51, 5


def share(W, H, n_src, seed):
    sc = scene.sphere_scene(W, H, n_src=n_src, seed=seed)
    c0 = sc.cameras[0]
    p = types.default_params(num_images=n_src + 1, depth_min=float(c0["depth_min"]) * 0.6,
                             depth_max=float(c0["depth_max"]) * 1.2)
    w = nss.all_weights(sc, p)
    sbw = w.sum(-1)
    live = ~(sbw < 1e-6)
    neg = live[:, :, None] & (w <= ns.TAU * sbw[:, :, None])     # a live pixel's mask
    out = {"width": W, "height": H, "n_src": n_src, "seed": seed, "tau": ns.TAU,
           "live_pixel_share": round(float(live.mean()), 4),
           "per_pixel_masked_share": round(float(neg[live].mean()), 4),
           "per_pixel_mean_masked_of_36": round(float(neg[live].sum(-1).mean()), 2)}
    # 64 consecutive pixels of a row
    padn = (-W) % 64
    lv = np.pad(live, ((0, 0), (0, padn))).reshape(H, -1, 64)
    skip = np.pad(neg | ~live[:, :, None], ((0, 0), (0, padn), (0, 0)), constant_values=True).reshape(H, -1, 64, 36).all(2)
    lw = lv.any(2)
    out["row64_live_wave_share"] = round(float(lw.mean()), 4)
    out["row64_skipped_pair_share"] = round(float(skip[lw].mean()), 4)
    # k_eval_ref: the colour grid's pixels in row-major order, 51 per block, lane t -> pixel t // 5, waves of 64 lanes
    lane_pix = np.arange(K_REF_PIX * K_REF_LANES) // K_REF_LANES
    wave_of = [np.unique(lane_pix[k:k + 64]) for k in range(0, K_REF_PIX * K_REF_LANES, 64)]
    tot = skipped = live_w = waves = 0
    for colour in (0, 1):
        ys, xs = np.nonzero((np.add.outer(np.arange(H), np.arange(W)) & 1) == colour)
        order = np.lexsort((xs, ys))
        n_, l_ = neg[ys[order], xs[order]], live[ys[order], xs[order]]
        padb = (-len(l_)) % K_REF_PIX
        n_ = np.pad(n_, ((0, padb), (0, 0))).reshape(-1, K_REF_PIX, 36)
        l_ = np.pad(l_, (0, padb)).reshape(-1, K_REF_PIX)
        for pix in wave_of:
            lw_ = l_[:, pix].any(1)
            sk = (n_[:, pix] | ~l_[:, pix][:, :, None]).all(1)[lw_]
            waves += len(lw_)
            live_w += int(lw_.sum())
            skipped += int(sk.sum())
            tot += sk.size
    out["ref_live_wave_share"] = round(live_w / waves, 4)
    out["ref_skipped_pair_share"] = round(skipped / tot, 4)
    out["ref_mean_skipped_of_36"] = round(36.0 * skipped / tot, 2)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=2000)
    ap.add_argument("--height", type=int, default=1500)
    ap.add_argument("--n-src", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = share(a.width, a.height, a.n_src, a.seed)
    print(json.dumps(res))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)
