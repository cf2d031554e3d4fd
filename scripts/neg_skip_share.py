#!/usr/bin/env python3
"""Share of (wave, sample) pairs the fast SPHERE k_eval_nb's negligible-sample mask skips on a bench scene
(DESIGN.md §2.4): the float64 restatement of stage_neg_mask (tests/np_neg_skip.py) over every wave of the
reference view -- 8 consecutive pixels of one colour in one row, aligned to the 8 x 4 tile.  CPU only.

  python scripts/neg_skip_share.py [--width 2000 --height 1500 --n-src 4 --seed 1234] [--json OUT] [--nodes]
(the defaults are bench.py's metric scene; bench.py --width 2000 --height 1000 is the other recorded shape)

--nodes adds the count of interpolation nodes a live wave still needs once its masked samples are gone (nodes_needed):
why dropping node rows / columns 0 and 5 with the mask does not pay.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "acmmp-spherical_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import np_neg_skip as ns  # noqa: E402
import np_reference as npr  # noqa: E402
from acmmp import scene, types  # noqa: E402


def all_weights(sc, p):
    """(H, W, 36) float64 bilateral weights of every reference pixel, np_neg_skip.weights vectorised."""
    ref = np.asarray(sc.images[0], np.float64)
    rc = sc.cameras[0]
    H, W = ref.shape
    R, inc = int(p["patch_size"]) // 2, int(p["radius_increment"])
    offs = np.arange(-R, R + 1, inc)
    pad = np.pad(ref, R, mode="edge")
    ys = np.arange(H)[:, None]
    latc = -(ys - rc["params"][2]) / rc["height"] * npr.PI_F
    scx, scy = 2 * npr.PI_F / rc["width"] * np.cos(latc), npr.PI_F / rc["height"]
    sig = float(p["sigma_spatial"]) * npr.PI_F / rc["height"]
    out = np.empty((H, W, len(offs) ** 2))
    k = 0
    for i in offs:
        for j in offs:
            r = pad[R + j:R + j + H, R + i:R + i + W]
            dx, dy = i * scx, j * scy
            out[:, :, k] = np.exp(-np.sqrt(dx * dx + dy * dy) / (2 * sig * sig)
                                  - np.abs(r - ref) / (2 * p["sigma_color"] ** 2))
            k += 1
    return out


NODE, MID = (0, 2, 3, 5), (1, 4)


def nodes_needed(kept):
    """kept: (..., 36) bool, the samples a wave keeps (sample ci * 6 + cj: patch column ci, row cj) -> (..., 4, 4) bool,
    the nodes (columns x rows {0, 2, 3, 5}) its kept samples depend on by ncc_chunk's node-column loop: a node sample
    on itself; rows 1 and 4 of a node column on that column's four nodes; a node row's samples in columns 1 and 4 on
    that row's four nodes; a sample in both an interpolated column and row on all sixteen.  (The four corners are
    read by the spread test whatever is kept; the caller adds them.)"""
    k = kept.reshape(kept.shape[:-1] + (6, 6))
    need = np.zeros(k.shape, bool)
    for a in NODE:
        for b in NODE:
            need[..., a, b] |= k[..., a, b]
    for a in NODE:
        mid = k[..., a, MID[0]] | k[..., a, MID[1]]
        for b in NODE:
            need[..., a, b] |= mid
    for b in NODE:
        mid = k[..., MID[0], b] | k[..., MID[1], b]
        for a in NODE:
            need[..., a, b] |= mid
    both = k[..., MID[0], MID[0]] | k[..., MID[0], MID[1]] | k[..., MID[1], MID[0]] | k[..., MID[1], MID[1]]
    for a in NODE:
        for b in NODE:
            need[..., a, b] |= both
    return need[..., NODE, :][..., :, NODE]


def share(W, H, n_src, seed, nodes=False):
    sc = scene.sphere_scene(W, H, n_src=n_src, seed=seed)
    c0 = sc.cameras[0]
    p = types.default_params(num_images=n_src + 1, depth_min=float(c0["depth_min"]) * 0.6,
                             depth_max=float(c0["depth_max"]) * 1.2)
    w = all_weights(sc, p)
    # spot check against the per-pixel restatement
    for x, y in ((5, 7), (W // 2, H // 5), (W - 3, H - 9)):
        assert np.allclose(w[y, x], ns.weights(sc.images, sc.cameras, p, x, y), rtol=1e-12, atol=0)
    sbw = w.sum(-1)
    live = ~(sbw < 1e-6)
    keep = live[:, :, None] & ~(w <= ns.TAU * sbw[:, :, None])
    Wh = (W + 1) // 2
    waves = live_waves = masked = 0
    hist = np.zeros(37, np.int64)
    rows5 = cols5 = 0
    all16 = node_sum = 0
    for colour in (0, 1):
        for par in (0, 1):                                   # rows with (py + colour) & 1 == par start at px = par
            rows = np.arange(H)[((np.arange(H) + colour) & 1) == par]
            kp = keep[rows][:, par::2]                       # (rows, <= Wh, 36)
            lv = live[rows][:, par::2]
            n = kp.shape[1]
            padn = (-n) % 8
            kp = np.pad(kp, ((0, 0), (0, padn), (0, 0)))
            lv = np.pad(lv, ((0, 0), (0, padn)))
            kw = kp.reshape(len(rows), -1, 8, 36).any(2)     # a sample kept by any live pixel of the wave
            lw = lv.reshape(len(rows), -1, 8).any(2)
            m = (~kw)[lw]                                    # masked samples of the waves with a live pixel
            waves += lw.size
            live_waves += int(lw.sum())
            masked += int(m.sum())
            hist += np.bincount(m.sum(-1), minlength=37)
            j5 = np.array([k % 6 in (0, 5) for k in range(36)])
            i5 = np.array([k // 6 in (0, 5) for k in range(36)])
            rows5 += int(m[:, j5].all(-1).sum())
            cols5 += int(m[:, i5].all(-1).sum())
            if nodes:
                nd = nodes_needed(~m)                        # (live waves, 4, 4)
                node_sum += int(nd.sum())
                nd[:, ::3, ::3] = True                       # the corners stay for the spread test
                all16 += int(nd.all((-1, -2)).sum())
    assert Wh >= n
    extra = {"live_waves_needing_all_16_nodes": round(all16 / live_waves, 4),
             "mean_nodes_needed_without_the_corner_rule": round(node_sum / live_waves, 2)} if nodes else {}
    return {**extra, "width": W, "height": H, "n_src": n_src, "seed": seed, "tau": ns.TAU, "waves": waves,
            "live_waves": live_waves, "live_wave_share": round(live_waves / waves, 4),
            "masked_pair_share_of_live_waves": round(masked / (36.0 * live_waves), 4),
            "mean_masked_samples_per_live_wave": round(masked / live_waves, 2),
            "live_waves_with_all_|j|=5_masked": round(rows5 / live_waves, 4),
            "live_waves_with_all_|i|=5_masked": round(cols5 / live_waves, 4),
            "masked_count_quantiles_10_50_90": [int(np.searchsorted(np.cumsum(hist), q * live_waves)) for q in (0.1, 0.5, 0.9)]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=2000)
    ap.add_argument("--height", type=int, default=1500)
    ap.add_argument("--n-src", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--json", default=None)
    ap.add_argument("--nodes", action="store_true", help="also count the interpolation nodes the live waves still need")
    a = ap.parse_args()
    out = share(a.width, a.height, a.n_src, a.seed, nodes=a.nodes)
    print(json.dumps(out))
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)
