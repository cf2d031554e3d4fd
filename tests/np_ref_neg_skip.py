"""Float64 restatement of the per-pixel negligible-sample mask of the fast SPHERE refinement (DESIGN.md §2.4;
ncc_chunk's PNEG instances) over the per-sample NCC of np_reference.  Test infrastructure beside np_neg_skip.py (no
GPU): tests/test_ref_neg_mask_design.py and tests/test_gpu_ref_neg_skip.py import it.

The rule: for a live pixel (bilateral weight sum at least 1e-6) sample k of the 36 is masked iff w_k <= tau * sbw.
A masked sample adds nothing to the source sums (sum w s, sum w r s, sum w s s); the reference sums (sum w, sum w r,
sum w r r) keep all 36 terms.  Nothing in it depends on any other pixel.
"""
import numpy as np

import np_interp as ni
import np_neg_skip as ns
import np_reference as npr

TAU = 2.0 ** -35                # capi.cpp build_kparams: KParams::ref_neg_tau


def pixel_mask(w, tau=TAU):
    """w: the pixel's 36 weights -> bool[36], True = masked (none for a pixel below the patch-sum floor)."""
    w = np.asarray(w, np.float64)
    sbw = w.sum()
    if tau < 0 or sbw < 1e-6:
        return np.zeros(w.shape, bool)
    return w <= tau * sbw


def masked_ncc(images, cams, params, src, px, py, plane, mask, terms=False):
    """The per-sample NCC (every sample projected, ACMMP.cu:456-516) with the masked samples' source terms left out
    -> cost, or (cost, terms) with the float64 terms np_neg_skip.on_off_bound takes (None where the cost is 2.0)."""
    rc, sc = cams[0], cams[src]
    ref, simg = images[0], images[src]
    R, inc = int(params["patch_size"]) // 2, int(params["radius_increment"])
    offs = np.arange(-R, R + 1, inc)
    ii, jj = np.meshgrid(offs, offs, indexing="ij")
    ii, jj = ii.ravel(), jj.ravel()
    W, H = sc["width"], sc["height"]
    dn = npr.depth_from_plane(rc, plane, px + ii, py + jj)
    sx, sy, _ = npr.project(sc, npr.world_point(rc, px + ii, py + jj, dn))
    sx, sy = np.asarray(sx, np.float64), np.asarray(sy, np.float64)
    sx = sx - np.floor(sx / W) * W
    sy = np.clip(sy, 0, H - 1)
    spix = npr.bilinear(simg, sx, sy)
    rpix = npr.texel(ref, px + ii, py + jj)
    w = ns.weights(images, cams, params, px, py)
    sbw = w.sum()
    none = (2.0, None) if terms else 2.0
    if sbw < 1e-6:
        return none
    ws = w * ~np.asarray(mask, bool)
    mr, ms = (w * rpix).sum() / sbw, (ws * spix).sum() / sbw
    vr = (w * rpix * rpix).sum() / sbw - mr * mr
    vs = (ws * spix * spix).sum() / sbw - ms * ms
    if vr < 1e-5 or vs < 1e-5:
        return none
    cov = (ws * rpix * spix).sum() / sbw - mr * ms
    cost = float(np.clip(1 - cov / np.sqrt(vr * vs), 0.0, 2.0))
    if terms:
        return cost, {"m_ref": mr, "m_src": ms, "var_ref": vr, "var_src": vs, "cov": cov,
                      "e_ss": (ws * spix * spix).sum() / sbw, "e_rs": (ws * rpix * spix).sum() / sbw}
    return cost


def hook_queries(sc, W, H):
    """The per-query sets of tests/test_gpu_ref_neg_skip.py: test_gpu_neg_skip.py's pixels (pole, seam, random, the
    dead band's edge rows, pole rows, seam columns, mixed dead / live runs) with the refinement's 5 planes each, 4
    near the surface and 1 far off it -> px, py, planes (n, 5, 4)."""
    from test_gpu_neg_skip import _queries
    px, py = _queries(sc, W, H)
    planes = ni.near_surface_planes(sc, px, py, 5, seed=31)
    planes[:, 4:] = ni.near_surface_planes(sc, px, py, 1, seed=33, spread=1.5, depth_jitter=0.4)
    return px, py, planes


# the entries of those sets held against float64: every STUDY_STEP-th query, a near-surface and the far plane, every view
STUDY_STEP, STUDY_PLANES = 5, (0, 4)


def float64_study(sc, params, px, py, planes, big_tau):
    """The float64 side of those entries, computed once per shape -> list of (q, h, v, unmasked cost, its terms or None,
    cost with the product threshold's mask, cost with big_tau's mask, the pixel's dropped share at the product
    threshold).  A pixel below the patch-sum floor has cost 2.0 and no terms throughout."""
    none = np.zeros(36, bool)
    out = []
    V = len(sc.images) - 1
    for q in range(0, len(px), STUDY_STEP):
        x, y = int(px[q]), int(py[q])
        w = ns.weights(sc.images, sc.cameras, params, x, y)
        m_tau, m_big = pixel_mask(w), pixel_mask(w, tau=big_tau)
        own = float((w * m_tau).sum() / w.sum())
        for h in STUDY_PLANES:
            plane = planes[q, h].astype(np.float64)
            for v in range(V):
                a = (sc.images, sc.cameras, params, v + 1, x, y, plane)
                c, t = masked_ncc(*a, none, terms=True)
                out.append((q, h, v, c, t, masked_ncc(*a, m_tau), masked_ncc(*a, m_big), own))
    return out
