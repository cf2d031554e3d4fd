"""Float64 restatement of the fast SPHERE k_eval_nb's negligible-sample mask (kernels.hip
stage_neg_mask and ncc_chunk's interpolated loop).  Test infrastructure beside np_interp.py (no GPU):
tests/test_neg_skip_design.py, tests/test_gpu_neg_skip.py and scripts/neg_skip_share.py import it.

The rule: a wave is 8 pixels; a pixel is live when it is staged (not dead) and its bilateral weight sum is at
least 1e-6.  Sample k of the 36 is masked for the wave when w_k(p) <= tau * sbw(p) for every live pixel p.  A
masked sample adds nothing to the source sums (sum w s, sum w r s, sum w s s); the reference sums (sum w,
sum w r, sum w r r) keep all 36 terms.
"""
import numpy as np

import np_interp as ni
import np_reference as npr

TAU = 2.0 ** -35                # capi.cpp build_kparams: KParams::neg_tau


def weights(images, cams, params, px, py):
    """The 36 bilateral weights of a patch (ACMMP.cu:398-403, 482-486), float64, in sample order."""
    rc, ref = cams[0], images[0]
    R, inc = int(params["patch_size"]) // 2, int(params["radius_increment"])
    offs = np.arange(-R, R + 1, inc)
    ii, jj = np.meshgrid(offs, offs, indexing="ij")
    ii, jj = ii.ravel(), jj.ravel()
    rpix = npr.texel(ref, px + ii, py + jj)
    center = npr.texel(ref, np.array(px), np.array(py))
    latc = -(py - rc["params"][2]) / rc["height"] * npr.PI_F
    scx, scy = 2 * npr.PI_F / rc["width"] * np.cos(latc), npr.PI_F / rc["height"]
    sig = float(params["sigma_spatial"]) * npr.PI_F / rc["height"]
    dx, dy = ii * scx, jj * scy
    return np.exp(-np.sqrt(dx * dx + dy * dy) / (2 * sig * sig) - np.abs(rpix - center) / (2 * params["sigma_color"] ** 2))


def wave_mask(w, dead=None, tau=TAU):
    """w: (pixels of the wave, 36) weights; dead: pixels that stage nothing.  -> bool[36], True = masked."""
    w = np.asarray(w, np.float64)
    sbw = w.sum(-1)
    live = ~(sbw < 1e-6)
    if dead is not None:
        live &= ~np.asarray(dead, bool)
    if tau < 0:
        return np.zeros(w.shape[-1], bool)
    keep = (live[:, None] & ~(w <= tau * sbw[:, None])).any(0)
    return ~keep


def masked_ncc(images, cams, params, src, px, py, plane, mask, terms=False):
    """np_interp.ncc's interpolated NCC (the kernel's nodes and spread test) with the masked samples' source
    terms left out -> (cost, fell back).  A fallback projects all 36 samples (k_nb_fix ignores the mask)."""
    rc, sc = cams[0], cams[src]
    ref, simg = images[0], images[src]
    R, inc = int(params["patch_size"]) // 2, int(params["radius_increment"])
    offs = np.arange(-R, R + 1, inc)
    ii, jj = np.meshgrid(offs, offs, indexing="ij")
    ii, jj = ii.ravel(), jj.ravel()
    W, H = sc["width"], sc["height"]

    def src_xy(di, dj):
        dn = npr.depth_from_plane(rc, plane, px + di, py + dj)
        x, y, _ = npr.project(sc, npr.world_point(rc, px + di, py + dj, dn))
        return np.asarray(x, np.float64), np.asarray(y, np.float64)

    nodes = np.asarray(ni.nodes_for(params), np.float64)
    n_i, n_j = np.meshgrid(nodes, nodes, indexing="ij")
    X, Y = src_xy(n_i.ravel(), n_j.ravel())
    X = X - np.round((X - X[0]) / W) * W
    k = [0, 3, 12, 15]
    fell = not (max(np.ptp(X[k]), np.ptp(Y[k])) <= ni.SPREAD_MAX)
    if fell:
        sx, sy = src_xy(ii, jj)
        use = np.ones(36, bool)
    else:
        L = ni.lagrange(ii.astype(np.float64), nodes)[:, :, None] * ni.lagrange(jj.astype(np.float64), nodes)[:, None, :]
        L = L.reshape(36, 16)
        sx, sy = L @ X, L @ Y
        use = ~np.asarray(mask, bool)
    sx = sx - np.floor(sx / W) * W
    sy = np.clip(sy, 0, H - 1)
    spix = npr.bilinear(simg, sx, sy)
    rpix = npr.texel(ref, px + ii, py + jj)
    w = weights(images, cams, params, px, py)
    sbw = w.sum()
    if sbw < 1e-6:
        return (2.0, fell, None) if terms else (2.0, fell)
    ws = w * use
    mr, ms = (w * rpix).sum() / sbw, (ws * spix).sum() / sbw
    vr = (w * rpix * rpix).sum() / sbw - mr * mr
    vs = (ws * spix * spix).sum() / sbw - ms * ms
    if vr < 1e-5 or vs < 1e-5:
        return (2.0, fell, None) if terms else (2.0, fell)
    cov = (ws * rpix * spix).sum() / sbw - mr * ms
    cost = float(np.clip(1 - cov / np.sqrt(vr * vs), 0.0, 2.0))
    if terms:
        return cost, fell, {"m_ref": mr, "m_src": ms, "var_ref": vr, "var_src": vs, "cov": cov,
                            "e_ss": (ws * spix * spix).sum() / sbw, "e_rs": (ws * rpix * spix).sum() / sbw}
    return cost, fell


def on_off_bound(t, tau=TAU, spacings=1, drop=None):
    """How far the NCC with the mask may lie from the one without, for a query with the float64 terms t
    (masked_ncc(..., terms=True)): the 36 tau bound of DESIGN.md §2.4 propagated through ncc_cost.  -> bound, or None
    where the source variance is too small for the first-order form (d var_src > var_src / 4).

    spacings = 0: exact arithmetic (the float64 restatement).  The dropped terms move a source sum by at most 36 tau
    of its scale: 255 for m_src, 255^2 for e_ss and e_rs.
    spacings = 1: binary32, the kernel.  The two runs add the same non-negative terms, one fma each, to running sums
    that start at most 36 tau of the scale apart -- less than one spacing of the sum.  Rounding to nearest is
    monotone, and the running sum only grows, so two sums at most one spacing apart stay at most one spacing apart
    after every step: whatever the number of steps, the final sums part by no more than the dropped mass or one
    spacing of the sum (2^-23 of it), whichever is larger -- both are allowed here.  The same holds for each later
    operation (the division by the weight sum, the two fmas that form var_src and cov): equal code on inputs one
    spacing apart, plus one spacing of its own result.
    var_src = e_ss - m_src^2 and cov = e_rs - m_ref m_src take those moves linearly; cost = 1 - cov / sqrt(var_ref
    var_src) then moves by (d cov + |cov| d var_src / (2 var_src)) / sqrt(var_ref var_src), times (1 - 1/4)^-3/2 < 1.6
    for the curvature over d var_src <= var_src / 4, plus (binary32) two spacings of the cost itself, 2^-23 below
    2.0, for the division, the root and the subtraction."""
    # drop: the query's own dropped share of the weight sum where the caller knows it (at most 36 tau by the rule)
    drop, sp = 36.0 * tau if drop is None else drop, spacings * 2.0 ** -23
    dm = 255.0 * drop + 2.0 * sp * abs(t["m_src"])                  # (the sum's spacing and the division's)
    dess = 255.0 ** 2 * drop + 2.0 * sp * abs(t["e_ss"])
    ders = 255.0 ** 2 * drop + 2.0 * sp * abs(t["e_rs"])
    dvs = dess + 2.0 * abs(t["m_src"]) * dm + sp * abs(t["var_src"])
    dcov = ders + abs(t["m_ref"]) * dm + sp * abs(t["cov"])
    if dvs > t["var_src"] / 4:
        return None
    lin = (dcov + abs(t["cov"]) * dvs / (2.0 * t["var_src"])) / np.sqrt(t["var_ref"] * t["var_src"])
    return 1.6 * lin + 2.0 * sp


def wave_pixels(px, py):
    """The 8 pixels of k_eval_nb's wave holding (px, py): same colour, same row, an aligned run of 8 of the
    colour grid (the 8 x 4 tile's row)."""
    k0 = ((px >> 1) // 8) * 8
    par = px & 1
    return [(2 * (k0 + t) + par, py) for t in range(8)]
