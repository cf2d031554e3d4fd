"""Shared infrastructure of the fast-math tests (no GPU): T1's gates, and the cases, query sets
and float64 reference of the small-shape instance matrix.  tests/test_gpu_fastmath.py,
tests/test_gpu_fast_instances.py and tests/test_fast_instance_inputs.py import it.

The instance matrix: model / size x source views x texel format, at shapes of about 100 pixels across (the
exact-mode matrix of tests/test_gpu_parity.py lives there too).  The per-sample fast arithmetic runs at any
size (interpolated coordinates start at 2000x1000), so every template instance of the hot kernels the workload's
own shapes never select -- fp32 texels, 1- and 2-view chunks, a partial last chunk, the separable staging --
is reached here in seconds.
"""
import functools

import numpy as np

import np_interp as ni
import np_reference as npr
from acmmp import scene, types

# ---- T1: one statement of the gates ------------------------------------------------------


def t1_fractions(f, e, ref):
    """Every fraction T1's gates use, from fast (f), exact (e) and float64 (ref) costs of the same queries,
    and the worst deviations from float64 over the queries valid in all three (recorded, not gated)."""
    f, e, ref = np.asarray(f), np.asarray(e), np.asarray(ref)
    valid = (e < 2.0) & (f < 2.0) & (ref < 2.0)
    df, de, dfe = np.abs(f - ref)[valid], np.abs(e - ref)[valid], np.abs(f - e)[valid]
    any_valid = bool(valid.any())
    return {
        "queries": int(f.size), "valid": int(valid.sum()), "valid_frac": float(valid.mean()),
        "fast_nan": int(np.isnan(f).sum()),
        "class_agree_fast_exact": float(np.mean((f >= 2.0) == (e >= 2.0))),
        "class_agree_exact_f64": float(np.mean((e >= 2.0) == (ref >= 2.0))),
        "frac_fast_within_1e-4_of_exact": float(np.mean(dfe <= 1e-4)) if any_valid else 1.0,
        "frac_exact_within_1e-4_of_f64": float(np.mean(de <= 1e-4)) if any_valid else 1.0,
        "fast_worse_than_exact_by_1e-4": float(np.mean(df > de + 1e-4)) if any_valid else 0.0,
        "exact_worse_than_fast_by_1e-4": float(np.mean(de > df + 1e-4)) if any_valid else 0.0,
        "worst_fast_vs_f64": float(df.max()) if any_valid else 0.0,
        "worst_exact_vs_f64": float(de.max()) if any_valid else 0.0,
        "worst_fast_vs_exact": float(dfe.max()) if any_valid else 0.0,
    }


def t1_gates(f, e, ref, sphere, what=""):
    """T1 of DESIGN.md §2.4 on fast / exact / float64 costs of the same queries -> t1_fractions.
    (a) a cost of 2.0 is the reference's "no match" (centre outside, weight sum < 1e-6, variance < 1e-5) or a
    clamped NCC; its thresholds are discontinuities the binary32 noise can cross, so the fast mode may flip a
    query's class no more often than the exact mode's own class differs from float64's (+ 0.2 pt), and never for
    more than 1% of the queries; (b) pinhole |fast - exact| <= 1e-4 for >= 99.5% of valid queries, SPHERE no more
    often beyond 1e-4 of exact than exact is of float64, + 5 pt; (c) fast farther from float64 than exact by
    > 1e-4 in at most 3 pt more queries than the converse; and no fast cost is NaN (the NCC clamp of
    ACMMP.cu:513 maps a NaN ratio to 2.0)."""
    fr = t1_fractions(f, e, ref)
    assert fr["fast_nan"] == 0, (what, fr["fast_nan"])
    agree_fe, agree_ef = fr["class_agree_fast_exact"], fr["class_agree_exact_f64"]
    assert agree_fe >= agree_ef - 0.002 and agree_fe >= 0.99, (what, agree_fe, agree_ef)
    near_fe, near_ef = fr["frac_fast_within_1e-4_of_exact"], fr["frac_exact_within_1e-4_of_f64"]
    if sphere:
        assert near_fe >= near_ef - 0.05, (what, near_fe, near_ef)
    else:
        assert near_fe >= 0.995, (what, near_fe)
    fast_worse, exact_worse = fr["fast_worse_than_exact_by_1e-4"], fr["exact_worse_than_fast_by_1e-4"]
    assert fast_worse <= exact_worse + 0.03, (what, fast_worse, exact_worse)
    return fr


# ---- the instance matrix ----------------------------------------------------------------------------------

MODELS = {"pinhole": (96, 64), "sphere": (128, 64)}
VIEWS = (1, 2, 3, 5, 9)
TEXELS = {"f16": True, "fp32": False}          # quantize: 8-bit images take the binary16 copy, floats fp32
CASES = [(k, v, t) for k in MODELS for v in VIEWS for t in TEXELS]
SETS = ("interior", "border", "source_edge", "wild")
MIN_VALID = 300                                 # (query, view) pairs valid in every mode, per set
PLANES = 8                                      # per pixel: k_eval_nb's hypotheses; the first 5 feed k_eval_ref
# pixels per set: >= 300 valid (query, view) pairs with 8 planes each from one view up -- the border, source-edge
# and wild sets lose queries to the 2.0 class (centre outside a source, variance thresholds), the wild set most
PIXELS = {1: 160, 2: 96, 3: 64, 5: 48, 9: 32}


def case_id(kind, V, tex):
    return f"{kind}-v{V}-{tex}"


def params_for(sc, **kw):
    c0 = sc.cameras[0]
    return types.default_params(num_images=len(sc.images), depth_min=float(c0["depth_min"]) * 0.6,
                                depth_max=float(c0["depth_max"]) * 1.2, **kw)


@functools.lru_cache(maxsize=None)
def make_case(kind, V, tex):
    """-> (scene, params) as tests/test_gpu_parity.make builds them."""
    W, H = MODELS[kind]
    make = scene.pinhole_scene if kind == "pinhole" else scene.sphere_scene
    sc = make(W, H, n_src=V, seed=W + V, quantize=TEXELS[tex])
    return sc, params_for(sc)


def sample_rays(sc, p, px, py):
    """Float64 reference rays of the patch samples of pixels (px, py): (n, S, 3), and the sample offsets."""
    R, inc = int(p["patch_size"]) // 2, int(p["radius_increment"])
    offs = np.arange(-R, R + 1, inc)
    ii, jj = np.meshgrid(offs, offs, indexing="ij")
    ii, jj = ii.ravel(), jj.ravel()
    return npr.pixel_to_dir(sc.cameras[0], px[:, None] + ii[None], py[:, None] + jj[None]), ii, jj


def grazing_plane(sc, p, px, py, sample, rng):
    """A near-surface plane turned until it contains the ray of patch sample `sample` of pixel (px, py):
    n . r_s = 0 up to rounding, far inside the 1e-6 clamp of ComputeDepthfromPlaneHypothesis (ACMMP.cu:187-193) in
    binary32 and float64 alike, so that sample's depth is the clamp's 1e6 and the depth changes sign beside it."""
    rays, _, _ = sample_rays(sc, p, np.array([px]), np.array([py]))
    rs = rays[0, sample]
    d = npr.pixel_to_dir(sc.cameras[0], px, py)
    n = -d + rng.normal(0, 0.2, 3)
    n -= (n @ rs) * rs
    n /= np.linalg.norm(n)
    depth = float(sc.gt_depth[py, px])
    return np.array([*n, -float(n @ (d * depth))], np.float32)


def source_edge_pixels(sc, p, n, seed, margin=6):
    """Interior reference pixels picked by float64 projection (f64_ncc's diagnostics on the ground-truth surface
    plane of every interior pixel), ranked by the share of source views they reach the edge of.
    Pinhole: the centre lands inside a source and part of the 36 samples outside it (the surface point is then
    within 6 pixels of that source's edge).  SPHERE: half the pixels have samples on both sides of a source's
    longitude seam (np_interp.special_pixels' "seam" set), half a sample row clamped at a source's pole -- a 64-row
    view has few of those, so that half is filled with the pixels whose surface point lands nearest a source pole
    (the "pole" set with its 10-degree threshold replaced by a ranking)."""
    rng = np.random.default_rng(seed)
    rc = sc.cameras[0]
    H, W = sc.images[0].shape
    ys, xs = np.mgrid[margin:H - margin, margin:W - margin]
    xs, ys = xs.ravel(), ys.ravel()
    d = npr.pixel_to_dir(rc, xs, ys)
    depth = sc.gt_depth[ys, xs].astype(np.float64)
    planes = np.concatenate([-d, depth[:, None]], axis=1).astype(np.float32)
    _, diag = f64_ncc(sc, p, xs, ys, planes, diagnostics=True)

    def top(score, k, taken):
        score = np.where(taken, 0.0, score)
        idx = np.nonzero(score > 0)[0]
        idx = idx[np.argsort(-(score[idx] + rng.uniform(0, 1e-3, len(idx))), kind="stable")][: 2 * k]
        return rng.choice(idx, size=min(k, len(idx)), replace=False)

    taken = np.zeros(len(xs), bool)
    if int(rc["model"]) != npr.SPHERE:
        pick = top(diag["out_of_image"].mean(axis=1), n, taken)
    else:
        pick = top(diag["seam"].mean(axis=1), n // 2, taken)
        taken[pick] = True
        pole = top(diag["pole"].mean(axis=1), n - len(pick), taken)
        taken[pole] = True
        pick = np.concatenate([pick, pole])
        if len(pick) < n:
            P = npr.world_point(rc, xs, ys, depth)
            lat = np.max([np.abs(npr.project(c, P)[1] / float(c["height"]) * 180.0 - 90.0) for c in sc.cameras[1:]], axis=0)
            pick = np.concatenate([pick, top(lat, n - len(pick), taken)])
    assert len(pick) == n, (len(pick), n)
    return xs[pick].astype(np.int32), ys[pick].astype(np.int32)


def query_sets_for(sc, p, seed, n=None):
    """The four query sets of any rig (scene, params): {set: (px (n,), py (n,), planes (n, 8, 4) float32)}, n
    pixels per set (default PIXELS[source views]).
      interior     random pixels at least 6 pixels inside, near-surface planes;
      border       the four corners and random pixels of the 6-pixel frame, near-surface planes;
      source_edge  pinhole: the surface point projects within 6 pixels of a source's edge; SPHERE: it lands
                   at a source's longitude seam or nearest a source's pole; near-surface planes;
      wild         interior pixels, planes of any orientation and +-40% depth (grazing planes, depth sign
                   flips inside the patch, centres outside the source), and on the first pixels one plane
                   each that contains a sample's ray (grazing_plane)."""
    H, W = sc.images[0].shape
    n = PIXELS[len(sc.images) - 1] if n is None else n
    out = {}
    px, py = ni.interior_pixels(W, H, n, seed + 1)
    out["interior"] = (px, py, ni.near_surface_planes(sc, px, py, PLANES, seed + 2))
    px, py = ni.border_pixels(W, H, n, seed + 3)
    out["border"] = (px, py, ni.near_surface_planes(sc, px, py, PLANES, seed + 4))
    px, py = source_edge_pixels(sc, p, n, seed + 5)
    out["source_edge"] = (px, py, ni.near_surface_planes(sc, px, py, PLANES, seed + 6))
    px, py = ni.interior_pixels(W, H, n, seed + 7)
    planes = ni.near_surface_planes(sc, px, py, PLANES, seed + 8, spread=1.5, depth_jitter=0.4)
    rng = np.random.default_rng(seed + 9)
    for q, sample in enumerate((0, 14, 21, 35)):            # a corner, two inner samples, the last corner
        planes[q, q % 5] = grazing_plane(sc, p, int(px[q]), int(py[q]), sample, rng)
    out["wild"] = (px, py, planes)
    return out


@functools.lru_cache(maxsize=None)
def query_sets(kind, V, tex):
    """query_sets_for on one case of the instance matrix."""
    sc, p = make_case(kind, V, tex)
    return query_sets_for(sc, p, 1000 * V + (0 if kind == "pinhole" else 500) + (0 if TEXELS[tex] else 250))


def f64_ncc(sc, p, px, py, planes, diagnostics=False):
    """np_reference.bilateral_ncc (ComputeBilateralNCC, ACMMP.cu:405-516, float64) over all queries and views at
    once: pixels (Q,), planes (Q, 4) -> costs (Q, V).  The same statements on arrays; test_fast_instance_inputs
    holds it to the scalar function.  With diagnostics, also a dict of what each query exercises:
      out_of_image (Q, V)  pinhole: the centre is inside the source and some sample falls outside it;
      seam (Q, V)          SPHERE: the samples straddle the source's longitude seam, or one's footprint touches it;
      pole (Q, V)          SPHERE: some sample's row is clamped at a pole;
      centre_out (Q, V)    pinhole: the centre projects outside the source (cost 2.0);
      clamp (Q,)           |n . r| < 1e-6 at the centre or a sample (depth 1e6);
      sign_flip (Q,)       the plane's depth changes sign inside the patch."""
    images, cams = sc.images, sc.cameras
    rc, ref = cams[0], images[0]
    sphere = int(rc["model"]) == npr.SPHERE
    px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
    pl = np.asarray(planes, np.float32).astype(np.float64)
    rays, ii, jj = sample_rays(sc, p, px, py)
    rx, ry = px[:, None] + ii[None], py[:, None] + jj[None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        den_c = np.einsum("qc,qc->q", npr.pixel_to_dir(rc, px, py), pl[:, :3])
        dref = np.where(np.abs(den_c) < 1e-6, 1e6, -pl[:, 3] / den_c)
        Pc = npr.world_point(rc, px, py, dref)
        den = np.einsum("qsc,qc->qs", rays, pl[:, :3])
        raw = -pl[:, 3:4] / den
        dn = np.where(np.abs(den) < 1e-6, 1e6, raw)
        P = npr.world_point(rc, rx, ry, dn)
        rpix = npr.texel(ref, rx, ry)
        center = npr.texel(ref, px, py)
        sig = float(p["sigma_spatial"])
        if sphere:
            latc = -(py - rc["params"][2]) / rc["height"] * npr.PI_F
            dx = ii[None] * (2 * npr.PI_F / rc["width"] * np.cos(latc))[:, None]
            dy = (jj * (npr.PI_F / rc["height"]))[None] * np.ones_like(dx)
            sig = sig * npr.PI_F / rc["height"]
        else:
            dx = ii[None].astype(np.float64) * np.ones(rx.shape)
            dy = jj[None].astype(np.float64) * np.ones(rx.shape)
        w0 = np.exp(-np.sqrt(dx * dx + dy * dy) / (2 * sig * sig)
                    - np.abs(rpix - center[:, None]) / (2 * p["sigma_color"] ** 2))
        V = len(images) - 1
        cost = np.full((len(px), V), 2.0)
        diag = {k: np.zeros((len(px), V), bool) for k in ("out_of_image", "seam", "pole", "centre_out")}
        diag["clamp"] = (np.abs(den) < 1e-6).any(axis=1) | (np.abs(den_c) < 1e-6)
        diag["sign_flip"] = (raw > 0).any(axis=1) & (raw < 0).any(axis=1)
        for v in range(1, V + 1):
            scam, simg = cams[v], images[v]
            W, H = scam["width"], scam["height"]
            cx, cy, _ = npr.project(scam, Pc)
            sx, sy, _ = npr.project(scam, P)
            if sphere:
                turns = np.floor(sx / W)
                sx = sx - turns * W
                diag["seam"][:, v - 1] = (turns.max(axis=1) != turns.min(axis=1)) | (sx > W - 1).any(axis=1)
                diag["pole"][:, v - 1] = ((sy < 0) | (sy > H - 1)).any(axis=1)
                sy = np.clip(sy, 0, H - 1)
                ok = np.ones(sx.shape, bool)
                c_out = np.zeros(len(px), bool)
            else:
                c_out = (cx < 0) | (cx >= W) | (cy < 0) | (cy >= H)
                ok = ~((sx < 0) | (sx >= W) | (sy < 0) | (sy >= H))
                diag["centre_out"][:, v - 1] = c_out
                diag["out_of_image"][:, v - 1] = ~c_out & ~ok.all(axis=1)
            spix = npr.bilinear(simg, np.where(ok, sx, 0), np.where(ok, sy, 0))
            w = np.where(ok, w0, 0.0)
            sbw = w.sum(axis=1)
            mr, ms = (w * rpix).sum(axis=1) / sbw, (w * spix).sum(axis=1) / sbw
            vr = (w * rpix * rpix).sum(axis=1) / sbw - mr * mr
            vs = (w * spix * spix).sum(axis=1) / sbw - ms * ms
            cov = (w * rpix * spix).sum(axis=1) / sbw - mr * ms
            ncc = np.clip(1 - cov / np.sqrt(vr * vs), 0.0, 2.0)
            none = c_out | (sbw < 1e-6) | (vr < 1e-5) | (vs < 1e-5)
            cost[:, v - 1] = np.where(none, 2.0, ncc)
    return (cost, diag) if diagnostics else cost


def flat_queries(px, py, planes):
    """(n,), (n,), (n, k, 4) -> one query per plane: (n k,), (n k,), (n k, 4)."""
    k = planes.shape[1]
    return np.repeat(px, k), np.repeat(py, k), planes.reshape(-1, 4)


def f64_costs_for(sc, p, px, py, planes):
    """Float64 costs of one set of any rig, (n, 8, V), with the diagnostics; the costs are left read-only."""
    cost, diag = f64_ncc(sc, p, *flat_queries(px, py, planes), diagnostics=True)
    cost = cost.reshape(len(px), planes.shape[1], len(sc.images) - 1)
    cost.setflags(write=False)
    return cost, diag


@functools.lru_cache(maxsize=None)
def f64_costs(kind, V, tex, name):
    """f64_costs_for on one set of one case -- computed once per process and left unchanged."""
    sc, p = make_case(kind, V, tex)
    return f64_costs_for(sc, p, *query_sets(kind, V, tex)[name])


def oracle_costs_for(oracle_mod, sc, p, px, py, planes):
    """oracle.ncc (binary32, CPU) of one set of any rig: (n, 8, V) float32."""
    V = len(sc.images) - 1
    prob = oracle_mod.Problem(sc.images, sc.cameras, p)
    out = np.empty((len(px), planes.shape[1], V), np.float32)
    for q in range(len(px)):
        for h in range(planes.shape[1]):
            for v in range(V):
                out[q, h, v] = oracle_mod.ncc(prob, v + 1, int(px[q]), int(py[q]), planes[q, h])
    return out


def oracle_costs(oracle_mod, kind, V, tex, name):
    """oracle_costs_for on one set of one case."""
    sc, p = make_case(kind, V, tex)
    return oracle_costs_for(oracle_mod, sc, p, *query_sets(kind, V, tex)[name])


def reform_initial_cost(costs, top_k):
    """ComputeMultiViewInitialCostandSelectedViews (ACMMP.cu:519-556) from per-view costs (P, V), in binary32 as
    initial_cost (kernels.hip) and the oracle do: sort ascending, sum the min(valid, top_k) smallest in order,
    divide; 2.0 where no view is valid."""
    c = np.asarray(costs, np.float32)
    k = np.minimum((c < 2.0).sum(axis=1), int(top_k))
    s = np.sort(c, axis=1)
    acc = np.zeros(len(c), np.float32)
    for i in range(min(int(top_k), c.shape[1])):
        acc = np.where(i < k, acc + s[:, i], acc).astype(np.float32)
    return np.where(k > 0, acc / np.maximum(k, 1).astype(np.float32), np.float32(2.0)).astype(np.float32)
