"""Test-side restatement of the whole-scene fusion (acmmp_fusion_run_scene, include/acmmp.h): per view the
provenance of every emitted point (pixel, consistent-source mask, the source pixels that were sampled) and
the duplicate-free mode's marking, built from the oracle alone -- or_world_point, or_project, (int)(x + 0.5f)
saturated and OracleFusion.run on depth copies zeroed at the used pixels.  TEST INFRASTRUCTURE: RestatedFusion
has capi.Fusion's scene surface so the pipeline and the GPU tests can be checked against it."""
import ctypes as C
import functools

import numpy as np

import oracle
from acmmp import pipeline, scene
from pipeline_support import OracleEngine, OracleFusion, small_dataset


def f2i_sat(x):
    """(int)x saturated as the kernels do it (detmath f2i_sat), on a float32 array."""
    return oracle.detmath("f2i_sat", np.ascontiguousarray(x, np.float32)).astype(np.int64)


def zeroed(depths, used):
    """Depth copies in which every used pixel reads as 0."""
    return [d if d is None or u is None else np.where(u != 0, np.float32(0), d).astype(np.float32)
            for d, u in zip(depths, used)]


def view_provenance(cams, depths, normals, ref, srcs):
    """(pixels r*W + c ascending, source masks) of the points SimpleFusionKernel emits for view `ref` on
    `depths`.  Source j alone, listed twice, emits a pixel exactly when j is consistent there (1 + 2 >= 3); the
    pixel is read back from a colour ramp given to the reference view (the sources' colours are zero, so
    the output colour is the ramp's 2x2 average * 255 / 3).  A pixel is emitted when two sources agree."""
    cams = np.ascontiguousarray(cams)
    H, W = depths[ref].shape
    probe = OracleFusion(cams)
    probe.depths, probe.normals = list(depths), list(normals)
    probe.rgba = [None if d is None else np.zeros((*d.shape, 4), np.float32) for d in depths]
    ramp = np.zeros((H, W, 4), np.float32)
    ramp[..., 2] = np.arange(W, dtype=np.float32)[None, :]      # slot c0 of the output
    ramp[..., 1] = np.arange(H, dtype=np.float32)[:, None]      # slot c1
    probe.rgba[ref] = ramp
    bits = np.zeros(H * W, np.uint32)
    for j, s in enumerate(srcs):
        if s < 0:
            continue
        pts = probe.run(ref, [s, s]).astype(np.float64)
        c = np.floor(pts[:, 6] * 3.0 / 255.0 + 0.75).astype(np.int64)   # average of columns (c-1, c) = c - 0.5; 0 at c = 0
        r = np.floor(pts[:, 7] * 3.0 / 255.0 + 0.75).astype(np.int64)
        assert ((c >= 0) & (c < W) & (r >= 0) & (r < H)).all()
        pix = r * W + c
        assert (np.diff(pix) > 0).all(), "the oracle emits in pixel order"
        bits[pix] |= np.uint32(1 << j)
    n = np.zeros(H * W, np.int64)
    for j in range(32):
        n += (bits >> np.uint32(j)) & np.uint32(1)
    pixels = np.flatnonzero(n >= 2)
    return pixels.astype(np.int32), bits[pixels]


def point_samples(cams, depths, ref, srcs, pixels, masks, want_xyz=False):
    """Per point the pixel index of every depth sample that contributed, an (n, 1 + len(srcs)) int64 array:
    column 0 the reference pixel, column 1 + j the pixel of view srcs[j] that was sampled -- (int)(p + 0.5f)
    of the projection of the reference pixel's world point -- or -1 where bit j of the mask is clear.
    want_xyz: also the point, the float32 average of those samples' world points, sources in ascending j."""
    cams = np.ascontiguousarray(cams)
    L, vp = oracle.lib(), C.c_void_p
    camp = [vp(cams[i:i + 1].ctypes.data) for i in range(len(cams))]
    W = depths[ref].shape[1]
    n = len(pixels)
    X, pt, d = np.zeros(3, np.float32), np.zeros(2, np.float32), C.c_float(0)
    Xp, ptp = X.ctypes.data_as(vp), pt.ctypes.data_as(vp)
    Xref, proj = np.zeros((n, 3), np.float32), np.zeros((n, len(srcs), 2), np.float32)
    rows, cols = np.divmod(np.asarray(pixels, np.int64), W)
    dref = depths[ref][rows, cols]
    for i in range(n):
        L.or_world_point(camp[ref], float(cols[i]), float(rows[i]), float(dref[i]), Xp)
        Xref[i] = X
        m = int(masks[i])
        for j, s in enumerate(srcs):
            if (m >> j) & 1:
                L.or_project(camp[s], Xp, ptp, C.byref(d))
                proj[i, j] = pt
    cr = f2i_sat(proj + np.float32(0.5))
    samples = np.full((n, 1 + len(srcs)), -1, np.int64)
    samples[:, 0] = pixels
    for j, s in enumerate(srcs):
        on = ((np.asarray(masks, np.uint32) >> np.uint32(j)) & np.uint32(1)).astype(bool)
        if s < 0:
            assert not on.any()
            continue
        Hs, Ws = depths[s].shape
        c, r = cr[on, j, 0], cr[on, j, 1]
        assert ((c >= 0) & (c < Ws) & (r >= 0) & (r < Hs)).all()
        samples[on, 1 + j] = r * Ws + c
    if not want_xyz:
        return samples
    xyz = np.zeros((n, 3), np.float32)
    for i in range(n):
        acc, k = Xref[i].copy(), 1
        for j, s in enumerate(srcs):
            q = int(samples[i, 1 + j])
            if q >= 0:
                sr, sc = divmod(q, depths[s].shape[1])
                L.or_world_point(camp[s], float(sc), float(sr), float(depths[s][sr, sc]), Xp)
                acc = (acc + X).astype(np.float32)
                k += 1
        xyz[i] = acc / np.float32(k)
    return samples, xyz


def mark_samples(marks, ref, srcs, samples):
    """The duplicate-free mode's marking: every contributing sample of every emitted point becomes used."""
    marks[ref].reshape(-1)[samples[:, 0]] = 1
    for j, s in enumerate(srcs):
        q = samples[:, 1 + j]
        if s >= 0:
            marks[s].reshape(-1)[q[q >= 0]] = 1


class RestatedFusion(OracleFusion):
    """capi.Fusion's scene surface (run_scene, scene_points, reset_used, used) computed by the restatement."""

    def __init__(self, cams):
        super().__init__(cams)
        self.marks = [None] * len(self.cams)
        self.result = None

    def set_view(self, k, depth, normals, bgr):
        super().set_view(k, depth, normals, bgr)
        self.marks[k] = np.zeros(self.depths[k].shape, np.uint8)

    def reset_used(self):
        for m in self.marks:
            if m is not None:
                m[...] = 0

    def used(self, view):
        return self.marks[view].copy()

    def run_scene(self, refs, src_lists, unique=False):
        pts, ref_idx, pix, msk, counts = [], [], [], [], []
        for k, (ref, srcs) in enumerate(zip(refs, src_lists)):
            depths = zeroed(self.depths, self.marks) if unique else self.depths
            p = oracle.fuse(self.cams, depths, self.normals, self.rgba, ref, srcs)
            pixels, masks = view_provenance(self.cams, depths, self.normals, ref, srcs)
            assert len(pixels) == p.shape[0]
            if unique:
                mark_samples(self.marks, ref, srcs, point_samples(self.cams, depths, ref, srcs, pixels, masks))
            pts.append(p); pix.append(pixels); msk.append(masks)
            ref_idx.append(np.full(len(pixels), k, np.int32)); counts.append(len(pixels))
        cat = lambda a, shape, dt: np.concatenate(a, 0) if a else np.zeros(shape, dt)
        self.result = (cat(pts, (0, 9), np.float32), cat(ref_idx, (0,), np.int32), cat(pix, (0,), np.int32),
                       cat(msk, (0,), np.uint32))
        return int(sum(counts)), np.array(counts, np.int32)

    def scene_points(self, first, n, provenance=False):
        out = tuple(a[first:first + n].copy() for a in self.result)
        return out if provenance else out[0]


@functools.lru_cache(maxsize=None)
def dataset_inputs(model, W=64, H=32, n=3):
    """Fusion inputs of a small_dataset run through the oracle pipeline: (cams, depths, normals, colours)."""
    ds = small_dataset(W, H, n, model=model)
    pipe = pipeline.Pipeline(ds, engine=OracleEngine(), order="reference", geom_iterations=1).run()
    return pipeline.fusion_inputs(ds, pipe.store, pipe.problems)


@functools.lru_cache(maxsize=None)
def rig_inputs(W, H, n, seed=3):
    """The ground-truth sphere rig of test_fusion.py: exact depth / normal maps of a convex room."""
    sc = scene.sphere_scene(W, H, n_src=n - 1, seed=seed)
    bgr = [np.repeat(np.asarray(im, np.uint8)[..., None], 3, 2) for im in sc.images]
    return np.array(sc.cameras), sc.extra["gt_depths"], sc.extra["gt_normals"], bgr


def all_others(n):
    return [[j for j in range(n) if j != k] for k in range(n)]


def fill(fu, cams, depths, normals, colours):
    for k in range(len(cams)):
        fu.set_view(k, depths[k], normals[k], colours[k])
    return fu


def assert_samples_used_once(cams, depths, refs, lists, ref_idx, pix, mask):
    """The cross-view invariant on a scene's provenance: a depth sample that contributed to a point of one
    reference view contributes to no point of another.  Returns the number of distinct samples."""
    owner = [np.full(d.size, -1, np.int64) for d in depths]

    def claim(v, q, k):
        assert np.isin(owner[v][q], (-1, k)).all(), f"view {v}: a sample of an earlier view is used again by view {refs[k]}"
        owner[v][q] = k
    for k, (ref, srcs) in enumerate(zip(refs, lists)):
        sel = ref_idx == k
        samples = point_samples(cams, depths, ref, srcs, pix[sel], mask[sel])
        claim(ref, samples[:, 0], k)
        for j, s in enumerate(srcs):
            q = samples[:, 1 + j]
            if s >= 0:
                claim(s, q[q >= 0], k)
    return sum(int((o >= 0).sum()) for o in owner)
