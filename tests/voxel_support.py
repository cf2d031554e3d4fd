"""Test-side restatement of the voxel-grid reduction of a scene cloud (acmmp_fusion_voxelize, include/acmmp.h):
numpy only, sequential, written from the header's six steps -- float32 cell index, 16.16 fixed-point channels,
int64 sums, float64 means rounded once, cells in order of first appearance.  TEST INFRASTRUCTURE:
RestatedVoxelFusion has capi.Fusion's voxel surface so the pipeline and the GPU tests can be checked against it,
and table_layout restates where linear probing puts the cells of a table filled one key after another."""
import functools

import numpy as np

from acmmp import pipeline
from fusion_scene_support import RestatedFusion, dataset_inputs, fill, rig_inputs
from pipeline_support import OracleFusion

F32 = np.float32
CELLS = 1 << 21


def ordered(x):
    """Order-preserving map of float32 bits to uint32 (-0 below +0)."""
    b = np.ascontiguousarray(x, F32).view(np.uint32)
    return np.where(b >> np.uint32(31) != 0, ~b, b | np.uint32(0x80000000))


def unordered(u):
    u = np.asarray(u, np.uint32)
    return np.where(u >> np.uint32(31) != 0, u ^ np.uint32(0x80000000), ~u).astype(np.uint32).view(F32)


def finite_points(pts):
    """Step 1: all nine floats finite, normal and colour within 2^20."""
    return np.isfinite(pts).all(1) & (np.abs(pts[:, 3:]) <= F32(1 << 20)).all(1)


def cloud_origin(pts):
    """The origin of a NULL-origin run: the minimum over the step-1 points, or zero when there is none."""
    ok = finite_points(pts)
    if not ok.any():
        return np.zeros(3, F32)
    return unordered(ordered(pts[ok, :3]).min(0))


def cells(pts, size, origin):
    """Steps 1-2: (accepted, keys uint64 of the accepted points, their fractions float32 (n, 3))."""
    pts = np.ascontiguousarray(pts, F32)
    size, o = F32(size), np.ascontiguousarray(origin, F32)
    with np.errstate(all="ignore"):
        inv = F32(1.0) / size
        t = (pts[:, :3] - o[None, :]) * inv
        g = np.floor(t)
        assert t.dtype == F32 and g.dtype == F32
        inside = ((g >= 0) & (g < F32(CELLS))).all(1)
        acc = finite_points(pts) & inside
        frac = t[acc] - g[acc]
    gi = g[acc].astype(np.uint64)
    keys = gi[:, 0] | (gi[:, 1] << np.uint64(21)) | (gi[:, 2] << np.uint64(42))
    return acc, keys, frac


def voxelize(pts, size, origin=None, min_points=1):
    """The whole definition.  Returns a dict: points (n, 9) float32, counts int32, keys uint64, first int64 (all of
    the kept voxels, in output order), n_occupied, n_rejected, origin float32 (3,)."""
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 9)
    size = F32(size)
    o = cloud_origin(pts) if origin is None else np.ascontiguousarray(origin, F32).reshape(3).copy()
    acc, keys, frac = cells(pts, size, o)
    idx = np.flatnonzero(acc).astype(np.int64)
    q = np.rint(np.concatenate([frac, pts[acc, 3:]], 1) * F32(65536.0))          # half to even
    assert q.dtype == F32
    q = q.astype(np.int64)
    uniq, inverse = np.unique(keys, return_inverse=True)
    inverse = inverse.reshape(-1)
    n = np.bincount(inverse, minlength=len(uniq)).astype(np.int64)
    first = np.full(len(uniq), np.iinfo(np.int64).max, np.int64)
    np.minimum.at(first, inverse, idx)
    S = np.zeros((len(uniq), 9), np.int64)
    np.add.at(S, inverse, q)
    keep = np.flatnonzero(n >= min_points)
    keep = keep[np.argsort(first[keep], kind="stable")]
    key, n_k, S_k = uniq[keep], n[keep], S[keep]
    mean = S_k.astype(np.float64) / (n_k.astype(np.float64) * 65536.0)[:, None]
    cell = np.stack([((key >> np.uint64(21 * a)) & np.uint64(CELLS - 1)).astype(np.float64) for a in range(3)], 1)
    out = np.zeros((len(keep), 9), F32)
    out[:, :3] = (o.astype(np.float64)[None, :] + (cell + mean[:, :3]) * np.float64(size)).astype(F32)
    out[:, 3:] = mean[:, 3:].astype(F32)
    return {"points": out, "counts": n_k.astype(np.int32), "keys": key, "first": first[keep],
            "n_occupied": int(len(uniq)), "n_rejected": int(pts.shape[0] - acc.sum()), "origin": o}


def scene_keys(pts, size, origin=None):
    """Keys of the accepted points in scene order (what the insert pass feeds the table)."""
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 9)
    o = cloud_origin(pts) if origin is None else np.ascontiguousarray(origin, F32)
    return cells(pts, size, o)[1]


def splitmix64(keys):
    with np.errstate(over="ignore"):
        z = np.asarray(keys, np.uint64) + np.uint64(0x9e3779b97f4a7c15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        return z ^ (z >> np.uint64(31))


def auto_slots(n_points):
    s = 1024
    while s < 2 * n_points:
        s *= 2
    return s


def table_layout(keys_in_scene_order, slots):
    """Linear probing from splitmix64(key) >> (64 - log2(slots)), one key after another in scene order.
    Returns (occupied, wrapped): the cells stored, and those stored at a slot index below their home slot."""
    assert slots >= 64 and slots & (slots - 1) == 0
    keys = np.asarray(keys_in_scene_order, np.uint64)
    _, at = np.unique(keys, return_index=True)
    keys = keys[np.sort(at)]                                   # first appearances, in order
    assert len(keys) < slots
    homes = (splitmix64(keys) >> np.uint64(64 - (slots.bit_length() - 1))).astype(np.int64).tolist()
    table = [False] * slots
    wrapped = 0
    for h in homes:
        s = h
        while table[s]:
            s = (s + 1) & (slots - 1)
        table[s] = True
        wrapped += s < h
    return len(homes), int(wrapped)


class RestatedVoxelFusion(RestatedFusion):
    """RestatedFusion with capi.Fusion's voxel surface (voxelize, voxel_points) computed by the restatement."""

    def __init__(self, cams):
        super().__init__(cams)
        self.voxels = None

    def run_scene(self, refs, src_lists, unique=False):
        out = super().run_scene(refs, src_lists, unique=unique)
        self.voxels = None
        return out

    def voxelize(self, size, origin=None, min_points=1):
        if self.result is None or not (np.isfinite(F32(size)) and F32(size) > 0) or min_points < 1 or \
                (origin is not None and not np.isfinite(np.asarray(origin, F32)).all()):
            raise ValueError("bad voxelize argument")
        self.voxels = voxelize(self.result[0], size, origin, min_points)
        v = self.voxels
        return v["points"].shape[0], {"n_occupied": v["n_occupied"], "n_rejected": v["n_rejected"], "origin": v["origin"]}

    def voxel_points(self, first, n, counts=False):
        total = 0 if self.voxels is None else self.voxels["points"].shape[0]
        if first < 0 or n < 0 or first + n > total:
            raise ValueError("range beyond the voxel result")
        if n == 0:
            return (np.zeros((0, 9), F32), np.zeros(0, np.int32)) if counts else np.zeros((0, 9), F32)
        p, c = self.voxels["points"][first:first + n].copy(), self.voxels["counts"][first:first + n].copy()
        return (p, c) if counts else p


# ---- the scenes of the voxel tests: fusion inputs, the reference views in order and their source lists

def edge_rig_inputs():
    """The ground-truth rig at 50x30 (1500 pixels: a ragged last 256-pixel chunk), 5 views, of which view 2 has an
    all-zero depth map and view 3 a depth map of half the size."""
    cams, depths, normals, bgr = rig_inputs(50, 30, 5)
    cams, depths, normals, bgr = cams.copy(), list(depths), list(normals), list(bgr)
    depths[2] = np.zeros_like(depths[2])
    depths[3] = np.ascontiguousarray(depths[3][::2, ::2])
    normals[3] = np.ascontiguousarray(normals[3][::2, ::2])
    bgr[3], cams[3] = pipeline.rescale_image_and_camera(bgr[3], depths[3].shape, cams[3])
    return cams, depths, normals, bgr


def _others(n):
    return [[j for j in range(n) if j != k] for k in range(n)]


SCENES = {
    "rig_256x128": lambda: (*rig_inputs(256, 128, 4), [0, 1, 2, 3], _others(4)),
    "rig_50x30": lambda: (*rig_inputs(50, 30, 5), [0, 1, 2, 3, 4], _others(5)),
    # a view with zero points in the middle, -1 sources, the half-size view as source and reference
    "rig_50x30_edges": lambda: (*edge_rig_inputs(), [4, 2, 0, 3], [[0, 1, -1, 3], [0, 1], [1, 2, 3, 4], [0, -1, 4, 1]]),
    "sphere_64x32": lambda: (*dataset_inputs("sphere"), [0, 1, 2], _others(3)),
    "pinhole_64x32": lambda: (*dataset_inputs("pinhole"), [0, 1, 2], _others(3)),
}

ROOM_EXTENT = 10.0                      # the rig's room is 10 x 6 x 8
RIG_SIZES = {"single": 10.01, "coarse": 1.25, "middle": 0.15625, "fine": 0.009765625,
             "overflow": ROOM_EXTENT / (1 << 22)}
# Forced-table cases: (voxel size, force_slots = the smallest power of two above the scene's point count).  A cell
# wraps only when a probe run crosses the table's end, which at size 0.009765625 happens on neither rig (the
# restatement counts 0 there); at these sizes it counts 4 and 3 (test_voxel_restatement.py asserts > 0).
FORCED_TABLES = {"rig_50x30": (float(F32(1.0 / 180.0)), 4096), "rig_256x128": (float(F32(1.0 / 368.0)), 131072)}


def scene_sizes(name, pts):
    """The voxel sizes of a scene's cases: the rig's are the issue's, a dataset's are taken from its extent
    (one cell for the whole cloud, 8, 64 and 1024 cells along the longest axis, and 2^22, which overflows the index)."""
    if name.startswith("rig"):
        return dict(RIG_SIZES)
    ok = finite_points(pts)
    extent = float((pts[ok, :3].max(0) - pts[ok, :3].min(0)).max())
    return {"single": extent * 1.001, "coarse": extent / 8, "middle": extent / 64, "fine": extent / 1024,
            "overflow": extent / (1 << 22)}


@functools.lru_cache(maxsize=None)
def oracle_cloud(name):
    """The plain scene cloud of SCENES[name] from the CPU oracle, view after view."""
    cams, depths, normals, colours, refs, lists = SCENES[name]()
    of = fill(OracleFusion(cams), cams, depths, normals, colours)
    pts = np.concatenate([of.run(r, s) for r, s in zip(refs, lists)], 0)
    pts.setflags(write=False)
    return pts
