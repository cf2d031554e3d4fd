"""Test-side restatement of the visibility check of the voxel cloud (acmmp_fusion_voxel_visibility,
include/acmmp.h): sequential over views and window pixels, written from the header's six steps -- the oracle's
or_project through ctypes for step 1, detmath's f2i_sat for step 2, numpy float32 for the comparisons of step 3.
TEST INFRASTRUCTURE: RestatedVisibilityFusion has capi.Fusion's visibility surface so the pipeline and the GPU tests
can be checked against it, and constructed_cloud builds scene clouds whose classes are known by construction
(surface points, floaters in front of a wall, points behind it, points nowhere)."""
import ctypes as C
import functools

import numpy as np

import oracle
import voxel_clean_support as cs
import voxel_support as vs
from fusion_scene_support import dataset_inputs, f2i_sat, rig_inputs

F32 = np.float32
SUPPORT, CONFLICT, OCCLUDED, UNOBSERVED = 0, 1, 2, 3
MAX_LIST = 4096


def _camera_pointers(cams):
    cams = np.ascontiguousarray(cams)
    return cams, [C.c_void_p(cams[i:i + 1].ctypes.data) for i in range(len(cams))]


def project(cams, X):
    """Step 1 for every view and entry: (V, N, 3) float32 of (px, py, pd) = or_project(cam_v, X_e)."""
    cams, camp = _camera_pointers(cams)
    X = np.ascontiguousarray(X, F32).reshape(-1, 3)
    L, vp = oracle.lib(), C.c_void_p
    x, pt, d = np.zeros(3, F32), np.zeros(2, F32), C.c_float(0)
    xp, ptp = x.ctypes.data_as(vp), pt.ctypes.data_as(vp)
    out = np.zeros((len(cams), X.shape[0], 3), F32)
    for v in range(len(cams)):
        for e in range(X.shape[0]):
            x[:] = X[e]
            pt[:] = 0
            L.or_project(camp[v], xp, ptp, C.byref(d))
            out[v, e, 0], out[v, e, 1], out[v, e, 2] = pt[0], pt[1], d.value
    return out


def world_points(cam, cols, rows, depths):
    """or_world_point of pixel centres (cols, rows) at `depths`: (n, 3) float32."""
    cams, camp = _camera_pointers(np.asarray(cam).reshape(1))
    L, vp = oracle.lib(), C.c_void_p
    x = np.zeros(3, F32)
    out = np.zeros((len(cols), 3), F32)
    for i, (c, r, d) in enumerate(zip(cols, rows, depths)):
        L.or_world_point(camp[0], float(c), float(r), float(F32(d)), x.ctypes.data_as(vp))
        out[i] = x
    return out


def view_classes(proj, depth, rel_tol, radius):
    """Steps 2-4 for one view: the class of every entry from its projection proj (N, 3) and the view's raw depth."""
    depth = np.ascontiguousarray(depth, F32)
    H, W = depth.shape
    rel_tol = F32(rel_tol)
    px, py, pd = proj[:, 0], proj[:, 1], proj[:, 2]
    with np.errstate(all="ignore"):
        ok = np.isfinite(px) & np.isfinite(py) & np.isfinite(pd) & (pd > 0)
        c = f2i_sat(np.where(ok, px, F32(0)) + F32(0.5))
        r = f2i_sat(np.where(ok, py, F32(0)) + F32(0.5))
        ok &= (c >= 0) & (c < W) & (r >= 0) & (r < H)
        n = len(pd)
        any_s, agree, behind = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                cc, rr = c + dx, r + dy
                inside = ok & (cc >= 0) & (cc < W) & (rr >= 0) & (rr < H)          # no wrap across the seam
                sd = depth[np.where(inside, rr, 0), np.where(inside, cc, 0)]
                sample = inside & np.isfinite(sd) & (sd > 0)
                t = rel_tol * sd
                d = pd - sd
                assert t.dtype == F32 and d.dtype == F32
                any_s |= sample
                agree |= sample & (np.abs(d) <= t)
                behind |= sample & (d > t)
    return np.where(~any_s, UNOBSERVED, np.where(agree, SUPPORT, np.where(behind, OCCLUDED, CONFLICT))).astype(np.int8)


def check_arguments(n_views, have_view, views, rel_tol, radius, min_support, max_conflicts):
    views = [int(v) for v in views]
    if not 1 <= len(views) <= MAX_LIST or any(v < 0 or v >= n_views or not have_view[v] for v in views):
        raise ValueError("bad view list")
    with np.errstate(over="ignore"):
        tol = F32(rel_tol)
    if not np.isfinite(tol) or not tol >= 0 or radius not in (0, 1) or min_support < 0 or max_conflicts < 0:
        raise ValueError("bad visibility argument")
    return views


def visibility(cams, depths, X, views, rel_tol, radius=0, min_support=1, max_conflicts=0, proj=None):
    """Steps 1-6 over the entries X (N, 3 or 9).  Returns a dict: tallies (N, 3) int32, kept (entry indices,
    ascending) int64, n_unsupported, n_conflicting, class_totals (4 ints).  proj: project(cams, X), when at hand."""
    views = check_arguments(len(cams), [d is not None for d in depths], views, rel_tol, radius, min_support, max_conflicts)
    X = np.ascontiguousarray(X, F32)
    X = X.reshape(-1, X.shape[-1])[:, :3]
    if proj is None:
        proj = project(cams, X)
    cls = {v: view_classes(proj[v], depths[v], rel_tol, radius) for v in sorted(set(views))}
    tallies = np.zeros((X.shape[0], 4), np.int64)
    for v in views:                                              # a view listed twice counts twice
        for k in range(4):
            tallies[:, k] += cls[v] == k
    keep = (tallies[:, SUPPORT] >= min_support) & (tallies[:, CONFLICT] <= max_conflicts)
    return {"tallies": tallies[:, :3].astype(np.int32), "kept": np.flatnonzero(keep).astype(np.int64),
            "n_unsupported": int((tallies[:, SUPPORT] < min_support).sum()),
            "n_conflicting": int((tallies[:, CONFLICT] > max_conflicts).sum()),
            "class_totals": [int(x) for x in tallies.sum(0)]}


class RestatedVisibilityFusion(cs.RestatedCleanFusion):
    """RestatedCleanFusion with capi.Fusion's visibility surface computed by the restatement."""

    def __init__(self, cams):
        super().__init__(cams)
        self.visible = None
        self._proj = (None, None)

    def run_scene(self, refs, src_lists, unique=False):
        out = super().run_scene(refs, src_lists, unique=unique)
        self.visible = None
        return out

    def set_scene(self, points, ref_index=None, pixel=None, src_mask=None):
        out = super().set_scene(points, ref_index, pixel, src_mask)
        self.visible = None
        return out

    def voxelize(self, size, origin=None, min_points=1):
        out = super().voxelize(size, origin, min_points)
        self.visible = None
        return out

    def voxel_clean(self, connectivity=26, min_neighbours=0, min_component_voxels=1, min_component_points=1):
        out = super().voxel_clean(connectivity, min_neighbours, min_component_voxels, min_component_points)
        if self.visible is not None and self.visible["source"] == "clean":
            self.visible = None
        return out

    def source_entries(self, source):
        """(points, counts) of the entries a visibility call over `source` covers."""
        if source == "voxel" and self.voxels is not None:
            return self.voxels["points"], self.voxels["counts"]
        if source == "clean" and self.cleaned is not None:
            idx = self.cleaned["kept"]
            return self.voxels["points"][idx], self.voxels["counts"][idx]
        raise ValueError("no such source result")

    def voxel_visibility(self, views, rel_tol, radius=0, min_support=1, max_conflicts=0, source="voxel"):
        if source not in ("voxel", "clean"):
            raise ValueError("bad source")
        pts, cnt = self.source_entries(source)
        key = (self.cams.tobytes(), pts[:, :3].tobytes())          # step 1 depends on nothing else
        if self._proj[0] != key:
            self._proj = (key, project(self.cams, pts[:, :3]))
        v = visibility(self.cams, self.depths, pts, views, rel_tol, radius, min_support, max_conflicts, proj=self._proj[1])
        self.visible = dict(v, source=source, points=pts[v["kept"]].copy(), counts=cnt[v["kept"]].copy())
        return len(v["kept"]), {"unsupported": v["n_unsupported"], "conflicting": v["n_conflicting"],
                                "class_totals": v["class_totals"]}

    def visible_points(self, first, n, counts=False, tallies=False):
        total = 0 if self.visible is None else len(self.visible["kept"])
        if first < 0 or n < 0 or first + n > total:
            raise ValueError("range beyond the visible result")
        if n == 0:
            pts, cnt, tal = np.zeros((0, 9), F32), np.zeros(0, np.int32), np.zeros((0, 3), np.int32)
        else:
            pts, cnt = self.visible["points"][first:first + n].copy(), self.visible["counts"][first:first + n].copy()
            tal = self.visible["tallies"][self.visible["kept"][first:first + n]].copy()
        extra = tuple(a for a, on in ((cnt, counts), (tal, tallies)) if on)
        return (pts, *extra) if extra else pts

    def visibility_tallies(self, first, n):
        total = 0 if self.visible is None else len(self.visible["tallies"])
        if first < 0 or n < 0 or first + n > total:
            raise ValueError("range beyond the tallied source")
        return np.zeros((0, 3), np.int32) if n == 0 else self.visible["tallies"][first:first + n].copy()


# ---- constructed clouds: the fusion inputs of a rig and a scene cloud for set_scene

RIGS = {"sphere": lambda: rig_inputs(50, 30, 4), "pinhole": lambda: dataset_inputs("pinhole")}
N_PIXELS = 300                              # pixels of view 0 that get a floater and a point behind the wall


def pixel_rays(cams, depths, view, scale, n=N_PIXELS, seed=11):
    """World points on the rays of `n` pixels of `view` that have a depth, at scale x that depth.  Pixels of the
    image's border are left out: a SPHERE point on the seam's ray may project to column W, outside the image."""
    d = depths[view]
    inner = np.zeros(d.shape, bool)
    inner[1:-1, 1:-1] = True
    ok = np.flatnonzero(inner.reshape(-1) & np.isfinite(d).reshape(-1) & (d.reshape(-1) > 0))
    pick = np.sort(np.random.default_rng(seed).permutation(ok)[:n])
    rows, cols = np.divmod(pick, d.shape[1])
    return world_points(cams[view], cols, rows, d[rows, cols] * F32(scale))


def as_cloud(xyz, colour):
    pts = np.zeros((len(xyz), 9), F32)
    pts[:, :3] = xyz
    pts[:, 5] = 1.0
    pts[:, 6:] = colour
    return pts


def camera_centres(cams):
    """C = -R^T t per camera, in float64 rounded once."""
    return np.stack([-(np.asarray(c["R"], np.float64).reshape(3, 3).T @ np.asarray(c["t"], np.float64)) for c in cams]).astype(F32)


@functools.lru_cache(maxsize=None)
def constructed(rig):
    """(cams, depths, normals, colours, cloud, voxel size) of a rig: the cloud is the surface points of every view
    (each view's pixels at their own depth, every third pixel), floaters at half the depth and points at 1.5 x the
    depth along N_PIXELS rays of view 0, the camera centres and four points 20 scene extents outside.  The voxel size
    is 1/64 of the surface's extent, so that the whole cloud lies well inside the 2^21 cells of an axis."""
    cams, depths, normals, colours = RIGS[rig]()
    surface = []
    for v in range(len(cams)):
        d = depths[v]
        ok = np.flatnonzero(np.isfinite(d).reshape(-1) & (d.reshape(-1) > 0))[::3]
        rows, cols = np.divmod(ok, d.shape[1])
        surface.append(world_points(cams[v], cols, rows, d[rows, cols]))
    surface = np.concatenate(surface, 0)
    centres = camera_centres(cams)
    lo, hi = np.percentile(surface, 1, axis=0), np.percentile(surface, 99, axis=0)      # (PatchMatch depths have outliers)
    span = float((hi - lo).max())
    mid = ((hi + lo) / 2).astype(F32)
    far = mid[None, :] + np.array([[20, 0, 0], [0, -20, 0], [0, 0, 20], [-12, 9, -15]], F32) * F32(span)
    cloud = np.concatenate([as_cloud(surface, (200, 200, 200)),
                            as_cloud(pixel_rays(cams, depths, 0, 0.5), (255, 0, 0)),
                            as_cloud(pixel_rays(cams, depths, 0, 1.5), (0, 0, 255)),
                            as_cloud(centres, (0, 255, 0)), as_cloud(far, (0, 255, 255))], 0)
    cloud.setflags(write=False)
    return cams, depths, normals, colours, cloud, float(F32(span / 64))


TOLERANCES = (0.0, 0.01, 0.05)
THRESHOLDS = ((0, 0), (1, 0), (2, 1), (0, 4096))
