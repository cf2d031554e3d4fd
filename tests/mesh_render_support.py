"""Test-side restatement of the mesh rendered into a view (acmmp_fusion_mesh_render, include/acmmp.h): every pixel
against every face, vectorised numpy float64 written from the header's eight steps -- no bound, no queue, no atomics.
SPHERE rays restate PixelToDir in numpy float32 with the oracle's deterministic sine and cosine.  TEST INFRASTRUCTURE:
RestatedRenderFusion has capi.Fusion's render surface so the pipeline and the GPU tests can be checked against it."""
import numpy as np

import oracle
import voxel_mesh_support as ms
from acmmp import types

F32, F64 = np.float32, np.float64
PI_F = F32(3.141592654)
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
COUNTS = ("agree", "mesh_in_front", "mesh_behind", "mesh_only", "raw_only", "neither", "back_facing")
FACE_CHUNK = 256


def camera_of(cam):
    return np.asarray(cam).reshape(-1)[0]


def rays(cam):
    """Step 3: (H * W, 3) float64, row-major over pixels."""
    cam = camera_of(cam)
    W, H = int(cam["width"]), int(cam["height"])
    c, r = np.meshgrid(np.arange(W), np.arange(H))
    c, r = c.reshape(-1), r.reshape(-1)
    if int(cam["model"]) == types.SPHERE:
        cx, cy = F32(cam["params"][1]), F32(cam["params"][2])
        lon = (c.astype(F32) - cx) / F32(W) * F32(2.0) * PI_F
        lat = -(r.astype(F32) - cy) / F32(H) * PI_F
        assert lon.dtype == F32 and lat.dtype == F32
        sl, cl = oracle.detmath("sin", lon), oracle.detmath("cos", lon)
        sa, ca = oracle.detmath("sin", lat), oracle.detmath("cos", lat)
        d = np.stack([ca * sl, -sa, ca * cl], 1)
        assert d.dtype == F32
        return d.astype(F64)
    K = np.asarray(cam["K"], F32).astype(F64)
    return np.stack([(c.astype(F64) - K[2]) / K[0], (r.astype(F64) - K[5]) / K[4], np.ones(len(c))], 1)


def camera_frame(cam, vertices, faces):
    """Step 2: (T (nf, 3, 3) float64, the camera-frame vertices A, B, C of every face; skipped (nf,) bool)."""
    cam = camera_of(cam)
    R = np.asarray(cam["R"], F32).astype(F64)
    t = np.asarray(cam["t"], F32).astype(F64)
    X = np.asarray(vertices, F32).reshape(-1, 9)[:, :3].astype(F64)
    with np.errstate(all="ignore"):
        T = np.stack([((R[3 * k] * X[:, 0] + R[3 * k + 1] * X[:, 1]) + R[3 * k + 2] * X[:, 2]) + t[k] for k in range(3)], 1)
    T = T[np.asarray(faces, np.int64).reshape(-1, 3)]
    skipped = ~np.isfinite(T).all((1, 2))
    if int(cam["model"]) != types.SPHERE:
        skipped |= (T[:, :, 2] <= 0).any(1)
    return T, skipped


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(b, c):
    return (b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0])


def hits(d, T, sphere):
    """Steps 4 and 5 for the rays d (P, 3) against the faces T (n, 3, 3): (hit (P, n) bool, u, v, w, s, md float32)."""
    dd = [d[:, k][:, None] for k in range(3)]
    A, B, C = ([T[:, j, k][None, :] for k in range(3)] for j in range(3))
    with np.errstate(all="ignore"):
        u, v, w = _dot(dd, _cross(B, C)), _dot(dd, _cross(C, A)), _dot(dd, _cross(A, B))
        s = (u + v) + w
        inside = ((s > 0) & (u >= 0) & (v >= 0) & (w >= 0)) | ((s < 0) & (u <= 0) & (v <= 0) & (w <= 0))
        P = [((u * A[k] + v * B[k]) + w * C[k]) / s for k in range(3)]
        front = _dot(P, dd) > 0
        depth = np.sqrt((P[0] * P[0] + P[1] * P[1]) + P[2] * P[2]) if sphere else P[2]
        md = depth.astype(F32)
        hit = inside & front & np.isfinite(md) & (md > 0)
    return hit, u, v, w, s, md


def render(cam, vertices, faces, raw=None, rel_tol=0.01):
    """The whole definition.  raw: the view's raw depth (H, W), or None for view == -1.  Returns a dict: depth (H, W)
    float32, face (H, W) int32, normal and colour (H, W, 3) float32, counts (7 ints), skipped."""
    cam = camera_of(cam)
    W, H = int(cam["width"]), int(cam["height"])
    sphere = int(cam["model"]) == types.SPHERE
    V = np.asarray(vertices, F32).reshape(-1, 9)
    F = np.asarray(faces, np.int32).reshape(-1, 3)
    T, skipped = camera_frame(cam, V, F)
    d = rays(cam)
    P = W * H
    best = np.full(P, NONE, np.uint64)
    uvws = np.zeros((P, 4), F64)
    live = np.flatnonzero(~skipped)
    rows = np.arange(P)
    chunk = max(1, min(FACE_CHUNK, (1 << 21) // max(P, 1)))          # bounds the (pixels, faces) temporaries
    for a in range(0, len(live), chunk):
        idx = live[a:a + chunk]
        hit, u, v, w, s, md = hits(d, T[idx], sphere)
        key = (md.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)[None, :]
        key = np.where(hit, key, NONE)
        j = key.argmin(1)
        k = key[rows, j]
        better = k < best
        best = np.where(better, k, best)
        uvws[better] = np.stack([u[rows, j], v[rows, j], w[rows, j], s[rows, j]], 1)[better]
    won = best != NONE
    face = np.where(won, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    depth = np.where(won, (best >> np.uint64(32)).astype(np.uint32).view(F32), F32(0)).astype(F32)
    tri = F[np.where(won, face, 0)]
    u, v, w, s = (uvws[:, k][:, None] for k in range(4))
    with np.errstate(all="ignore"):
        attr = [V[tri[:, j]].astype(F64) for j in range(3)]
        N = ((u * attr[0][:, 3:6] + v * attr[1][:, 3:6]) + w * attr[2][:, 3:6]) / s
        length = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])[:, None]
        normal = np.where(won[:, None] & (length > 0), N / length, 0.0).astype(F32)
        col = ((u * attr[0][:, 6:9] + v * attr[1][:, 6:9]) + w * attr[2][:, 6:9]) / s
        colour = np.where(won[:, None], col, 0.0).astype(F32)
    out = {"depth": depth.reshape(H, W), "face": face.reshape(H, W), "normal": normal.reshape(H, W, 3),
           "colour": colour.reshape(H, W, 3), "back": (won & (uvws[:, 3] > 0)).reshape(H, W), "skipped": int(skipped.sum()),
           "width": W, "height": H}
    out["counts"] = counts_of(out, raw, rel_tol)
    return out


def counts_of(out, raw, rel_tol):
    """Step 8: the seven counts of a restated render against the raw depth map `raw` (None: view == -1, all zero)."""
    if raw is None:
        return [0] * 7
    depth, won = out["depth"].reshape(-1), out["face"].reshape(-1) >= 0
    sd = np.ascontiguousarray(raw, F32).reshape(-1)
    assert sd.shape == depth.shape
    with np.errstate(all="ignore"):
        have = np.isfinite(sd) & (sd > 0)
        t = F32(rel_tol) * sd
        diff = np.abs(depth - sd)
        assert t.dtype == F32 and diff.dtype == F32
        both = have & won
        agree = both & (diff <= t)
        front = both & ~agree & (depth < sd)
    return [int(agree.sum()), int(front.sum()), int((both & ~agree & ~front).sum()), int((won & ~have).sum()),
            int((have & ~won).sum()), int((~have & ~won).sum()), int(out["back"].sum())]


def info_of(out):
    """capi.Fusion.render_mesh's return value of a restated render."""
    return {"width": out["width"], "height": out["height"], "skipped": out["skipped"],
            "counts": dict(zip(COUNTS, out["counts"]))}


def check_mesh(vertices, faces):
    v = np.ascontiguousarray(vertices, F32).reshape(-1, 9)
    t = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    if t.size and (t.min() < 0 or t.max() >= v.shape[0]):
        raise ValueError("vertex index out of range")
    return v, t


class RestatedRenderFusion(ms.RestatedMeshFusion):
    """RestatedMeshFusion with capi.Fusion's set_mesh / render_mesh / render_maps computed by the restatement."""

    def __init__(self, cams):
        super().__init__(cams)
        self._rendered = None                      # (the mesh it shows, the restated render)

    def _keeping_a_set_mesh(self, call):
        kept = self.meshed if self.meshed is not None and self.meshed["source"] == "set" else None
        out = call()
        if kept is not None:
            self.meshed = kept                     # a mesh without a source outlives the scene and the voxels
        return out

    def run_scene(self, refs, src_lists, unique=False):
        return self._keeping_a_set_mesh(lambda: super(RestatedRenderFusion, self).run_scene(refs, src_lists, unique=unique))

    def set_scene(self, points, ref_index=None, pixel=None, src_mask=None):
        return self._keeping_a_set_mesh(lambda: super(RestatedRenderFusion, self).set_scene(points, ref_index, pixel, src_mask))

    def voxelize(self, size, origin=None, min_points=1):
        return self._keeping_a_set_mesh(lambda: super(RestatedRenderFusion, self).voxelize(size, origin, min_points))

    def set_mesh(self, vertices, faces):
        v, t = check_mesh(vertices, faces)
        self.meshed = {"vertices": v.copy(), "faces": t.copy(), "cells": np.zeros((0, 3), np.int32),
                       "tsdf": np.zeros((0, 2), np.int32), "entry": np.zeros(0, np.int64), "source": "set"}
        return v.shape[0], t.shape[0]

    def render_mesh(self, view=None, camera=None, rel_tol=0.01):
        if self.meshed is None:
            raise ValueError("no mesh result")
        with np.errstate(over="ignore"):
            tol = F32(rel_tol)
        if not np.isfinite(tol) or not tol >= 0:
            raise ValueError("bad rel_tol")
        if view is None:
            if camera is None:
                raise ValueError("view None needs a camera")
            cam, raw = camera_of(camera), None
            if int(cam["model"]) != int(self.cams[0]["model"]) or cam["width"] <= 0 or cam["height"] <= 0:
                raise ValueError("bad camera")
        else:
            if camera is not None or not 0 <= view < len(self.cams) or self.depths[view] is None:
                raise ValueError("bad view")
            cam, raw = self.cams[view], self.depths[view]
        out = render(cam, self.meshed["vertices"], self.meshed["faces"], raw, rel_tol)
        self._rendered = (self.meshed, out)
        return info_of(out)

    def render_maps(self):
        if self._rendered is None or self._rendered[0] is not self.meshed:
            raise ValueError("no render result")
        out = self._rendered[1]
        return tuple(out[k].copy() for k in ("depth", "face", "normal", "colour"))


# ---- the hand-built meshes of the render tests

def as_mesh(xyz, faces, normals=None, colours=None):
    """(vertices (n, 9) float32, faces (m, 3) int32) from positions; default normal (0, 0, 1), colour by vertex number."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    v = np.zeros((len(xyz), 9), F32)
    v[:, :3] = xyz
    v[:, 3:6] = (0, 0, 1) if normals is None else normals
    v[:, 6:9] = (np.arange(len(xyz), dtype=F32)[:, None] * F32(10) + np.array([1, 2, 3], F32)) if colours is None else colours
    return v, np.asarray(faces, np.int32).reshape(-1, 3)


BOX_FACES = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4),
             (1, 5, 7), (1, 7, 3)]


def box_mesh(half=(1.0, 1.5, 2.0), frame=None):
    """A closed box of twelve triangles around the origin: corner k at ((k&1), (k>>1)&1, k>>2) * 2 - 1 times `half` in
    the box's own frame, mapped by `frame` (3 x 3; its columns are the box's axes, orthogonal and of one length, in
    small integers so that every coordinate is exact in float32).  Vertex normals point outwards from the centre."""
    corners = np.array([[(k & 1) * 2 - 1, ((k >> 1) & 1) * 2 - 1, (k >> 2) * 2 - 1] for k in range(8)], F64) * np.asarray(half, F64)
    if frame is not None:
        corners = corners @ np.asarray(frame, F64).T
    assert (corners.astype(F32).astype(F64) == corners).all()
    normals = corners / np.linalg.norm(corners, axis=1)[:, None]
    return as_mesh(corners, BOX_FACES, normals=normals.astype(F32))


def box_distance(d, half, frame=None):
    """The float64 distance from the origin along the rays d (P, 3) to the box of box_mesh."""
    q = d if frame is None else np.linalg.solve(np.asarray(frame, F64), d.T).T
    with np.errstate(divide="ignore"):
        t = (np.asarray(half, F64)[None, :] / np.abs(q)).min(1)
    return t * np.sqrt((d * d).sum(1))


# Axes (1, 2, 2), (2, 1, -2), (-2, 2, -1): orthogonal, of length 3.  The corner 2 e1 + e2 + 2 e3 of the box of
# half-extents (2, 1, 2) is (0, 9, 0) and its opposite (0, -9, 0): the two poles of the SPHERE model, exactly.
POLE_FRAME, POLE_HALF = np.array([[1, 2, -2], [2, 1, 2], [2, -2, -1]], F64), (2.0, 1.0, 2.0)
# Axes (1, 0, -1), (0, 1, 0), (1, 0, 1): the vertical edge x = 0, z = -2 of the box of half-extents (1, 1.5, 1) lies in
# the half-plane of longitude +-pi, the seam.
SEAM_FRAME, SEAM_HALF = np.array([[1, 0, 1], [0, 1, 0], [-1, 0, 1]], F64), (1.0, 1.5, 1.0)


def sphere_camera(W, H):
    return types.make_camera(types.SPHERE, params=[W / (2 * np.pi), W / 2, H / 2], width=W, height=H, depth_min=0.1,
                             depth_max=100.0).reshape(1)


def pinhole_camera(W, H, f=40.0):
    return types.make_camera(types.PINHOLE, K=[f, 0, W // 2, 0, f, H // 2, 0, 0, 1], width=W, height=H, depth_min=0.1,
                             depth_max=100.0).reshape(1)
