"""Test-side restatement of the surface mesh of the voxel cloud (acmmp_fusion_voxel_mesh, include/acmmp.h): sequential
numpy and dicts, written from the header's four steps -- a dict from cell to sample for step 1, the oracle's
or_project (visibility_support.project) and numpy float32 for the distances of step 2, Python floats (IEEE float64,
no contraction) for the vertices of step 3, plain loops for the faces of step 4.  TEST INFRASTRUCTURE:
RestatedMeshFusion has capi.Fusion's mesh surface so the pipeline and the GPU tests can be checked against it."""
import math

import numpy as np

import visibility_support as vis
import voxel_clean_support as cs
import voxel_support as vs
from fusion_scene_support import f2i_sat

F32 = np.float32
CELLS = vs.CELLS
MAX_LIST = vis.MAX_LIST
EDGES = ((0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7))
QUAD = ((0, 0), (1, 0), (1, 1), (0, 1))
FALLBACK = 128.0


def pack(cells):
    c = np.asarray(cells, np.uint64).reshape(-1, 3)
    return c[:, 0] | (c[:, 1] << np.uint64(21)) | (c[:, 2] << np.uint64(42))


def samples_of(cells):
    """Step 1: (sample cells in sample order as a list of tuples, dict cell -> sample, remembered entry per sample)."""
    index, order, entry = {}, [], []
    for e, (x, y, z) in enumerate(cells):
        for dz in (-1, 0, 1):                                  # ascending (dz+1)*9 + (dy+1)*3 + (dx+1)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    c = (x + dx, y + dy, z + dz)
                    if min(c) < 0 or max(c) >= CELLS:
                        continue
                    s = index.get(c)
                    if s is None:                              # first seen in ascending (e, d): the smallest rank
                        s = index[c] = len(order)
                        order.append(c)
                        entry.append(-1)
                    if dx == dy == dz == 0:
                        assert entry[s] == -1, "at most one entry has a cell"
                        entry[s] = e
    return order, index, np.array(entry, np.int64).reshape(len(order))


def centres(sample_cells, origin, size):
    """X(s): per axis (float)((double)o + ((double)g + 0.5) * (double)voxel_size)."""
    g = np.asarray(sample_cells, np.float64).reshape(-1, 3)
    return (np.asarray(origin, F32).astype(np.float64)[None, :] + (g + 0.5) * np.float64(F32(size))).astype(F32)


def view_distance(proj, depth, trunc):
    """Step 2 for one view: (q int64, contributes bool) per sample from its projection proj (N, 3)."""
    depth = np.ascontiguousarray(depth, F32)
    H, W = depth.shape
    trunc = F32(trunc)
    k = F32(1024.0) / trunc
    px, py, pd = proj[:, 0], proj[:, 1], proj[:, 2]
    with np.errstate(all="ignore"):
        ok = np.isfinite(px) & np.isfinite(py) & np.isfinite(pd) & (pd > 0)
        c = f2i_sat(np.where(ok, px, F32(0)) + F32(0.5))
        r = f2i_sat(np.where(ok, py, F32(0)) + F32(0.5))
        ok &= (c >= 0) & (c < W) & (r >= 0) & (r < H)
        sd = depth[np.where(ok, r, 0), np.where(ok, c, 0)]
        ok &= np.isfinite(sd) & (sd > 0)
        u = np.where(ok, sd - pd, F32(0))
        assert u.dtype == F32 and k.dtype == F32
        ok &= ~(u < -trunc)
        q = np.rint(np.minimum(u, trunc) * k)
        assert q.dtype == F32
    return np.where(ok, q, 0).astype(np.int64), ok


def check_arguments(n_views, have_view, views, trunc, min_weight):
    views = [int(v) for v in views]
    if not 1 <= len(views) <= MAX_LIST or any(v < 0 or v >= n_views or not have_view[v] for v in views):
        raise ValueError("bad view list")
    with np.errstate(over="ignore"):
        t = F32(trunc)
    if not np.isfinite(t) or not t > 0 or min_weight < 1:
        raise ValueError("bad mesh argument")
    return views


def tsdf_of(cams, depths, X, views, trunc, proj=None):
    """(S, n) int64 per sample over the list `views` (a view listed twice counts twice).  proj: vis.project(cams, X),
    when at hand."""
    S, n = np.zeros(len(X), np.int64), np.zeros(len(X), np.int64)
    if proj is None:
        proj = vis.project(cams, X)
    per = {v: view_distance(proj[v], depths[v], trunc) for v in sorted(set(views))}
    for v in views:
        S += per[v][0]
        n += per[v][1]
    return S, n


def extract(order, index, entry, S, n, colours, origin, size, min_weight):
    """Steps 3 and 4 from the samples' cells, sums and remembered entries.  Returns (vertices (nv, 9) float32, faces
    (nf, 3) int32, cube_exists bool per sample, n_uncoloured, face_stats {(axis, s_inside): pairs})."""
    ns = len(order)
    S, n = [int(x) for x in S], [int(x) for x in n]
    valid = [k >= min_weight for k in n]
    inside = [x < 0 for x in S]
    o = [float(x) for x in np.asarray(origin, F32)]
    size = float(F32(size))
    exists, corners_of, vid = [False] * ns, [None] * ns, [-1] * ns
    verts, uncoloured = [], 0
    for s, g in enumerate(order):
        cs_ = [index.get((g[0] + (c & 1), g[1] + ((c >> 1) & 1), g[2] + (c >> 2))) for c in range(8)]
        if any(q is None or not valid[q] for q in cs_):
            continue
        exists[s], corners_of[s] = True, cs_
        if len({inside[q] for q in cs_}) == 1:
            continue
        L, G, crossings = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], 0
        for k, (p, q) in enumerate(EDGES):
            ax = k // 4
            sp, sq = cs_[p], cs_[q]
            fp, fq = S[sp] / (1024.0 * n[sp]), S[sq] / (1024.0 * n[sq])
            G[ax] += fq - fp
            if inside[sp] == inside[sq]:
                continue
            A, B = float(S[sp] * n[sq]), float(S[sq] * n[sp])
            t = A / (A - B)
            for a in range(3):
                L[a] += float((p >> a) & 1) + (t if a == ax else 0.0)
            crossings += 1
        length = math.sqrt(G[0] * G[0] + G[1] * G[1] + G[2] * G[2])
        pos = [o[a] + ((g[a] + 0.5) + L[a] / crossings) * size for a in range(3)]
        nrm = [G[a] / length if length > 0.0 else 0.0 for a in range(3)]
        mem = [int(entry[q]) for q in cs_ if entry[q] >= 0]
        if mem:
            col = [0.0, 0.0, 0.0]
            for e in mem:
                for a in range(3):
                    col[a] += float(colours[e][a])
            col = [c / len(mem) for c in col]
        else:
            col = [FALLBACK] * 3
            uncoloured += 1
        vid[s] = len(verts)
        verts.append(pos + nrm + col)
    faces, stats = [], {}
    for s, g in enumerate(order):
        for a in range(3):
            e_a = [int(k == a) for k in range(3)]
            o_s = index.get((g[0] + e_a[0], g[1] + e_a[1], g[2] + e_a[2]))
            if o_s is None or not (valid[s] and valid[o_s]) or inside[s] == inside[o_s]:
                continue
            b, c = (a + 1) % 3, (a + 2) % 3
            quad = []
            for u, v in QUAD:
                cell = list(g)
                cell[b] -= u
                cell[c] -= v
                quad.append(index.get(tuple(cell)))
            if any(q is None or not exists[q] for q in quad):
                continue
            Q = [vid[q] for q in quad]
            assert min(Q) >= 0, "four cubes around a sign change are active"
            faces += [(Q[0], Q[1], Q[2]), (Q[0], Q[2], Q[3])] if inside[s] else [(Q[0], Q[3], Q[2]), (Q[0], Q[2], Q[1])]
            stats[(a, inside[s])] = stats.get((a, inside[s]), 0) + 1
    with np.errstate(over="ignore"):
        V = np.array(verts, np.float64).reshape(-1, 9).astype(F32)
    return V, np.array(faces, np.int32).reshape(-1, 3), np.array(exists, bool).reshape(ns), uncoloured, stats


def mesh(cells, colours, origin, size, cams, depths, views, trunc, min_weight=1, cache=None):
    """The whole definition over entries given by their cells (ne, 3) and colour floats (ne, 3).  cache: a dict that
    keeps the projections of the last sample set (they depend on the cells and the cameras alone)."""
    views = check_arguments(len(cams), [d is not None for d in depths], views, trunc, min_weight)
    cells = [tuple(int(x) for x in c) for c in np.asarray(cells, np.int64).reshape(-1, 3)]
    order, index, entry = samples_of(cells)
    if order:
        X = centres(order, origin, size)
        key = (np.ascontiguousarray(cams).tobytes(), X.tobytes())
        if cache is None or cache.get("key") != key:
            cache = {} if cache is None else cache
            cache["key"], cache["proj"] = key, vis.project(cams, X)
        S, n = tsdf_of(cams, depths, X, views, trunc, proj=cache["proj"])
    else:
        S, n = np.zeros(0, np.int64), np.zeros(0, np.int64)
    V, F, exists, uncoloured, stats = extract(order, index, entry, S, n, colours, origin, size, min_weight)
    return {"vertices": V, "faces": F, "cells": np.array(order, np.int32).reshape(-1, 3),
            "tsdf": np.stack([S, n], 1).astype(np.int32), "entry": entry, "face_stats": stats,
            "info": {"samples": len(order), "valid": int((n >= min_weight).sum()), "cubes": int(exists.sum()),
                     "uncoloured": int(uncoloured)}}


def table_wrapped(sample_cells, slots):
    """The sample table's cells stored below their home slot (independent of the order of arrival)."""
    return vs.table_layout(pack(sample_cells), slots)[1]


def auto_slots(n_entries):
    s = 1024
    while s < 54 * n_entries:
        s *= 2
    return s


class RestatedMeshFusion(vis.RestatedVisibilityFusion):
    """RestatedVisibilityFusion with capi.Fusion's mesh surface computed by the restatement."""

    def __init__(self, cams):
        super().__init__(cams)
        self.meshed = None
        self.voxel_size = None
        self._mesh_cache = {}

    def run_scene(self, refs, src_lists, unique=False):
        out = super().run_scene(refs, src_lists, unique=unique)
        self.meshed = None
        return out

    def set_scene(self, points, ref_index=None, pixel=None, src_mask=None):
        out = super().set_scene(points, ref_index, pixel, src_mask)
        self.meshed = None
        return out

    def voxelize(self, size, origin=None, min_points=1):
        out = super().voxelize(size, origin, min_points)
        self.meshed, self.voxel_size = None, F32(size)
        return out

    def voxel_clean(self, *args, **kw):
        vis_gone = self.visible is not None and self.visible["source"] == "clean"
        out = super().voxel_clean(*args, **kw)
        if self.meshed is not None and (self.meshed["source"] == "clean" or (self.meshed["source"] == "visible" and vis_gone)):
            self.meshed = None
        return out

    def voxel_visibility(self, *args, **kw):
        out = super().voxel_visibility(*args, **kw)
        if self.meshed is not None and self.meshed["source"] == "visible":
            self.meshed = None
        return out

    def mesh_entries(self, source):
        """(voxel index per entry, the entries' 9 floats) of a mesh call over `source`."""
        if source == "voxel" and self.voxels is not None:
            idx = np.arange(len(self.voxels["keys"]), dtype=np.int64)
        elif source == "clean" and self.cleaned is not None:
            idx = self.cleaned["kept"]
        elif source == "visible" and self.visible is not None:
            idx = self.visible["kept"] if self.visible["source"] == "voxel" else self.cleaned["kept"][self.visible["kept"]]
        else:
            raise ValueError("no such source result")
        return idx, self.voxels["points"][idx]

    def voxel_mesh(self, views, trunc, min_weight=1, source="voxel"):
        if source not in ("voxel", "clean", "visible"):
            raise ValueError("bad source")
        idx, pts = self.mesh_entries(source)
        cells = np.array(cs.unpack(self.voxels["keys"][idx]), np.int64).reshape(-1, 3)
        m = mesh(cells, pts[:, 6:9], self.voxels["origin"], self.voxel_size, self.cams, self.depths, views, trunc, min_weight,
                 cache=self._mesh_cache)
        self.meshed = dict(m, source=source)
        return len(m["vertices"]), len(m["faces"]), dict(m["info"])

    def _range(self, key, first, n, what):
        total = 0 if self.meshed is None else len(self.meshed[key])
        if first < 0 or n < 0 or first + n > total:
            raise ValueError(f"range beyond the mesh result's {what}")

    def mesh_vertices(self, first, n):
        self._range("vertices", first, n, "vertices")
        return np.zeros((0, 9), F32) if n == 0 else self.meshed["vertices"][first:first + n].copy()

    def mesh_faces(self, first, n):
        self._range("faces", first, n, "faces")
        return np.zeros((0, 3), np.int32) if n == 0 else self.meshed["faces"][first:first + n].copy()

    def mesh_samples(self, first, n):
        self._range("cells", first, n, "samples")
        if n == 0:
            return np.zeros((0, 3), np.int32), np.zeros((0, 2), np.int32), np.zeros(0, np.int64)
        return tuple(self.meshed[k][first:first + n].copy() for k in ("cells", "tsdf", "entry"))


# ---- the inputs of the mesh tests

# rig -> (voxel size as a fraction of visibility_support.constructed's, trunc in voxel sizes, the small trunc at which
# most contributions saturate or are hidden).  test_voxel_mesh_restatement.py asserts what the GPU cases rely on.
BASE = {"sphere": (1.0, 3.0, 0.05), "pinhole": (1.0, 3.0, 0.05)}


def base_case(rig):
    """(cams, depths, normals, colours, cloud, voxel size, trunc, small trunc) of a rig's base case."""
    cams, depths, normals, colours, cloud, size = vis.constructed(rig)
    k, t, small = BASE[rig]
    size = float(F32(size * k))
    return cams, depths, normals, colours, cloud, size, float(F32(size * t)), float(F32(size * small))


def wall_scene(n=12, depth=4.0, size=0.25, W=64, H=48):
    """One pinhole camera at the origin looking down +z at a wall z = depth: (cams, depths, cells, origin, size).  The
    cells are an n x n block of the grid, two cells from its boundary and centred on the optical axis, that the wall's plane passes through."""
    from acmmp import types
    cam = types.make_camera(types.PINHOLE, K=[40.0, 0, W / 2, 0, 40.0, H / 2, 0, 0, 1], width=W, height=H,
                            depth_min=0.1, depth_max=100.0).reshape(1)
    depths = [np.full((H, W), depth, F32)]
    origin = np.array([-(n / 2 + 2) * size, -(n / 2 + 2) * size, 0.0], F32)
    gz = int(math.floor(depth / size))
    cells = [(x, y, gz) for y in range(2, n + 2) for x in range(2, n + 2)]
    return cam, depths, cells, origin, size
