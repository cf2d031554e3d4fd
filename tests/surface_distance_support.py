"""Point-to-triangle distances (acmmp_fusion_surface_distance, include/acmmp.h) restated in numpy: every valid query
against every valid face, step 3 in float64 in the stated operation order, the minimum of the 64-bit (distance bits,
face index) key, the summary in Python integers.  Also the restated plan of the device's face grid and the meshes and
queries the GPU tests measure."""
import functools
import math

import numpy as np

import cloud_align_support as ca
import cloud_distance_support as cd
import mesh_render_support as rs

F32, F64 = np.float32, np.float64
QUERIES = ("scene", "voxels", "clean", "visible", "reference")
SMALL_MAX = 64                                                    # kSurfSmallMax
NO_KEY = np.uint64(0xffffffffffffffff)


def transformed(xyz, M=None):
    """Step 1: the float32 positions read under the (3, 4) transform M as dist_load reads a point -- float64,
    ((M0 x + M1 y) + M2 z) + M3, rounded once to float32; without M the positions themselves."""
    P = cd.xyz_of(xyz)
    if M is None:
        return P
    M = np.asarray(M, F64).reshape(3, 4)
    x, y, z = (P[:, k].astype(F64) for k in range(3))
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([(((M[k, 0] * x + M[k, 1] * y) + M[k, 2] * z) + M[k, 3]).astype(F32) for k in range(3)], 1)


def corners(vertices, faces, M=None):
    """(A, B, C, ok): the float32 corners of every face after step 1, each (F, 3), and step 2's validity."""
    V = transformed(vertices, M)
    T = np.asarray(faces, np.int64).reshape(-1, 3)
    A, B, C = V[T[:, 0]], V[T[:, 1]], V[T[:, 2]]
    ok = np.isfinite(A).all(1) & np.isfinite(B).all(1) & np.isfinite(C).all(1)
    return A, B, C, ok


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def pair_d2(P, A, B, C):
    """Step 3 for every pair: (len(P), len(A)) float32; NaN where the pair is no candidate.  The lines are those of
    surf_pair_d2 (fusion_kernels.hip)."""
    p = np.asarray(P, F32).astype(F64)[:, None, :]
    a, b, c = (np.asarray(x, F32).astype(F64)[None, :, :] for x in (A, B, C))
    with np.errstate(all="ignore"):
        ap, bp, cp = p - a, p - b, p - c
        ab, ac, bc = b - a, c - a, c - b
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        k = lambda x: x[..., None]
        s = (va + vb) + vc
        cases = [(d1 <= 0) & (d2 <= 0),
                 (d3 >= 0) & (d4 <= d3),
                 (vc <= 0) & (d1 >= 0) & (d3 <= 0),
                 (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0),
                 (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
        offsets = [-ap,
                   -bp,
                   k(d1 / (d1 - d3)) * ab - ap,
                   -cp,
                   k(d2 / (d2 - d6)) * ac - ap,
                   k((d4 - d3) / ((d4 - d3) + (d5 - d6))) * bc - bp]
        e = np.select([k(c) for c in cases], offsets, default=(k(vb / s) * ab + k(vc / s) * ac) - ap)
        lo = np.minimum(np.minimum(-ap, -bp), -cp)
        hi = np.maximum(np.maximum(-ap, -bp), -cp)
        e = np.where(e < lo, lo, np.where(e > hi, hi, e))
        return ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]).astype(F32)


def summarise(n_query, n_valid, d2, nearest, md, taus):
    """Step 5: the SUMMARY_WORDS Python integers."""
    matched = nearest >= 0
    k = 1048576.0 / float(md)
    q = np.rint(np.sqrt(d2[matched].astype(F64)) * k).astype(np.int64)
    summary = [int(n_query), int(n_valid), int(matched.sum()), sum(int(x) for x in q)]
    for i in range(cd.MAX_TAU):
        summary.append(int((d2[matched] <= taus[i] * taus[i]).sum()) if i < len(taus) else 0)
    summary += [int(x) for x in np.bincount(np.minimum(q >> 12, cd.HIST_BINS - 1), minlength=cd.HIST_BINS)]
    assert len(summary) == cd.SUMMARY_WORDS
    return summary


def distances(Q, vertices, faces, max_dist, taus=(), M=None, rows=32):
    """Steps 1-5 of queries Q against the faces of the mesh, the vertices read under M.  Returns (d2 float32,
    nearest_face int32, summary, n_skipped)."""
    md, taus = cd.check_arguments(max_dist, taus)
    Q = cd.xyz_of(Q)
    A, B, C, ok = corners(vertices, faces, M)
    fidx = np.nonzero(ok)[0].astype(np.uint64)
    A, B, C = A[ok], B[ok], C[ok]
    vq = cd.valid(Q)
    d2 = np.full(len(Q), np.inf, F32)
    nearest = np.full(len(Q), -1, np.int32)
    m2 = md * md
    assert m2.dtype == F32
    qi = np.nonzero(vq)[0]
    if len(fidx):
        for r in range(0, len(qi), rows):
            part = qi[r:r + rows]
            d = pair_d2(Q[part], A, B, C)
            key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | fidx[None, :]
            key[np.isnan(d)] = NO_KEY                                     # step 3: not a candidate
            win = key.min(1)                                              # step 4: the order of the faces is invisible
            w = (win >> np.uint64(32)).astype(np.uint32).view(F32)
            with np.errstate(invalid="ignore"):
                hit = (win != NO_KEY) & (w <= m2)
            d2[part[hit]] = w[hit]
            nearest[part[hit]] = (win[hit] & np.uint64(0xffffffff)).astype(np.int64).astype(np.int32)
    assert not np.isnan(d2).any()
    return d2, nearest, summarise(len(Q), vq.sum(), d2, nearest, md, taus), int((~ok).sum())


# ---- the device's face grid, restated for the counts of acmmp_fusion_surface_plan

def auto_cell(lo, hi, n_faces):
    """surface_cell (fusion.cpp) without a forced cell (a box without area: the cube root is the platform's)."""
    e = [float(hi[k]) - float(lo[k]) for k in range(3)]
    cell = 2.0 * math.sqrt(((e[0] * e[1] + e[1] * e[2]) + e[2] * e[0]) / float(n_faces))
    if not cell > 0.0:
        cell = max(e) / float(np.cbrt(float(n_faces)))
    cell = max(cell, max(e) / 1048576.0)
    return cell if cell > 0.0 else 1.0


def plan(vertices, faces, small_max=0, force_cell=0.0, M=None):
    """{"small", "large", "registrations", "skipped", "cell"} of a surface call over the mesh: the valid faces' box, the
    cell, the cells floor(((double)x - o) * (1 / cell)) clamped to the grid that every face's vertex box spans."""
    A, B, C, ok = corners(vertices, faces, M)
    out = {"small": 0, "large": 0, "registrations": 0, "skipped": int((~ok).sum()), "cell": 0.0}
    if not ok.any():
        return out
    X = np.stack([A[ok], B[ok], C[ok]], 1)                                # (F, 3 corners, 3 axes)
    lo, hi = X.min((0, 1)).astype(F64), X.max((0, 1)).astype(F64)
    cell = auto_cell(lo, hi, len(X)) if force_cell == 0.0 else max(float(F32(force_cell)), float((hi - lo).max()) / 1048576.0)
    inv = 1.0 / cell
    cmax = np.floor((hi - lo) * inv)
    index = lambda x: np.clip(np.floor((x.astype(F64) - lo) * inv), 0, cmax)
    cells = (index(X.max(1)) - index(X.min(1)) + 1).prod(1)
    limit = SMALL_MAX if small_max == 0 else small_max
    large = np.ones(len(X), bool) if limit < 0 else cells > limit
    out.update(small=int((~large).sum()), large=int(large.sum()), registrations=int(cells[~large].sum()), cell=float(F32(cell)))
    return out


# ---- meshes and queries of the tests

def cube():
    """The 12-face unit cube around the origin: every coordinate +-0.5."""
    return rs.box_mesh((0.5, 0.5, 0.5))


def cube_surface_distance(P):
    """The float64 distance from the points P to the surface of cube()."""
    q = np.abs(np.asarray(P, F32).astype(F64)) - 0.5
    outside = np.sqrt((np.maximum(q, 0.0) ** 2).sum(1))
    return np.where((q <= 0).all(1), -q.max(1), outside)


def cube_surface_points(n, seed=0):
    """n float32 points on the faces of cube(): one coordinate +-0.5, the others uniform in [-0.5, 0.5)."""
    rng = np.random.default_rng(seed)
    P = (rng.random((n, 3), dtype=F32) - F32(0.5)).astype(F32)
    axis, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
    P[np.arange(n), axis] = np.where(side == 1, F32(0.5), F32(-0.5))
    return P


@functools.lru_cache(maxsize=None)
def rig_mesh():
    """The surface-nets mesh of the constructed sphere rig's voxel cloud, from the restated chain: a few thousand faces
    of about one voxel.  Returns (vertices (n, 9), faces (m, 3), voxel size)."""
    import voxel_mesh_support as ms
    from fusion_scene_support import fill
    cams, depths, normals, colours, cloud, size, trunc, _ = ms.base_case("sphere")
    rf = fill(ms.RestatedMeshFusion(cams), cams, depths, normals, colours)
    rf.set_scene(cloud)
    rf.voxelize(size)
    nv, nf, _ = rf.voxel_mesh(list(range(len(cams))), trunc)
    assert 2000 < nf < 20000
    return rf.mesh_vertices(0, nv), rf.mesh_faces(0, nf), size


@functools.lru_cache(maxsize=None)
def mixed_mesh(seed=3, n=16):
    """About 500 small faces -- a jittered n x n sheet in the unit cube -- and two faces that span the whole box: the
    overflow list together with the grid."""
    rng = np.random.default_rng(seed)
    g = np.linspace(0.0, 1.0, n + 1)
    x, y = np.meshgrid(g, g, indexing="ij")
    z = 0.5 + 0.1 * np.sin(5 * x) * np.cos(4 * y) + 0.01 * rng.standard_normal(x.shape)
    sheet = np.stack([x, y, z], -1).reshape(-1, 3)
    idx = lambda i, j: i * (n + 1) + j
    faces = [f for i in range(n) for j in range(n)
             for f in ((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))]
    k = len(sheet)
    span = np.array([[0, 0, 0], [1, 1, 0.1], [0, 1, 1], [1, 0, 1]], F64)
    faces += [(k, k + 1, k + 2), (k + 1, k + 2, k + 3)]
    return rs.as_mesh(np.concatenate([sheet, span]), faces)


def boundary_mesh():
    """A 4 x 4 sheet in the plane z = 0.5 of the unit box -- with cells of 0.25 from the origin, the plane between two
    cells -- and one face through the box's corners (0, 0, 0), (1, 1, 1), (1, 0, 0)."""
    g = np.arange(5) / 4.0
    x, y = np.meshgrid(g, g, indexing="ij")
    sheet = np.stack([x, y, np.full_like(x, 0.5)], -1).reshape(-1, 3)
    idx = lambda i, j: i * 5 + j
    faces = [t for i in range(4) for j in range(4)
             for t in ((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))]
    return rs.as_mesh(np.concatenate([sheet, [[0, 0, 0], [1, 1, 1], [1, 0, 0]]]), faces + [(25, 26, 27)])


def invalid_mesh():
    """Six faces: 0 and 2 have a non-finite vertex, 1 and 5 are one proper triangle in both orders, 3 is a needle
    (A == B), 4 a point (A == B == C)."""
    A = [0.25, -0.5, 0.125]
    v = rs.as_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, np.nan], [np.inf, 0, 5], A, A, [1.25, -0.5, 0.125], A], [[0, 1, 2]])[0]
    return v, np.array([[0, 1, 3], [0, 1, 2], [4, 1, 2], [5, 6, 7], [5, 6, 8], [2, 1, 0]], np.int32)


# A rotation about z by atan(7 / 24) and a shift: the transform of the GPU tests.
M_TEST = np.array([[0.96, -0.28, 0.0, 0.25], [0.28, 0.96, 0.0, -0.5], [0.0, 0.0, 1.0, 0.125]], F64)


def rig_part():
    """The first 1500 faces of rig_mesh() over all its vertices: the mesh of the GPU tests' chain."""
    v, f, _ = rig_mesh()
    return v, f[:1500]


def gpu_test_meshes():
    """name -> (vertices, faces, M): every mesh test_gpu_surface_distance.py measures, with the transform its vertices
    are read under."""
    moved = (cube()[0].copy(), cube()[1])
    moved[0][:, :3] += F32(1e4)
    rv, rf, _ = rig_mesh()
    return {"cube": (*cube(), None), "cube + 1e4": (*moved, None), "rig": (rv, rf, None), "mixed": (*mixed_mesh(), None),
            "boundary plane": (*boundary_mesh(), None), "invalid and degenerate": (*invalid_mesh(), None),
            "rig part": (*rig_part(), None), "rig part under M_TEST": (*rig_part(), M_TEST)}


def near_queries(vertices, faces, n, spread, seed=0):
    """n float32 queries: points of random faces moved by a normal deviate of `spread`, a tenth of them ten times as
    far, and a few far outside the box."""
    rng = np.random.default_rng(seed)
    V, T = cd.xyz_of(vertices).astype(F64), np.asarray(faces, np.int64)
    t = T[rng.integers(0, len(T), n)]
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    P = (w[:, :, None] * V[t]).sum(1)
    scale = np.where(rng.random(n) < 0.1, 10.0 * spread, spread)
    P += scale[:, None] * rng.standard_normal((n, 3))
    P[::37] += 50.0 * spread
    return P.astype(F32)


def summary_of(r):
    return cd.summary_of(r)


class RestatedSurfaceFusion(ca.RestatedAlignFusion):
    """RestatedAlignFusion with capi.Fusion's surface_distance / surface_results computed by the restatement: reference
    queries see the mesh under the transform, data queries do not.  The result is per call; the lifetimes are the GPU
    tests' matter."""

    def __init__(self, cams):
        super().__init__(cams)
        self._surface = None

    def surface_distance(self, query="reference", max_dist=1.0, thresholds=()):
        if query not in QUERIES:
            raise ValueError("bad query")
        if self.meshed is None:
            raise ValueError("no mesh result")
        if query == "reference":
            if self.reference is None:
                raise ValueError("no reference cloud")
            q, M = self.reference, self._transform
        else:
            q, M = cd.RestatedDistanceFusion._data(self, query)[1], None
        d2, nearest, words, _ = distances(q, self.meshed["vertices"], self.meshed["faces"], max_dist, thresholds, M=M)
        self._surface = (d2, nearest)
        return cd.Summary(words, max_dist, len(tuple(thresholds)))

    def surface_results(self, first=0, n=None, squared=False):
        d2, nn = self._surface if self._surface is not None else (np.zeros(0, F32), np.zeros(0, np.int32))
        n = len(d2) - first if n is None else n
        if first < 0 or n < 0 or first + n > len(d2):
            raise ValueError("range beyond the surface result")
        d2 = d2[first:first + n].copy()
        return (d2 if squared else np.sqrt(d2)), nn[first:first + n].copy()
