"""Evaluation regions (acmmp_fusion_set_region, include/acmmp.h) restated in numpy float64: the class byte of every point
under planes, a polygon prism and a bit grid, every part evaluated for every valid point; and the fixtures the tests
classify -- a concave polygon with queries on its vertices and edges, a 5 x 7 x 9 grid with queries at exact half-cell
offsets, eight planes with queries at s == 0 and s == -0.0, invalid points, 2 051 points in all."""
import functools
import os

import numpy as np

import cloud_align_support as ca
import cloud_distance_support as cd
from acmmp import io

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INVALID, PLANES, PRISM, GRID = 1, 2, 4, 8                      # ACMMP_REGION_CLASS_*
COUNTS = ("points", "invalid", "inside", "planes", "prism", "grid")
N_CLOUD = 2051                                                  # 8 full workgroups and a partial wave


# ---- the definition

def crossing_parity(polygon, pu, pv):
    """Bit 2's parity for points (pu, pv), float64 arrays: True = odd.  Edge i runs to j = (i + 1) mod n and toggles when
    (v_i > p_v) != (v_j > p_v) and p_u < (((u_j - u_i) * (p_v - v_i)) / (v_j - v_i)) + u_i."""
    poly = np.asarray(polygon, np.float64).reshape(-1, 2)
    odd = np.zeros(len(pu), bool)
    n = len(poly)
    for i in range(n):
        (ui, vi), (uj, vj) = poly[i], poly[(i + 1) % n]
        straddle = (vi > pv) != (vj > pv)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            cross = (((uj - ui) * (pv - vi)) / (vj - vi)) + ui
            odd ^= straddle & (pu < cross)
    return odd


def grid_indices(region, p):
    """i_a = rint((p_a - o_a) / c) per axis, float64 (ties to even), for valid points p (n, 3) float64."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.rint((p - np.asarray(region.origin, np.float64)[None, :]) / np.float64(region.cell))


def grid_bit(region, ix, iy, iz):
    """The bit of cell (ix, iy, iz), Python integers inside the grid."""
    nx, ny, _ = region.dims
    k = ix + nx * (iy + ny * iz)
    return (int(region.bits[k >> 3]) >> (k & 7)) & 1


def classify(xyz, region, M=None):
    """The class bytes of the definition: xyz (n, 3) float32 read under M (3x4, None: as they are), region an io.Region
    or None (every valid point is inside)."""
    x32 = cd.xyz_of(xyz) if M is None else ca.transform_points(M, xyz)
    cls = np.zeros(len(x32), np.uint8)
    ok = np.isfinite(x32).all(1)
    cls[~ok] = INVALID
    if region is None or not ok.any():
        return cls
    p = x32[ok].astype(np.float64)
    out = np.zeros(len(p), np.uint8)
    if region.planes is not None:
        fail = np.zeros(len(p), bool)
        for a, b, c, d in np.asarray(region.planes, np.float64).reshape(-1, 4):
            with np.errstate(over="ignore", invalid="ignore"):
                s = ((a * p[:, 0] + b * p[:, 1]) + c * p[:, 2]) + d
            fail |= ~(s >= 0.0)
        out[fail] |= PLANES
    if region.polygon is not None:
        w = int(region.axis)
        u, v = [k for k in range(3) if k != w]
        inside = (p[:, w] >= region.axis_min) & (p[:, w] <= region.axis_max) & crossing_parity(region.polygon, p[:, u], p[:, v])
        out[~inside] |= PRISM
    if region.dims is not None:
        idx = grid_indices(region, p)
        dims = np.asarray(region.dims, np.float64)
        inside = ((idx >= 0.0) & (idx < dims[None, :])).all(1)                 # compared in float64, before any conversion
        for r in np.nonzero(inside)[0]:
            inside[r] = bool(grid_bit(region, *(int(t) for t in idx[r])))
        out[~inside] |= GRID
    cls[ok] = out
    return cls


def counts(cls):
    """acmmp_fusion_region_classify's six integers."""
    cls = np.asarray(cls, np.uint8)
    return {"points": len(cls), "invalid": int((cls == INVALID).sum()), "inside": int((cls == 0).sum()),
            "planes": int(((cls & PLANES) != 0).sum()), "prism": int(((cls & PRISM) != 0).sum()),
            "grid": int(((cls & GRID) != 0).sum())}


def substituted(points, cls):
    """The cloud with x replaced by NaN where the class is not 0: what the measuring calls must see."""
    out = np.array(points, F32, copy=True)
    out[np.asarray(cls) != 0, 0] = np.nan
    return out


def as_points(xyz, seed=7):
    """cloud_distance_support.as_points with unit normals in every direction, the same for the same row whatever its
    position holds: the point-to-plane fit is singular on parallel normals."""
    p = cd.as_points(xyz)
    n = np.random.default_rng(seed).standard_normal((len(p), 3))
    p[:, 3:6] = (n / np.linalg.norm(n, axis=1)[:, None]).astype(F32)
    return p


# ---- the fixtures

# nine vertices, concave: the unit square with a notch cut down from its top edge between u = 0.5 and 0.75 to v = 0.5, and
# its top left corner cut off from (0.25, 1) to (0, 0.5).  Every coordinate is a binary fraction.
POLYGON = np.array([(0, 0), (1, 0), (1, 1), (0.75, 1), (0.75, 0.5), (0.5, 0.5), (0.5, 1), (0.25, 1), (0, 0.5)], np.float64)
AXIS_MIN, AXIS_MAX = -0.25, 0.75
TRIANGLE = np.array([(0.125, 0.125), (0.875, 0.25), (0.375, 0.875)], np.float64)

# (u, v) -> inside, by the rule: points on a left or a bottom edge of the interior are inside, on a right or a top edge
# outside (the derivations are in test_eval_region_restatement.py)
ON_BOUNDARY = (
    ((0.5, 0.0), True),       # the bottom edge
    ((0.875, 1.0), False),    # the top edge: nothing is above v = 1
    ((0.375, 1.0), False),
    ((1.0, 0.5), False),      # the right edge
    ((0.0, 0.25), True),      # the left edge
    ((0.625, 0.5), False),    # the notch's floor: a top edge of the interior below it, collinear with v = 0.5
    ((0.75, 0.75), True),     # the notch's right wall: a left edge of the interior beside it
    ((0.5, 0.75), False),     # the notch's left wall: a right edge
    ((0.125, 0.75), True),    # the cut corner: a left edge
    ((0.0, 0.0), True), ((1.0, 0.0), False), ((1.0, 1.0), False), ((0.75, 1.0), False), ((0.75, 0.5), True),
    ((0.5, 0.5), False), ((0.5, 1.0), False), ((0.25, 1.0), False), ((0.0, 0.5), True),          # the nine vertices
)
# v = 0.5 is collinear with the notch's floor; these are on no edge
COLLINEAR = (((0.25, 0.5), True), ((0.875, 0.5), True), ((-0.5, 0.5), False), ((2.0, 0.5), False), ((-1.0, 1.0), False),
             ((0.625, 1.0), False), ((-1.0, 0.0), False), ((2.0, 0.0), False))

GRID_DIMS, GRID_ORIGIN, GRID_CELL = (5, 7, 9), (0.0, 0.125, -0.25), 0.125


def grid_cell_set(ix, iy, iz):
    """The fixture's ObsMask: three cells of four are set."""
    return (3 * ix + 5 * iy + 7 * iz) % 4 != 0


def grid_bits(dims=GRID_DIMS):
    nx, ny, nz = dims
    bits = np.zeros((nx * ny * nz + 7) // 8, np.uint8)
    for iz in range(nz):
        for iy in range(ny):
            for ix in range(nx):
                if grid_cell_set(ix, iy, iz):
                    k = ix + nx * (iy + ny * iz)
                    bits[k >> 3] |= 1 << (k & 7)
    return bits


PLANE_ROWS = np.array([(1, 0, 0, 0.25), (-1, 0, 0, 1.25), (0, 1, 0, 0.25), (0, -1, 0, 1.25), (0, 0, 1, 0.5), (0, 0, -1, 1.0),
                       (-1, -1, -1, 2.0), (1, 1, 1, -0.0)], np.float64)


def region(planes=False, prism=False, grid=False, axis=2, polygon=POLYGON):
    r = io.Region()
    if planes:
        r.planes = PLANE_ROWS.copy()
    if prism:
        r.axis, r.axis_min, r.axis_max, r.polygon = axis, AXIS_MIN, AXIS_MAX, np.array(polygon, np.float64)
    if grid:
        r.origin, r.cell, r.dims, r.bits = np.array(GRID_ORIGIN, np.float64), GRID_CELL, GRID_DIMS, grid_bits()
    return r


def prism_queries():
    """(n, 3) float32: the boundary and the collinear queries at three heights, and the heights' own edges."""
    uv = np.array([q for q, _ in ON_BOUNDARY + COLLINEAR], np.float64)
    rows = [np.column_stack([uv, np.full(len(uv), z)]) for z in (0.25, AXIS_MIN, AXIS_MAX)]
    below, above = np.nextafter(F32(AXIS_MIN), F32(-1)), np.nextafter(F32(AXIS_MAX), F32(1))
    rows.append(np.array([(0.25, 0.25, below), (0.25, 0.25, above), (0.25, 0.25, AXIS_MIN), (0.25, 0.25, AXIS_MAX)], np.float64))
    return np.concatenate(rows).astype(F32)


def grid_queries():
    """(n, 3) float32, all exact: every cell's centre, the half-cell offsets along each axis from index -1 to n_a (ties
    to even, both parities), one cell outside each face, negative indices and index n_a - 1."""
    o, c = np.array(GRID_ORIGIN), GRID_CELL
    rows = [o + c * np.array([ix, iy, iz]) for ix in range(GRID_DIMS[0]) for iy in range(GRID_DIMS[1]) for iz in range(GRID_DIMS[2])]
    mid = np.array([2, 3, 4])
    for a in range(3):
        for i in range(-2, GRID_DIMS[a] + 1):
            for off in (0.5, 0.0):                                  # i + 0.5 rounds to the even neighbour
                idx = mid.astype(np.float64)
                idx[a] = i + off
                rows.append(o + c * idx)
        for i in (-1, -3, GRID_DIMS[a] - 1, GRID_DIMS[a]):
            idx = np.array([1.0, 1.0, 1.0])
            idx[a] = i
            rows.append(o + c * idx)
    q = np.array(rows, np.float64)
    assert np.array_equal(q.astype(F32).astype(np.float64), q)      # exact in float32
    return q.astype(F32)


def plane_queries():
    """(n, 3) float32: s == 0 on planes 0, 1 and 6, s == -0.0 on plane 7, and their neighbours on both sides."""
    nz = F32(-0.0)
    rows = [(-0.25, 0.5, 0.25), (1.25, 0.5, 0.25), (0.75, 0.75, 0.5), (nz, nz, nz), (0.0, 0.0, 0.0),
            (np.nextafter(F32(-0.25), F32(-1)), 0.5, 0.25), (np.nextafter(F32(-0.25), F32(1)), 0.5, 0.25),
            (np.nextafter(F32(1.25), F32(2)), 0.5, 0.25), (0.75, 0.75, np.nextafter(F32(0.5), F32(1))),
            (-F32(2.0) ** -149, nz, nz), (F32(2.0) ** -149, nz, nz)]
    return np.array(rows, F32)


INVALID_ROWS = np.array([(np.nan, 0.5, 0.5), (0.5, np.inf, 0.5), (0.5, 0.5, -np.inf), (np.nan, np.nan, np.nan),
                         (np.inf, 0.25, np.nan), (-np.inf, 0.25, 0.25)], F32)


@functools.lru_cache(maxsize=None)
def cloud(seed=0):
    """(N_CLOUD, 3) float32, shuffled: the parts' special queries, the invalid rows, and uniform points of a box that
    every part cuts."""
    rng = np.random.default_rng(seed)
    special = np.concatenate([prism_queries(), grid_queries(), plane_queries(), INVALID_ROWS])
    fill = (rng.random((N_CLOUD - len(special), 3), dtype=F32) * F32(1.75) - F32(0.375)).astype(F32)
    out = np.concatenate([special, fill])[rng.permutation(N_CLOUD)]
    assert out.shape == (N_CLOUD, 3)
    return np.ascontiguousarray(out)


@functools.lru_cache(maxsize=None)
def reference_cloud(seed=1):
    """The other side: the data cloud's valid points moved a little, a few more, a few invalid."""
    rng = np.random.default_rng(seed)
    base = cloud()[np.isfinite(cloud()).all(1)]
    near = base[::2] + (F32(0.01) * rng.standard_normal((len(base[::2]), 3))).astype(F32)
    more = (rng.random((300, 3), dtype=F32) * F32(1.75) - F32(0.375)).astype(F32)
    out = np.concatenate([near.astype(F32), more, INVALID_ROWS[:3]])
    return np.ascontiguousarray(out[rng.permutation(len(out))])


# a small motion about the cloud's middle, and the regions of the two sides in the measuring tests
MOTION = ca.about(ca.rotation((1, 2, -1), 4.0), (0.5, 0.5, 0.25), (0.03, -0.02, 0.01))
