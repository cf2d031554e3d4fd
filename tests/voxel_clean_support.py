"""Test-side restatement of the cleaning of the voxel cloud (acmmp_fusion_voxel_clean, include/acmmp.h): plain
Python, sequential, written from the header's six steps -- a dict from cell to voxel index for the neighbours, a
plain union-find for the components.  TEST INFRASTRUCTURE: RestatedCleanFusion has capi.Fusion's clean surface so
the pipeline and the GPU tests can be checked against it, and the constructed clouds below have a topology that is
known by construction (voxel size 1, origin (0, 0, 0), points at cell centres, one to three points per cell)."""
import functools
import itertools

import numpy as np

import voxel_support as vs

F32 = np.float32
CELLS = vs.CELLS
LAST = CELLS - 1
MAX_L1 = {6: 1, 18: 2, 26: 3}


def offsets(connectivity):
    """Step 1's offsets: d != 0, |d_a| <= 1, |dx| + |dy| + |dz| <= 1, 2 or 3."""
    return [d for d in itertools.product((-1, 0, 1), repeat=3)
            if 0 < abs(d[0]) + abs(d[1]) + abs(d[2]) <= MAX_L1[connectivity]]


def unpack(keys):
    """The cells (gx, gy, gz) of packed keys, as a list of tuples of Python ints."""
    return [(k & LAST, (k >> 21) & LAST, (k >> 42) & LAST) for k in (int(k) for k in np.asarray(keys, np.uint64))]


def neighbour_lists(keys, connectivity):
    """Step 1: per voxel the indices of its neighbours.  Offsets are applied per axis to the unpacked indices; a
    cell with an index outside [0, 2^21) does not exist."""
    cells = unpack(keys)
    index = {c: i for i, c in enumerate(cells)}
    assert len(index) == len(cells), "a voxel result holds a cell once"
    offs = offsets(connectivity)
    out = []
    for x, y, z in cells:
        nb = []
        for dx, dy, dz in offs:
            c = (x + dx, y + dy, z + dz)
            if min(c) < 0 or max(c) >= CELLS:
                continue
            u = index.get(c)
            if u is not None:
                nb.append(u)
        out.append(nb)
    return out


def clean(keys, counts, connectivity=26, min_neighbours=0, min_component_voxels=1, min_component_points=1,
          neighbours=None):
    """Steps 1-6 over a voxel result given by its keys and counts (in voxel order).  Returns a dict: label int64 and
    support int32 per voxel; root, voxels, points int64 per component; kept (voxel indices, ascending) and component
    (id per kept voxel) int64; n_unsupported.  `neighbours`: neighbour_lists(keys, connectivity), when at hand."""
    if connectivity not in MAX_L1 or min_neighbours < 0 or min_component_voxels < 1 or min_component_points < 1:
        raise ValueError("bad clean argument")
    counts = np.asarray(counts, np.int64)
    nv = len(counts)
    nbrs = neighbour_lists(keys, connectivity) if neighbours is None else neighbours
    support = np.array([len(nb) for nb in nbrs], np.int32).reshape(nv)
    in_s = support >= min_neighbours
    parent = list(range(nv))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for v in range(nv):
        if not in_s[v]:
            continue
        for u in nbrs[v]:
            if in_s[u]:
                a, b = find(v), find(u)
                if a != b:
                    parent[max(a, b)] = min(a, b)           # the root is the smallest index
    label = np.array([find(v) if in_s[v] else -1 for v in range(nv)], np.int64).reshape(nv)
    root = np.unique(label[label >= 0])                      # ascending
    cid = np.full(nv, -1, np.int64)
    cid[root] = np.arange(len(root))
    comp_of = np.where(label >= 0, cid[np.maximum(label, 0)], -1)
    voxels = np.bincount(comp_of[comp_of >= 0], minlength=len(root)).astype(np.int64)
    points = np.zeros(len(root), np.int64)
    np.add.at(points, comp_of[comp_of >= 0], counts[comp_of >= 0])
    comp_kept = (voxels >= min_component_voxels) & (points >= min_component_points)
    kept = np.array([v for v in range(nv) if comp_of[v] >= 0 and comp_kept[comp_of[v]]], np.int64)
    return {"label": label, "support": support, "root": root.astype(np.int64), "voxels": voxels, "points": points,
            "kept": kept, "component": comp_of[kept].astype(np.int64), "n_unsupported": int(nv - in_s.sum()),
            "n_components_kept": int(comp_kept.sum())}


class RestatedCleanFusion(vs.RestatedVoxelFusion):
    """RestatedVoxelFusion with capi.Fusion's set_scene and clean surface computed by the restatement."""

    def __init__(self, cams):
        super().__init__(cams)
        self.cleaned = None

    def run_scene(self, refs, src_lists, unique=False):
        out = super().run_scene(refs, src_lists, unique=unique)
        self.cleaned = None
        return out

    def set_scene(self, points, ref_index=None, pixel=None, src_mask=None):
        pts = np.ascontiguousarray(points, F32).reshape(-1, 9).copy()
        n = pts.shape[0]
        self.result = (pts, np.full(n, -1, np.int32) if ref_index is None else np.asarray(ref_index, np.int32).copy(),
                       np.full(n, -1, np.int32) if pixel is None else np.asarray(pixel, np.int32).copy(),
                       np.zeros(n, np.uint32) if src_mask is None else np.asarray(src_mask, np.uint32).copy())
        self.voxels = self.cleaned = None
        return n

    def voxelize(self, size, origin=None, min_points=1):
        out = super().voxelize(size, origin, min_points)
        self.cleaned = None
        return out

    def voxel_clean(self, connectivity=26, min_neighbours=0, min_component_voxels=1, min_component_points=1):
        if self.voxels is None:
            raise ValueError("no voxel result")
        c = clean(self.voxels["keys"], self.voxels["counts"], connectivity, min_neighbours, min_component_voxels,
                  min_component_points)
        self.cleaned = c
        return len(c["kept"]), {"components": len(c["root"]), "components_kept": c["n_components_kept"],
                                "unsupported": c["n_unsupported"], "rounds": 0}

    def clean_points(self, first, n, counts=False, component=False):
        total = 0 if self.cleaned is None else len(self.cleaned["kept"])
        if first < 0 or n < 0 or first + n > total:
            raise ValueError("range beyond the clean result")
        if n == 0:
            idx = np.zeros(0, np.int64)
            pts, cnt, comp = np.zeros((0, 9), F32), np.zeros(0, np.int32), np.zeros(0, np.int64)
        else:
            idx = self.cleaned["kept"][first:first + n]
            pts, cnt = self.voxels["points"][idx].copy(), self.voxels["counts"][idx].copy()
            comp = self.cleaned["component"][first:first + n].copy()
        extra = tuple(a for a, on in ((cnt, counts), (comp, component)) if on)
        return (pts, *extra) if extra else pts

    def voxel_labels(self, first, n):
        return self.cleaned["label"][first:first + n].copy(), self.cleaned["support"][first:first + n].copy()

    def component_table(self, first, n):
        return tuple(self.cleaned[k][first:first + n].copy() for k in ("root", "voxels", "points"))


# ---- constructed clouds: cells in scene order -> points at the cell centres, 1 + (i % 3) points per cell

def cloud_of(cells, order=None):
    """The scene cloud of `cells` (a list of (x, y, z)): cell i has 1 + i % 3 points at its centre, normal (0, 0, 1),
    colour (i % 251, 7, 9).  Point p of the cloud is the point order[p] of that list (default: as they come)."""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    per = 1 + np.arange(len(cells)) % 3
    which = np.repeat(np.arange(len(cells)), per)
    if order is not None:
        which = which[order(which)]
    pts = np.zeros((len(which), 9), F32)
    pts[:, :3] = (cells[which].astype(np.float64) + 0.5).astype(F32)       # exact up to 2097151.5
    pts[:, 5] = 1.0
    pts[:, 6] = (which % 251).astype(F32)
    pts[:, 7:] = (7.0, 9.0)
    return pts


SNAKE = (32, 32, 16)
SNAKE_CELLS = SNAKE[0] * SNAKE[1] * SNAKE[2]                  # L = 16384


def snake_cells():
    """A face-connected path through every cell of a 32 x 32 x 16 block: x back and forth within a row, the rows
    back and forth within a layer, layer after layer."""
    X, Y, Z = SNAKE
    out = []
    for z in range(Z):
        for yi, y in enumerate(range(Y) if z % 2 == 0 else range(Y - 1, -1, -1)):
            xs = range(X) if (z * Y + yi) % 2 == 0 else range(X - 1, -1, -1)
            out += [(x, y, z) for x in xs]
    return out


def _head_first_shuffled(which):
    """Scene order of the snake: the head's points first, the others shuffled (fixed seed), so that voxel 0 is the
    head and the voxel indices along the path are in no order: neighbour-to-neighbour propagation of the smallest
    label needs L - 1 rounds to reach the tail."""
    head, rest = np.flatnonzero(which == 0), np.flatnonzero(which != 0)
    return np.concatenate([head, np.random.default_rng(20240607).permutation(rest)])


def cube(corner, side):
    return [(corner[0] + x, corner[1] + y, corner[2] + z) for x in range(side) for y in range(side) for z in range(side)]


CUBE_SIDES = (1, 2, 3, 5)
N_SINGLES = 40


def blob_cells():
    """Solid cubes of 1, 8, 27 and 125 cells and 40 isolated cells, all far from one another."""
    out = []
    for k, side in enumerate(CUBE_SIDES):
        out += cube((10 + 20 * k, 10, 10), side)
    out += [(200 + 3 * i, 50 + 3 * (i % 5), 70) for i in range(N_SINGLES)]
    return out


def dumbbell_cells():
    """Two 3^3 cubes joined through the centres of two faces by a bridge one cell wide and three long."""
    return cube((100, 100, 100), 3) + [(103 + i, 101, 101) for i in range(3)] + cube((106, 100, 100), 3)


def contact_cells():
    """Three pairs far apart: touching by a face, by an edge, by a corner."""
    return [(10, 10, 10), (11, 10, 10), (30, 30, 30), (31, 31, 30), (50, 50, 50), (51, 51, 51)]


def edge_cells():
    """Cells on the grid's boundary: two whose packed keys differ by exactly 1, the two opposite corners of the grid
    (wrapped key arithmetic would join either pair), and per axis a face-adjacent pair on the last index."""
    return [(0, 5, 5), (LAST, 4, 5), (0, 0, 0), (LAST, LAST, LAST),
            (LAST - 1, 200, 200), (LAST, 200, 200), (300, LAST - 1, 300), (300, LAST, 300),
            (400, 400, LAST - 1), (400, 400, LAST)]


@functools.lru_cache(maxsize=None)
def constructed(name):
    """The scene cloud (read-only) of a constructed case."""
    pts = {"snake": lambda: cloud_of(snake_cells(), _head_first_shuffled),
           "blobs": lambda: cloud_of(blob_cells()),
           "dumbbell": lambda: cloud_of(dumbbell_cells()),
           "contacts": lambda: cloud_of(contact_cells()),
           "edge": lambda: cloud_of(edge_cells())}[name]()
    pts.setflags(write=False)
    return pts


CONSTRUCTED = ("snake", "blobs", "dumbbell", "contacts", "edge")
ORIGIN = [0.0, 0.0, 0.0]
# (min_neighbours, min_component_voxels, min_component_points) of the constructed cases: everything kept; the
# thresholds between the cube sizes 1 / 8 / 27 / 125; the support cuts 1 (isolated cells go), 3 (the dumbbell's bridge
# goes), 7 (a 2^3 cube's cells have exactly 7 neighbours at connectivity 26) and 26 (interior cells only); a cut on points.
THRESHOLDS = [(0, 1, 1), (0, 2, 1), (0, 9, 1), (0, 28, 1), (0, 126, 1), (1, 1, 1), (3, 1, 1), (7, 9, 1), (26, 1, 1),
              (0, 1, 20), (2, 3, 60)]

# The fused scenes of the GPU test: scene -> [(voxel size, connectivity, min_neighbours, min_component_voxels,
# min_component_points)].  test_voxel_clean_restatement.py asserts that on the oracle's cloud each has at least two
# components of different sizes, at least one kept and at least one dropped.  The rigs' room is one closed surface:
# at RIG_SIZES' "coarse" it is a single component at every connectivity (nothing to drop), at "fine" no component has
# more than a handful of cells, so the rigs' cases use "middle", where the 50x30 rig's samples are already sparser
# than the cells (hundreds of components, the largest of 100-200 cells) and the 256x128 rig is one large component
# with a few dozen small ones at connectivity 6 and six at 26.  0.0625 is added for the 256x128 rig because no size
# of RIG_SIZES gives it a component table of thousands of entries of many sizes together with a support cut that bites.
SCENE_CASES = {
    "rig_50x30": [(vs.RIG_SIZES["middle"], 6, 1, 4, 1), (vs.RIG_SIZES["middle"], 26, 2, 10, 30),
                  (vs.RIG_SIZES["middle"], 18, 0, 3, 1)],
    "rig_256x128": [(vs.RIG_SIZES["middle"], 6, 1, 10, 1), (vs.RIG_SIZES["middle"], 26, 0, 2, 1), (0.0625, 26, 3, 20, 100)],
    "sphere_64x32": None,                  # from the cloud's extent: scene_cases()
}


def scene_cases(name, pts):
    if SCENE_CASES[name] is not None:
        return SCENE_CASES[name]
    ok = vs.finite_points(pts)
    extent = float((pts[ok, :3].max(0) - pts[ok, :3].min(0)).max())
    return [(extent / 16, 26, 1, 3, 1), (extent / 32, 6, 0, 3, 4)]
