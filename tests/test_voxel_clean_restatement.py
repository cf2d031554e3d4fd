"""The restatement of the voxel-cloud cleaning (voxel_clean_support) gives the answers its constructed clouds have
by construction, the fused-scene cases of the GPU test are not vacuous, and the new entry points are declared,
bound and exported (no GPU)."""
import os
import re
import subprocess

import numpy as np
import pytest

import voxel_clean_support as cs
import voxel_support as vs
from acmmp import capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["acmmp_fusion_set_scene", "acmmp_fusion_voxel_clean", "acmmp_fusion_clean_points",
               "acmmp_fusion_voxel_labels", "acmmp_fusion_component_table"]


def _voxels(name):
    v = vs.voxelize(cs.constructed(name), 1.0, cs.ORIGIN)
    assert v["n_rejected"] == 0
    return v


def _clean(name, connectivity, min_neighbours=0, min_voxels=1, min_points=1):
    v = _voxels(name)
    c = cs.clean(v["keys"], v["counts"], connectivity, min_neighbours, min_voxels, min_points)
    # label = the smallest index of the component, the table in ascending label order, sizes that add up
    lab = c["label"]
    for r, n, p in zip(c["root"], c["voxels"], c["points"]):
        members = np.flatnonzero(lab == r)
        assert members.min() == r and len(members) == n and v["counts"][members].sum() == p
    assert (np.diff(c["root"]) > 0).all() and (lab >= 0).sum() == c["voxels"].sum()
    assert (lab < 0).sum() == c["n_unsupported"] and (np.diff(c["kept"]) > 0).all()
    return v, c


def _cells_of(v, idx):
    return set(cs.unpack(v["keys"][idx]))


def test_snake():
    cells = cs.snake_cells()
    assert len(cells) == len(set(cells)) == cs.SNAKE_CELLS == 16384
    steps = np.abs(np.diff(np.asarray(cells), axis=0)).sum(1)
    assert (steps == 1).all()                                     # face-connected, end to end
    v = _voxels("snake")
    assert len(v["counts"]) == cs.SNAKE_CELLS and cs.unpack(v["keys"][:1]) == [cells[0]]   # voxel 0 is the head
    # the voxel indices along the path are in no order: plain propagation has to carry label 0 cell by cell
    index = {c: i for i, c in enumerate(cs.unpack(v["keys"]))}
    along = np.array([index[c] for c in cells])
    assert (np.diff(along) < 0).sum() > cs.SNAKE_CELLS // 3
    for conn in (6, 18, 26):
        _, c = _clean("snake", conn)
        assert c["root"].tolist() == [0] and c["voxels"].tolist() == [cs.SNAKE_CELLS] and (c["label"] == 0).all()
        assert c["points"].tolist() == [cs.constructed("snake").shape[0]] and len(c["kept"]) == cs.SNAKE_CELLS
    # at connectivity 6 an inner cell of the path has its two path neighbours and those of the rows beside it
    _, c = _clean("snake", 6)
    assert c["support"].min() >= 1 and c["support"].max() <= 6
    assert c["support"][index[cells[0]]] == 3                     # the block's corner: one cell along each axis


def test_contacts():
    for conn, comps in ((26, 3), (18, 4), (6, 5)):
        _, c = _clean("contacts", conn)
        assert len(c["root"]) == comps == 6 - (c["voxels"] == 2).sum()
        assert c["root"].tolist() == sorted(c["root"].tolist()) and sorted(c["voxels"].tolist()) == [1] * (2 * comps - 6) + [2] * (6 - comps)
    _, c = _clean("contacts", 26, min_voxels=2)
    assert c["kept"].tolist() == list(range(6)) and c["component"].tolist() == [0, 0, 1, 1, 2, 2]
    _, c = _clean("contacts", 6, min_voxels=2)
    assert c["kept"].tolist() == [0, 1] and c["component"].tolist() == [0, 0] and c["n_components_kept"] == 1
    _, c = _clean("contacts", 6, min_neighbours=1)
    assert c["label"].tolist() == [0, 0, -1, -1, -1, -1] and c["n_unsupported"] == 4


def test_edge():
    v = _voxels("edge")
    keys = v["keys"].astype(np.uint64)
    assert int(keys[0]) - int(keys[1]) == 1                       # (0, 5, 5) and (2^21 - 1, 4, 5)
    assert cs.unpack(keys[2:4]) == [(0, 0, 0), (cs.LAST,) * 3]
    for conn in (6, 18, 26):
        _, c = _clean("edge", conn)
        assert c["label"].tolist() == [0, 1, 2, 3, 4, 4, 6, 6, 8, 8]
        assert c["support"].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 1, 1]
        assert c["voxels"].tolist() == [1, 1, 1, 1, 2, 2, 2]
    _, c = _clean("edge", 26, min_neighbours=1)
    assert c["kept"].tolist() == [4, 5, 6, 7, 8, 9] and c["component"].tolist() == [0, 0, 1, 1, 2, 2]


def test_blobs():
    v, c = _clean("blobs", 26)
    sizes = [s ** 3 for s in cs.CUBE_SIDES]
    assert sorted(c["voxels"].tolist()) == [1] * (cs.N_SINGLES + 1) + sizes[1:]
    assert len(c["root"]) == len(sizes) + cs.N_SINGLES and c["n_unsupported"] == 0
    for min_voxels, kept_cubes in ((1, 4), (2, 3), (9, 2), (28, 1), (126, 0)):
        _, c = _clean("blobs", 26, min_voxels=min_voxels)
        assert c["n_components_kept"] == kept_cubes + (cs.N_SINGLES if min_voxels == 1 else 0)
        assert len(c["kept"]) == sum(s for s in sizes if s >= min_voxels) + (cs.N_SINGLES if min_voxels == 1 else 0)
    for conn in (6, 18, 26):                                      # a solid cube is one component at every connectivity
        assert len(_clean("blobs", conn)[1]["root"]) == len(sizes) + cs.N_SINGLES
    _, c = _clean("blobs", 26, min_neighbours=1)                  # the isolated cells and the 1-cube go
    assert c["n_unsupported"] == cs.N_SINGLES + 1 and sorted(c["voxels"].tolist()) == sizes[1:]
    _, c = _clean("blobs", 26, min_neighbours=7)                  # a 2^3 cube's cells have exactly 7 neighbours
    assert c["n_unsupported"] == cs.N_SINGLES + 1 and sorted(c["voxels"].tolist()) == sizes[1:]
    _, c = _clean("blobs", 26, min_neighbours=8)
    assert sorted(c["voxels"].tolist()) == [27 - 8, 125 - 8]      # the corners of the larger cubes go too
    v, c = _clean("blobs", 26, min_neighbours=26)                 # interior cells only
    assert sorted(c["voxels"].tolist()) == [1, 27]
    assert _cells_of(v, c["kept"]) == {(51, 11, 11)} | set(cs.cube((71, 11, 11), 3))
    _, c = _clean("blobs", 6, min_neighbours=7)                   # nothing has 7 face neighbours
    assert len(c["root"]) == 0 and len(c["kept"]) == 0 and c["n_unsupported"] == len(c["label"])
    # a cut on points: cell i holds 1 + i % 3 points, so the 1-cube (cell 0) holds one and an isolated cell up to 3
    v, c = _clean("blobs", 26, min_points=20)
    assert sorted(c["voxels"][c["points"] >= 20].tolist()) == sizes[2:] and len(c["kept"]) == 27 + 125


def test_dumbbell():
    v, c = _clean("dumbbell", 26)
    assert c["voxels"].tolist() == [27 + 3 + 27]
    v, c = _clean("dumbbell", 26, min_neighbours=3)               # the middle of the bridge has two neighbours
    assert c["n_unsupported"] == 1 and c["voxels"].tolist() == [28, 28]
    dropped = np.flatnonzero(c["label"] < 0)
    assert _cells_of(v, dropped) == {(104, 101, 101)}
    # voxels 0 .. 26 and bridge cell 27; bridge cell 29 and voxels 30 .. 56 (28, the middle, is gone)
    assert c["root"].tolist() == [0, 29] and c["component"].tolist() == [0] * 28 + [1] * 28
    assert c["kept"].tolist() == list(range(28)) + list(range(29, 57))
    v, c = _clean("dumbbell", 6, min_neighbours=2)                # at connectivity 6 the bridge's ends have 2, the middle 2
    assert c["voxels"].tolist() == [57]


def test_bad_arguments():
    v = _voxels("contacts")
    for kw in (dict(connectivity=8), dict(min_neighbours=-1), dict(min_component_voxels=0), dict(min_component_points=0)):
        with pytest.raises(ValueError):
            cs.clean(v["keys"], v["counts"], **kw)
    c = cs.clean(np.zeros(0, np.uint64), np.zeros(0, np.int32))
    assert len(c["label"]) == len(c["root"]) == len(c["kept"]) == 0 and c["n_unsupported"] == 0


@pytest.mark.parametrize("name", ["rig_50x30", "rig_256x128"])
def test_scene_cases_are_not_vacuous(name):
    """The (voxel size, thresholds) of the GPU test's fused scenes, on the oracle's cloud of the same scene: at least
    two components of different sizes, at least one kept, at least one dropped."""
    pts = vs.oracle_cloud(name)
    for size, conn, min_nb, min_vox, min_pts in cs.scene_cases(name, pts):
        v = vs.voxelize(pts, size)
        c = cs.clean(v["keys"], v["counts"], conn, min_nb, min_vox, min_pts)
        print(name, size, conn, min_nb, min_vox, min_pts, "voxels", len(v["counts"]), "components", len(c["root"]),
              "kept", c["n_components_kept"], "largest", np.sort(c["voxels"])[::-1][:4].tolist(), "unsupported", c["n_unsupported"])
        assert len(set(c["voxels"].tolist())) >= 2
        assert 1 <= c["n_components_kept"] < len(c["root"])
        assert 0 < len(c["kept"]) < len(v["counts"])


def test_new_entry_points_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "acmmp.h")).read(), flags=re.S)
    L = capi.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in capi.EXPORTS and hasattr(L, name), name
        assert re.search(rf"\bT {name}$", out, re.M), name
    for method in ("set_scene", "voxel_clean", "clean_points", "voxel_labels", "component_table"):
        assert callable(getattr(capi.Fusion, method, None)), method


def test_restated_fusion_surface():
    """RestatedCleanFusion on a constructed cloud: the lifetimes the header states."""
    rf = cs.RestatedCleanFusion(np.zeros(1, capi.CAMERA_DTYPE))
    with pytest.raises(ValueError):
        rf.voxel_clean()
    assert rf.set_scene(cs.constructed("contacts")) == cs.constructed("contacts").shape[0]
    pts, ref, pix, mask = rf.scene_points(0, 3, provenance=True)
    assert ref.tolist() == [-1] * 3 and pix.tolist() == [-1] * 3 and mask.tolist() == [0] * 3
    assert rf.voxelize(1.0, origin=cs.ORIGIN)[0] == 6
    n, info = rf.voxel_clean(6, min_component_voxels=2)
    assert (n, info["components"], info["components_kept"], info["unsupported"]) == (2, 5, 1, 0)
    p, cnt, comp = rf.clean_points(0, n, counts=True, component=True)
    assert p.shape == (2, 9) and cnt.tolist() == [1, 2] and comp.tolist() == [0, 0]
    assert rf.voxel_labels(0, 6)[0].tolist() == [0, 0, 2, 3, 4, 5]
    assert [a.tolist() for a in rf.component_table(0, 5)] == [[0, 2, 3, 4, 5], [2, 1, 1, 1, 1], [3, 3, 1, 2, 3]]
    rf.voxelize(1.0, origin=cs.ORIGIN)
    with pytest.raises(ValueError):
        rf.clean_points(0, 1)
