"""The restatement of the surface mesh (voxel_mesh_support, written from include/acmmp.h) pinned by properties on the
CPU: a hand-built wall gives one correctly oriented sheet on the wall's plane, S == 0 is outside, the grid's boundary
does not wrap, and the base inputs of the GPU tests exercise every axis, both windings, both colour paths and the
min_weight cut."""
import functools
from collections import Counter

import numpy as np
import pytest

import visibility_support as vis
import voxel_clean_support as cs
import voxel_mesh_support as ms
from fusion_scene_support import fill

F32 = np.float32


def _wall(depth, trunc=0.5, n=12):
    cam, depths, cells, origin, size = ms.wall_scene(n=n, depth=depth)
    colours = np.tile(np.array([[10.0, 20.0, 30.0]], F32), (len(cells), 1))
    return ms.mesh(cells, colours, origin, size, cam, depths, [0], trunc), size, n


def _edge_use(faces):
    use = Counter()
    for a, b, c in faces.tolist():
        for e in ((a, b), (b, c), (c, a)):
            use[tuple(sorted(e))] += 1
    return use


def test_single_wall_is_one_oriented_sheet_on_the_plane():
    depth, trunc = 4.1, 0.5
    m, size, n = _wall(depth, trunc)
    V, F = m["vertices"].astype(np.float64), m["faces"]
    # one sheet: a vertex per cube column of the dilated block, two triangles per interior sign change
    assert V.shape[0] == (n + 1) ** 2 and F.shape[0] == 2 * n * n
    assert F.min() >= 0 and F.max() < V.shape[0]
    tri = V[F][:, :, :3]
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (np.linalg.norm(normal, axis=1) > 0).all()
    to_camera = -tri.mean(1)                                     # the camera is at the world's origin
    assert ((normal * to_camera).sum(1) > 0).all()
    for k in range(3):
        assert ((normal * V[F[:, k], 3:6]).sum(1) > 0).all()
    assert np.allclose(np.linalg.norm(V[:, 3:6], axis=1), 1.0, atol=1e-6)
    # The cell-centre TSDF of a plane is linear along z, so the interpolated crossing is the plane itself up to the
    # quantisation of the two sums: each q is off by at most half a unit, 0.5 * trunc / 1024, which moves the crossing
    # of an edge of length `size` by at most size * 2 * (0.5 trunc / 1024) / (size - trunc / 1024); the float32
    # roundings of the sample centre, of pd = z, of u and of the final position add a few ulp of the depth (2^-21 each).
    q = trunc / 1024.0
    bound = size * q / (size - q) + 8 * depth * 2.0 ** -21
    off = np.abs(V[:, 2] - depth)
    print("wall: max distance", off.max(), "bound", bound)
    assert off.max() <= bound < size
    assert (V[:, 6:9] == np.array([10.0, 20.0, 30.0])).all() and m["info"]["uncoloured"] == 0
    # only rim edges are used by exactly one triangle, every other edge by two
    use = _edge_use(F)
    assert set(use.values()) == {1, 2}
    lo, hi = V[:, :2].min(0), V[:, :2].max(0)
    on_rim = lambda v: bool((np.abs(V[v, :2] - lo) < 1e-6).any() or (np.abs(V[v, :2] - hi) < 1e-6).any())
    rim = [e for e, k in use.items() if k == 1]
    assert len(rim) == 4 * n and all(on_rim(a) and on_rim(b) for a, b in rim)


def test_zero_sum_is_outside():
    """The wall through the centres of the block's own layer: those samples have u = 0, S = 0, and are outside, so the
    sheet lies between that layer and the next, with t = 0: exactly on the plane."""
    depth = 4.125                                                # the centre of layer 16 at size 0.25, exact in float32
    m, size, n = _wall(depth)
    layer = m["cells"][:, 2] == 16
    assert layer.sum() == (n + 2) ** 2 and (m["tsdf"][layer, 0] == 0).all() and (m["tsdf"][layer, 1] == 1).all()
    assert (m["tsdf"][m["cells"][:, 2] == 15, 0] > 0).all() and (m["tsdf"][m["cells"][:, 2] == 17, 0] < 0).all()
    V = m["vertices"]
    assert V.shape[0] == (n + 1) ** 2 and (V[:, 2] == F32(depth)).all()
    assert (V[:, 5] < 0).all()                                   # towards the camera


def test_grid_boundary_does_not_wrap():
    cam, depths, _, _, size = ms.wall_scene()
    last = cs.LAST
    cells = [(0, 0, 0), (last, last, last), (0, 5, last)]
    colours = np.zeros((3, 3), F32)
    m = ms.mesh(cells, colours, np.zeros(3, F32), size, cam, depths, [0], 0.5)
    got = {tuple(c) for c in m["cells"].tolist()}
    assert len(got) == m["info"]["samples"] == 8 + 8 + 12
    assert all(0 <= x <= last for c in got for x in c)
    assert (m["entry"] >= 0).sum() == 3


@functools.lru_cache(maxsize=None)
def _base(rig, source="voxel"):
    cams, depths, normals, colours, cloud, size, trunc, small = ms.base_case(rig)
    rf = fill(ms.RestatedMeshFusion(cams), cams, depths, normals, colours)
    rf.set_scene(cloud)
    rf.voxelize(size)
    return rf, list(range(len(cams))), trunc, small


@pytest.mark.parametrize("rig", list(vis.RIGS))
def test_base_inputs_exercise_every_path(rig):
    rf, views, trunc, small = _base(rig)
    nv, nf, info = rf.voxel_mesh(views, trunc)
    stats = rf.meshed["face_stats"]
    print(rig, "entries", len(rf.voxels["keys"]), "vertices", nv, "faces", nf, info, stats)
    assert nv > 0 and nf > 0
    for a in range(3):
        for inside in (False, True):
            assert stats.get((a, inside), 0) > 0, (a, inside)
    assert 0 < info["uncoloured"] < nv
    assert info["valid"] <= info["samples"] and 0 < info["cubes"]
    _, _, info2 = rf.voxel_mesh(views, trunc, min_weight=2)
    assert info2["valid"] < info2["samples"] == info["samples"]
    # the small trunc: most contributions saturate or are hidden
    nv_s, nf_s, info_s = rf.voxel_mesh(views, small)
    S, n = rf.meshed["tsdf"][:, 0].astype(np.int64), rf.meshed["tsdf"][:, 1].astype(np.int64)
    saturated = int(((S == 1024 * n) | (n < len(views))).sum())   # every contribution at +trunc, or one hidden / unobserved
    print(rig, "small trunc:", nv_s, nf_s, info_s, "saturated or hidden", saturated, "of", len(S))
    assert saturated > len(S) // 2


def test_forced_table_case_wraps():
    """The collision case of the GPU test: the sphere rig's visible entries in the smallest table above their samples."""
    rf, views, trunc, _ = _base("sphere")
    rf.voxel_clean(26, 1, 2, 1)
    rf.voxel_visibility(views, 0.05, 1, 1, 4096, source="clean")
    idx, _ = rf.mesh_entries("visible")
    order, _, _ = ms.samples_of([tuple(c) for c in cs.unpack(rf.voxels["keys"][idx])])
    slots = 1 << len(order).bit_length()
    assert slots < ms.auto_slots(len(idx)) and ms.table_wrapped(order, slots) > 0
