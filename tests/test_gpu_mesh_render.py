"""The mesh rendered into a view on the GPU (acmmp_fusion_mesh_render, include/acmmp.h), bit for bit against the
exhaustive restatement (mesh_render_support): four maps, seven counts and the skipped faces."""
import functools

import numpy as np
import pytest

import mesh_render_support as rs
import voxel_mesh_support as ms
from acmmp import capi
from conftest import assert_bitwise_equal
from fusion_scene_support import fill

pytestmark = pytest.mark.gpu
F32 = np.float32
NAMES = ("depth", "face", "normal", "colour")
TOLERANCES = (0.0, 0.01, 0.05)


def _single(cam, raw_value=2.0):
    """A fusion object over the one camera `cam`, its view set to a constant raw depth."""
    H, W = int(cam[0]["height"]), int(cam[0]["width"])
    raw = np.full((H, W), raw_value, F32)
    raw[0, 0], raw[-1, -1] = 0.0, np.nan
    gf = capi.Fusion(0, cam)
    gf.set_view(0, raw, np.zeros((H, W, 3), F32), np.zeros((H, W, 3), np.uint8))
    return gf, raw


def _assert_render(gf, want, info, what):
    print(what, info, gf.render_plan())
    assert info == rs.info_of(want), what
    for g, name in zip(gf.render_maps(), NAMES):
        assert g.dtype == want[name].dtype and g.shape == want[name].shape, f"{what}: {name}"
        assert_bitwise_equal(g, want[name], f"{what}: {name}")


def _quads():
    xyz, tri = [], []
    for z, first in ((2.0, 0), (1.5, 4)):
        f, c = 8.0, 8.0
        x = [(p - c) / f * z for p in (4, 12)]
        xyz += [(x[0], x[0], z), (x[1], x[0], z), (x[1], x[1], z), (x[0], x[1], z)]
        tri += [(first, first + 1, first + 2), (first, first + 2, first + 3)]
    xyz += [(0.0, 0.0, -1.0), (0.5, 0.0, 0.0), (float("nan"), 0.0, 3.0)]
    tri += [(0, 1, 2), (0, 1, 8), (0, 1, 9), (0, 1, 10)]             # a duplicate, behind, on the camera plane, not finite
    return rs.as_mesh(xyz, tri)


HAND = {
    "pole 16x8": lambda: (rs.sphere_camera(16, 8), rs.box_mesh(rs.POLE_HALF, rs.POLE_FRAME)),
    "pole 64x32": lambda: (rs.sphere_camera(64, 32), rs.box_mesh(rs.POLE_HALF, rs.POLE_FRAME)),
    "seam 16x8": lambda: (rs.sphere_camera(16, 8), rs.box_mesh(rs.SEAM_HALF, rs.SEAM_FRAME)),
    "seam 64x32": lambda: (rs.sphere_camera(64, 32), rs.box_mesh(rs.SEAM_HALF, rs.SEAM_FRAME)),
    "quads pinhole": lambda: (rs.pinhole_camera(16, 16, f=8.0), _quads()),
    "quads sphere": lambda: (rs.sphere_camera(33, 17), _quads()),
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_built_meshes(name):
    cam, (V, T) = HAND[name]()
    gf, raw = _single(cam)
    assert gf.set_mesh(V, T) == (len(V), len(T))
    for tol in TOLERANCES:
        want = rs.render(cam, V, T, raw, tol)
        _assert_render(gf, want, gf.render_mesh(0, rel_tol=tol), f"{name} tol {tol}")
    if name.startswith("quads"):
        assert want["skipped"] == (3 if "pinhole" in name else 1)
    gf.close()


@functools.lru_cache(maxsize=None)
def _base(rig):
    """(cams, depths, normals, colours, the rig's base-case mesh as the device extracts it, its restated render per view)."""
    cams, depths, normals, colours, cloud, size, trunc, _ = ms.base_case(rig)
    gf = fill(capi.Fusion(0, cams), cams, depths, normals, colours)
    gf.set_scene(cloud)
    gf.voxelize(size)
    nv, nf, _ = gf.voxel_mesh(list(range(len(cams))), trunc)
    V, T = gf.mesh_vertices(0, nv), gf.mesh_faces(0, nf)
    gf.close()
    assert nv > 0 and nf > 0
    renders = [rs.render(cams[k], V, T) for k in range(len(cams))]
    return cams, depths, normals, colours, V, T, renders


def _with_counts(out, raw, tol):
    return dict(out, counts=rs.counts_of(out, raw, tol))


@pytest.mark.parametrize("rig", ["sphere", "pinhole"])
def test_base_case_meshes_in_every_view(rig):
    cams, depths, normals, colours, V, T, renders = _base(rig)
    gf = fill(capi.Fusion(0, cams), cams, depths, normals, colours)
    gf.set_mesh(V, T)
    for k in range(len(cams)):
        for tol in TOLERANCES:
            want = _with_counts(renders[k], depths[k], tol)
            _assert_render(gf, want, gf.render_mesh(k, rel_tol=tol), f"{rig} view {k} tol {tol}")
        assert (renders[k]["face"] >= 0).sum() > 100
    # view None with a copy of view 1's camera: view 1's maps, no agreement
    want = _with_counts(renders[1], None, 0.01)
    _assert_render(gf, want, gf.render_mesh(camera=cams[1].copy()), f"{rig} camera of view 1")
    # the small and the large path give the same maps on a real mesh
    plans = []
    for small_max in (1, 1 << 30, 0):
        gf.render_plan(small_max)
        _assert_render(gf, _with_counts(renders[0], depths[0], 0.01), gf.render_mesh(0), f"{rig} small_max {small_max}")
        plans.append(gf.render_plan(small_max))
    assert plans[0]["small"] < plans[1]["small"] and plans[1]["large"] == 0 and plans[0]["candidates"] == plans[1]["candidates"]
    assert plans[0]["small"] + plans[0]["large"] == len(T) - renders[0]["skipped"]
    gf.close()


@pytest.mark.parametrize("model", ["sphere", "pinhole"])
def test_one_triangle_over_the_whole_image(model):
    if model == "pinhole":
        cam = rs.pinhole_camera(48, 20, f=30.0)
        V, T = rs.as_mesh([(-40.0, -30.0, 3.0), (40.0, -30.0, 3.0), (0.0, 60.0, 3.0)], [(0, 1, 2)])
    else:
        # the camera just under a huge triangle: it fills the upper hemisphere's rows and touches a pole
        cam = rs.sphere_camera(48, 20)
        V, T = rs.as_mesh([(-400.0, -0.25, -300.0), (400.0, -0.25, -300.0), (0.0, -0.25, 600.0)], [(0, 1, 2)])
    gf, raw = _single(cam, raw_value=3.0)
    gf.set_mesh(V, T)
    want = rs.render(cam, V, T, raw, 0.01)
    hit = int((want["face"] >= 0).sum())
    assert hit == 48 * 20 if model == "pinhole" else hit > 48 * 8
    results = []
    for small_max, large in ((1, 1), (1 << 30, 0)):
        gf.render_plan(small_max)
        _assert_render(gf, want, gf.render_mesh(0), f"{model} small_max {small_max}")
        plan = gf.render_plan(small_max)
        assert (plan["small"], plan["large"]) == (1 - large, large) and plan["candidates"] >= hit
        results.append([a.tobytes() for a in gf.render_maps()])
    assert results[0] == results[1]
    gf.close()


def test_two_renders_give_identical_bytes():
    cams, depths, normals, colours, V, T, _ = _base("sphere")
    out = []
    for _ in range(2):
        gf = fill(capi.Fusion(0, cams), cams, depths, normals, colours)
        gf.set_mesh(V, T)
        first = (gf.render_mesh(2), [a.tobytes() for a in gf.render_maps()])
        again = (gf.render_mesh(2), [a.tobytes() for a in gf.render_maps()])
        assert first == again
        out.append(first)
        gf.close()
    assert out[0] == out[1]


def _gone(gf):
    with pytest.raises(capi.AcmmpError):
        gf.render_maps()


def test_lifetimes():
    cams, depths, normals, colours, cloud, size, trunc, _ = ms.base_case("sphere")
    _, _, _, _, V, T, renders = _base("sphere")
    views = list(range(len(cams)))
    gf = fill(capi.Fusion(0, cams), cams, depths, normals, colours)
    _gone(gf)
    with pytest.raises(capi.AcmmpError):
        gf.render_mesh(0)                                               # no mesh result
    # a set mesh and its render outlive the scene, the voxels and set_view
    gf.set_mesh(V, T)
    gf.render_mesh(0)
    state = [a.tobytes() for a in gf.render_maps()]
    gf.set_scene(cloud)
    gf.voxelize(size)
    gf.voxel_clean(26, 1, 2, 1)
    gf.set_view(1, depths[1], normals[1], colours[1])
    assert [a.tobytes() for a in gf.render_maps()] == state
    assert gf.mesh_samples(0, 0)[0].shape == (0, 3)
    with pytest.raises(capi.AcmmpError):
        gf.mesh_samples(0, 1)                                           # a set mesh has no samples
    # set_mesh and voxel_mesh each discard the render
    gf.set_mesh(V, T)
    _gone(gf)
    gf.render_mesh(0)
    nv, nf, _ = gf.voxel_mesh(views, trunc)
    _gone(gf)
    assert (nv, nf) == (len(V), len(T))
    _assert_render(gf, dict(renders[3], counts=rs.counts_of(renders[3], depths[3], 0.01)), gf.render_mesh(3), "voxel mesh")
    # whatever discards the mesh's source discards the render: voxelize, set_scene, run_scene; clean for a clean mesh
    for discard in (lambda: gf.voxelize(size), lambda: gf.set_scene(cloud), lambda: gf.run_scene([0], [[1, 2]])):
        gf.set_scene(cloud)
        gf.voxelize(size)
        gf.voxel_mesh(views, trunc)
        gf.render_mesh(0)
        discard()
        _gone(gf)
        with pytest.raises(capi.AcmmpError):
            gf.render_mesh(0)
    gf.set_scene(cloud)
    gf.voxelize(size)
    gf.voxel_clean(26, 1, 2, 1)
    gf.voxel_mesh(views, trunc, source="clean")
    gf.render_mesh(0)
    gf.voxel_visibility(views, 0.05, 1, 1, 4096, source="clean")        # leaves a mesh of the clean result alone
    assert gf.render_maps()[0].shape == depths[0].shape
    gf.voxel_clean(26, 1, 2, 1)
    _gone(gf)
    gf.close()


def test_refused_arguments_leave_the_object_unchanged():
    cams, depths, normals, colours, V, T, _ = _base("sphere")
    gf = fill(capi.Fusion(0, cams), cams[:3], depths, normals, colours)    # view 3 is never set
    gf.set_mesh(V, T)
    info = gf.render_mesh(1, rel_tol=0.05)
    plan = gf.render_plan()
    state = [a.tobytes() for a in gf.render_maps()]
    other = rs.pinhole_camera(16, 16)
    empty = cams[0:1].copy()
    empty["width"] = 0
    flat = cams[0:1].copy()
    flat["height"] = -4
    for bad in (dict(view=4), dict(view=-2), dict(view=3), dict(view=None, camera=None), dict(view=None, camera=other),
                dict(view=None, camera=empty), dict(view=None, camera=flat), dict(view=0, rel_tol=float("nan")),
                dict(view=0, rel_tol=float("inf")), dict(view=0, rel_tol=-0.5)):
        with pytest.raises(capi.AcmmpError):
            gf.render_mesh(**bad)
        assert [a.tobytes() for a in gf.render_maps()] == state and gf.render_plan() == plan
    with pytest.raises(ValueError):
        gf.render_mesh(0, camera=cams[0])
    # set_mesh: an index outside the vertices, a negative one; the mesh and its render stay
    for faces in ([[0, 1, len(V)]], [[0, -1, 2]]):
        with pytest.raises(capi.AcmmpError):
            gf.set_mesh(V, np.array(faces, np.int32))
    assert gf.L.acmmp_fusion_set_mesh(gf.h, 2 ** 31, None, 0, None) == 1
    assert gf.L.acmmp_fusion_set_mesh(gf.h, 3, None, 0, None) == 1
    assert [a.tobytes() for a in gf.render_maps()] == state
    assert gf.mesh_vertices(0, len(V)).tobytes() == V.tobytes() and gf.mesh_faces(0, len(T)).tobytes() == T.tobytes()
    # every output pointer may be NULL
    assert gf.L.acmmp_fusion_mesh_render(gf.h, 1, None, 0.05, None, None) == 0
    assert gf.L.acmmp_fusion_render_maps(gf.h, None, None, None, None) == 0
    assert [a.tobytes() for a in gf.render_maps()] == state and gf.render_mesh(1, rel_tol=0.05) == info
    # an empty mesh renders to empty maps
    gf.set_mesh(np.zeros((0, 9), F32), np.zeros((0, 3), np.int32))
    out = gf.render_mesh(0)
    depth, face, normal, colour = gf.render_maps()
    assert not depth.any() and (face == -1).all() and not normal.any() and not colour.any()
    assert out["counts"]["agree"] == 0 and out["counts"]["raw_only"] + out["counts"]["neither"] == depth.size
    gf.close()
