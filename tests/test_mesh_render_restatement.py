"""The restatement of the mesh render (mesh_render_support, written from acmmp_fusion_mesh_render's definition in
include/acmmp.h) pinned by properties that do not come from it: analytic distances, coverage without cracks, the tie
rule, independence of the face order, the pinhole skip rule and the wall of the mesh tests."""
import numpy as np
import pytest

import mesh_render_support as rs
import voxel_mesh_support as ms

F32, F64 = np.float32, np.float64


@pytest.mark.parametrize("size", [(16, 8), (64, 32)])
@pytest.mark.parametrize("name", ["pole", "seam"])
def test_closed_box_around_a_sphere_camera(name, size):
    """A box corner exactly on both poles, or a box edge in the seam's half-plane: every pixel is hit, and the depth is
    the float64 ray-box distance rounded to float32, give or take one ulp (the definition's float64 operations carry a
    few 2^-53 of relative error, far below half an ulp of float32, so the two roundings differ by one ulp at most)."""
    frame, half = (rs.POLE_FRAME, rs.POLE_HALF) if name == "pole" else (rs.SEAM_FRAME, rs.SEAM_HALF)
    V, T = rs.box_mesh(half, frame)
    cam = rs.sphere_camera(*size)
    out = rs.render(cam, V, T)
    assert T.shape == (12, 3) and out["skipped"] == 0
    assert (out["face"] >= 0).all() and (out["depth"] > 0).all()
    want = rs.box_distance(rs.rays(cam), half, frame).astype(F32).reshape(out["depth"].shape)
    ulps = np.abs(out["depth"].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    print(name, size, "max ulps", ulps.max(), "faces seen", np.unique(out["face"]).size)
    assert ulps.max() <= 1
    assert np.unique(out["face"]).size == 12
    if name == "pole":
        # row 0 looks at the pole: its rays are within 2^-23 of the corner's direction
        assert np.abs(out["depth"][0].astype(F64) - 9.0).max() <= 9.0 * 2.0 ** -22
    else:
        # column 0 looks along the seam, where the edge x = 0, z = -2 is; columns 1 and W - 1 see its two sides
        mid = out["depth"].shape[0] // 2
        assert abs(float(out["depth"][mid, 0]) - 2.0) < 1e-5 and out["face"][mid, 1] != out["face"][mid, -1]
    nrm = np.linalg.norm(out["normal"].astype(F64), axis=2)
    assert np.abs(nrm - 1.0).max() < 1e-6


def _quad(z, first=0):
    """A fronto-parallel quad covering pixels [4, 12] x [4, 12] of pinhole_camera(16, 16, f=8) at depth z: corners on
    pixel centres, the diagonal through pixel centres."""
    f, c = 8.0, 8.0
    x = [(p - c) / f * z for p in (4, 12)]
    xyz = [(x[0], x[0], z), (x[1], x[0], z), (x[1], x[1], z), (x[0], x[1], z)]
    return xyz, [(first, first + 1, first + 2), (first, first + 2, first + 3)]


def test_quad_diagonal_and_ties():
    cam = rs.pinhole_camera(16, 16, f=8.0)
    xyz, tri = _quad(2.0)
    out = rs.render(cam, *rs.as_mesh(xyz, tri))
    inside = np.zeros((16, 16), bool)
    inside[4:13, 4:13] = True
    assert ((out["face"] >= 0) == inside).all()                          # no pixel of the quad is missed, none outside hit
    assert (out["depth"][inside] == F32(2.0)).all()
    diag = np.arange(4, 13)
    assert (out["face"][diag, diag] == 0).all()                          # the shared edge goes to the lower index
    assert (out["face"][5, 7] == 0) and (out["face"][7, 5] == 1)
    # two parallel quads: the nearer wins; a duplicated face loses to its lower index
    near, tn = _quad(1.5, 4)
    far, tf = _quad(2.0, 0)
    out2 = rs.render(cam, *rs.as_mesh(far + near, tf + tn))
    assert (out2["depth"][inside] == F32(1.5)).all() and (out2["face"][inside] >= 2).all()
    out3 = rs.render(cam, *rs.as_mesh(xyz, tri + tri))
    assert (out3["face"] == out["face"]).all() and out3["depth"].tobytes() == out["depth"].tobytes()
    # colour is interpolated with the hit's weights: at a corner it is the corner's
    V, _ = rs.as_mesh(xyz, tri)
    assert (out["colour"][4, 4] == V[0, 6:9]).all() and (out["colour"][12, 12] == V[2, 6:9]).all()


def test_face_order_does_not_change_the_depth():
    V, T = rs.box_mesh(rs.POLE_HALF, rs.POLE_FRAME)
    cam = rs.sphere_camera(32, 16)
    base = rs.render(cam, V, T)
    for seed in range(3):
        perm = np.random.default_rng(seed).permutation(len(T))
        out = rs.render(cam, V, T[perm])
        assert out["depth"].tobytes() == base["depth"].tobytes()
        # the winner is the same triangle wherever no other face hits at the same depth (off the shared edges)
        same = perm[out["face"]] == base["face"]
        assert same.mean() > 0.8


def test_pinhole_skips_faces_behind_the_camera():
    cam = rs.pinhole_camera(16, 16, f=8.0)
    xyz, tri = _quad(2.0)
    xyz = xyz + [(0.0, 0.0, -1.0), (0.5, 0.0, 0.0), (float("nan"), 0.0, 3.0)]
    tri = tri + [(0, 1, 4), (0, 1, 5), (0, 1, 6)]                        # behind, on the camera plane, not finite
    out = rs.render(cam, *rs.as_mesh(xyz, tri))
    assert out["skipped"] == 3 and set(np.unique(out["face"])) == {-1, 0, 1}
    scam = rs.sphere_camera(16, 8)
    assert rs.render(scam, *rs.as_mesh(xyz, tri))["skipped"] == 1         # SPHERE skips the non-finite one only


def test_agreement_classes():
    cam = rs.pinhole_camera(16, 16, f=8.0)
    xyz, tri = _quad(2.0)
    raw = np.full((16, 16), 2.0, F32)
    raw[0, 0], raw[0, 1], raw[5, 5], raw[6, 6], raw[7, 7], raw[8, 8] = 0.0, np.nan, 2.5, 1.5, 2.02, np.inf
    out = rs.render(cam, *rs.as_mesh(xyz, tri), raw=raw, rel_tol=0.01)
    # 81 pixels of the quad: one in front of 2.5, one behind 1.5, one with no raw depth, 2.02 within 1%
    assert out["counts"][:6] == [78, 1, 1, 1, 256 - 81 - 2, 2] and sum(out["counts"][:6]) == 256
    assert out["counts"][6] in (0, 81)
    assert rs.render(cam, *rs.as_mesh(xyz, tri), raw=raw, rel_tol=0.0)["counts"][0] == 77
    assert rs.render(cam, *rs.as_mesh(xyz, tri))["counts"] == [0] * 7


def test_wall_mesh_rendered_into_its_view():
    """The wall of test_voxel_mesh_restatement: every vertex lies within `bound` of the plane z = depth (derived there:
    size * q / (size - q) + 8 * depth * 2^-21, q = trunc / 1024), so every point of every triangle does, a triangle
    being the convex hull of its vertices.  A ray that meets the plane at incidence angle a meets the mesh within
    bound / cos a of that point along the ray; the pinhole depth is the z of the hit, which is within bound itself of
    `depth`.  md adds one float32 rounding, depth * 2^-24.  Both forms are asserted; neither is fitted."""
    depth, trunc = 4.1, 0.5
    camw, depths, cells, origin, size = ms.wall_scene(depth=depth)
    colours = np.tile(np.array([[10.0, 20.0, 30.0]], F32), (len(cells), 1))
    m = ms.mesh(cells, colours, origin, size, camw, depths, [0], trunc)
    out = rs.render(camw, m["vertices"], m["faces"], raw=depths[0], rel_tol=0.01)
    q = trunc / 1024.0
    bound = size * q / (size - q) + 8 * depth * 2.0 ** -21
    d = rs.rays(camw)
    cos = (1.0 / np.sqrt((d * d).sum(1))).reshape(out["depth"].shape)
    won = out["face"] >= 0
    err = np.abs(out["depth"].astype(F64) - depth)
    print("wall: pixels hit", int(won.sum()), "max error", err[won].max(), "bound", bound)
    assert won.sum() > 100
    assert (err[won] <= bound / cos[won] + depth * 2.0 ** -24).all()
    assert (err[won] <= bound + depth * 2.0 ** -24).all()
    assert out["counts"][0] == won.sum() and out["counts"][6] == 0      # all agree with the raw wall, none back-facing
    assert (out["colour"][won] == np.array([10.0, 20.0, 30.0], F32)).all()
    assert (out["normal"][won][:, 2] < -0.99).all()                      # towards the camera
