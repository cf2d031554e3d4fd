"""Point-to-triangle distances on the GPU (acmmp_fusion_surface_distance, include/acmmp.h), bit for bit against the
exhaustive restatement (surface_distance_support): d2, nearest_face, every word of the summary and n_skipped; the plan's
counts against a restated count.  The cell of the face grid is forced through acmmp_fusion_surface_grid, the call's own
hook: acmmp_fusion_distance_grid's forced cell is for the cloud distances and the align calls, and its outputs are theirs."""
import functools

import numpy as np
import pytest

import cloud_distance_support as cd
import mesh_render_support as rs
import surface_distance_support as sd
import visibility_support as vis
from acmmp import capi
from conftest import assert_bitwise_equal
from fusion_scene_support import fill

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
CAM = np.zeros(1, capi.CAMERA_DTYPE)
CAM["width"], CAM["height"] = 8, 8
TAUS = (0.0, 0.25, 0.5, 1.0)                                       # in units of the case's max_dist


def _fusion():
    return capi.Fusion(0, CAM)


def _taus(max_dist):
    return tuple(float(F32(t * max_dist)) for t in TAUS)


def _assert_surface(fu, query, want, max_dist, what="", small_max=0, cell=0.0, mesh=None, M=None):
    """One surface_distance under a plan and a forced cell, every output against the restatement's (d2, nearest,
    summary, skipped), the plan against the restated count when the mesh is given.  Returns the bytes read."""
    fu.surface_plan(small_max)
    fu.surface_grid(cell)
    r = fu.surface_distance(query, max_dist, _taus(max_dist))
    d2, nn = fu.surface_results(squared=True)
    plan, grid = fu.surface_plan(small_max), fu.surface_grid(cell)
    print(what, query, "queries", r.n_query, "valid", r.n_valid, "matched", r.n_matched, "mean", r.mean, plan, grid)
    assert d2.dtype == F32 and nn.dtype == np.int32
    assert_bitwise_equal(d2, want[0], f"{what}: d2")
    assert np.array_equal(nn, want[1]), f"{what}: nearest_face"
    assert sd.summary_of(r) == want[2], f"{what}: summary"
    assert plan["skipped"] == want[3], f"{what}: n_skipped"
    assert_bitwise_equal(fu.surface_results(0, len(nn))[0], np.sqrt(want[0]), f"{what}: dist")
    if mesh is not None:
        p = sd.plan(*mesh, small_max=small_max, force_cell=cell, M=M)
        assert plan == {k: p[k] for k in plan}, f"{what}: plan"
        if p["small"] + p["large"]:
            assert grid["cell"] == F32(p["cell"]), f"{what}: cell"
    return d2.tobytes() + nn.tobytes() + np.array(sd.summary_of(r), np.int64).tobytes()


# ---- the cases: (mesh, 1000 queries, max_dist), the restatement computed once

@functools.lru_cache(maxsize=None)
def _case(name):
    if name == "cube":
        mesh, md = sd.cube(), 0.25
        rng = np.random.default_rng(1)
        Q = np.concatenate([sd.cube_surface_points(400), (1.6 * (rng.random((600, 3)) - 0.5)).astype(F32)])
    elif name == "rig":
        v, f, size = sd.rig_mesh()
        mesh, md = (v, f), 1.5 * size
        Q = sd.near_queries(v, f, 1000, 0.5 * size, seed=2)
    else:
        mesh, md = sd.mixed_mesh(), 0.06
        Q = np.concatenate([sd.near_queries(*mesh, 700, 0.02, seed=3),
                            np.random.default_rng(4).random((300, 3)).astype(F32)])
    assert len(Q) == 1000
    return mesh, Q, md


@functools.lru_cache(maxsize=None)
def _want(name, n=1000):
    mesh, Q, md = _case(name)
    return sd.distances(Q[:n], *mesh, md, _taus(md))


def _loaded(name, n=1000):
    mesh, Q, md = _case(name)
    fu = _fusion()
    assert fu.set_mesh(*mesh) == (len(mesh[0]), len(mesh[1])) and fu.set_reference_cloud(Q[:n]) == n
    return fu, mesh, md


@pytest.mark.parametrize("name", ["cube", "rig", "mixed"])
def test_basic_meshes_twice(name):
    fu, mesh, md = _loaded(name)
    want = _want(name)
    first = _assert_surface(fu, "reference", want, md, name, mesh=mesh)
    assert _assert_surface(fu, "reference", want, md, "again", mesh=mesh) == first        # two runs: identical bytes
    s = want[2]
    assert 0 < s[2] < s[1] == s[0] == 1000                                  # matched and unmatched queries
    if name == "mixed":
        assert fu.surface_plan()["large"] == 2 and fu.surface_plan()["small"] == len(mesh[1]) - 2
        assert (want[1] >= len(mesh[1]) - 2).any() and (want[1][want[1] >= 0] < len(mesh[1]) - 2).any()
    fu.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_query_counts(n):
    """Less than a wave, a wave, one lane more (1000, four workgroups, is every other test)."""
    fu, mesh, md = _loaded("mixed", n)
    _assert_surface(fu, "reference", _want("mixed", n), md, f"{n} queries", mesh=mesh)
    fu.close()


@pytest.mark.parametrize("name", ["rig", "mixed"])
def test_plans_and_cells(name):
    """Every face large, every face small (over a forced coarse cell, so that the registrations stay bounded), the
    default; a tiny, a huge and the automatic cell: the same bits, and the restated counts."""
    fu, mesh, md = _loaded(name)
    want = _want(name)
    A, B, C, _ = sd.corners(*mesh)
    ext = float((np.stack([A, B, C]).max((0, 1)).astype(F64) - np.stack([A, B, C]).min((0, 1))).max())
    auto = sd.plan(*mesh)["cell"]
    seen = {}
    for what, small_max, cell in (("default", 0, 0.0), ("all large", -1, 0.0), ("all small", 2 ** 31 - 1, ext / 3),
                                  ("tiny cell", 0, auto / 3), ("huge cell", 0, 1e6), ("small_max 4", 4, 0.0)):
        seen[what] = _assert_surface(fu, "reference", want, md, what, small_max, cell, mesh=mesh)
        plan, grid = fu.surface_plan(), fu.surface_grid()
        if what == "all large":
            assert plan["small"] == 0 and plan["registrations"] == 0 and plan["large"] == len(mesh[1])
        if what == "all small":
            assert plan["large"] == 0 and plan["small"] == len(mesh[1]) <= plan["registrations"]
        if what == "huge cell":
            assert grid["cells"] == 1 and grid["rings"] == 0 and plan["registrations"] == plan["small"] == len(mesh[1])
        if what == "tiny cell":
            assert grid["rings"] >= 2
    assert len(set(seen.values())) == 1
    fu.surface_plan(0)
    fu.close()


def test_extreme_geometry():
    """Mesh and queries moved by 1e4 on every axis; a sheet exactly in a cell boundary plane; queries exactly on
    vertices, edges and faces; queries outside the box, nearer and further than the cap."""
    cube, Q, md = _case("cube")
    moved = (cube[0].copy(), cube[1])
    moved[0][:, :3] += F32(1e4)
    Qm = (Q + F32(1e4)).astype(F32)
    fu = _fusion()
    fu.set_mesh(*moved)
    fu.set_reference_cloud(Qm)
    want = sd.distances(Qm, *moved, md, _taus(md))
    assert 0 < want[2][2] < 1000
    a = _assert_surface(fu, "reference", want, md, "moved by 1e4", mesh=moved)
    assert _assert_surface(fu, "reference", want, md, "moved, cell 0.01", cell=0.01, mesh=moved) == a
    mesh = sd.boundary_mesh()                                              # a sheet in the plane between two cells of 0.25
    A, B, C, _ = sd.corners(*mesh)
    on = np.concatenate([A, (A + B) / 2, (B + C) / 2, A / 2 + B / 4 + C / 4]).astype(F32)
    md = 0.125
    outside = np.array([[1.0625, 0.5, 0.5], [1.125, 0.5, 0.5], [1.1875, 0.5, 0.5], [0.5, -0.125, 0.5], [0.5, 0.5, 3.0],
                        [0.5, -0.12500001, 0.5], [-5, -5, -5], [0.3, 0.3, 0.625], [0.3, 0.3, 0.62500006]], F32)
    Qs = np.concatenate([on, on + F32(0.03125), outside])
    fu.set_mesh(*mesh)
    fu.set_reference_cloud(Qs)
    want = sd.distances(Qs, *mesh, md, _taus(md))
    assert (want[0][:len(on)] == 0).all() and want[1][-2] >= 0 and want[1][-1] == -1 and want[1][-3] == -1
    b = _assert_surface(fu, "reference", want, md, "boundary plane", cell=0.25, mesh=mesh)
    assert fu.surface_grid(0.25)["cell"] == F32(0.25)
    assert _assert_surface(fu, "reference", want, md, "boundary plane, automatic cell", mesh=mesh) == b
    fu.close()


def _chain():
    """A fusion object holding a scene, a voxel, a clean and a visible result of the constructed sphere rig and, as
    its mesh, the first 1500 faces of the rig's restated mesh (the same frame)."""
    cams, depths, normals, colours, cloud, size = vis.constructed("sphere")
    fu = fill(capi.Fusion(0, cams), cams, depths, normals, colours)
    fu.set_scene(cloud)
    nv = fu.voxelize(size)[0]
    nc = fu.voxel_clean(26, 1, 2, 1)[0]
    nk = fu.voxel_visibility(list(range(len(cams))), 0.01, 1, 1, 0, source="clean")[0]
    assert 0 < nk <= nc < nv
    mesh = sd.rig_part()
    fu.set_mesh(*mesh)
    data = {"scene": fu.scene_points(0, len(cloud))[::4], "voxels": fu.voxel_points(0, nv), "clean": fu.clean_points(0, nc),
            "visible": fu.visible_points(0, nk)}
    return fu, size, mesh, data


M_TEST = sd.M_TEST


def test_query_sources_and_transform():
    """All five query sources.  With a transform set the reference queries see the moved vertices and the data queries do
    not; the restatement is given the same float32 vertices (sd.transformed)."""
    fu, size, mesh, data = _chain()
    md = 1.5 * size
    fu.set_scene(data["scene"])                                            # every fourth point: the restatement's time
    nv = fu.voxelize(size)[0]
    nc = fu.voxel_clean(26, 1, 2, 1)[0]
    nk = fu.voxel_visibility([0, 1, 2], 0.01, 1, 1, 0, source="clean")[0]
    data = {"scene": data["scene"], "voxels": fu.voxel_points(0, nv), "clean": fu.clean_points(0, nc),
            "visible": fu.visible_points(0, nk)}
    ref = sd.near_queries(*mesh, 500, 0.5 * size, seed=6)
    fu.set_reference_cloud(ref)
    wants = {q: sd.distances(data[q], *mesh, md, _taus(md)) for q in data}
    wants["reference"] = sd.distances(ref, *mesh, md, _taus(md))
    for q in sd.QUERIES:
        assert 0 < wants[q][2][2] < wants[q][2][1], q
        _assert_surface(fu, q, wants[q], md, "no transform", mesh=mesh)
    fu.set_cloud_transform(M_TEST)
    ref_m = sd.transformed(ref, M_TEST)                                    # queries that follow the mesh, as float32
    fu.set_reference_cloud(ref_m)
    moved = sd.distances(ref_m, *mesh, md, _taus(md), M=M_TEST)
    assert 0 < moved[2][2] and moved[2] != wants["reference"][2]
    _assert_surface(fu, "reference", moved, md, "transform", mesh=mesh, M=M_TEST)
    for q in ("scene", "voxels", "clean", "visible"):
        _assert_surface(fu, q, wants[q], md, "transform, data query", mesh=mesh)
    assert np.array_equal(fu.cloud_transform(), M_TEST)                    # the call leaves the transform,
    assert_bitwise_equal(fu.mesh_vertices(0, len(mesh[0])), mesh[0], "mesh")   # the mesh
    assert_bitwise_equal(fu.voxel_points(0, nv), data["voxels"], "voxels")     # and the sources alone
    fu.close()


def test_empty_and_invalid_input():
    Q = np.concatenate([np.random.default_rng(8).standard_normal((200, 3)).astype(F32),
                        [[np.nan, 0, 0], [0, np.inf, 0], [0.25, 0.25, 1]]]).astype(F32)
    v, f = sd.invalid_mesh()                                               # invalid faces, the needle, the point
    fu = _fusion()
    fu.set_reference_cloud(Q)
    for what, faces in (("invalid and degenerate", f), ("only invalid", f[[0, 2]]), ("only the needle", f[[3]]),
                        ("empty mesh", f[:0])):
        fu.set_mesh(v, faces)
        want = sd.distances(Q, v, faces, 1.0, _taus(1.0))
        for small_max in (0, -1):
            _assert_surface(fu, "reference", want, 1.0, what, small_max, mesh=(v, faces))
    assert fu.set_mesh(v[:0], f[:0]) == (0, 0)
    _assert_surface(fu, "reference", sd.distances(Q, v[:0], f[:0], 1.0, _taus(1.0)), 1.0, "no vertex")
    fu.set_mesh(v, f)
    fu.set_reference_cloud(Q[:0])                                          # no queries
    r = fu.surface_distance("reference", 1.0, _taus(1.0))
    assert sd.summary_of(r) == [0] * cd.SUMMARY_WORDS and len(fu.surface_results()[0]) == 0
    assert fu.surface_plan() == {"small": 4, "large": 0, "registrations": fu.surface_plan()["registrations"], "skipped": 2}
    fu.set_scene(np.zeros((0, 9), F32))
    assert sd.summary_of(fu.surface_distance("scene", 1.0)) == [0] * cd.SUMMARY_WORDS
    fresh = _fusion()                                                      # no reference cloud: refused
    fresh.set_mesh(v, f)
    with pytest.raises(capi.AcmmpError):
        fresh.surface_distance("reference", 1.0)
    with pytest.raises(capi.AcmmpError):
        fresh.surface_results(0, 1)
    fresh.close()
    fu.close()


def test_invalid_arguments_leave_everything():
    fu, mesh, md = _loaded("mixed")
    want = _want("mixed")
    _assert_surface(fu, "reference", want, md, "before")
    L, h = fu.L, fu.h
    tau = np.array(_taus(md), F32)
    p = lambda a: a.ctypes.data
    out = np.zeros(cd.SUMMARY_WORDS, np.int64)

    def call(query=5, max_dist=md, n_tau=4, taus=tau):
        return L.acmmp_fusion_surface_distance(h, query, max_dist, n_tau, None if taus is None else p(taus), p(out))
    bad_tau = lambda x: np.array([0.01, x], F32)
    cases = {"query 4": dict(query=4), "query 6": dict(query=6), "query -1": dict(query=-1),
             "no scene result": dict(query=0), "no voxel result": dict(query=1), "no clean result": dict(query=2),
             "no visible result": dict(query=3), "max_dist 0": dict(max_dist=0.0), "max_dist < 0": dict(max_dist=-1.0),
             "max_dist nan": dict(max_dist=float("nan")), "max_dist inf": dict(max_dist=float("inf")),
             "n_tau 9": dict(n_tau=9), "n_tau -1": dict(n_tau=-1), "tau NULL": dict(n_tau=1, taus=None),
             "tau nan": dict(n_tau=2, taus=bad_tau(np.nan)), "tau < 0": dict(n_tau=2, taus=bad_tau(-0.01)),
             "tau inf": dict(n_tau=2, taus=bad_tau(np.inf)), "tau > max_dist": dict(n_tau=2, taus=bad_tau(md * 1.01))}

    def unchanged(what):
        d2, nn = fu.surface_results(0, 1000, squared=True)
        assert_bitwise_equal(d2, want[0], f"after {what}: d2")
        assert np.array_equal(nn, want[1]), f"after {what}: nearest_face"
    for what, kw in cases.items():
        assert call(**kw) == 1, what                                       # ACMMP_ERR_INVALID_ARGUMENT
        unchanged(what)
    for cell in (-1.0, float("nan"), float("inf")):                        # a forced cell that is not finite and > 0
        fu.surface_grid(cell)
        assert call() == 1
        unchanged(f"forced cell {cell}")
    fu.surface_grid(0.0)
    for first, n in ((0, 1001), (1000, 1), (-1, 1), (0, -1)):
        assert L.acmmp_fusion_surface_results(h, first, n, None, None) == 1
    assert L.acmmp_fusion_surface_results(h, 1000, 0, None, None) == 0
    assert L.acmmp_fusion_surface_distance(None, 5, md, 0, None, None) == 1
    assert call() == 0 and out.tolist() == want[2]                         # and the call still works
    fresh = _fusion()                                                      # no mesh result
    fresh.set_reference_cloud(_case("mixed")[1])
    with pytest.raises(capi.AcmmpError):
        fresh.surface_distance("reference", md)
    fresh.close()
    fu.close()


def test_lifetimes():
    fu, size, mesh, data = _chain()
    cams, depths, normals, colours = vis.constructed("sphere")[:4]
    ref = (data["voxels"][::2, :3] + F32(0.25 * size)).astype(F32)
    fu.set_reference_cloud(ref)
    gone = lambda: fu.L.acmmp_fusion_surface_results(fu.h, 0, 1, None, None) == 1
    run = lambda q: fu.surface_distance(q, size, (size,))
    dist_gone = lambda: fu.L.acmmp_fusion_distance_results(fu.h, 0, 1, None, None) == 1
    assert gone()
    r = run("reference")
    assert r.n_query == len(ref) and not gone()
    fu.set_view(0, depths[0], normals[0], colours[0])                      # set_view,
    fu.cloud_distance("voxels", "data_to_ref", size, (size,))              # a distance call
    fu.cloud_align("voxels", "rigid", size, 2)                        # and the align calls leave it alone
    fu.cloud_align_plane("voxels", size, 2)
    assert not gone()
    d_before = fu.distance_results(squared=True)
    rec_before = fu.align_plane_records(0, 1, size)
    grid_before = fu.distance_grid()
    fu.surface_grid(size / 2)
    run("voxels")                                                          # and it leaves their results alone,
    assert not dist_gone()
    assert fu.distance_grid() == grid_before and fu.surface_grid()["cell"] == F32(size / 2)   # their grid hook too
    fu.distance_grid(size / 3)                                             # whose forced cell is not this call's
    run("voxels")
    assert fu.surface_grid()["cell"] != F32(size / 3)
    fu.distance_grid(0.0)
    after = fu.distance_results(squared=True)
    assert_bitwise_equal(after[0], d_before[0], "distance result")
    assert np.array_equal(after[1], d_before[1])
    assert fu.align_plane_records(0, 1, size)[0].words.tolist() == rec_before[0].words.tolist()
    fu.set_reference_cloud(ref)                                            # a data query's result outlives the reference cloud
    fu.set_cloud_transform(M_TEST)                                         # and the transform
    assert not gone()
    run("reference")
    fu.set_cloud_transform(M_TEST)                                         # a reference query's goes when the transform is set,
    assert gone()
    run("reference")
    fu.set_cloud_transform(None)                                           # cleared,
    assert gone()
    run("reference")
    fu.set_reference_cloud(ref)                                            # or the reference cloud replaced
    assert gone()
    run("reference")
    fu.voxelize(size)                                                      # not its source
    assert not gone()
    run("voxels")
    fu.voxelize(size)                                                      # the query source replaced
    assert gone()
    fu.voxel_clean(26, 1, 2, 1)
    run("clean")
    fu.voxel_clean(26, 1, 2, 1)
    assert gone()
    fu.voxel_visibility([0, 1], 0.01, 1, 1, 0, source="clean")
    run("visible")
    fu.voxel_clean(26, 1, 2, 1)                                            # the visible cloud goes with the clean cloud
    assert gone()
    run("scene")
    fu.set_mesh(*mesh)                                                     # the mesh replaced
    assert gone()
    run("scene")
    fu.set_scene(data["scene"])                                            # the scene replaced: a set mesh stays, the result goes
    assert gone()
    run("scene")
    fu.voxelize(size)
    fu.voxel_mesh([0, 1, 2], 3 * size)                                     # the mesh replaced by a mesh call
    assert gone()
    run("reference")
    fu.set_scene(data["scene"])                                            # which the scene takes with it
    assert gone()
    with pytest.raises(capi.AcmmpError):
        run("reference")
    fu.close()
