"""Visibility check of the voxel cloud on the GPU (acmmp_fusion_voxel_visibility, include/acmmp.h), bit for bit
against the sequential restatement (visibility_support) run on the very cloud the device holds."""
import numpy as np
import pytest

import visibility_support as vis
import voxel_support as vs
from acmmp import capi, pipeline
from conftest import assert_bitwise_equal
from fusion_scene_support import f2i_sat, fill
from pipeline_support import small_dataset

pytestmark = pytest.mark.gpu

CLEAN = (26, 1, 2, 1)               # the clean that the "clean" source cases run first


def _pair(rig, cloud=None, size=None, n_set=None):
    """The device object and the restated one over the rig's views, holding the same scene cloud and voxel result
    (checked bit for bit).  n_set: only the first n_set views are given to set_view."""
    cams, depths, normals, colours, built, built_size = vis.constructed(rig)
    cloud = built if cloud is None else cloud
    size = built_size if size is None else size
    k = len(cams) if n_set is None else n_set
    gf = fill(capi.Fusion(0, cams), cams[:k], depths, normals, colours)
    rf = fill(vis.RestatedVisibilityFusion(cams), cams[:k], depths, normals, colours)
    assert gf.set_scene(cloud) == rf.set_scene(cloud)
    _voxelize(gf, rf, size)
    return gf, rf, size


def _voxelize(gf, rf, size):
    n, want = gf.voxelize(size)[0], rf.voxelize(size)[0]
    assert n == want > 0
    pts, cnt = gf.voxel_points(0, n, counts=True)
    assert_bitwise_equal(pts, rf.voxels["points"], "voxel points")
    assert np.array_equal(cnt, rf.voxels["counts"])
    return n


def _clean(gf, rf, args=CLEAN):
    n, want = gf.voxel_clean(*args)[0], rf.voxel_clean(*args)[0]
    assert 0 < n == want < rf.voxels["points"].shape[0]
    assert_bitwise_equal(gf.clean_points(0, n), rf.clean_points(0, n), "clean points")
    return n


def _read(gf, n, entries):
    """Everything a visibility call leaves: the kept points, counts and tallies, and every entry's tallies."""
    return (*gf.visible_points(0, n, counts=True, tallies=True), gf.visibility_tallies(0, entries))


def _assert_visibility(gf, rf, views, tol, radius, th, source, what):
    """One voxel_visibility, every output against the restatement.  Returns (n, info, the four arrays read)."""
    n, info = gf.voxel_visibility(views, tol, radius, *th, source=source)
    wn, winfo = rf.voxel_visibility(views, tol, radius, *th, source=source)
    entries = rf.visible["tallies"].shape[0]
    print(what, source, "tol", tol, "radius", radius, "thresholds", th, "entries", entries, "kept", n, info)
    assert (n, info) == (wn, winfo), what
    got, want = _read(gf, n, entries), _read(rf, n, entries)
    for g, w, name in zip(got, want, ("points", "counts", "kept tallies", "tallies")):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name}"
        assert_bitwise_equal(g, w, f"{what}: {name}")
    return n, info, got


@pytest.mark.parametrize("source", ["voxel", "clean"])
@pytest.mark.parametrize("rig", list(vis.RIGS))
def test_base(rig, source):
    gf, rf, _ = _pair(rig)
    if source == "clean":
        _clean(gf, rf)
    views = list(range(len(rf.cams)))
    totals = set()
    for radius in (0, 1):
        for tol in vis.TOLERANCES:
            for th in vis.THRESHOLDS:
                n, info, _ = _assert_visibility(gf, rf, views, tol, radius, th, source, rig)
                totals.add(tuple(info["class_totals"]))
            assert n == rf.visible["tallies"].shape[0]                # (0, 4096) keeps every entry
    assert len(totals) == 6 and all(min(t) > 0 for t in totals)       # radius and tolerance each change the classes
    gf.close()


def test_long_view_list():
    """70 positions cycling the 4 views: more than one chunk of the tally kernel, and more than a wave is wide."""
    gf, rf, _ = _pair("sphere")
    single = [_assert_visibility(gf, rf, [k], 0.01, 1, (1, 0), "voxel", f"view {k}")[2][3].astype(np.int64) for k in range(4)]
    _, _, got = _assert_visibility(gf, rf, [k % 4 for k in range(70)], 0.01, 1, (17, 18), "voxel", "70 positions")
    assert np.array_equal(got[3], 18 * (single[0] + single[1]) + 17 * (single[2] + single[3]))
    assert 0 < got[0].shape[0] < got[3].shape[0]
    # the two sides of the chunk boundary, and the longest list
    for n_list in (capi_chunk(), capi_chunk() + 1, 4096):
        _assert_visibility(gf, rf, [(3 * k) % 4 for k in range(n_list)], 0.05, 0, (n_list // 4, n_list // 8), "voxel", f"{n_list} positions")
    gf.close()


def capi_chunk():
    return 32                       # kVisChunk of csrc/fusion.h


@pytest.mark.parametrize("source", ["voxel", "clean"])
def test_segments(source, monkeypatch):
    """Compaction segments of 256 entries over an entry count that is no multiple of 256."""
    def run():
        gf, rf, _ = _pair("sphere")
        entries = _clean(gf, rf) if source == "clean" else rf.voxels["points"].shape[0]
        assert entries > 512 and entries % 256 != 0
        out = [_assert_visibility(gf, rf, [0, 1, 2, 3], 0.01, radius, th, source, "segments")
               for radius, th in ((0, (1, 0)), (1, (2, 1)), (1, (0, 4096)), (0, (5, 0)))]
        gf.close()
        return out
    plain = run()
    monkeypatch.setenv("ACMMP_VOXEL_SEGMENT_POINTS", "256")
    for (n, info, got), (wn, winfo, want) in zip(run(), plain):
        assert (n, info) == (wn, winfo)
        for a, b in zip(got, want):
            assert_bitwise_equal(a, b, "segmented")
    assert plain[3][0] == 0                                             # nothing kept: an empty result through the same path


def _edge_cloud(cams, depths):
    """The pixel centres of view 0's last column, last row and first row at their depth.  A SPHERE view's first row is
    the pole, one point whatever the column, so the points at row coordinate 0.4 are added: they round to row 0 too."""
    H, W = depths[0].shape
    cols = np.concatenate([np.full(H, W - 1), np.arange(W), np.arange(W), np.arange(W)])
    rows = np.concatenate([np.arange(H), np.full(W, H - 1), np.zeros(W, np.int64), np.zeros(W, np.int64)])
    at = rows.astype(np.float64)
    at[-W:] = 0.4
    return vis.as_cloud(vis.world_points(cams[0], cols, at, depths[0][rows, cols]), (9, 9, 9))


def test_image_edges_and_a_hole():
    cams, depths, normals, colours, _, size = vis.constructed("sphere")
    H, W = depths[0].shape
    gf, rf, _ = _pair("sphere", cloud=_edge_cloud(cams, depths), size=size / 64)
    pts = rf.voxels["points"]
    proj = vis.project(cams[:1], pts[:, :3])[0]
    c, r = f2i_sat(proj[:, 0] + np.float32(0.5)), f2i_sat(proj[:, 1] + np.float32(0.5))
    assert (c == W - 1).sum() >= H // 2 and ((r == H - 1) & (c < W)).sum() >= W // 2 and ((r == 0) & (c >= 0) & (c < W)).sum() >= W // 2
    views = [0, 1, 2, 3]
    for radius in (0, 1):
        _, info, got = _assert_visibility(gf, rf, views, 0.01, radius, (1, 0), "voxel", "edges")
        assert info["class_totals"][0] >= len(pts)                      # every entry lies on view 0's surface
    # a hole in view 1: support there turns into unobserved, and a visible result survives set_view
    _, _, before = _assert_visibility(gf, rf, [1], 0.01, 1, (1, 0), "voxel", "view 1")
    p1 = vis.project(cams[1:2], pts[:, :3])[0]
    c1, r1 = f2i_sat(p1[:, 0] + np.float32(0.5)), f2i_sat(p1[:, 1] + np.float32(0.5))
    mid = np.flatnonzero(before[3][:, 0] == 1)
    mid = mid[len(mid) // 2]                                          # a rectangle around an entry that view 1 supports
    r_lo, r_hi, c_lo, c_hi = max(int(r1[mid]) - 3, 0), int(r1[mid]) + 4, max(int(c1[mid]) - 6, 0), int(c1[mid]) + 7
    holed = depths[1].copy()
    holed[r_lo:r_hi, c_lo:c_hi] = 0
    for fu in (gf, rf):
        fu.set_view(1, holed, normals[1], colours[1])
    for a, b in zip(_read(gf, before[0].shape[0], len(pts)), before):
        assert_bitwise_equal(a, b, "visible result after set_view")
    _, _, after = _assert_visibility(gf, rf, [1], 0.01, 1, (1, 0), "voxel", "view 1 with a hole")
    lost = (before[3][:, 0] == 1) & (after[3].sum(1) == 0)
    assert lost.sum() > 0 and (after[3].sum(1) <= before[3].sum(1)).all()
    assert lost[mid] and ((c1[lost] >= c_lo) & (c1[lost] < c_hi) & (r1[lost] >= r_lo) & (r1[lost] < r_hi)).all()
    gf.close()


def _gone(gf):
    for read in (gf.visible_points, gf.visibility_tallies):
        with pytest.raises(capi.AcmmpError):
            read(0, 1)
        read(0, 0)


def test_lifetimes_and_errors():
    cams, depths, normals, colours, cloud, size = vis.constructed("sphere")
    gf, rf, _ = _pair("sphere", n_set=3)                             # view 3 is never set
    nv = rf.voxels["points"].shape[0]
    _gone(gf)
    with pytest.raises(capi.AcmmpError):
        gf.voxel_visibility([0], 0.01, source="clean")               # no clean result yet
    views = [0, 1, 2]
    n, _, first = _assert_visibility(gf, rf, views, 0.01, 1, (1, 0), "voxel", "lifetimes")
    assert 0 < n < nv
    nc = _clean(gf, rf)                                              # a clean leaves a visible result of the voxel result
    state = lambda: (*_read(gf, n, nv), *gf.voxel_points(0, nv, counts=True), *gf.clean_points(0, nc, counts=True, component=True),
                     gf.scene_points(0, cloud.shape[0]))
    before = state()
    for a, b in zip(before, first):
        assert_bitwise_equal(a, b, "after voxel_clean")
    # every bad argument: refused, and the visible, voxel, clean and scene results are bitwise what they were
    ok = dict(views=views, rel_tol=0.01, radius=1, min_support=1, max_conflicts=0)
    for bad in (dict(views=[]), dict(views=[0] * 4097), dict(views=[0, 4]), dict(views=[-1, 0]), dict(views=[0, 3]),
                dict(rel_tol=float("nan")), dict(rel_tol=float("inf")), dict(rel_tol=-0.01), dict(radius=2), dict(radius=-1),
                dict(min_support=-1), dict(max_conflicts=-1)):
        for source in ("voxel", "clean"):
            with pytest.raises(capi.AcmmpError):
                gf.voxel_visibility(**{**ok, **bad}, source=source)
        with pytest.raises(ValueError):
            rf.voxel_visibility(**{**ok, **bad})
    v = np.array(views, np.int32)
    for source in (2, -1):
        assert gf.L.acmmp_fusion_voxel_visibility(gf.h, source, 3, v.ctypes.data, 0.01, 1, 1, 0, None, None, None, None) == 1
    assert gf.L.acmmp_fusion_voxel_visibility(gf.h, 0, 3, None, 0.01, 1, 1, 0, None, None, None, None) == 1
    with pytest.raises(ValueError):
        gf.voxel_visibility(views, 0.01, source="scene")
    for a, k in ((1, n), (n + 1, 0), (-1, 1), (0, -1)):
        with pytest.raises(capi.AcmmpError):
            gf.visible_points(a, k)
    for a, k in ((1, nv), (nv + 1, 0), (-1, 1), (0, -1)):
        with pytest.raises(capi.AcmmpError):
            gf.visibility_tallies(a, k)
    for a, b in zip(state(), before):
        assert_bitwise_equal(a, b, "after the refusals")
    # every output pointer may be NULL; ranges concatenate
    assert gf.L.acmmp_fusion_voxel_visibility(gf.h, 0, 3, v.ctypes.data, 0.01, 1, 1, 0, None, None, None, None) == 0
    step = n // 3 + 1
    parts = [gf.visible_points(a, min(step, n - a), counts=True, tallies=True) for a in range(0, n, step)]
    for k in range(3):
        assert_bitwise_equal(np.concatenate([p[k] for p in parts], 0), first[k], "ranges")
    assert_bitwise_equal(gf.visible_points(1, 2), first[0][1:3], "points alone")
    # the clean result as source: the next clean discards it; one of the voxel result it leaves alone (above)
    _assert_visibility(gf, rf, views, 0.01, 1, (1, 0), "clean", "lifetimes")
    assert gf.visibility_tallies(0, nc).shape == (nc, 3)
    with pytest.raises(capi.AcmmpError):
        gf.visibility_tallies(0, nc + 1)                             # the tallies cover the clean result's entries
    _clean(gf, rf)
    _gone(gf)
    # voxelize, set_scene and run_scene each discard it
    for discard in (lambda: gf.voxelize(size), lambda: gf.set_scene(cloud), lambda: gf.run_scene([0], [[1, 2]])):
        gf.set_scene(cloud)
        gf.voxelize(size)
        assert gf.voxel_visibility(views, 0.01, 1)[0] == n
        discard()
        _gone(gf)
    # an empty source gives zeros
    gf.set_scene(cloud)
    assert gf.voxelize(size, min_points=10 ** 6)[0] == 0
    assert gf.voxel_visibility(views, 0.01) == (0, {"unsupported": 0, "conflicting": 0, "class_totals": [0, 0, 0, 0]})
    assert gf.visible_points(0, 0).shape == (0, 9) and gf.visibility_tallies(0, 0).shape == (0, 3)
    with pytest.raises(capi.AcmmpError):
        gf.visible_points(0, 1)
    gf.close()


def test_pipeline_visibility_fusion(tmp_path):
    ds = small_dataset(64, 32, 3)
    pipe = pipeline.Pipeline(ds, order="reference", geom_iterations=1).run()
    plain = pipe.run_fusion(ply_path=str(tmp_path / "plain.ply"))
    ok = vs.finite_points(plain)
    size = float((plain[ok, :3].max(0) - plain[ok, :3].min(0)).max()) / 16
    # the new arguments at their defaults: today's voxel path, its bytes and its fusion_info
    voxel = pipe.run_fusion(ply_path=str(tmp_path / "voxel.ply"), voxel_size=size)
    voxel_info = dict(pipe.fusion_info)
    same = pipe.run_fusion(ply_path=str(tmp_path / "same.ply"), voxel_size=size, visibility_tol=None, visibility_radius=0,
                           visibility_min_support=1, visibility_max_conflicts=0)
    assert pipe.fusion_info == voxel_info and not any(k.startswith("vis") for k in voxel_info)
    assert_bitwise_equal(same, voxel, "defaults")
    assert (tmp_path / "same.ply").read_bytes() == (tmp_path / "voxel.ply").read_bytes()
    with pytest.raises(ValueError):
        pipe.run_fusion(visibility_tol=0.01)                         # the check needs voxel_size
    for kw in (dict(visibility_tol=0.01),
               dict(visibility_tol=0.002, visibility_radius=1, visibility_min_support=2, visibility_max_conflicts=1,
                    voxel_min_neighbours=1, voxel_min_component_voxels=3)):
        got = pipe.run_fusion(ply_path=str(tmp_path / "gpu.ply"), chunk_points=5, voxel_size=size, **kw)
        info = dict(pipe.fusion_info)
        want = pipe.run_fusion(fusion_factory=vis.RestatedVisibilityFusion, ply_path=str(tmp_path / "restated.ply"),
                               voxel_size=size, **kw)
        print(kw, info)
        assert 0 < got.shape[0] == info["visible_voxels"] < info.get("clean_voxels", info["voxels"])
        assert_bitwise_equal(got, want, "Pipeline.run_fusion visible cloud")
        info.pop("rounds", None), pipe.fusion_info.pop("rounds", None)
        assert info == pipe.fusion_info
        assert (tmp_path / "gpu.ply").read_bytes() == (tmp_path / "restated.ply").read_bytes()
