"""Voxel-grid reduction of the scene cloud on the GPU (acmmp_fusion_voxelize, include/acmmp.h), bit for bit
against the numpy restatement (voxel_support) run on the very cloud the device holds."""
import numpy as np
import pytest

import voxel_support as vs
from acmmp import capi, pipeline
from conftest import assert_bitwise_equal
from fusion_scene_support import fill
from pipeline_support import small_dataset

pytestmark = pytest.mark.gpu


def _scene(name, unique=False):
    cams, depths, normals, colours, refs, lists = vs.SCENES[name]()
    gf = fill(capi.Fusion(0, cams), cams, depths, normals, colours)
    total, _ = gf.run_scene(refs, lists, unique=unique)
    return gf, total, gf.scene_points(0, total)


def _assert_equals_restatement(gf, cloud, size, origin, min_points, what):
    n, info = gf.voxelize(size, origin=origin, min_points=min_points)
    want = vs.voxelize(cloud, size, origin, min_points)
    print(what, "voxels", n, "occupied", info["n_occupied"], "rejected", info["n_rejected"], "of", cloud.shape[0])
    assert (n, info["n_occupied"], info["n_rejected"]) == (want["points"].shape[0], want["n_occupied"], want["n_rejected"]), what
    assert_bitwise_equal(info["origin"], want["origin"], f"{what}: origin")
    pts, cnt = gf.voxel_points(0, n, counts=True)
    assert_bitwise_equal(pts, want["points"], f"{what}: points")
    assert np.array_equal(cnt, want["counts"]) and cnt.dtype == np.int32, what
    return pts, cnt


CASES = [("rig_256x128", False), ("rig_256x128", True), ("rig_50x30_edges", False), ("sphere_64x32", False),
         ("pinhole_64x32", False)]


@pytest.mark.parametrize("name,unique", CASES, ids=[f"{n}{'_unique' if u else ''}" for n, u in CASES])
def test_voxels_equal_restatement(name, unique):
    gf, total, cloud = _scene(name, unique)
    assert total > 0
    sizes = vs.scene_sizes(name, cloud)
    for which, size in sizes.items():
        for m in (1, 3):
            pts, cnt = _assert_equals_restatement(gf, cloud, size, None, m, f"{name} {which} min_points {m}")
            if which == "single" and m == 1:
                assert cnt.tolist() == [total]                       # every point adds to one slot
    for m in (1, 3):
        pts, cnt = _assert_equals_restatement(gf, cloud, sizes["middle"], [0, 0, 0], m, f"{name} centred origin {m}")
    pts, cnt = _assert_equals_restatement(gf, cloud, sizes["middle"], None, 1, f"{name} middle again")
    n = pts.shape[0]
    assert n > 3
    # streamed in three ranges, the range rules of scene_points
    step = n // 3 + 1
    parts = [gf.voxel_points(a, min(step, n - a), counts=True) for a in range(0, n, step)]
    assert len(parts) == 3
    assert_bitwise_equal(np.concatenate([p for p, _ in parts], 0), pts, f"{name}: ranges")
    assert np.array_equal(np.concatenate([c for _, c in parts], 0), cnt)
    assert_bitwise_equal(gf.voxel_points(1, 2), pts[1:3], "points alone")
    for first, k in ((1, n), (n + 1, 0), (-1, 1), (0, -1)):
        with pytest.raises(capi.AcmmpError):
            gf.voxel_points(first, k)
    assert gf.voxel_points(n, 0).shape == (0, 9)
    gf.close()


def test_segmented_compaction(monkeypatch):
    """A scene of several compaction segments (the scan's offsets are 32-bit, so a large scene is cut): the 50x30
    rig in segments of 1024 and of 256 points, the second with a ragged last one."""
    gf, total, cloud = _scene("rig_50x30")
    assert total > 2048 and total % 256 != 0
    for seg in ("1024", "256"):
        monkeypatch.setenv("ACMMP_VOXEL_SEGMENT_POINTS", seg)
        for which in ("single", "middle", "fine"):
            for m in (1, 3):
                _assert_equals_restatement(gf, cloud, vs.RIG_SIZES[which], None, m, f"segments of {seg}: {which} {m}")
    gf.close()


@pytest.mark.parametrize("name", list(vs.FORCED_TABLES))
def test_forced_table(name):
    gf, total, cloud = _scene(name)
    size, slots = vs.FORCED_TABLES[name]
    assert slots > total >= slots // 2
    n, info = gf.voxelize(size)
    auto = gf.voxel_points(0, n, counts=True)
    st = gf.voxel_table(slots)
    assert st["slots"] == vs.auto_slots(total) and st["occupied"] == info["n_occupied"]
    assert st["wrapped"] == vs.table_layout(vs.scene_keys(cloud, size), st["slots"])[1]
    n2, info2 = gf.voxelize(size)
    forced = gf.voxel_points(0, n2, counts=True)
    st = gf.voxel_table(slots)
    want = vs.table_layout(vs.scene_keys(cloud, size), slots)
    print(name, "forced", st, "restated (occupied, wrapped)", want)
    assert st["slots"] == slots and st["occupied"] == info2["n_occupied"] == want[0]
    assert st["wrapped"] == want[1] > 0 and st["max_probe"] >= 1
    assert n2 == n and info2["n_rejected"] == info["n_rejected"]
    assert_bitwise_equal(forced[0], auto[0], f"{name}: forced vs automatic table")
    assert np.array_equal(forced[1], auto[1])
    assert_bitwise_equal(forced[0], vs.voxelize(cloud, size)["points"], f"{name}: forced table vs restatement")
    # a power of two <= N, a size that is no power of two, one below 64: refused, the object unchanged
    for bad in (slots // 2, slots + 1, 32, -64):
        gf.voxel_table(bad)
        with pytest.raises(capi.AcmmpError):
            gf.voxelize(size)
        again = gf.voxel_points(0, n, counts=True)
        assert_bitwise_equal(again[0], forced[0], f"voxel result after refusing {bad} slots")
        assert np.array_equal(again[1], forced[1])
        assert_bitwise_equal(gf.scene_points(0, total), cloud, "scene result")
    assert gf.voxel_table(0)["slots"] == slots                      # still the last successful run's
    assert gf.voxelize(size)[0] == n and gf.voxel_table(0)["slots"] == vs.auto_slots(total)
    gf.close()


def test_voxelize_is_repeatable_and_isolated():
    cams, depths, normals, colours, refs, lists = vs.SCENES["rig_50x30_edges"]()
    gf = fill(capi.Fusion(0, cams), cams, depths, normals, colours)
    with pytest.raises(capi.AcmmpError):
        gf.voxelize(0.5)                                            # no scene result yet
    with pytest.raises(capi.AcmmpError):
        gf.voxel_points(0, 1)
    total, _ = gf.run_scene(refs, lists)
    before = gf.scene_points(0, total, provenance=True)
    size = vs.RIG_SIZES["middle"]
    n, info = gf.voxelize(size, min_points=2)
    first = gf.voxel_points(0, n, counts=True)
    n2, info2 = gf.voxelize(size, min_points=2)
    second = gf.voxel_points(0, n2, counts=True)
    assert n == n2 > 1 and info["n_occupied"] == info2["n_occupied"] and info["n_rejected"] == info2["n_rejected"]
    assert_bitwise_equal(second[0], first[0], "second run")
    assert np.array_equal(second[1], first[1])
    assert_bitwise_equal(info2["origin"], info["origin"], "origin")
    bad = [dict(size=0.0), dict(size=-1.0), dict(size=float("inf")), dict(size=float("nan")),
           dict(size=size, min_points=0), dict(size=size, min_points=-3), dict(size=size, origin=[0, float("nan"), 0]),
           dict(size=size, origin=[float("inf"), 0, 0])]
    for kw in bad:
        with pytest.raises(capi.AcmmpError):
            gf.voxelize(**kw)
        again = gf.voxel_points(0, n, counts=True)
        assert_bitwise_equal(again[0], first[0], f"voxel result after refusing {kw}")
        assert np.array_equal(again[1], first[1])
    for a, b in zip(gf.scene_points(0, total, provenance=True), before):
        assert_bitwise_equal(a, b, "scene result after voxelize")
    # a new scene discards the voxel result
    total2, _ = gf.run_scene(refs[:1], lists[:1])
    with pytest.raises(capi.AcmmpError):
        gf.voxel_points(0, 1)
    assert gf.voxel_points(0, 0).shape == (0, 9)
    assert gf.voxelize(size)[0] > 0
    # an empty scene: the all-zero view as the only reference
    assert gf.run_scene([2], [[0, 1]])[0] == 0
    n0, info0 = gf.voxelize(size)
    assert n0 == 0 and info0["n_occupied"] == 0 and info0["n_rejected"] == 0 and not info0["origin"].any()
    n0, info0 = gf.voxelize(size, origin=[1, 2, 3])
    assert n0 == 0 and info0["origin"].tolist() == [1, 2, 3]
    assert gf.voxel_points(0, 0, counts=True)[1].shape == (0,)
    with pytest.raises(capi.AcmmpError):
        gf.voxel_points(0, 1)
    gf.close()


def test_rejected_points_on_the_device():
    """Non-finite and oversized values cannot come out of k_fuse on these scenes, so the rejection of step 1 is
    exercised through view inputs: NaN normals and a NaN depth travel into the scene cloud."""
    cams, depths, normals, colours, refs, lists = vs.SCENES["rig_50x30"]()
    normals = [n.copy() for n in normals]
    normals[0][::3, ::2, 1] = np.nan
    normals[1][5:9, :, 0] = np.inf
    gf = fill(capi.Fusion(0, cams), cams, depths, normals, colours)
    total, _ = gf.run_scene(refs, lists)
    cloud = gf.scene_points(0, total)
    bad = int((~vs.finite_points(cloud)).sum())
    print("points", total, "non-finite", bad)
    assert 0 < bad < total
    for m in (1, 2):
        _assert_equals_restatement(gf, cloud, vs.RIG_SIZES["middle"], None, m, f"non-finite normals {m}")
    gf.close()


def test_pipeline_voxel_fusion(tmp_path):
    ds = small_dataset(64, 32, 3)
    pipe = pipeline.Pipeline(ds, order="reference", geom_iterations=1).run()
    plain = pipe.run_fusion(ply_path=str(tmp_path / "plain.ply"))
    assert pipe.fusion_info is None and plain.shape[0] > 0
    ok = vs.finite_points(plain)
    size = float((plain[ok, :3].max(0) - plain[ok, :3].min(0)).max()) / 16
    for unique, m in ((False, 1), (True, 2)):
        got = pipe.run_fusion(ply_path=str(tmp_path / "gpu.ply"), unique=unique, chunk_points=7, voxel_size=size,
                              voxel_min_points=m)
        info = dict(pipe.fusion_info)
        want = pipe.run_fusion(fusion_factory=vs.RestatedVoxelFusion, ply_path=str(tmp_path / "restated.ply"),
                               unique=unique, voxel_size=size, voxel_min_points=m)
        print("unique", unique, "min_points", m, info)
        assert 1 < got.shape[0] < info["scene_points"]
        assert_bitwise_equal(got, want, "Pipeline.run_fusion voxel cloud")
        assert info == pipe.fusion_info
        assert (tmp_path / "gpu.ply").read_bytes() == (tmp_path / "restated.ply").read_bytes()
