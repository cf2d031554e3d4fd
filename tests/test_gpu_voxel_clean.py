"""Cleaning of the voxel cloud on the GPU (acmmp_fusion_voxel_clean, acmmp_fusion_set_scene; include/acmmp.h), bit
for bit against the sequential restatement (voxel_clean_support) run on the very voxel cloud the device holds."""
import numpy as np
import pytest

import voxel_clean_support as cs
import voxel_support as vs
from acmmp import capi, pipeline, types
from conftest import assert_bitwise_equal
from fusion_scene_support import fill
from pipeline_support import small_dataset

pytestmark = pytest.mark.gpu


def _bare_fusion():
    """A fusion object for clouds that come from the host: one camera, no view ever set."""
    return capi.Fusion(0, np.array([types.make_camera(width=4, height=4)]))


def _voxelize(gf, cloud, size, origin, what):
    """voxelize on the device, held to the restatement on the same cloud; returns the restated voxel result."""
    n, info = gf.voxelize(size, origin=origin)
    want = vs.voxelize(cloud, size, origin)
    assert (n, info["n_occupied"], info["n_rejected"]) == (want["points"].shape[0], want["n_occupied"], want["n_rejected"]), what
    pts, cnt = gf.voxel_points(0, n, counts=True)
    assert_bitwise_equal(pts, want["points"], f"{what}: voxel points")
    assert np.array_equal(cnt, want["counts"]), what
    return want


def _read_clean(gf, n_kept, nv, n_comp):
    return (*gf.clean_points(0, n_kept, counts=True, component=True), *gf.voxel_labels(0, nv), *gf.component_table(0, n_comp))


def _assert_clean(gf, vox, conn, th, what, neighbours=None):
    """One voxel_clean, every output against the restatement.  Returns (info, the nine arrays read)."""
    n, info = gf.voxel_clean(conn, *th)
    want = cs.clean(vox["keys"], vox["counts"], conn, *th, neighbours=neighbours)
    nv = len(vox["counts"])
    print(what, "connectivity", conn, "thresholds", th, "voxels", nv, "kept", n, info)
    assert (n, info["components"], info["components_kept"], info["unsupported"]) == \
        (len(want["kept"]), len(want["root"]), want["n_components_kept"], want["n_unsupported"]), what
    assert info["rounds"] >= (1 if nv else 0)
    got = _read_clean(gf, n, nv, info["components"])
    pts, cnt, comp, lab, sup, root, voxels, points = got
    assert_bitwise_equal(pts, vox["points"][want["kept"]], f"{what}: clean points")
    for g, w, dt, name in ((cnt, vox["counts"][want["kept"]], np.int32, "counts"), (comp, want["component"], np.int64, "component"),
                           (lab, want["label"], np.int64, "label"), (sup, want["support"], np.int32, "support"),
                           (root, want["root"], np.int64, "root"), (voxels, want["voxels"], np.int64, "voxels"),
                           (points, want["points"], np.int64, "points")):
        assert g.dtype == dt and np.array_equal(g, w), f"{what}: {name}"
    return info, got


def _run_constructed(name, monkeypatch=None, segment=None, force_table=False, conns=(6, 18, 26), thresholds=cs.THRESHOLDS):
    cloud = cs.constructed(name)
    if segment:
        monkeypatch.setenv("ACMMP_VOXEL_SEGMENT_POINTS", segment)
    gf = _bare_fusion()
    assert gf.set_scene(cloud) == cloud.shape[0]
    if force_table:
        slots = 64
        while slots <= cloud.shape[0]:
            slots *= 2                                            # the smallest power of two above N (voxel_support)
        gf.voxel_table(slots)
    vox = _voxelize(gf, cloud, 1.0, cs.ORIGIN, name)
    if force_table:
        st = gf.voxel_table(slots)
        print(name, "forced table", st)
        assert st["slots"] == slots and st["max_probe"] > 1       # neighbour lookups cross collisions
    out = {}
    for conn in conns:
        nbrs = cs.neighbour_lists(vox["keys"], conn)
        for th in thresholds:
            out[(conn, th)] = _assert_clean(gf, vox, conn, th, name, nbrs)
    gf.close()
    return out


@pytest.mark.parametrize("name", cs.CONSTRUCTED)
def test_constructed_clouds(name):
    out = _run_constructed(name)
    if name == "snake":
        for conn in (6, 18, 26):
            info, got = out[(conn, (0, 1, 1))]
            print("snake: connectivity", conn, "rounds", info["rounds"])
            assert info["components"] == 1 and got[6].tolist() == [cs.SNAKE_CELLS] and (got[3] == 0).all()
            # plain neighbour-to-neighbour propagation needs L - 1 rounds on this cloud; anything that shortcuts is
            # orders of magnitude below L / 16
            assert info["rounds"] <= cs.SNAKE_CELLS // 16
    if name == "contacts":
        assert [out[(c, (0, 1, 1))][0]["components"] for c in (26, 18, 6)] == [3, 4, 5]
    if name == "dumbbell":
        assert out[(26, (0, 1, 1))][0]["components"] == 1 and out[(26, (3, 1, 1))][0]["components"] == 2
    if name == "edge":
        assert all(out[(c, (0, 1, 1))][0]["components"] == 7 for c in (6, 18, 26))


@pytest.mark.parametrize("name", ["snake", "blobs"])
def test_forced_table_and_segments(name, monkeypatch):
    """The same results through a table of the smallest power of two above the point count (long probe runs, runs
    that cross the table's end) and through compaction segments of 256 voxels."""
    some = dict(conns=(6, 26), thresholds=[(0, 1, 1), (3, 1, 1), (26, 1, 1), (2, 3, 60)])
    plain = _run_constructed(name, **some)
    forced = _run_constructed(name, force_table=True, **some)
    segmented = _run_constructed(name, monkeypatch, segment="256", **some)
    for key, (info, got) in plain.items():
        for other in (forced[key], segmented[key]):
            assert {k: v for k, v in other[0].items() if k != "rounds"} == {k: v for k, v in info.items() if k != "rounds"}
            for a, b in zip(other[1], got):
                assert_bitwise_equal(a, b, f"{name} {key}")


def test_set_scene():
    cloud = vs.oracle_cloud("rig_50x30").copy()
    n = cloud.shape[0]
    gf = _bare_fusion()
    with pytest.raises(capi.AcmmpError):
        gf.voxelize(0.5)                                          # no scene result yet
    assert gf.set_scene(cloud) == n
    pts, ref, pix, mask = gf.scene_points(0, n, provenance=True)
    assert_bitwise_equal(pts, cloud, "uploaded points")
    assert (ref == -1).all() and (pix == -1).all() and (mask == 0).all()
    _voxelize(gf, cloud, vs.RIG_SIZES["middle"], None, "uploaded rig cloud")
    # provenance that is given comes back; a NaN point is taken as it is and rejected by voxelize as before
    cloud[7, 1] = np.nan
    prov = (np.arange(n, dtype=np.int32) % 5, np.arange(n, dtype=np.int32)[::-1].copy(), np.arange(n, dtype=np.uint32) * 3)
    gf.set_scene(cloud, *prov)
    with pytest.raises(capi.AcmmpError):
        gf.voxel_points(0, 1)                                     # the voxel result went with the old scene
    got = gf.scene_points(0, n, provenance=True)
    assert_bitwise_equal(got[0], cloud, "uploaded points with a NaN")
    for a, b in zip(got[1:], prov):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    want = _voxelize(gf, cloud, vs.RIG_SIZES["middle"], None, "uploaded cloud with a NaN")
    assert want["n_rejected"] == 1
    # refused: the object stays as it was
    with pytest.raises(ValueError):
        gf.set_scene(cloud, ref_index=np.zeros(3, np.int32))
    assert gf.L.acmmp_fusion_set_scene(gf.h, -1, None, None, None, None) != 0
    assert gf.L.acmmp_fusion_set_scene(gf.h, 5, None, None, None, None) != 0
    assert_bitwise_equal(gf.scene_points(0, n), cloud, "scene result after refusals")
    assert gf.voxel_points(0, want["points"].shape[0]).shape[0] == want["points"].shape[0]
    # an empty scene
    assert gf.set_scene(np.zeros((0, 9), np.float32)) == 0
    assert gf.scene_points(0, 0).shape == (0, 9)
    with pytest.raises(capi.AcmmpError):
        gf.scene_points(0, 1)
    assert gf.voxelize(0.5)[0] == 0
    assert gf.voxel_clean()[0] == 0
    gf.close()


def _fused(name, unique=False):
    cams, depths, normals, colours, refs, lists = vs.SCENES[name]()
    gf = fill(capi.Fusion(0, cams), cams, depths, normals, colours)
    total, _ = gf.run_scene(refs, lists, unique=unique)
    return gf, total, gf.scene_points(0, total), (refs, lists)


FUSED = [("rig_50x30", False), ("rig_256x128", False), ("rig_256x128", True), ("sphere_64x32", False)]


@pytest.mark.parametrize("name,unique", FUSED, ids=[f"{n}{'_unique' if u else ''}" for n, u in FUSED])
def test_fused_scenes(name, unique):
    gf, total, cloud, _ = _fused(name, unique)
    for size, conn, *th in cs.scene_cases(name, cloud):
        vox = _voxelize(gf, cloud, size, None, name)
        info, _ = _assert_clean(gf, vox, conn, tuple(th), f"{name} size {size}")
        assert 1 <= info["components_kept"] < info["components"]          # (validated on the CPU for the plain rigs)
    gf.close()


def _state(gf, total, nv, n_kept, n_comp):
    return (*gf.scene_points(0, total, provenance=True), *gf.voxel_points(0, nv, counts=True), *_read_clean(gf, n_kept, nv, n_comp))


def test_lifetimes_and_errors():
    gf, total, cloud, (refs, lists) = _fused("rig_50x30")
    size = vs.RIG_SIZES["middle"]
    with pytest.raises(capi.AcmmpError):
        gf.voxel_clean()                                          # no voxel result yet
    for read in (gf.clean_points, gf.voxel_labels, gf.component_table):
        with pytest.raises(capi.AcmmpError):
            read(0, 1)
        read(0, 0)
    vox = _voxelize(gf, cloud, size, None, "lifetimes")
    nv = len(vox["counts"])
    with pytest.raises(capi.AcmmpError):
        gf.voxel_labels(0, 1)                                     # voxelize alone labels nothing
    args = (6, 1, 4, 1)
    info, first = _assert_clean(gf, vox, args[0], args[1:], "lifetimes")
    n, nc = first[0].shape[0], info["components"]
    assert 3 < n < nv and nc > 3
    before = _state(gf, total, nv, n, nc)
    # bad arguments: refused, and the clean, voxel and scene results are bitwise what they were
    for bad in ((8, 0, 1, 1), (0, 0, 1, 1), (26, -1, 1, 1), (26, 0, 0, 1), (26, 0, 1, 0), (6, 1, -4, 1)):
        with pytest.raises(capi.AcmmpError):
            gf.voxel_clean(*bad)
        for a, b in zip(_state(gf, total, nv, n, nc), before):
            assert_bitwise_equal(a, b, f"after refusing {bad}")
    # a second identical clean repeats bitwise
    n2, info2 = gf.voxel_clean(*args)
    assert n2 == n and {k: v for k, v in info2.items() if k != "rounds"} == {k: v for k, v in info.items() if k != "rounds"}
    for a, b in zip(_state(gf, total, nv, n, nc), before):
        assert_bitwise_equal(a, b, "second clean")
    # the range rules of voxel_points: three ranges concatenate to the whole, out-of-range requests fail
    for read, count, whole in ((lambda a, k: gf.clean_points(a, k, counts=True, component=True), n, first[0:3]),
                               (gf.voxel_labels, nv, first[3:5]), (gf.component_table, nc, first[5:8])):
        step = count // 3 + 1
        parts = [read(a, min(step, count - a)) for a in range(0, count, step)]
        assert len(parts) == 3
        for k, w in enumerate(whole):
            assert_bitwise_equal(np.concatenate([p[k] for p in parts], 0), w, "ranges")
        for a, k in ((1, count), (count + 1, 0), (-1, 1), (0, -1)):
            with pytest.raises(capi.AcmmpError):
                read(a, k)
        assert read(count, 0)[0].shape[0] == 0
    assert_bitwise_equal(gf.clean_points(1, 2), first[0][1:3], "points alone")
    # voxelize, run_scene and set_scene each discard the clean result
    for discard in (lambda: gf.voxelize(size), lambda: gf.run_scene(refs, lists), lambda: gf.set_scene(cloud)):
        discard()
        for read in (gf.clean_points, gf.voxel_labels, gf.component_table):
            with pytest.raises(capi.AcmmpError):
                read(0, 1)
        gf.voxelize(size)
        assert gf.voxel_clean(*args)[0] == n
    # a clean result survives a refused voxelize, and the table it needs does too
    with pytest.raises(capi.AcmmpError):
        gf.voxelize(-1.0)
    gf.voxel_table(32)
    with pytest.raises(capi.AcmmpError):
        gf.voxelize(size)
    gf.voxel_table(0)
    _assert_clean(gf, vox, 26, (2, 10, 30), "after refused voxelize")
    # an empty voxel result: min_points above every cell's count
    assert gf.voxelize(size, min_points=10 ** 6)[0] == 0
    n0, info0 = gf.voxel_clean(26, 1, 2, 3)
    assert (n0, info0["components"], info0["components_kept"], info0["unsupported"], info0["rounds"]) == (0, 0, 0, 0, 0)
    assert gf.clean_points(0, 0).shape == (0, 9) and gf.component_table(0, 0)[0].shape == (0,)
    with pytest.raises(capi.AcmmpError):
        gf.clean_points(0, 1)
    gf.close()


def test_pipeline_clean_fusion(tmp_path):
    ds = small_dataset(64, 32, 3)
    pipe = pipeline.Pipeline(ds, order="reference", geom_iterations=1).run()
    plain = pipe.run_fusion(ply_path=str(tmp_path / "plain.ply"))
    ok = vs.finite_points(plain)
    size = float((plain[ok, :3].max(0) - plain[ok, :3].min(0)).max()) / 16
    # the four parameters at their defaults: today's voxel path, its bytes and its fusion_info
    voxel = pipe.run_fusion(ply_path=str(tmp_path / "voxel.ply"), voxel_size=size)
    voxel_info = dict(pipe.fusion_info)
    same = pipe.run_fusion(ply_path=str(tmp_path / "same.ply"), voxel_size=size, voxel_connectivity=26, voxel_min_neighbours=0,
                           voxel_min_component_voxels=1, voxel_min_component_points=1)
    assert pipe.fusion_info == voxel_info and set(voxel_info) == {"scene_points", "voxels", "rejected", "occupied", "origin",
                                                                  "voxel_size", "min_points"}
    assert_bitwise_equal(same, voxel, "defaults")
    assert (tmp_path / "same.ply").read_bytes() == (tmp_path / "voxel.ply").read_bytes()
    want_voxel = pipe.run_fusion(fusion_factory=vs.RestatedVoxelFusion, ply_path=str(tmp_path / "voxel_restated.ply"), voxel_size=size)
    assert_bitwise_equal(voxel, want_voxel, "voxel path")
    with pytest.raises(ValueError):
        pipe.run_fusion(voxel_min_neighbours=1)                   # cleaning needs voxel_size
    for unique, kw in ((False, dict(voxel_min_neighbours=1, voxel_min_component_voxels=3)),
                       (True, dict(voxel_connectivity=6, voxel_min_component_points=4))):
        got = pipe.run_fusion(ply_path=str(tmp_path / "gpu.ply"), unique=unique, chunk_points=5, voxel_size=size, **kw)
        info = dict(pipe.fusion_info)
        want = pipe.run_fusion(fusion_factory=cs.RestatedCleanFusion, ply_path=str(tmp_path / "restated.ply"), unique=unique,
                               voxel_size=size, **kw)
        print("unique", unique, kw, info)
        assert 0 < got.shape[0] == info["clean_voxels"] < info["voxels"] and info["components_kept"] < info["components"]
        assert_bitwise_equal(got, want, "Pipeline.run_fusion clean cloud")
        assert info.pop("rounds") >= 1 and pipe.fusion_info.pop("rounds") == 0
        assert info == pipe.fusion_info
        assert (tmp_path / "gpu.ply").read_bytes() == (tmp_path / "restated.ply").read_bytes()
