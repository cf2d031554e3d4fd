"""Surface mesh of the voxel cloud on the GPU (acmmp_fusion_voxel_mesh, include/acmmp.h), bit for bit against the
sequential restatement (voxel_mesh_support) run on the very voxel, clean and visible results the device holds."""
import numpy as np
import pytest

import visibility_support as vis
import voxel_clean_support as cs
import voxel_mesh_support as ms
from acmmp import capi
from conftest import assert_bitwise_equal
from fusion_scene_support import fill

pytestmark = pytest.mark.gpu

CLEAN = (26, 1, 2, 1)
VISIBILITY = (0.05, 1, 1, 4096)         # rel_tol, radius, min_support, max_conflicts of the "visible" source cases
NAMES = ("vertices", "faces", "cells", "tsdf", "entry")


def _pair(rig, cloud=None, size=None, origin=None, n_set=None):
    """The device object and the restated one over the rig's views, holding the same scene cloud and voxel result
    (checked bit for bit).  Returns (gf, rf, views, trunc, small trunc)."""
    cams, depths, normals, colours, built, built_size, trunc, small = ms.base_case(rig)
    cloud = built if cloud is None else cloud
    size = built_size if size is None else size
    k = len(cams) if n_set is None else n_set
    gf = fill(capi.Fusion(0, cams), cams[:k], depths, normals, colours)
    rf = fill(ms.RestatedMeshFusion(cams), cams[:k], depths, normals, colours)
    assert gf.set_scene(cloud) == rf.set_scene(cloud)
    _voxelize(gf, rf, size, origin)
    return gf, rf, list(range(k)), trunc, small


def _voxelize(gf, rf, size, origin=None, min_points=1):
    n, want = gf.voxelize(size, origin, min_points)[0], rf.voxelize(size, origin, min_points)[0]
    assert n == want
    pts, cnt = gf.voxel_points(0, n, counts=True)
    assert_bitwise_equal(pts, rf.voxels["points"], "voxel points")
    assert np.array_equal(cnt, rf.voxels["counts"])
    return n


def _source(gf, rf, views, source):
    """Brings both sides to hold `source`, checked bit for bit: "clean" cleans, "visible" cleans and checks the clean
    result's visibility, so that the visible entries' voxels are two compactions away."""
    if source == "voxel":
        return
    n, want = gf.voxel_clean(*CLEAN)[0], rf.voxel_clean(*CLEAN)[0]
    assert 0 < n == want < rf.voxels["points"].shape[0]
    assert_bitwise_equal(gf.clean_points(0, n), rf.clean_points(0, n), "clean points")
    if source == "visible":
        tol, radius, sup, con = VISIBILITY
        k, want = gf.voxel_visibility(views, tol, radius, sup, con, source="clean")[0], \
            rf.voxel_visibility(views, tol, radius, sup, con, source="clean")[0]
        assert 0 < k == want < n
        assert_bitwise_equal(gf.visible_points(0, k), rf.visible_points(0, k), "visible points")


def _read(fu, nv, nf, ns):
    return (fu.mesh_vertices(0, nv), fu.mesh_faces(0, nf), *fu.mesh_samples(0, ns))


def _assert_mesh(gf, rf, views, trunc, min_weight, source, what):
    """One voxel_mesh, every output against the restatement.  Returns (nv, nf, info, the five arrays read)."""
    nv, nf, info = gf.voxel_mesh(views, trunc, min_weight, source=source)
    wv, wf, winfo = rf.voxel_mesh(views, trunc, min_weight, source=source)
    print(what, source, "views", len(views), "trunc", trunc, "min_weight", min_weight, "->", nv, nf, info)
    assert (nv, nf, info) == (wv, wf, winfo), what
    got, want = _read(gf, nv, nf, info["samples"]), _read(rf, nv, nf, info["samples"])
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name}"
        assert_bitwise_equal(g, w, f"{what}: {name}")
    return nv, nf, info, got


@pytest.mark.parametrize("source", ["voxel", "clean", "visible"])
@pytest.mark.parametrize("rig", list(vis.RIGS))
def test_base(rig, source):
    gf, rf, views, trunc, small = _pair(rig)
    _source(gf, rf, views, source)
    seen = set()
    for min_weight in (1, 2):
        for t in (trunc, small):
            nv, nf, info, _ = _assert_mesh(gf, rf, views, t, min_weight, source, rig)
            seen.add((nv, nf))
            assert nv > 0 and (nf > 0 or t == small) and (info["valid"] < info["samples"] or min_weight == 1)
    assert len(seen) == 4                                              # min_weight and trunc each change the mesh
    gf.close()


def test_view_lists():
    """Both sides of the tally kernel's chunk boundary, more positions than a wave is wide, the longest list; a list
    repeated m times gives m times the sums."""
    gf, rf, views, trunc, _ = _pair("sphere")
    single = [_assert_mesh(gf, rf, [k], trunc, 1, "voxel", f"view {k}")[3][3].astype(np.int64) for k in range(4)]
    once = _assert_mesh(gf, rf, views, trunc, 1, "voxel", "once")[3][3].astype(np.int64)
    assert np.array_equal(once, sum(single))
    for n_list in (capi_chunk(), capi_chunk() + 1, 70, 4096):
        got = _assert_mesh(gf, rf, [k % 4 for k in range(n_list)], trunc, n_list // 2, "voxel", f"{n_list} positions")[3][3]
        full, rest = divmod(n_list, 4)
        assert np.array_equal(got, full * once + sum(single[:rest], np.zeros_like(once)))
    gf.close()


def capi_chunk():
    return 32                       # kVisChunk of csrc/fusion.h


@pytest.mark.parametrize("source", ["voxel", "visible"])
def test_segments(source, monkeypatch):
    """Compaction segments of 256 lanes over entry, sample and pair counts that are no multiple of 256."""
    def run():
        gf, rf, views, trunc, small = _pair("pinhole")
        _source(gf, rf, views, source)
        out = [_assert_mesh(gf, rf, views, t, w, source, "segments") for t, w in ((trunc, 1), (small, 2), (trunc, 99))]
        gf.close()
        return out
    plain = run()
    monkeypatch.setenv("ACMMP_VOXEL_SEGMENT_POINTS", "256")
    for (nv, nf, info, got), (wv, wf, winfo, want) in zip(run(), plain):
        assert (nv, nf, info) == (wv, wf, winfo)
        for a, b in zip(got, want):
            assert_bitwise_equal(a, b, "segmented")
    nv, nf, info, got = plain[0]
    assert all(k % 256 != 0 and k > 512 for k in (nv, nf // 2, info["samples"]))
    # min_weight above the list length: an empty mesh through the same path
    assert plain[2][:2] == (0, 0) and plain[2][2]["valid"] == 0 and plain[2][2]["samples"] == info["samples"]


def test_one_chunk_segments_across_stages(monkeypatch):
    """The compaction primitive every stage shares, at one 256-item chunk per segment: the carry of the output position
    from segment to segment is taken at every boundary of the voxel, root, clean, visible, sample, vertex and face
    passes.  The device against itself at the default segment size, array for array."""
    def run():
        cams, depths, normals, colours, cloud, size, trunc, _ = ms.base_case("pinhole")
        views = list(range(len(cams)))
        gf = fill(capi.Fusion(0, cams), cams, depths, normals, colours)
        gf.set_scene(cloud)
        n = gf.voxelize(size, None, 1)[0]
        kept, info = gf.voxel_clean(*CLEAN)
        tol, radius, sup, con = VISIBILITY
        seen = gf.voxel_visibility(views, tol, radius, sup, con, source="clean")[0]
        nv, nf, mesh = gf.voxel_mesh(views, trunc, 1, source="visible")
        out = [*gf.voxel_points(0, n, counts=True), *gf.component_table(0, info["components"]),
               *gf.clean_points(0, kept, counts=True, component=True), *gf.visible_points(0, seen, counts=True, tallies=True),
               *_read(gf, nv, nf, mesh["samples"])]
        gf.close()
        return (n, kept, info, seen, nv, nf, mesh), out
    plain, want = run()
    monkeypatch.setenv("ACMMP_VOXEL_SEGMENT_POINTS", "256")
    split, got = run()
    assert split == plain
    n, kept, info, seen, nv, nf, mesh = plain
    assert min(n, kept, seen, mesh["samples"], nv, nf // 2) > 256                      # more than one segment each
    assert len(got) == len(want) == 16
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), k


def test_collisions_and_a_full_table():
    """The visible source of the sphere rig: at the smallest table above its samples the restatement counts cells
    stored below their home slot (test_voxel_mesh_restatement.py asserts > 0)."""
    gf, rf, views, trunc, _ = _pair("sphere")
    _source(gf, rf, views, "visible")
    nv, nf, info, auto = _assert_mesh(gf, rf, views, trunc, 1, "visible", "automatic table")
    ns, ne = info["samples"], len(rf.visible["kept"])
    table = gf.mesh_table()
    assert table["slots"] == ms.auto_slots(ne) and table["occupied"] == ns
    assert table["wrapped"] == ms.table_wrapped(rf.meshed["cells"], table["slots"])
    small = 1 << ns.bit_length()                                        # the smallest power of two above the samples
    gf.mesh_table(small)
    _, _, _, forced = _assert_mesh(gf, rf, views, trunc, 1, "visible", "forced table")
    table = gf.mesh_table(small // 2)                                   # ... and the next one cannot hold them
    want = ms.table_wrapped(rf.meshed["cells"], small)
    print("forced table", table, "restated wrapped", want)
    assert table["slots"] == small and table["occupied"] == ns and table["wrapped"] == want > 0 and table["max_probe"] > 1
    for a, b in zip(forced, auto):
        assert_bitwise_equal(a, b, "forced table")
    with pytest.raises(capi.AcmmpError):
        gf.voxel_mesh(views, trunc, source="visible")
    for a, b in zip(_read(gf, nv, nf, ns), auto):
        assert_bitwise_equal(a, b, "after the full table")
    assert gf.mesh_table(48)["slots"] == small                         # the failed call left the last successful one's
    with pytest.raises(capi.AcmmpError):
        gf.voxel_mesh(views, trunc, source="visible")                   # not a power of two >= 64
    gf.mesh_table(0)
    _assert_mesh(gf, rf, views, trunc, 2, "visible", "automatic again")
    gf.close()


def test_grid_boundary():
    """Entries in cell 0 and cell 2^21 - 1 of every axis, the origin given: no wrapped neighbours."""
    gf, rf, views, _, _ = _pair("sphere", cloud=cs.constructed("edge"), size=1.0, origin=cs.ORIGIN)
    _, _, info, got = _assert_mesh(gf, rf, views, 4.0, 1, "voxel", "edge")
    cells = got[2]
    assert cells.min() == 0 and cells.max() == cs.LAST
    corner = lambda c: int((np.abs(cells.astype(np.int64) - np.array(c)).max(1) <= 1).sum())
    assert corner((0, 0, 0)) == 8 and corner((cs.LAST,) * 3) == 8
    gf.close()


def test_small_and_empty_cases():
    cams, depths, normals, colours, cloud, size, trunc, _ = ms.base_case("sphere")
    away = cloud[0, :3] - np.float32(10 * size)                        # the voxel's cell is (10, 10, 10): 27 samples
    gf, rf, views, _, _ = _pair("sphere", cloud=cloud[:1], origin=away)
    _, _, info, _ = _assert_mesh(gf, rf, views, trunc, 1, "voxel", "single voxel")
    assert info["samples"] == 27
    _assert_mesh(gf, rf, views, trunc, len(views) + 1, "voxel", "min_weight above the list")
    for fu in (gf, rf):
        fu.set_scene(cloud)
    _voxelize(gf, rf, size, min_points=10 ** 6)                         # an empty source: an empty mesh
    empty = {"samples": 0, "valid": 0, "cubes": 0, "uncoloured": 0}
    assert gf.voxel_mesh(views, trunc) == rf.voxel_mesh(views, trunc) == (0, 0, empty)
    assert gf.mesh_vertices(0, 0).shape == (0, 9) and gf.mesh_faces(0, 0).shape == (0, 3)
    with pytest.raises(capi.AcmmpError):
        gf.mesh_vertices(0, 1)
    gf.close()


def _gone(gf):
    for read in (gf.mesh_vertices, gf.mesh_faces, gf.mesh_samples):
        with pytest.raises(capi.AcmmpError):
            read(0, 1)
        read(0, 0)


def test_errors_and_lifetimes():
    cams, depths, normals, colours, cloud, size, trunc, _ = ms.base_case("sphere")
    gf, rf, views, _, _ = _pair("sphere", n_set=3)                      # view 3 is never set
    _gone(gf)
    for source in ("clean", "visible"):
        with pytest.raises(capi.AcmmpError):
            gf.voxel_mesh(views, trunc, source=source)                  # no such result yet
    nv, nf, info, first = _assert_mesh(gf, rf, views, trunc, 1, "voxel", "lifetimes")
    ns = info["samples"]
    state = lambda: _read(gf, nv, nf, ns)
    # every bad argument: refused, and the mesh result is bitwise what it was
    ok = dict(views=views, trunc=trunc, min_weight=1)
    for bad in (dict(views=[]), dict(views=[0] * 4097), dict(views=[0, 4]), dict(views=[-1, 0]), dict(views=[0, 3]),
                dict(trunc=float("nan")), dict(trunc=float("inf")), dict(trunc=0.0), dict(trunc=-1.0), dict(min_weight=0),
                dict(min_weight=-3)):
        with pytest.raises(capi.AcmmpError):
            gf.voxel_mesh(**{**ok, **bad})
        with pytest.raises(ValueError):
            rf.voxel_mesh(**{**ok, **bad})
    v = np.array(views, np.int32)
    for source in (3, -1):
        assert gf.L.acmmp_fusion_voxel_mesh(gf.h, source, 3, v.ctypes.data, trunc, 1, *[None] * 6) == 1
    assert gf.L.acmmp_fusion_voxel_mesh(gf.h, 0, 3, None, trunc, 1, *[None] * 6) == 1
    with pytest.raises(ValueError):
        gf.voxel_mesh(views, trunc, source="scene")
    for read, total in ((gf.mesh_vertices, nv), (gf.mesh_faces, nf), (gf.mesh_samples, ns)):
        for a, k in ((1, total), (total + 1, 0), (-1, 1), (0, -1)):
            with pytest.raises(capi.AcmmpError):
                read(a, k)
    for a, b in zip(state(), first):
        assert_bitwise_equal(a, b, "after the refusals")
    # every output pointer may be NULL; ranges concatenate
    assert gf.L.acmmp_fusion_voxel_mesh(gf.h, 0, 3, v.ctypes.data, trunc, 1, *[None] * 6) == 0
    step = nv // 3 + 1
    assert_bitwise_equal(np.concatenate([gf.mesh_vertices(a, min(step, nv - a)) for a in range(0, nv, step)], 0), first[0], "ranges")
    assert_bitwise_equal(gf.mesh_faces(1, 2), first[1][1:3], "faces alone")
    # a mesh of the voxel result survives set_view, a clean and a visibility call
    gf.set_view(1, depths[1], normals[1], colours[1])
    _source(gf, rf, views, "visible")
    for a, b in zip(state(), first):
        assert_bitwise_equal(a, b, "after set_view, voxel_clean and voxel_visibility")
    # a mesh of the visible result goes with the next visibility call, and with a clean when that was its source's source
    tol, radius, sup, con = VISIBILITY
    _assert_mesh(gf, rf, views, trunc, 1, "visible", "lifetimes")
    gf.voxel_visibility(views, tol, radius, sup, con, source="voxel"), rf.voxel_visibility(views, tol, radius, sup, con, source="voxel")
    _gone(gf)
    _assert_mesh(gf, rf, views, trunc, 1, "visible", "visible of the voxel result")
    gf.voxel_clean(*CLEAN), rf.voxel_clean(*CLEAN)                      # leaves a visible result of the voxel result alone
    assert gf.mesh_vertices(0, 1).shape == (1, 9)
    gf.voxel_visibility(views, tol, radius, sup, con, source="clean"), rf.voxel_visibility(views, tol, radius, sup, con, source="clean")
    _assert_mesh(gf, rf, views, trunc, 1, "visible", "visible of the clean result")
    gf.voxel_clean(*CLEAN), rf.voxel_clean(*CLEAN)
    _gone(gf)
    # a mesh of the clean result goes with the next clean; a visibility call leaves it alone
    _assert_mesh(gf, rf, views, trunc, 1, "clean", "lifetimes")
    gf.voxel_visibility(views, tol, radius, sup, con, source="clean")
    assert gf.mesh_vertices(0, 1).shape == (1, 9)
    gf.voxel_clean(*CLEAN)
    _gone(gf)
    # voxelize, set_scene and run_scene each discard it, whatever its source
    for discard in (lambda: gf.voxelize(size), lambda: gf.set_scene(cloud), lambda: gf.run_scene([0], [[1, 2]])):
        gf.set_scene(cloud)
        gf.voxelize(size)
        assert gf.voxel_mesh(views, trunc)[:2] == (nv, nf)
        discard()
        _gone(gf)
    gf.close()


def test_repeatable():
    out = []
    for _ in range(2):
        gf, rf, views, trunc, _ = _pair("sphere")
        nv, nf, info = gf.voxel_mesh(views, trunc)
        again = gf.voxel_mesh(views, trunc)
        assert again == (nv, nf, info)
        out.append(_read(gf, nv, nf, info["samples"]))
        gf.close()
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()
