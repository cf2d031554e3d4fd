"""Whole-scene fusion on the GPU (acmmp_fusion_run_scene, include/acmmp.h), bit for bit: plain mode against
per-view acmmp_fusion_run and the oracle, the provenance of every point, and the duplicate-free mode against
the oracle on depth maps zeroed at the used pixels and the test-side restatement of the marking."""
import numpy as np
import pytest

import oracle
from acmmp import capi, pipeline
from conftest import assert_bitwise_equal
from fusion_scene_support import (RestatedFusion, all_others, assert_samples_used_once, dataset_inputs, fill,
                                  point_samples, rig_inputs, view_provenance, zeroed)
from pipeline_support import OracleFusion

pytestmark = pytest.mark.gpu


def _edge_case_rig():
    """The ground-truth rig at 50x30 (1500 pixels: the last 256-pixel chunk is ragged), 5 views, of which
    view 2 has an all-zero depth map and view 3 a depth map of half the size."""
    cams, depths, normals, bgr = rig_inputs(50, 30, 5)
    cams, depths, normals, bgr = cams.copy(), list(depths), list(normals), list(bgr)
    depths[2] = np.zeros_like(depths[2])
    depths[3] = np.ascontiguousarray(depths[3][::2, ::2])
    normals[3] = np.ascontiguousarray(normals[3][::2, ::2])
    bgr[3], cams[3] = pipeline.rescale_image_and_camera(bgr[3], depths[3].shape, cams[3])
    return cams, depths, normals, bgr


PLAIN_SCENES = {
    # 768x384 = 1152 chunks: the scan walks more than one tile of 1024
    "rig_768x384": lambda: (*rig_inputs(768, 384, 4), [0, 1, 2, 3], all_others(4)),
    # a reordered subset with the all-zero view in the middle, -1 sources, the half-size view as source and reference
    "rig_50x30_edges": lambda: (*_edge_case_rig(), [4, 2, 0, 3], [[0, 1, -1, 3], [0, 1], [1, 2, 3, 4], [0, -1, 4, 1]]),
    "pinhole_64x32": lambda: (*dataset_inputs("pinhole"), [1, 0, 2], [[0, 2, -1], [-1, 1, 2], [0, 1]]),
}


@pytest.mark.parametrize("name", list(PLAIN_SCENES))
def test_plain_scene_equals_per_view_runs_and_oracle(name):
    cams, depths, normals, colours, refs, lists = PLAIN_SCENES[name]()
    gf = fill(capi.Fusion(0, cams), cams, depths, normals, colours)
    of = fill(OracleFusion(cams), cams, depths, normals, colours)
    total, counts = gf.run_scene(refs, lists)
    pts, ref_idx, pix, mask = gf.scene_points(0, total, provenance=True)
    per_view = [gf.run(r, s) for r, s in zip(refs, lists)]
    want = [of.run(r, s) for r, s in zip(refs, lists)]
    print(name, "counts", counts.tolist(), "oracle", [w.shape[0] for w in want])
    assert counts.tolist() == [w.shape[0] for w in want] and total == int(counts.sum()) > 0
    assert_bitwise_equal(pts, np.concatenate(per_view, 0), f"{name}: scene vs per-view runs")
    assert_bitwise_equal(pts, np.concatenate(want, 0), f"{name}: scene vs oracle")
    assert np.array_equal(ref_idx, np.repeat(np.arange(len(refs)), counts))
    if name == "rig_768x384":
        assert (counts > 0.7 * 768 * 384).all()
    if name == "rig_50x30_edges":
        assert counts[1] == 0 and counts[0] > 0 and counts[2] > 0
    # streamed in ranges, and a result that survives the per-view runs made above
    step = max(1, total // 3 + 1)
    parts = [gf.scene_points(a, min(step, total - a)) for a in range(0, total, step)]
    assert_bitwise_equal(np.concatenate(parts, 0), pts, f"{name}: ranges")
    assert all(not gf.used(v).any() for v in range(len(cams)))            # plain mode marks nothing
    gf.close()


@pytest.mark.parametrize("model", ["sphere", "pinhole"])
def test_plain_scene_provenance(model):
    cams, depths, normals, colours = dataset_inputs(model)
    refs, lists = [0, 1, 2], [[1, 2, -1], [-1, 0, 2], [0, 1]]
    gf = fill(capi.Fusion(0, cams), cams, depths, normals, colours)
    total, counts = gf.run_scene(refs, lists)
    pts, ref_idx, pix, mask = gf.scene_points(0, total, provenance=True)
    gf.close()
    assert total == int(counts.sum()) > 0
    for k, (ref, srcs) in enumerate(zip(refs, lists)):
        sel = ref_idx == k
        assert int(sel.sum()) == counts[k]
        assert (np.diff(pix[sel]) > 0).all()
        _, xyz = point_samples(cams, depths, ref, srcs, pix[sel], mask[sel], want_xyz=True)
        assert_bitwise_equal(pts[sel][:, :3], xyz, f"{model} view {ref}: xyz from (pixel, src_mask)")
        want_pix, want_mask = view_provenance(cams, depths, normals, ref, srcs)
        assert np.array_equal(pix[sel], want_pix) and np.array_equal(mask[sel], want_mask)


UNIQUE_SCENES = {
    "sphere_64x32": lambda: dataset_inputs("sphere"),
    "pinhole_64x32": lambda: dataset_inputs("pinhole"),
    "rig_256x128": lambda: rig_inputs(256, 128, 4),
}


@pytest.mark.parametrize("name", list(UNIQUE_SCENES))
def test_unique_scene(name):
    cams, depths, normals, colours = UNIQUE_SCENES[name]()
    n = len(cams)
    refs, lists = list(range(n)), all_others(n)
    gf = fill(capi.Fusion(0, cams), cams, depths, normals, colours)
    of = fill(OracleFusion(cams), cams, depths, normals, colours)
    rf = fill(RestatedFusion(cams), cams, depths, normals, colours)
    assert all(not gf.used(v).any() for v in range(n))
    plain_total, _ = gf.run_scene(refs, lists)

    # one view per call: the points are the oracle's on depths zeroed by the masks downloaded before the view,
    # the masks after it are the restatement's
    seq = []
    for k in refs:
        before = [gf.used(v) for v in range(n)]
        total, counts = gf.run_scene([k], [lists[k]], unique=True)
        got = gf.scene_points(0, total, provenance=True)
        want = oracle.fuse(cams, zeroed(depths, before), of.normals, of.rgba, k, lists[k])
        print(name, "view", k, "unique points", total, "oracle", want.shape[0])
        assert counts.tolist() == [total]
        assert_bitwise_equal(got[0], want, f"{name} view {k}: points on zeroed depths")
        rf.marks = [b.copy() for b in before]
        rf.run_scene([k], [lists[k]], unique=True)
        for v in range(n):
            assert np.array_equal(gf.used(v), rf.marks[v]), f"{name}: used mask of view {v} after view {k}"
        seq.append(got)
    marks = [gf.used(v) for v in range(n)]
    seq_pts = np.concatenate([g[0] for g in seq], 0)
    seq_pix = np.concatenate([g[2] for g in seq], 0)
    seq_mask = np.concatenate([g[3] for g in seq], 0)
    seq_ref = np.concatenate([np.full(len(g[2]), k, np.int32) for k, g in enumerate(seq)], 0)

    # without a reset a second run emits nothing from used pixels
    total2, _ = gf.run_scene(refs, lists, unique=True)
    _, ref2, pix2, _ = gf.scene_points(0, total2, provenance=True)
    for k in refs:
        assert not marks[k].reshape(-1)[pix2[ref2 == k]].any()

    # all views in one call after a reset: the same concatenated result and the same masks
    gf.reset_used()
    assert all(not gf.used(v).any() for v in range(n))
    total, counts = gf.run_scene(refs, lists, unique=True)
    pts, ref_idx, pix, mask = gf.scene_points(0, total, provenance=True)
    print(name, "unique", total, "plain", plain_total, "ratio", total / plain_total)
    assert counts.tolist() == [len(g[2]) for g in seq] and total == int(counts.sum())
    assert_bitwise_equal(pts, seq_pts, f"{name}: one call vs one view per call")
    assert np.array_equal(pix, seq_pix) and np.array_equal(mask, seq_mask) and np.array_equal(ref_idx, seq_ref)
    for v in range(n):
        assert np.array_equal(gf.used(v), marks[v])
    assert 0 < total < plain_total
    n_samples = assert_samples_used_once(cams, depths, refs, lists, ref_idx, pix, mask)
    assert n_samples == sum(int(m.sum()) for m in marks)

    # a plain run reads and writes no mask
    assert gf.run_scene(refs, lists)[0] == plain_total
    for v in range(n):
        assert np.array_equal(gf.used(v), marks[v])
    gf.close()


def test_scene_errors_leave_the_object_unchanged():
    cams, depths, normals, colours = dataset_inputs("sphere")
    cams4 = np.concatenate([cams, cams[:1]])                  # a fourth view that is never set
    gf = capi.Fusion(0, cams4)
    for k in range(3):
        gf.set_view(k, depths[k], normals[k], colours[k])
    refs, lists = [0, 1], [[1, 2], [0, 2]]
    total, counts = gf.run_scene(refs, lists, unique=True)
    assert total > 0
    before = gf.scene_points(0, total, provenance=True)
    marks = [gf.used(v) for v in range(4)]
    assert any(m.any() for m in marks) and not marks[3].any()
    bad = [([2, 0], [[0, 1], list(range(3)) * 11]),           # 33 sources
           ([2, 4], [[0, 1], [0, 1]]),                        # reference out of range
           ([2, -1], [[0, 1], [0, 1]]),
           ([2, 0], [[0, 1], [1, 4]]),                        # source out of range
           ([2, 3], [[0, 1], [0, 1]]),                        # reference never set
           ([2, 0], [[0, 1], [1, 3]])]                        # source never set
    for unique in (True, False):
        for r, l in bad:
            with pytest.raises(capi.AcmmpError):
                gf.run_scene(r, l, unique=unique)
            after = gf.scene_points(0, total, provenance=True)
            for a, b in zip(after, before):
                assert_bitwise_equal(a, b, f"previous result after refusing {r} {l}")
            for v in range(4):
                assert np.array_equal(gf.used(v), marks[v])
    with pytest.raises(capi.AcmmpError):
        gf.scene_points(1, total)                             # beyond the result
    with pytest.raises(capi.AcmmpError):
        gf.scene_points(-1, 1)
    assert gf.scene_points(total, 0).shape == (0, 9)
    # set_view clears that view's mask only
    gf.set_view(1, depths[1], normals[1], colours[1])
    assert not gf.used(1).any() and np.array_equal(gf.used(0), marks[0]) and np.array_equal(gf.used(2), marks[2])
    gf.close()


def _same(got, want, what):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert_bitwise_equal(a, b, what)


def _scene(fu, refs, lists, unique=False):
    """(counts, points, reference positions, pixels, source masks) of one run_scene."""
    total, counts = fu.run_scene(refs, lists, unique=unique)
    assert total == int(counts.sum())
    return (counts, *fu.scene_points(0, total, provenance=True))


def _voxels(fu):
    """(points, counts per voxel, [voxels, occupied, rejected], origin) of voxelize(0.25)."""
    nv, info = fu.voxelize(0.25)
    return (*fu.voxel_points(0, nv, counts=True), np.array([nv, info["n_occupied"], info["n_rejected"]], np.int64),
            info["origin"])


def _oracle_scene(cams, depths, normals, colours, refs, lists):
    of = fill(OracleFusion(cams), cams, depths, normals, colours)
    want = [of.run(r, s) for r, s in zip(refs, lists)]
    return np.array([w.shape[0] for w in want], np.int32), np.concatenate(want, 0)


def test_one_object_across_regrowth_and_replacement():
    """One capi.Fusion reused while its buffers are reallocated and replaced: scratch sized for the half-size
    view then grown, a scene result replaced by a larger one (and the voxel result dropped with it), a view's
    buffers replaced by set_view, the used masks filled and reset.  After each step the object gives what a fresh
    object given the same inputs gives, and what the oracle / the restatement give."""
    cams, depths, normals, colours, refs, lists = PLAIN_SCENES["rig_50x30_edges"]()
    gf = fill(capi.Fusion(0, cams), cams, depths, normals, colours)
    first_total, _ = gf.run_scene([3], [[0, 4]])                          # scratch sized for 25x15
    first_vox = _voxels(gf)
    assert first_total > 0 and first_vox[0].shape[0] > 0

    # the whole list: the scratch grows, the scene result is replaced, the voxel result is gone
    got4 = _scene(gf, refs, lists)
    with pytest.raises(capi.AcmmpError):
        gf.voxel_points(0, 1)
    fresh = fill(capi.Fusion(0, cams), cams, depths, normals, colours)
    _same(got4, _scene(fresh, refs, lists), "first full run vs a fresh object")
    fresh.close()
    want_counts, want_pts = _oracle_scene(cams, depths, normals, colours, refs, lists)
    print("counts with view 2 empty", got4[0].tolist(), "after", first_total, "points of view 3 alone")
    assert got4[0].tolist() == want_counts.tolist() and got4[0][1] == 0 and int(got4[0].sum()) > first_total
    assert_bitwise_equal(got4[1], want_pts, "first full run vs oracle")

    # view 2 gets its real depth map
    depths = list(depths)
    depths[2] = rig_inputs(50, 30, 5)[1][2]
    gf.set_view(2, depths[2], normals[2], colours[2])
    fresh = fill(capi.Fusion(0, cams), cams, depths, normals, colours)
    rf = fill(RestatedFusion(cams), cams, depths, normals, colours)

    got_u = _scene(gf, refs, lists, unique=True)
    _same(got_u, _scene(fresh, refs, lists, unique=True), "unique run vs a fresh object")
    rf_total, rf_counts = rf.run_scene(refs, lists, unique=True)
    _same(got_u, (rf_counts, *rf.scene_points(0, rf_total, provenance=True)), "unique run vs the restatement")
    for v in range(len(cams)):
        assert np.array_equal(gf.used(v), rf.marks[v]) and np.array_equal(fresh.used(v), rf.marks[v])

    gf.reset_used()
    fresh.reset_used()
    got6 = _scene(gf, refs, lists)
    _same(got6, _scene(fresh, refs, lists), "second full run vs a fresh object")
    want_counts, want_pts = _oracle_scene(cams, depths, normals, colours, refs, lists)
    print("counts with view 2 set", got6[0].tolist(), "unique", got_u[0].tolist())
    assert got6[0].tolist() == want_counts.tolist() and got6[0][1] > 0 and got6[0].tolist() != got4[0].tolist()
    assert_bitwise_equal(got6[1], want_pts, "second full run vs oracle")

    got_vox = _voxels(gf)
    _same(got_vox, _voxels(fresh), "voxels vs a fresh object")
    assert got_vox[0].shape[0] > 0
    fresh.close()
    gf.close()
