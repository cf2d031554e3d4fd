"""Whole-scene fusion, the parts that need no GPU: the test-side restatement of one view's provenance and
marking (fusion_scene_support) shown equal to the oracle in plain mode, the incremental PLY writer, and
Pipeline.run_fusion's scene path driven by a run_scene-capable stub over that restatement."""
import numpy as np
import pytest

from acmmp import io, pipeline
from conftest import assert_bitwise_equal
from fusion_scene_support import (RestatedFusion, all_others, assert_samples_used_once, dataset_inputs, fill,
                                  point_samples, view_provenance)
from pipeline_support import OracleEngine, OracleFusion, small_dataset


@pytest.mark.parametrize("model", ["sphere", "pinhole"])
def test_restatement_equals_oracle_in_plain_mode(model):
    """Validates the restatement, not the feature: the pixels and source masks it derives give, averaged in
    ascending source order, exactly the points OracleFusion.run emits, in the same order."""
    cams, depths, normals, colours = dataset_inputs(model)
    of = fill(OracleFusion(cams), cams, depths, normals, colours)
    total = 0
    for k, srcs in enumerate(all_others(len(cams))):
        srcs = srcs + [-1]
        want = of.run(k, srcs)
        pixels, masks = view_provenance(cams, depths, normals, k, srcs)
        assert len(pixels) == want.shape[0]
        assert (np.diff(pixels) > 0).all() and (masks != 0).all() and (masks >> np.uint32(len(srcs) - 1) == 0).all()
        samples, xyz = point_samples(cams, depths, k, srcs, pixels, masks, want_xyz=True)
        assert_bitwise_equal(xyz, want[:, :3], f"{model} view {k}")
        assert (samples[:, 0] == pixels).all() and ((samples[:, 1:] >= 0).sum(1) >= 2).all()
        total += len(pixels)
    assert total > 0


def test_restated_scene_plain_is_the_concatenation():
    cams, depths, normals, colours = dataset_inputs("sphere")
    of = fill(OracleFusion(cams), cams, depths, normals, colours)
    rf = fill(RestatedFusion(cams), cams, depths, normals, colours)
    refs, lists = [2, 0], [[0, 1], [1, 2, -1]]
    total, counts = rf.run_scene(refs, lists)
    want = [of.run(r, s) for r, s in zip(refs, lists)]
    assert counts.tolist() == [w.shape[0] for w in want] and total == sum(counts)
    pts, ref_idx, pix, mask = rf.scene_points(0, total, provenance=True)
    assert_bitwise_equal(pts, np.concatenate(want, 0), "scene")
    assert ref_idx.tolist() == [0] * counts[0] + [1] * counts[1]
    assert all(not m.any() for m in rf.marks)                 # plain mode marks nothing
    assert_bitwise_equal(rf.scene_points(3, 4), pts[3:7], "range")


def _cloud(n=23, seed=0):
    rng = np.random.default_rng(seed)
    pts = rng.normal(size=(n, 9)).astype(np.float32)
    pts[:, 6:9] = rng.uniform(-20, 300, size=(n, 3))
    pts[3, 0] = np.inf
    pts[5, 2] = -np.finfo(np.float32).max
    pts[7, 7] = np.nan
    return pts


@pytest.mark.parametrize("chunk", [1, 7, 23])
def test_incremental_ply_writer_gives_write_ply_bytes(tmp_path, chunk):
    pts = _cloud()
    io.write_ply(str(tmp_path / "whole.ply"), pts)
    with io.PlyWriter(str(tmp_path / "parts.ply"), pts.shape[0]) as w:
        for a in range(0, pts.shape[0], chunk):
            w.write(pts[a:a + chunk])
    assert (tmp_path / "parts.ply").read_bytes() == (tmp_path / "whole.ply").read_bytes()


def test_incremental_ply_writer_checks_the_count(tmp_path):
    pts = _cloud(8)
    w = io.PlyWriter(str(tmp_path / "short.ply"), 9)
    w.write(pts)
    with pytest.raises(ValueError):
        w.close()
    w = io.PlyWriter(str(tmp_path / "long.ply"), 7)
    with pytest.raises(ValueError):
        w.write(pts)
    w.f.close()
    with io.PlyWriter(str(tmp_path / "empty.ply"), 0):
        pass
    assert io.read_ply(str(tmp_path / "empty.ply")).shape == (0,)


def test_pipeline_scene_path_with_stub(tmp_path):
    ds = small_dataset(64, 32, 3)
    pipe = pipeline.Pipeline(ds, engine=OracleEngine(), order="reference", geom_iterations=1).run()
    per_view = pipe.run_fusion(fusion_factory=OracleFusion, ply_path=str(tmp_path / "views.ply"))
    plain = pipe.run_fusion(fusion_factory=RestatedFusion, ply_path=str(tmp_path / "scene.ply"), chunk_points=7)
    assert per_view.shape[0] > 0
    assert_bitwise_equal(plain, per_view, "plain scene path")
    assert plain.dtype == per_view.dtype and pipe.fused is plain
    assert (tmp_path / "scene.ply").read_bytes() == (tmp_path / "views.ply").read_bytes()

    made = []

    def factory(cams):
        made.append(RestatedFusion(cams))
        return made[-1]
    uniq = pipe.run_fusion(fusion_factory=factory, ply_path=str(tmp_path / "unique.ply"), unique=True, chunk_points=5)
    n = made[0].result[0].shape[0]
    assert 0 < n < per_view.shape[0]
    assert uniq.shape == (n, 9) and io.read_ply(str(tmp_path / "unique.ply")).shape[0] == n
    assert_bitwise_equal(uniq, made[0].result[0], "unique scene path")

    # a cloud above the caller's limit is streamed to the PLY only
    assert pipe.run_fusion(fusion_factory=RestatedFusion, ply_path=str(tmp_path / "streamed.ply"),
                           max_host_points=per_view.shape[0] - 1) is None
    assert pipe.fused is None
    assert (tmp_path / "streamed.ply").read_bytes() == (tmp_path / "views.ply").read_bytes()
    with pytest.raises(ValueError):
        pipe.run_fusion(fusion_factory=OracleFusion, unique=True)


def test_restated_unique_scene_uses_every_sample_once():
    """The invariant of the duplicate-free mode, on the restatement itself: no depth sample contributes to
    points of two reference views, and a second run without a reset emits nothing from used pixels."""
    cams, depths, normals, colours = dataset_inputs("sphere")
    rf = fill(RestatedFusion(cams), cams, depths, normals, colours)
    refs, lists = [0, 1, 2], all_others(3)
    total, counts = rf.run_scene(refs, lists, unique=True)
    pts, ref_idx, pix, mask = rf.scene_points(0, total, provenance=True)
    n_samples = assert_samples_used_once(cams, depths, refs, lists, ref_idx, pix, mask)
    marks = [rf.used(v) for v in range(3)]
    assert sum(int(m.sum()) for m in marks) == n_samples
    again, _ = rf.run_scene(refs, lists, unique=True)
    _, ref2, pix2, _ = rf.scene_points(0, again, provenance=True)
    assert all(not marks[refs[k]].reshape(-1)[p] for k, p in zip(ref2.tolist(), pix2.tolist()))
