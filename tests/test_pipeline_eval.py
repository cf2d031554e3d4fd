"""Pipeline.run_fusion's evaluation options (CPU, through the restated fusion): eval.json, the untouched outputs."""
import json
import os

import numpy as np
import pytest

import cloud_distance_support as cd
import voxel_support as vs
from acmmp import io, pipeline
from pipeline_support import OracleEngine, small_dataset

F32 = np.float32


def test_pipeline_eval_with_the_restated_fusion(tmp_path):
    ds = small_dataset(64, 32, 3)
    folder = str(tmp_path / "out")
    pipe = pipeline.Pipeline(ds, engine=OracleEngine(), order="reference", geom_iterations=1, out_folder=folder).run()
    plain = pipe.run_fusion(fusion_factory=cd.RestatedDistanceFusion, ply_path=str(tmp_path / "a" / "cloud.ply"))
    assert pipe.eval_info is None and not os.path.exists(tmp_path / "a" / "eval.json")      # the defaults write nothing
    ok = vs.finite_points(plain)
    assert ok.all() and len(plain) > 50
    ext = float((plain[ok, :3].max(0) - plain[ok, :3].min(0)).max())
    # the reference cloud: the run's own cloud moved by a known offset, as a PLY
    shift = ext / 200
    moved = plain.copy()
    moved[:, 0] += F32(shift)
    io.write_ply(str(tmp_path / "reference.ply"), moved)
    ref = pipeline.reference_xyz(str(tmp_path / "reference.ply"))
    assert ref.shape == (len(plain), 3) and ref.dtype == F32
    max_dist, taus = 4 * shift, (2 * shift, shift / 64)
    got = pipe.run_fusion(fusion_factory=cd.RestatedDistanceFusion, ply_path=str(tmp_path / "b" / "cloud.ply"),
                          eval_cloud=str(tmp_path / "reference.ply"), eval_max_dist=max_dist, eval_thresholds=taus)
    # every existing output is byte for byte what it is without the options
    assert (tmp_path / "b" / "cloud.ply").read_bytes() == (tmp_path / "a" / "cloud.ply").read_bytes()
    assert got.tobytes() == plain.tobytes()
    info = json.load(open(tmp_path / "b" / "eval.json"))
    assert info == json.loads(json.dumps(pipe.eval_info)) and info["source"] == "scene"
    assert info["max_dist"] == float(F32(max_dist))
    # the counts are the restatement's
    for name, (q, t) in (("accuracy", (plain, ref)), ("completeness", (ref, plain))):
        d2, nn, s = cd.distances(q, t, max_dist, taus)
        row = info[name]
        assert [row["n_query"], row["n_valid"], row["n_matched"]] == s[:3] and row["within"] == s[4:6]
        assert row["n_valid"] == row["n_matched"] > 50                    # every point has its moved copy within the cap
        assert row["mean"] == s[3] / (s[2] * (1048576.0 / float(F32(max_dist)))) and 0 < row["mean"] <= shift * 1.001
        assert 0 < row["median_upper"] <= max_dist
    above, below = info["thresholds"]
    assert above["threshold"] == float(F32(taus[0])) and (above["precision"], above["recall"], above["f_score"]) == (1.0, 1.0, 1.0)
    assert (below["precision"], below["recall"], below["f_score"]) == (0.0, 0.0, 0.0)
    # an array instead of a file, another source
    size = ext / 16
    pipe.run_fusion(fusion_factory=cd.RestatedDistanceFusion, voxel_size=size, eval_cloud=ref, eval_max_dist=size,
                    eval_thresholds=(size,), eval_source="scene")
    assert pipe.eval_info["source"] == "scene" and pipe.eval_info["accuracy"]["n_query"] == len(plain)
    pipe.run_fusion(fusion_factory=cd.RestatedDistanceFusion, voxel_size=size, eval_cloud=ref, eval_max_dist=size)
    assert pipe.eval_info["source"] == "voxels" and pipe.eval_info["accuracy"]["n_query"] == pipe.fusion_info["voxels"]
    assert pipe.eval_info["thresholds"] == []
    # the options need the cloud, the cloud needs the cap, and a fusion object that can measure
    for kw in (dict(eval_max_dist=1.0), dict(eval_thresholds=(0.1,)), dict(eval_source="scene"), dict(eval_cloud=ref),
               dict(eval_cloud=ref, eval_max_dist=1.0, eval_source="cloud")):
        with pytest.raises(ValueError):
            pipe.run_fusion(fusion_factory=cd.RestatedDistanceFusion, **kw)
    with pytest.raises(ValueError):
        pipe.run_fusion(fusion_factory=cd.rs.RestatedRenderFusion, eval_cloud=ref, eval_max_dist=1.0)


def test_cli_eval_options():
    a = pipeline.arg_parser().parse_args(["folder", "--eval-cloud", "gt.ply", "--eval-max-dist", "0.02", "--eval-threshold", "0.005",
                                          "--eval-threshold", "0.01", "--eval-source", "mesh"])
    assert (a.eval_cloud, a.eval_max_dist, a.eval_threshold, a.eval_source) == ("gt.ply", 0.02, [0.005, 0.01], "mesh")
    a = pipeline.arg_parser().parse_args(["folder"])
    assert (a.eval_cloud, a.eval_max_dist, a.eval_threshold, a.eval_source) == (None, None, [], None)


def test_restated_distance_lifetimes():
    """The restated object keeps capi.Fusion's rules: a distance result goes with its source and with the reference."""
    rf = cd.RestatedDistanceFusion(np.zeros(1, pipeline.capi.CAMERA_DTYPE))
    Q, T = cd.clouds()
    rf.set_scene(cd.as_points(Q[:200]))
    with pytest.raises(ValueError):
        rf.cloud_distance("scene", "data_to_ref", 1.0)
    rf.set_reference_cloud(T[:300])
    with pytest.raises(ValueError):
        rf.cloud_distance("voxels", "data_to_ref", 1.0)
    r = rf.cloud_distance("scene", "ref_to_data", 0.1, (0.05,))
    assert r.n_query == 300 and len(rf.distance_results()[0]) == 300
    rf.set_reference_cloud(T[:300])
    with pytest.raises(ValueError):
        rf.distance_results(0, 1)
    rf.cloud_distance("scene", "data_to_ref", 0.1)
    rf.set_scene(cd.as_points(Q[:100]))
    with pytest.raises(ValueError):
        rf.distance_results(0, 1)
