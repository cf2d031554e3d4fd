"""Pipeline.run_fusion's point-to-plane stage and scripts/compare_clouds.py --align-plane-iterations (CPU, through the
restated fusion): eval.json's "align"."plane", the option errors, and eval.json untouched without the option."""
import importlib.util
import json
import os

import numpy as np
import pytest

import cloud_align_plane_support as cp
import cloud_align_support as ca
import cloud_distance_support as cd
import voxel_support as vs
from acmmp import io, pipeline
from pipeline_support import OracleEngine, small_dataset

F32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANE_FIELDS = {"M", "stop_reason", "iterations", "n_no_normal", "rms_first", "rms_last"}


def test_pipeline_plane_stage_with_the_restated_fusion(tmp_path):
    ds = small_dataset(64, 32, 3)
    pipe = pipeline.Pipeline(ds, engine=OracleEngine(), order="reference", geom_iterations=1,
                             out_folder=str(tmp_path / "out")).run()
    plain = pipe.run_fusion(fusion_factory=cp.RestatedAlignPlaneFusion, ply_path=str(tmp_path / "a" / "cloud.ply"))
    assert vs.finite_points(plain).all() and len(plain) > 50
    xyz = plain[:, :3]
    ext = float((xyz.max(0) - xyz.min(0)).max())
    known = ca.about(ca.rotation((1, -1, 2), 0.5), xyz.astype(np.float64).mean(0), (ext / 300, -ext / 400, ext / 500))
    moved = plain.copy()
    moved[:, :3] = ca.transform_points(known, xyz)
    io.write_ply(str(tmp_path / "reference.ply"), moved)
    max_dist, taus = ext / 20, (ext / 200,)
    common = dict(fusion_factory=cp.RestatedAlignPlaneFusion, eval_cloud=str(tmp_path / "reference.ply"),
                  eval_max_dist=max_dist, eval_thresholds=taus)
    # without the option eval.json is byte for byte what the point stage alone writes, with either fusion object
    pipe.run_fusion(ply_path=str(tmp_path / "b" / "cloud.ply"), eval_align="rigid", eval_align_iterations=4, **common)
    point_only = pipe.eval_info
    pipe.run_fusion(ply_path=str(tmp_path / "b0" / "cloud.ply"), eval_align="rigid", eval_align_iterations=4,
                    **{**common, "fusion_factory": ca.RestatedAlignFusion})
    assert (tmp_path / "b" / "eval.json").read_bytes() == (tmp_path / "b0" / "eval.json").read_bytes()
    assert "plane" not in point_only["align"]
    got = pipe.run_fusion(ply_path=str(tmp_path / "c" / "cloud.ply"), eval_align="rigid", eval_align_iterations=4,
                          eval_align_plane_iterations=3, **common)
    assert (tmp_path / "c" / "cloud.ply").read_bytes() == (tmp_path / "a" / "cloud.ply").read_bytes()   # never transformed
    assert got.tobytes() == plain.tobytes()
    info = json.load(open(tmp_path / "c" / "eval.json"))
    assert info == json.loads(json.dumps(pipe.eval_info))
    al = info["align"]
    assert {k: v for k, v in al.items() if k != "plane"} == json.loads(json.dumps(point_only["align"]))   # the point stage is the same
    pl = al["plane"]
    assert set(pl) == PLANE_FIELDS and pl["stop_reason"] in ca.STOP_REASONS and 1 <= len(pl["iterations"]) <= 3
    assert set(pl["iterations"][0]) == {"n_matched", "mean", "shift"} and np.array(pl["M"]).shape == (3, 4)
    # the figures are the restatement's: the plane loop from the point stage's M, and the measurement under its M
    want = cp.align_plane(plain, pipeline.reference_xyz(moved), max_dist, 3, init=np.array(al["M"]))
    assert np.array_equal(np.array(pl["M"]), want.M) and pl["stop_reason"] == want.stop_reason
    assert pl["n_no_normal"] == want.records[-1].n_no_normal
    assert pl["rms_first"] == want.records[0].rms_plane and pl["rms_last"] == want.records[-1].rms_plane
    s = cd.distances(ca.transform_points(want.M, xyz), moved[:, :3], max_dist, taus)[2]
    assert [info["accuracy"][k] for k in ("n_query", "n_valid", "n_matched")] == s[:3]
    print("plane stage", pl["stop_reason"], "rms", pl["rms_first"], "->", pl["rms_last"], "accuracy mean",
          point_only["accuracy"]["mean"], "->", info["accuracy"]["mean"])
    # stride and cap reach the plane call
    pipe.run_fusion(eval_align="rigid", eval_align_max_dist=max_dist / 2, eval_align_iterations=2, eval_align_stride=3,
                    eval_align_plane_iterations=1, **common)
    pl = pipe.eval_info["align"]["plane"]
    assert len(pl["iterations"]) == 1 and pl["iterations"][0]["n_matched"] <= -(-len(plain) // 3)
    # option errors
    ref = moved[:, :3]
    for kw in (dict(eval_align_plane_iterations=3), dict(eval_cloud=ref, eval_max_dist=1.0, eval_align_plane_iterations=3),
               dict(eval_cloud=ref, eval_max_dist=1.0, eval_align="rigid", eval_align_plane_iterations=0),
               dict(eval_cloud=ref, eval_max_dist=1.0, eval_align="rigid", eval_align_plane_iterations=1025)):
        with pytest.raises(ValueError):
            pipe.run_fusion(fusion_factory=cp.RestatedAlignPlaneFusion, **kw)
    with pytest.raises(ValueError):                                        # a fusion object without the plane call
        pipe.run_fusion(fusion_factory=ca.RestatedAlignFusion, eval_cloud=ref, eval_max_dist=1.0, eval_align="rigid",
                        eval_align_plane_iterations=2)


def test_cli_plane_option():
    a = pipeline.arg_parser().parse_args(["folder", "--eval-cloud", "gt.ply", "--eval-max-dist", "0.02", "--eval-align", "rigid",
                                          "--eval-align-plane-iterations", "7"])
    assert a.eval_align_plane_iterations == 7
    assert pipeline.arg_parser().parse_args(["folder"]).eval_align_plane_iterations is None


def test_compare_clouds_plane_stage(tmp_path, monkeypatch, capsys):
    spec = importlib.util.spec_from_file_location("compare_clouds", os.path.join(REPO, "scripts", "compare_clouds.py"))
    cc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cc)
    data, b, known = cp.two_samplings(800, 4)
    a, normals = data[:, :3], data[:, 3:6]
    io.write_ply(str(tmp_path / "a.ply"), data)
    io.write_ply(str(tmp_path / "b.ply"), cd.as_points(b))
    make = cp.RestatedAlignPlaneFusion
    point = cc.compare(a, b, 0.08, (0.01,), make=make, align="rigid", align_iterations=4)
    assert "plane" not in point["align"]
    got = cc.compare(a, b, 0.08, (0.01,), make=make, align="rigid", align_iterations=4, align_plane_iterations=4, a_normals=normals)
    assert set(got["align"]["plane"]) == PLANE_FIELDS
    ep, eq = cp.corner_error(np.array(got["align"]["plane"]["M"]), known), cp.corner_error(np.array(point["align"]["M"]), known)
    print("corner error: point stage", eq, "after the plane stage", ep)
    assert ep < eq and got["align"]["M"] == point["align"]["M"]
    for kw in (dict(align_plane_iterations=2, a_normals=normals), dict(align="rigid", align_plane_iterations=2)):
        with pytest.raises(ValueError):
            cc.compare(a, b, 0.08, make=make, **kw)
    # the command line, with the restated object in capi.Fusion's place: the normals come from A's PLY
    monkeypatch.setattr(cc.capi, "Fusion", lambda device, cams: make(cams))
    out = str(tmp_path / "eval.json")
    args = [str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), "--max-dist", "0.08", "--threshold", "0.01", "--align", "rigid",
            "--align-iterations", "4"]
    assert cc.main(args + ["--align-plane-iterations", "4", "--out", out]) == 0
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert printed == json.load(open(out)) and printed["align"] == json.loads(json.dumps(got["align"]))
    assert cc.main(args) == 0
    assert "plane" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])["align"]
    with pytest.raises(SystemExit):
        cc.main(args[:6] + ["--align-plane-iterations", "4"])


def test_restated_plane_lifetimes():
    """The restated object keeps capi.Fusion's rules: one set of records, of the last align call of either kind."""
    rf = cp.RestatedAlignPlaneFusion(np.zeros(1, pipeline.capi.CAMERA_DTYPE))
    data, ref, _ = cp.two_samplings(300, 5)
    rf.set_scene(data)
    with pytest.raises(ValueError):
        rf.cloud_align_plane("scene", 0.1)                                 # no reference cloud
    rf.set_reference_cloud(ref)
    r = rf.cloud_align_plane("scene", 0.1, 2)
    assert rf.cloud_transform() is None and len(rf.align_plane_records(0, r.iterations)) == r.iterations
    with pytest.raises(ValueError):
        rf.align_records(0, 1)
    rf.cloud_align("scene", "rigid", 0.1, 1)
    assert len(rf.align_records(0, 1)) == 1
    with pytest.raises(ValueError):
        rf.align_plane_records(0, 1)
    rf.cloud_align_plane("scene", 0.1, 1)
    rf.set_reference_cloud(ref)
    with pytest.raises(ValueError):
        rf.align_plane_records(0, 1)
    rf.cloud_align_plane("scene", 0.1, 1)
    rf.set_scene(data[:100])
    with pytest.raises(ValueError):
        rf.align_plane_records(0, 1)
    for bad in (dict(max_dist=0.0), dict(max_iterations=0), dict(stride=0), dict(min_shift=-1.0), dict(init=np.full((3, 4), np.nan))):
        with pytest.raises(ValueError):
            rf.cloud_align_plane("scene", **{"max_dist": 0.1, **bad})
    with pytest.raises(ValueError):
        rf.cloud_align_plane("cloud", 0.1)
