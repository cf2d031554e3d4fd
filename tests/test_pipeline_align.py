"""Pipeline.run_fusion's alignment options and scripts/compare_clouds.py --align (CPU, through the restated fusion):
eval.json's "align", the untouched outputs, the option errors."""
import importlib.util
import json
import os

import numpy as np
import pytest

import cloud_align_support as ca
import cloud_distance_support as cd
import voxel_support as vs
from acmmp import io, pipeline
from pipeline_support import OracleEngine, small_dataset

F32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pipeline_align_with_the_restated_fusion(tmp_path):
    ds = small_dataset(64, 32, 3)
    pipe = pipeline.Pipeline(ds, engine=OracleEngine(), order="reference", geom_iterations=1,
                             out_folder=str(tmp_path / "out")).run()
    plain = pipe.run_fusion(fusion_factory=ca.RestatedAlignFusion, ply_path=str(tmp_path / "a" / "cloud.ply"))
    ok = vs.finite_points(plain)
    assert ok.all() and len(plain) > 50
    xyz = plain[:, :3]
    ext = float((xyz.max(0) - xyz.min(0)).max())
    # the reference cloud: the run's own cloud turned by half a degree about its centre and shifted
    known = ca.about(ca.rotation((1, -1, 2), 0.5), xyz.astype(np.float64).mean(0), (ext / 300, -ext / 400, ext / 500))
    moved = plain.copy()
    moved[:, :3] = ca.transform_points(known, xyz)
    io.write_ply(str(tmp_path / "reference.ply"), moved)
    max_dist, taus = ext / 20, (ext / 200,)
    common = dict(fusion_factory=ca.RestatedAlignFusion, eval_cloud=str(tmp_path / "reference.ply"), eval_max_dist=max_dist,
                  eval_thresholds=taus)
    pipe.run_fusion(ply_path=str(tmp_path / "b" / "cloud.ply"), **common)
    unaligned = pipe.eval_info
    assert "align" not in unaligned
    got = pipe.run_fusion(ply_path=str(tmp_path / "c" / "cloud.ply"), eval_align="rigid", eval_align_iterations=8, **common)
    # the written cloud is never transformed, and eval.json without the option is what it was
    assert (tmp_path / "c" / "cloud.ply").read_bytes() == (tmp_path / "a" / "cloud.ply").read_bytes()
    assert got.tobytes() == plain.tobytes()
    info = json.load(open(tmp_path / "c" / "eval.json"))
    assert info == json.loads(json.dumps(pipe.eval_info))
    assert json.load(open(tmp_path / "b" / "eval.json")) == {k: v for k, v in unaligned.items()}
    al = info["align"]
    assert al["mode"] == "rigid" and al["max_dist"] == float(F32(max_dist)) and al["stop_reason"] in ca.STOP_REASONS
    assert 1 <= len(al["iterations"]) <= 8 and set(al["iterations"][0]) == {"n_matched", "mean", "shift"}
    M = np.array(al["M"])
    print("accuracy mean", unaligned["accuracy"]["mean"], "->", info["accuracy"]["mean"], "error", np.abs(M - known).max())
    assert M.shape == (3, 4) and info["accuracy"]["mean"] < unaligned["accuracy"]["mean"]
    assert info["completeness"]["mean"] < unaligned["completeness"]["mean"]
    assert info["thresholds"][0]["f_score"] >= unaligned["thresholds"][0]["f_score"]
    # the figures are the restatement's under that M, and the loop is align()'s
    want = ca.align(xyz, pipeline.reference_xyz(moved), "rigid", max_dist, 8)
    assert np.array_equal(M, want.M) and [r["n_matched"] for r in al["iterations"]] == [r.n_matched for r in want.records]
    s = cd.distances(ca.transform_points(M, xyz), moved[:, :3], max_dist, taus)[2]
    assert [info["accuracy"][k] for k in ("n_query", "n_valid", "n_matched")] == s[:3]
    # the other options reach the call
    pipe.run_fusion(eval_align="similarity", eval_align_max_dist=max_dist / 2, eval_align_iterations=2, eval_align_stride=3, **common)
    al = pipe.eval_info["align"]
    assert al["mode"] == "similarity" and al["max_dist"] == float(F32(max_dist / 2)) and len(al["iterations"]) <= 2
    assert al["iterations"][0]["n_matched"] <= -(-len(plain) // 3)
    # option errors
    ref = moved[:, :3]
    for kw in (dict(eval_align="rigid"), dict(eval_align_stride=2), dict(eval_cloud=ref, eval_max_dist=1.0, eval_align_iterations=3),
               dict(eval_cloud=ref, eval_max_dist=1.0, eval_align_max_dist=0.5), dict(eval_cloud=ref, eval_max_dist=1.0, eval_align="affine"),
               dict(eval_cloud=ref, eval_max_dist=1.0, eval_align="rigid", eval_align_iterations=0),
               dict(eval_cloud=ref, eval_max_dist=1.0, eval_align="rigid", eval_align_stride=0)):
        with pytest.raises(ValueError):
            pipe.run_fusion(fusion_factory=ca.RestatedAlignFusion, **kw)
    with pytest.raises(ValueError):                                        # a fusion object that cannot align
        pipe.run_fusion(fusion_factory=cd.RestatedDistanceFusion, eval_cloud=ref, eval_max_dist=1.0, eval_align="rigid")


def test_cli_align_options():
    a = pipeline.arg_parser().parse_args(["folder", "--eval-cloud", "gt.ply", "--eval-max-dist", "0.02", "--eval-align", "similarity",
                                          "--eval-align-max-dist", "0.05", "--eval-align-iterations", "12", "--eval-align-stride", "4"])
    assert (a.eval_align, a.eval_align_max_dist, a.eval_align_iterations, a.eval_align_stride) == ("similarity", 0.05, 12, 4)
    a = pipeline.arg_parser().parse_args(["folder"])
    assert (a.eval_align, a.eval_align_max_dist, a.eval_align_iterations, a.eval_align_stride) == (None, None, None, None)
    with pytest.raises(SystemExit):
        pipeline.arg_parser().parse_args(["folder", "--eval-align", "affine"])


def test_compare_clouds_align(tmp_path, monkeypatch, capsys):
    spec = importlib.util.spec_from_file_location("compare_clouds", os.path.join(REPO, "scripts", "compare_clouds.py"))
    cc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cc)
    rng = np.random.default_rng(4)
    b = rng.random((400, 3), dtype=F32)
    known = ca.about(ca.rotation((0, 1, 1), 1.0), (0.5, 0.5, 0.5), (0.004, 0.0, -0.003))
    a = ca.transform_points(ca.inverse(known), b[:300])
    for name, xyz in (("a.ply", a), ("b.ply", b)):
        io.write_ply(str(tmp_path / name), cd.as_points(xyz))
    make = ca.RestatedAlignFusion
    plain = cc.compare(a, b, 0.05, (0.002,), make=make)
    assert "align" not in plain
    got = cc.compare(a, b, 0.05, (0.002,), make=make, align="rigid", align_iterations=6)
    assert np.abs(np.array(got["align"]["M"]) - known).max() < 1e-3
    assert got["accuracy"]["mean"] < 0.1 * plain["accuracy"]["mean"] and got["thresholds"][0]["precision"] > plain["thresholds"][0]["precision"]
    # the command line, with the restated object in capi.Fusion's place
    monkeypatch.setattr(cc.capi, "Fusion", lambda device, cams: make(cams))
    out = str(tmp_path / "eval.json")
    assert cc.main([str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), "--max-dist", "0.05", "--threshold", "0.002", "--align", "rigid",
                    "--align-iterations", "6", "--out", out]) == 0
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert printed == json.load(open(out)) and printed["align"] == json.loads(json.dumps(got["align"]))
    assert cc.main([str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), "--max-dist", "0.05"]) == 0
    assert "align" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_restated_align_lifetimes():
    """The restated object keeps capi.Fusion's rules: the transform is the object's, a set discards the distance result,
    the records go with their source and with the reference cloud."""
    rf = ca.RestatedAlignFusion(np.zeros(1, pipeline.capi.CAMERA_DTYPE))
    Q, T = cd.clouds()
    rf.set_scene(cd.as_points(Q[:200]))
    with pytest.raises(ValueError):
        rf.cloud_align("scene", "rigid", 0.1)                              # no reference cloud
    rf.set_reference_cloud(T[:300])
    M = ca.SMALL_ROTATION
    rf.set_cloud_transform(M)
    assert np.array_equal(rf.cloud_transform(), M)
    under = rf.cloud_distance("scene", "data_to_ref", 0.1)
    assert cd.summary_of(under) == cd.distances(ca.transform_points(M, Q[:200]), T[:300], 0.1)[2]
    rf.set_cloud_transform(None)
    with pytest.raises(ValueError):
        rf.distance_results(0, 1)                                          # discarded by the clear
    r = rf.cloud_align("scene", "rigid", 0.1, 2)
    assert rf.cloud_transform() is None and len(rf.align_records(0, r.iterations)) == r.iterations
    for bad in (dict(mode="affine"), dict(max_dist=0.0), dict(max_iterations=0), dict(max_iterations=1025), dict(stride=0),
                dict(min_shift=-1.0), dict(init=np.full((3, 4), np.nan))):
        with pytest.raises(ValueError):
            rf.cloud_align("scene", **{"mode": "rigid", "max_dist": 0.1, **bad})
    with pytest.raises(ValueError):
        rf.set_cloud_transform(np.full((3, 4), np.inf))
    assert len(rf.align_records(0, r.iterations)) == r.iterations
    rf.set_reference_cloud(T[:300])
    with pytest.raises(ValueError):
        rf.align_records(0, 1)
    rf.cloud_align("scene", "rigid", 0.1, 1)
    rf.set_scene(cd.as_points(Q[:100]))
    with pytest.raises(ValueError):
        rf.align_records(0, 1)
