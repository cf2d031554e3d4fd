"""Pipeline.run_fusion(eval_mesh_samples=SPACING) / --eval-mesh-samples: the "mesh_samples" block of eval.json against
the direct calls, the untouched outputs without the option, the refused combinations; compare_clouds.py --mesh-samples."""
import importlib.util
import json
import os

import numpy as np
import pytest

import cloud_distance_support as cd
import mesh_sample_support as mss
import voxel_support as vs
from acmmp import capi, io, pipeline
from pipeline_support import OracleEngine, small_dataset

F32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path, factory):
    """The small dataset through the pipeline and two fusions with a mesh and an evaluation: without the option ("a")
    and with it ("b").  Returns (pipe, the reference cloud, the options, the spacing)."""
    ds = small_dataset(64, 32, 3)
    pipe = pipeline.Pipeline(ds, engine=OracleEngine(), order="reference", geom_iterations=1, out_folder=str(tmp_path / "out")).run()
    plain = pipe.run_fusion(fusion_factory=factory)
    ok = vs.finite_points(plain)
    ext = float((plain[ok, :3].max(0) - plain[ok, :3].min(0)).max())
    size = ext / 24
    ref = (plain[ok, :3] + F32(size / 8)).astype(F32)
    opts = dict(voxel_size=size, mesh_trunc=3 * size, eval_cloud=ref, eval_max_dist=2 * size, eval_thresholds=(size / 2, size),
                eval_surface=True)
    for name, extra in (("a", {}), ("b", dict(eval_mesh_samples=size / 2))):
        pipe.run_fusion(fusion_factory=factory, ply_path=str(tmp_path / name / "cloud.ply"),
                        mesh_path=str(tmp_path / name / "mesh.ply"), **opts, **extra)
    return pipe, ref, opts, size / 2


def _rows(q, t, md, taus):
    s = cd.distances(q, t, md, taus)[2]
    return {"n_query": s[0], "n_valid": s[1], "n_matched": s[2], "within": s[4:4 + len(taus)],
            "mean": s[3] / (s[2] * (1048576.0 / float(F32(md)))) if s[2] else 0.0}


def _check(tmp_path, pipe, ref, opts, spacing, make):
    a, b = json.load(open(tmp_path / "a" / "eval.json")), json.load(open(tmp_path / "b" / "eval.json"))
    assert "mesh_samples" not in a and b == json.loads(json.dumps(pipe.eval_info))
    block = b.pop("mesh_samples")
    assert a == b and "surface" in a                                       # the rest of eval.json is the parent's
    for name in ("cloud.ply", "mesh.ply"):                                 # and so is every other output
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes()
    # the block is that of the direct calls on a fusion object given the written mesh
    rec, faces = io.read_mesh_ply(str(tmp_path / "b" / "mesh.ply"))
    verts = np.zeros((len(rec), 9), F32)
    for k, name in enumerate(("x", "y", "z", "nx", "ny", "nz")):
        verts[:, k] = rec[name]
    assert len(faces) > 20
    cam = np.zeros(1, capi.CAMERA_DTYPE)
    cam["width"], cam["height"] = 8, 8
    fu = make(cam)
    fu.set_mesh(verts, faces)
    got = fu.mesh_sample(spacing, 0)
    pts, face = fu.sample_points()
    if hasattr(fu, "close"):
        fu.close()
    taus = [float(F32(t)) for t in opts["eval_thresholds"]]
    assert block["spacing"] == float(F32(spacing)) and block["seed"] == 0
    assert block["n_samples"] == got.n_samples == len(pts) > len(faces) and block["n_skipped"] == got.n_skipped == 0
    want = mss.sample(verts, faces, spacing, 0)                            # positions depend on the vertices' positions only
    assert np.array_equal(pts[:, :3], want[0][:, :3]) and np.array_equal(face, want[1])
    for name, (q, t) in (("accuracy", (pts, ref)), ("completeness", (ref, pts))):
        row, w = block[name], _rows(q, t, opts["eval_max_dist"], taus)
        assert {k: row[k] for k in w} == w, name
        assert set(row) == set(a[name])                                    # the format of the existing directions
    assert block["accuracy"]["n_matched"] > 0
    for i, row in enumerate(block["thresholds"]):
        acc, com = block["accuracy"], block["completeness"]
        p, r = acc["within"][i] / acc["n_valid"], com["within"][i] / com["n_valid"]
        assert row == {"threshold": taus[i], "precision": p, "recall": r, "f_score": 2 * p * r / (p + r) if p + r > 0 else 0.0}
    assert set(block) == {"spacing", "seed", "n_samples", "n_skipped", "accuracy", "completeness", "thresholds"}


def test_pipeline_mesh_samples_with_the_restated_fusion(tmp_path):
    make = mss.RestatedSampleFusion
    pipe, ref, opts, spacing = _run(tmp_path, make)
    _check(tmp_path, pipe, ref, opts, spacing, make)
    # the option needs the reference cloud, the mesh, and a fusion object that can sample one
    with pytest.raises(ValueError):
        pipe.run_fusion(fusion_factory=make, eval_mesh_samples=spacing)
    with pytest.raises(ValueError):
        pipe.run_fusion(fusion_factory=make, voxel_size=opts["voxel_size"], eval_cloud=ref, eval_max_dist=1.0,
                        eval_mesh_samples=spacing)
    with pytest.raises(ValueError):
        pipe.run_fusion(fusion_factory=make, voxel_size=opts["voxel_size"], mesh_trunc=opts["mesh_trunc"], eval_mesh_samples=spacing)
    with pytest.raises(ValueError):
        pipe.run_fusion(fusion_factory=mss.sd.RestatedSurfaceFusion, **opts, eval_mesh_samples=spacing)


def test_compare_clouds_mesh_samples(tmp_path, monkeypatch, capsys):
    """compare_clouds.py --mesh-samples: A a mesh PLY, loaded through set_mesh; the block against the direct calls;
    without the option the output is what it was."""
    spec = importlib.util.spec_from_file_location("compare_clouds", os.path.join(REPO, "scripts", "compare_clouds.py"))
    cc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cc)
    v, f = mss.sd.mixed_mesh()
    b = mss.sd.near_queries(v, f, 300, 0.02, seed=12)
    io.write_mesh_ply(str(tmp_path / "a.ply"), v, f)
    io.write_ply(str(tmp_path / "b.ply"), cd.as_points(b))
    make = mss.RestatedSampleFusion
    taus = (0.01, 0.03)
    plain = cc.compare(v[:, :3], b, 0.06, taus, make=make, a_faces=f)
    got = cc.compare(v[:, :3], b, 0.06, taus, make=make, a_faces=f, mesh_samples=0.05)
    block = got.pop("mesh_samples")
    assert got == plain and "mesh_samples" not in plain and "surface" in plain
    only = cc.compare(v[:, :3], b, 0.06, taus, make=make, a_faces=f, surface=False, mesh_samples=0.05)
    assert "surface" not in only and only["mesh_samples"] == block
    mesh = np.zeros((len(v), 9), F32)
    mesh[:, :3] = v[:, :3]                                                 # compare loads positions (and normals on request)
    pts, face, skipped = mss.sample(mesh, f, 0.05, 0)
    assert block["n_samples"] == len(pts) > 1000 and block["n_skipped"] == skipped == 0
    assert (np.bincount(face, minlength=len(f))[-2:] > 100).all()          # the two spanning faces carry their area
    ft = [float(F32(t)) for t in taus]
    for name, (q, t) in (("accuracy", (pts, b)), ("completeness", (b, pts))):
        w = _rows(q, t, 0.06, ft)
        assert {k: block[name][k] for k in w} == w, name
    with pytest.raises(ValueError):
        cc.compare(v[:, :3], b, 0.06, taus, make=make, mesh_samples=0.05)    # no faces
    monkeypatch.setattr(cc.capi, "Fusion", lambda device, cams: make(cams))
    assert cc.main([str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), "--max-dist", "0.06", "--threshold", "0.01",
                    "--threshold", "0.03", "--mesh-samples", "0.05"]) == 0
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert printed["mesh_samples"] == json.loads(json.dumps(block)) and "surface" not in printed


def test_cli_eval_mesh_samples():
    a = pipeline.arg_parser().parse_args(["folder", "--eval-cloud", "gt.ply", "--eval-max-dist", "0.02", "--mesh", "m.ply",
                                          "--voxel-size", "0.01", "--eval-mesh-samples", "0.005"])
    assert a.eval_mesh_samples == 0.005
    assert pipeline.arg_parser().parse_args(["folder"]).eval_mesh_samples is None
    with pytest.raises(SystemExit):
        pipeline.arg_parser().parse_args(["folder", "--eval-mesh-samples"])
    with pytest.raises(SystemExit):
        pipeline.arg_parser().parse_args(["folder", "--eval-mesh-samples", "dense"])


@pytest.mark.gpu
def test_pipeline_mesh_samples_on_the_device(tmp_path):
    factory = lambda cams: capi.Fusion(0, cams)
    pipe, ref, opts, spacing = _run(tmp_path, factory)
    _check(tmp_path, pipe, ref, opts, spacing, factory)
