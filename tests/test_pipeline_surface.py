"""Pipeline.run_fusion(eval_surface=True) / --eval-surface: the "surface" block of eval.json against the direct calls,
the untouched outputs without the option, the refused combinations."""
import importlib.util
import json
import os

import numpy as np
import pytest

import surface_distance_support as sd
import voxel_support as vs
from acmmp import capi, io, pipeline
from pipeline_support import OracleEngine, small_dataset

F32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path, factory):
    """The small dataset through the pipeline and three fusions: plain, with the parent's evaluation options, and with
    eval_surface on top (and first, into "c", with an alignment as well).  Returns (pipe, the surface run's eval info, folder names, the options)."""
    ds = small_dataset(64, 32, 3)
    pipe = pipeline.Pipeline(ds, engine=OracleEngine(), order="reference", geom_iterations=1, out_folder=str(tmp_path / "out")).run()
    plain = pipe.run_fusion(fusion_factory=factory)
    ok = vs.finite_points(plain)
    ext = float((plain[ok, :3].max(0) - plain[ok, :3].min(0)).max())
    size = ext / 24
    ref = (plain[ok, :3] + F32(size / 8)).astype(F32)
    opts = dict(voxel_size=size, mesh_trunc=3 * size, eval_cloud=ref, eval_max_dist=2 * size, eval_thresholds=(size / 2, size))
    aligned = dict(eval_surface=True, eval_align="rigid", eval_align_iterations=3)
    for name, extra in (("c", aligned), ("a", {}), ("b", dict(eval_surface=True))):
        pipe.run_fusion(fusion_factory=factory, ply_path=str(tmp_path / name / "cloud.ply"),
                        mesh_path=str(tmp_path / name / "mesh.ply"), **opts, **extra)
    return pipe, ref, opts


def _check(tmp_path, pipe, ref, opts, factory):
    a, b = json.load(open(tmp_path / "a" / "eval.json")), json.load(open(tmp_path / "b" / "eval.json"))
    assert "surface" not in a and b == json.loads(json.dumps(pipe.eval_info))
    surface = b.pop("surface")
    assert a == b                                                          # the rest of eval.json is the parent's
    for name in ("cloud.ply", "mesh.ply"):                                 # and so is every other output
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes()
    # the counts are those of the direct calls on the written cloud and mesh
    rec, faces = io.read_mesh_ply(str(tmp_path / "b" / "mesh.ply"))
    verts = np.stack([rec[k] for k in ("x", "y", "z")], 1).astype(F32)
    cloud = pipeline.reference_xyz(str(tmp_path / "b" / "cloud.ply"))
    assert len(faces) > 20
    taus = [float(F32(t)) for t in opts["eval_thresholds"]]
    for name, q in (("completeness", ref), ("fidelity", cloud)):
        d2, nn, s, _ = sd.distances(q, verts, faces, opts["eval_max_dist"], taus)
        row = surface[name]
        assert [row["n_query"], row["n_valid"], row["n_matched"]] == s[:3] and row["within"] == s[4:6], name
        assert row["mean"] == (s[3] / (s[2] * (1048576.0 / float(F32(opts["eval_max_dist"])))) if s[2] else 0.0)
    assert surface["fidelity"]["n_matched"] > 0
    # after an alignment the reference queries see the mesh under the installed transform, the written cloud's do not
    c = json.load(open(tmp_path / "c" / "eval.json"))
    M = np.array(c["align"]["M"])
    assert np.abs(M - np.eye(3, 4)).max() > 1e-6
    for name, q, m in (("completeness", ref, M), ("fidelity", cloud, None)):
        s = sd.distances(q, verts, faces, opts["eval_max_dist"], taus, M=m)[2]
        row = c["surface"][name]
        assert [row["n_query"], row["n_valid"], row["n_matched"]] == s[:3] and row["within"] == s[4:6], name
    assert c["surface"]["fidelity"] == surface["fidelity"]
    assert (tmp_path / "c" / "mesh.ply").read_bytes() == (tmp_path / "a" / "mesh.ply").read_bytes()
    for i, row in enumerate(surface["thresholds"]):
        c = surface["completeness"]
        assert row["threshold"] == taus[i] and row["recall"] == c["within"][i] / c["n_valid"]
        assert row["precision"] == b["thresholds"][i]["precision"]
        p, r = row["precision"], row["recall"]
        assert row["f_score"] == (2 * p * r / (p + r) if p + r > 0 else 0.0)


def test_pipeline_surface_with_the_restated_fusion(tmp_path):
    pipe, ref, opts = _run(tmp_path, sd.RestatedSurfaceFusion)
    _check(tmp_path, pipe, ref, opts, sd.RestatedSurfaceFusion)
    # the option needs the reference cloud, the mesh, and a fusion object that can measure a surface
    with pytest.raises(ValueError):
        pipe.run_fusion(fusion_factory=sd.RestatedSurfaceFusion, eval_surface=True)
    with pytest.raises(ValueError):
        pipe.run_fusion(fusion_factory=sd.RestatedSurfaceFusion, voxel_size=opts["voxel_size"], eval_cloud=ref, eval_max_dist=1.0,
                        eval_surface=True)
    with pytest.raises(ValueError):
        pipe.run_fusion(fusion_factory=sd.cd.RestatedDistanceFusion, **opts, eval_surface=True)


def test_compare_clouds_surface(tmp_path, monkeypatch, capsys):
    """compare_clouds.py --surface: A a mesh PLY, loaded through set_scene and set_mesh; the block against the direct
    calls; without the option the output is what it was."""
    spec = importlib.util.spec_from_file_location("compare_clouds", os.path.join(REPO, "scripts", "compare_clouds.py"))
    cc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cc)
    v, f = sd.mixed_mesh()
    b = sd.near_queries(v, f, 300, 0.02, seed=12)
    io.write_mesh_ply(str(tmp_path / "a.ply"), v, f)
    io.write_ply(str(tmp_path / "b.ply"), sd.cd.as_points(b))
    make = sd.RestatedSurfaceFusion
    taus = (0.01, 0.03)
    plain = cc.compare(v[:, :3], b, 0.06, taus, make=make)
    got = cc.compare(v[:, :3], b, 0.06, taus, make=make, a_faces=f)
    surface = got.pop("surface")
    assert got == plain and "surface" not in plain
    for name, q in (("completeness", b), ("fidelity", v[:, :3])):
        s = sd.distances(q, v, f, 0.06, [float(F32(t)) for t in taus])[2]
        row = surface[name]
        assert [row["n_query"], row["n_valid"], row["n_matched"]] == s[:3] and row["within"] == s[4:6], name
    assert surface["fidelity"]["n_matched"] == len(v) and surface["fidelity"]["mean"] == 0.0     # vertices lie on their faces
    assert [r["precision"] for r in surface["thresholds"]] == [r["precision"] for r in plain["thresholds"]]
    assert all(r["recall"] >= p["recall"] for r, p in zip(surface["thresholds"], plain["thresholds"]))   # every vertex has a face
    monkeypatch.setattr(cc.capi, "Fusion", lambda device, cams: make(cams))
    assert cc.main([str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), "--max-dist", "0.06", "--threshold", "0.01",
                    "--threshold", "0.03", "--surface"]) == 0
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert printed["surface"] == json.loads(json.dumps(surface))


def test_cli_eval_surface():
    a = pipeline.arg_parser().parse_args(["folder", "--eval-cloud", "gt.ply", "--eval-max-dist", "0.02", "--eval-surface"])
    assert a.eval_surface is True
    assert pipeline.arg_parser().parse_args(["folder"]).eval_surface is False


@pytest.mark.gpu
def test_pipeline_surface_on_the_device(tmp_path):
    factory = lambda cams: capi.Fusion(0, cams)
    pipe, ref, opts = _run(tmp_path, factory)
    _check(tmp_path, pipe, ref, opts, factory)
