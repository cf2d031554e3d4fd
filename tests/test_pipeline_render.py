"""Pipeline.run_fusion's render options (CPU, through the restated fusion): the .dmb files, the untouched outputs."""
import os

import numpy as np
import pytest

import mesh_render_support as rs
import voxel_mesh_support as ms
import voxel_support as vs
from acmmp import io, pipeline
from conftest import assert_bitwise_equal
from fusion_scene_support import dataset_inputs
from pipeline_support import OracleEngine, small_dataset


class _Recording(rs.RestatedRenderFusion):
    """RestatedRenderFusion that keeps what render_mesh and render_maps handed out."""
    seen = None

    def render_mesh(self, view=None, camera=None, rel_tol=0.01):
        out = super().render_mesh(view, camera, rel_tol)
        type(self).seen.append([view, rel_tol, out, None])
        return out

    def render_maps(self):
        out = super().render_maps()
        type(self).seen[-1][3] = [a.copy() for a in out]
        return out


def test_pipeline_render_with_the_restated_fusion(tmp_path):
    ds = small_dataset(64, 32, 3)
    folder = str(tmp_path / "out")
    pipe = pipeline.Pipeline(ds, engine=OracleEngine(), order="reference", geom_iterations=1, out_folder=folder).run()
    plain = pipe.run_fusion(fusion_factory=ms.RestatedMeshFusion)
    ok = vs.finite_points(plain)
    size = float((plain[ok, :3].max(0) - plain[ok, :3].min(0)).max()) / 16
    kw = dict(voxel_size=size, mesh_trunc=3 * size)
    pipe.run_fusion(fusion_factory=ms.RestatedMeshFusion, ply_path=str(tmp_path / "cloud.ply"), mesh_path=str(tmp_path / "mesh.ply"), **kw)
    before = dict(pipe.fusion_info)
    dmbs = lambda: sorted(os.path.join(d, f) for d, _, fs in os.walk(folder) for f in fs if f.endswith("_mesh.dmb"))
    assert dmbs() == []                                                  # the defaults write nothing new
    _Recording.seen = []
    got = pipe.run_fusion(fusion_factory=_Recording, ply_path=str(tmp_path / "cloud2.ply"), mesh_path=str(tmp_path / "mesh2.ply"),
                          render_mesh=True, render_tol=0.05, **kw)
    info = pipe.fusion_info
    # every existing output is byte for byte what it is without the option
    assert (tmp_path / "cloud2.ply").read_bytes() == (tmp_path / "cloud.ply").read_bytes()
    assert (tmp_path / "mesh2.ply").read_bytes() == (tmp_path / "mesh.ply").read_bytes()
    assert {k: v for k, v in info.items() if not k.startswith("render")} == before
    assert_bitwise_equal(got, pipe.fused, "cloud")
    # one render per view, in problem order, at the tolerance asked; its maps are the files
    assert [s[0] for s in _Recording.seen] == [0, 1, 2] and all(s[1] == 0.05 for s in _Recording.seen)
    assert info["render_tol"] == 0.05 and len(info["render_views"]) == 3 and len(dmbs()) == 6
    for k, (prob, seen) in enumerate(zip(pipe.problems, _Recording.seen)):
        d = os.path.join(folder, "ACMMP", f"2333_{prob.ref_image_id:08d}")
        assert os.path.exists(os.path.join(d, "depths.dmb"))
        depth, _, normal, _ = seen[3]
        assert_bitwise_equal(io.read_dmb(os.path.join(d, "depths_mesh.dmb")), depth, "depths_mesh.dmb")
        assert_bitwise_equal(io.read_dmb(os.path.join(d, "normals_mesh.dmb")), normal, "normals_mesh.dmb")
        row = info["render_views"][k]
        assert row["view"] == prob.ref_image_id and row["skipped"] == seen[2]["skipped"]
        assert {n: row[n] for n in rs.COUNTS} == seen[2]["counts"]
        assert sum(row[n] for n in rs.COUNTS[:6]) == depth.size and (depth > 0).sum() > 0
    # render_mesh needs the mesh, and a fusion object that can render
    with pytest.raises(ValueError):
        pipe.run_fusion(fusion_factory=_Recording, voxel_size=size, render_mesh=True)
    with pytest.raises(ValueError):
        pipe.run_fusion(fusion_factory=_Recording, render_mesh=True)
    with pytest.raises(ValueError):
        pipe.run_fusion(fusion_factory=ms.RestatedMeshFusion, render_mesh=True, **kw)


def test_cli_render_options():
    a = pipeline.arg_parser().parse_args(["folder", "--voxel-size", "0.1", "--mesh", "m.ply", "--render-mesh", "--render-tol", "0.02"])
    assert (a.render_mesh, a.render_tol) == (True, 0.02)
    a = pipeline.arg_parser().parse_args(["folder"])
    assert (a.render_mesh, a.render_tol) == (False, 0.01)


def test_restated_set_mesh_lifetimes():
    """The restated object keeps capi.Fusion's rules: a set mesh outlives the scene, a render goes with its mesh."""
    cams, depths, normals, colours = dataset_inputs("pinhole")
    rf = rs.RestatedRenderFusion(cams)
    for k in range(len(cams)):
        rf.set_view(k, depths[k], normals[k], colours[k])
    with pytest.raises(ValueError):
        rf.render_mesh(0)
    V, T = rs.as_mesh([(-1, -1, 3), (1, -1, 3), (0, 1, 3)], [(0, 1, 2)])
    rf.set_mesh(V, T)
    rf.render_mesh(0)
    first = rf.render_maps()
    rf.set_scene(np.zeros((1, 9), np.float32))
    assert rf.render_maps()[0].tobytes() == first[0].tobytes()
    rf.set_mesh(V, T)
    with pytest.raises(ValueError):
        rf.render_maps()
    for bad in (dict(view=None), dict(view=7), dict(view=0, rel_tol=-1.0), dict(view=0, camera=cams[0])):
        with pytest.raises(ValueError):
            rf.render_mesh(**bad)
    with pytest.raises(ValueError):
        rf.set_mesh(V, [(0, 1, 3)])
