"""The mesh above the ABI: io's mesh PLY writer (CPU) and Pipeline.run_fusion's mesh options on the GPU."""
import numpy as np
import pytest

import voxel_mesh_support as ms
import voxel_support as vs
from acmmp import capi, io, pipeline
from conftest import assert_bitwise_equal
from pipeline_support import small_dataset


def _mesh():
    rng = np.random.default_rng(5)
    v = rng.normal(size=(7, 9)).astype(np.float32)
    v[:, 6:] = rng.integers(0, 256, (7, 3))
    v[2, 0] = np.inf                                                   # written as 0, as write_ply does
    return v, np.array([[0, 1, 2], [2, 1, 3], [6, 5, 4], [0, 6, 3]], np.int32)


def test_mesh_ply_round_trip(tmp_path):
    v, t = _mesh()
    io.write_mesh_ply(str(tmp_path / "m.ply"), v, t)
    io.write_ply(str(tmp_path / "c.ply"), v)
    got_v, got_t = io.read_mesh_ply(str(tmp_path / "m.ply"))
    assert got_v.tobytes() == io.read_ply(str(tmp_path / "c.ply")).tobytes() and got_v["x"][2] == 0
    assert got_t.dtype == np.int32 and np.array_equal(got_t, t)
    data = (tmp_path / "m.ply").read_bytes()
    head = data[:data.index(b"end_header\n")].decode()
    assert "element vertex 7" in head and "element face 4" in head and "property list uchar int vertex_indices" in head
    assert len(data) == len(head) + len("end_header\n") + 7 * 27 + 4 * 13
    assert io.read_ply(str(tmp_path / "m.ply")).tobytes() == got_v.tobytes()          # a cloud reader sees the vertices
    # streamed in pieces: the same bytes
    with io.MeshPlyWriter(str(tmp_path / "s.ply"), 7, 4) as w:
        w.write_vertices(v[:3]), w.write_vertices(v[3:])
        w.write_faces(t[:1]), w.write_faces(t[1:])
    assert (tmp_path / "s.ply").read_bytes() == data
    io.write_mesh_ply(str(tmp_path / "e.ply"), np.zeros((0, 9), np.float32), np.zeros((0, 3), np.int32))
    ev, et = io.read_mesh_ply(str(tmp_path / "e.ply"))
    assert ev.shape == (0,) and et.shape == (0, 3)


def test_mesh_ply_checks_counts(tmp_path):
    v, t = _mesh()
    path = str(tmp_path / "m.ply")
    with pytest.raises(ValueError):
        with io.MeshPlyWriter(path, 8, 4) as w:                        # a vertex short
            w.write_vertices(v)
    with pytest.raises(ValueError):
        with io.MeshPlyWriter(path, 7, 4) as w:                        # faces before the last vertex
            w.write_vertices(v[:6])
            w.write_faces(t)
    with pytest.raises(ValueError):
        with io.MeshPlyWriter(path, 7, 5) as w:                        # a face short
            w.write_vertices(v)
            w.write_faces(t)
    with pytest.raises(ValueError):
        with io.MeshPlyWriter(path, 7, 3) as w:                        # a face too many
            w.write_vertices(v)
            w.write_faces(t)
    with pytest.raises(ValueError):
        with io.MeshPlyWriter(path, 6, 4) as w:                        # a vertex too many
            w.write_vertices(v)
    with pytest.raises(ValueError):
        io.write_mesh_ply(path, v, np.array([[0, 1, 7]], np.int32))    # an index outside the vertices
    with pytest.raises(ValueError):
        io.write_mesh_ply(path, v, np.array([[0, -1, 2]], np.int32))


def test_cli_mesh_options():
    a = pipeline.arg_parser().parse_args(["folder", "--voxel-size", "0.1", "--mesh", "out.ply", "--mesh-trunc", "0.4",
                                          "--mesh-min-weight", "2"])
    assert (a.mesh, a.mesh_trunc, a.mesh_min_weight) == ("out.ply", 0.4, 2)
    a = pipeline.arg_parser().parse_args(["folder"])
    assert (a.mesh, a.mesh_trunc, a.mesh_min_weight) == (None, None, 1)


class _Recording(capi.Fusion):
    """capi.Fusion that keeps what mesh_vertices and mesh_faces handed out."""
    seen = None

    def mesh_vertices(self, first, n):
        out = super().mesh_vertices(first, n)
        type(self).seen["vertices"].append(out.copy())
        return out

    def mesh_faces(self, first, n):
        out = super().mesh_faces(first, n)
        type(self).seen["faces"].append(out.copy())
        return out


@pytest.mark.gpu
def test_pipeline_mesh_fusion(tmp_path):
    ds = small_dataset(64, 32, 3)
    pipe = pipeline.Pipeline(ds, order="reference", geom_iterations=1).run()
    plain = pipe.run_fusion(ply_path=str(tmp_path / "plain.ply"))
    ok = vs.finite_points(plain)
    size = float((plain[ok, :3].max(0) - plain[ok, :3].min(0)).max()) / 16
    for kw in (dict(), dict(voxel_min_neighbours=1, voxel_min_component_voxels=3),
               dict(voxel_min_neighbours=1, visibility_tol=0.05, visibility_radius=1)):
        cloud = pipe.run_fusion(ply_path=str(tmp_path / "cloud.ply"), voxel_size=size, **kw)
        cloud_info = dict(pipe.fusion_info)
        assert not any(k.startswith("mesh") for k in cloud_info)
        _Recording.seen = {"vertices": [], "faces": []}
        got = pipe.run_fusion(fusion_factory=lambda c: _Recording(pipe.device, c), ply_path=str(tmp_path / "with.ply"),
                              chunk_points=7, voxel_size=size, mesh_trunc=3 * size, mesh_min_weight=1,
                              mesh_path=str(tmp_path / "mesh.ply"), **kw)
        info = dict(pipe.fusion_info)
        print(kw, info)
        # the cloud and its PLY are what they are without the mesh options
        assert_bitwise_equal(got, cloud, "cloud")
        assert (tmp_path / "with.ply").read_bytes() == (tmp_path / "cloud.ply").read_bytes()
        rounds = lambda d: {k: v for k, v in d.items() if k != "rounds" and not k.startswith("mesh")}
        assert rounds(info) == rounds(cloud_info)
        # the mesh PLY holds mesh_vertices and mesh_faces
        V = np.concatenate(_Recording.seen["vertices"], 0)
        T = np.concatenate(_Recording.seen["faces"], 0)
        assert 0 < V.shape[0] == info["mesh_vertices"] and 0 < T.shape[0] == info["mesh_faces"]
        assert len(_Recording.seen["vertices"]) > 1 and len(_Recording.seen["faces"]) > 1        # streamed in chunks
        io.write_mesh_ply(str(tmp_path / "direct.ply"), V, T)
        assert (tmp_path / "mesh.ply").read_bytes() == (tmp_path / "direct.ply").read_bytes()
        rv, rt = io.read_mesh_ply(str(tmp_path / "mesh.ply"))
        assert np.array_equal(rt, T) and np.array_equal(rv["x"], V[:, 0]) and np.array_equal(rv["nz"], V[:, 5])
        # and the restatement gives the same file and the same counts
        pipe.run_fusion(fusion_factory=ms.RestatedMeshFusion, voxel_size=size, mesh_trunc=3 * size,
                        mesh_path=str(tmp_path / "restated.ply"), **kw)
        assert (tmp_path / "mesh.ply").read_bytes() == (tmp_path / "restated.ply").read_bytes()
        assert {k: v for k, v in pipe.fusion_info.items() if k.startswith("mesh")} == {k: v for k, v in info.items() if k.startswith("mesh")}
    with pytest.raises(ValueError):
        pipe.run_fusion(mesh_trunc=0.1)                                 # the mesh needs voxel_size
    with pytest.raises(ValueError):
        pipe.run_fusion(voxel_size=size, mesh_path=str(tmp_path / "x.ply"))   # and mesh_trunc
