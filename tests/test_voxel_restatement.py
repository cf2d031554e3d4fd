"""The voxel-grid reduction, the parts that need no GPU: the numpy restatement (voxel_support) held to properties
it cannot fake, the conditions that make the GPU cases of test_gpu_voxel.py meaningful, and Pipeline.run_fusion's
voxel path and command line driven by RestatedVoxelFusion."""
import numpy as np
import pytest

import voxel_support as vs
from acmmp import io, pipeline
from conftest import assert_bitwise_equal
from pipeline_support import OracleEngine, OracleFusion, small_dataset

F32 = np.float32


def _random_cloud(n=4000, seed=1, spread=3.0):
    rng = np.random.default_rng(seed)
    pts = np.zeros((n, 9), F32)
    pts[:, :3] = rng.uniform(-spread, spread, size=(n, 3))
    pts[:, 3:6] = rng.normal(size=(n, 3))
    pts[:, 6:9] = rng.uniform(0, 255, size=(n, 3))
    return pts


@pytest.mark.parametrize("name", ["rig_256x128", "rig_50x30", "rig_50x30_edges"])
@pytest.mark.parametrize("which", ["coarse", "middle", "fine"])
def test_invariants(name, which):
    pts = vs.oracle_cloud(name)
    size = F32(vs.scene_sizes(name, pts)[which])
    v = vs.voxelize(pts, size)
    P, n, o = v["points"], v["counts"].astype(np.int64), v["origin"]
    N = pts.shape[0]
    assert n.sum() == N - v["n_rejected"] and len(n) == v["n_occupied"] and (n >= 1).all()
    # order of first appearance, and `first` really is a point of the voxel
    assert (np.diff(v["first"]) > 0).all() and v["first"][0] == np.flatnonzero(vs.cells(pts, size, o)[0])[0]
    acc, keys, _ = vs.cells(pts, size, o)
    assert np.array_equal(keys[np.searchsorted(np.flatnonzero(acc), v["first"])], v["keys"])
    # every centroid lies in its cell (closed: the float32 rounding of the position may land on a face)
    cell = np.stack([((v["keys"] >> np.uint64(21 * a)) & np.uint64(vs.CELLS - 1)).astype(np.float64) for a in range(3)], 1)
    lo = o.astype(np.float64) + cell * np.float64(size)
    tol = np.spacing(np.abs(P[:, :3]).astype(F32)).astype(np.float64)
    assert (P[:, :3] >= lo - tol).all() and (P[:, :3] <= lo + np.float64(size) + tol).all()
    # the key of a centroid is the voxel's key, but for round trips that land on a face
    back_acc, back_keys, _ = vs.cells(P, size, o)
    off = int((~back_acc).sum()) + int((back_keys != v["keys"][back_acc]).sum())
    print(name, which, "voxels", len(n), "face round trips", off)
    assert off <= 0.01 * len(n)
    # min_points = m is the min_points = 1 result filtered
    for m in (2, 3):
        w = vs.voxelize(pts, size, min_points=m)
        sel = n >= m
        assert_bitwise_equal(w["points"], P[sel], f"min_points {m}")
        assert np.array_equal(w["counts"], v["counts"][sel]) and w["n_occupied"] == v["n_occupied"]
        assert w["n_rejected"] == v["n_rejected"]


def test_distinct_cells_return_the_cloud():
    """One point per cell: the output is the input to within the quantisation, in the input's order."""
    rng = np.random.default_rng(7)
    size = F32(0.25)
    g = rng.permutation(40 * 40 * 40)[:5000]
    pts = _random_cloud(5000, seed=2)
    pts[:, :3] = (np.stack([g % 40, (g // 40) % 40, g // 1600], 1) + rng.uniform(0.05, 0.95, size=(5000, 3))) * size - 4.0
    v = vs.voxelize(pts, size, origin=[-4, -4, -4])
    assert v["points"].shape[0] == 5000 and (v["counts"] == 1).all() and v["n_rejected"] == 0
    assert np.abs(v["points"][:, :3].astype(np.float64) - pts[:, :3]).max() <= float(size) / 65536
    assert np.abs(v["points"][:, 3:].astype(np.float64) - pts[:, 3:]).max() <= 2.0 ** -17
    assert np.array_equal(v["first"], np.arange(5000))


def test_rejection_and_sums_by_hand():
    pts = np.zeros((7, 9), F32)
    pts[:, 3] = [1, 2, 3, 4, 5, 6, 7]
    pts[:, 0] = [0.25, 0.75, 1.5, np.nan, 0.5, -0.5, 0.5]
    pts[4, 5] = np.inf                       # non-finite normal
    pts[6, 8] = F32(2 ** 20 + 1)             # colour too large
    v = vs.voxelize(pts, 1.0, origin=[0, 0, 0])
    assert v["n_rejected"] == 4 and v["n_occupied"] == 2          # NaN, inf, x < origin, magnitude
    assert v["counts"].tolist() == [2, 1]
    assert_bitwise_equal(v["points"][:, 0], np.array([0.5, 1.5], F32), "centroid x")
    assert_bitwise_equal(v["points"][:, 3], np.array([1.5, 3.0], F32), "mean nx")
    auto = vs.voxelize(pts, 1.0)
    assert_bitwise_equal(auto["origin"], np.array([-0.5, 0, 0], F32), "minimum over the finite points")
    assert auto["n_rejected"] == 3
    # -0 orders below +0 in the automatic origin; an all-rejected cloud has origin 0 and no voxel
    z = np.zeros((2, 9), F32)
    z[1, 0] = -0.0
    assert np.signbit(vs.voxelize(z, 1.0)["origin"][0])
    bad = np.full((3, 9), np.nan, F32)
    e = vs.voxelize(bad, 1.0)
    assert e["points"].shape == (0, 9) and e["n_rejected"] == 3 and not e["origin"].any()
    assert vs.voxelize(np.zeros((0, 9), F32), 1.0)["points"].shape == (0, 9)
    # round half to even in the quantisation
    h = np.zeros((2, 9), F32)
    h[:, 3] = [0.5 / 65536, 1.5 / 65536]
    assert vs.voxelize(h[:1], 1.0)["points"][0, 3] == 0.0 and vs.voxelize(h[1:], 1.0)["points"][0, 3] == F32(2.0 / 65536)


def test_table_layout_by_hand():
    """Keys chosen by their home slot: a run that crosses the end of a 64-slot table wraps, in any order."""
    keys = np.arange(1, 200000, dtype=np.uint64)
    home = (vs.splitmix64(keys) >> np.uint64(58)).astype(np.int64)
    pick = lambda h, k: keys[home == h][:k]
    ks = np.concatenate([pick(63, 3), pick(62, 2), pick(5, 2)])
    assert vs.table_layout(ks, 64) == (7, 3)            # five keys homed at 62 and 63: three of them land at 0, 1, 2
    assert vs.table_layout(ks[::-1], 64) == (7, 3)
    assert vs.table_layout(np.concatenate([ks, ks]), 64) == (7, 3)
    assert vs.table_layout(pick(5, 4), 64) == (4, 0)
    rng = np.random.default_rng(0)
    many = rng.choice(keys, 50, replace=False)
    assert len({vs.table_layout(rng.permutation(many), 64) for _ in range(20)}) == 1     # independent of the order


@pytest.mark.parametrize("name", list(vs.SCENES))
def test_input_conditions(name):
    """What makes the GPU cases meaningful, asserted on the oracle's cloud of every scene."""
    pts = vs.oracle_cloud(name)
    N = pts.shape[0]
    sizes = vs.scene_sizes(name, pts)
    got = {k: vs.voxelize(pts, s) for k, s in sizes.items()}
    print(name, "points", N, {k: (v["points"].shape[0], v["n_rejected"], int(v["counts"].max())) for k, v in got.items()})
    assert N > 0
    assert got["single"]["points"].shape[0] == 1 and got["single"]["counts"][0] == N and got["single"]["n_rejected"] == 0
    for k in ("coarse", "middle", "fine"):
        assert got[k]["points"].shape[0] > 1 and got[k]["n_rejected"] == 0
    assert got["coarse"]["points"].shape[0] < got["middle"]["points"].shape[0] <= got["fine"]["points"].shape[0]
    assert (got["middle"]["counts"] >= 3).any() and (got["middle"]["counts"] == 1).any()
    assert (got["fine"]["counts"] > 1).any()
    assert 0 < got["overflow"]["n_rejected"] < N                      # an index at or beyond 2^21
    centred = vs.voxelize(pts, sizes["middle"], origin=[0, 0, 0])
    print(name, "centred origin", centred["points"].shape[0], "voxels", centred["n_rejected"], "rejected")
    assert 0 < centred["n_rejected"] < N                              # negative indices
    assert vs.voxelize(pts, sizes["middle"], min_points=3)["points"].shape[0] < got["middle"]["points"].shape[0]


@pytest.mark.parametrize("name", list(vs.FORCED_TABLES))
def test_forced_tables_wrap(name):
    pts = vs.oracle_cloud(name)
    size, slots = vs.FORCED_TABLES[name]
    assert slots > pts.shape[0] >= slots // 2                         # the smallest admissible power of two
    occupied, wrapped = vs.table_layout(vs.scene_keys(pts, size), slots)
    print(name, size, slots, "occupied", occupied, "wrapped", wrapped)
    assert occupied == vs.voxelize(pts, size)["n_occupied"] and wrapped > 0
    assert vs.auto_slots(pts.shape[0]) == 2 * slots


def test_pipeline_voxel_path_with_stub(tmp_path):
    ds = small_dataset(64, 32, 3)
    pipe = pipeline.Pipeline(ds, engine=OracleEngine(), order="reference", geom_iterations=1).run()
    plain = pipe.run_fusion(fusion_factory=vs.RestatedVoxelFusion, ply_path=str(tmp_path / "plain.ply"))
    per_view = pipe.run_fusion(fusion_factory=OracleFusion, ply_path=str(tmp_path / "views.ply"))
    assert pipe.fusion_info is None
    assert (tmp_path / "plain.ply").read_bytes() == (tmp_path / "views.ply").read_bytes()    # the default call is today's
    assert_bitwise_equal(plain, per_view, "default call")
    ok = vs.finite_points(plain)
    size = float((plain[ok, :3].max(0) - plain[ok, :3].min(0)).max()) / 16
    for unique, m in ((False, 1), (False, 2), (True, 1)):
        made = []

        def factory(cams):
            made.append(vs.RestatedVoxelFusion(cams))
            return made[-1]
        got = pipe.run_fusion(fusion_factory=factory, ply_path=str(tmp_path / "voxel.ply"), unique=unique, chunk_points=5,
                              voxel_size=size, voxel_min_points=m)
        scene = made[0].result[0]
        want = vs.voxelize(scene, size, min_points=m)
        assert 1 < want["points"].shape[0] < scene.shape[0]
        assert_bitwise_equal(got, want["points"], "voxel cloud")
        assert pipe.fused is got
        io.write_ply(str(tmp_path / "want.ply"), want["points"])
        assert (tmp_path / "voxel.ply").read_bytes() == (tmp_path / "want.ply").read_bytes()
        assert io.read_ply(str(tmp_path / "voxel.ply")).shape[0] == want["points"].shape[0]
        info = pipe.fusion_info
        assert (info["scene_points"], info["voxels"], info["rejected"]) == (scene.shape[0], want["points"].shape[0],
                                                                           want["n_rejected"])
        if not unique:
            assert scene.shape[0] == plain.shape[0]
    # above the caller's limit the voxel cloud is streamed only; the limit applies to it, not to the scene cloud
    n_vox = vs.voxelize(plain, size)["points"].shape[0]
    kept = pipe.run_fusion(fusion_factory=vs.RestatedVoxelFusion, ply_path=str(tmp_path / "kept.ply"), voxel_size=size,
                           max_host_points=n_vox)
    assert kept.shape[0] == n_vox < plain.shape[0]
    assert pipe.run_fusion(fusion_factory=vs.RestatedVoxelFusion, ply_path=str(tmp_path / "streamed.ply"),
                           voxel_size=size, max_host_points=n_vox - 1) is None
    assert pipe.fused is None and pipe.fusion_info["voxels"] == n_vox
    assert (tmp_path / "streamed.ply").read_bytes() == (tmp_path / "kept.ply").read_bytes()
    # fusion objects without voxelize are refused when a size is given
    with pytest.raises(ValueError):
        pipe.run_fusion(fusion_factory=OracleFusion, voxel_size=size)
    with pytest.raises(ValueError):
        pipe.run_fusion(fusion_factory=vs.RestatedFusion, voxel_size=size)


def test_command_line_flags_parse():
    a = pipeline.arg_parser().parse_args(["folder", "--voxel-size", "0.05", "--voxel-min-points", "3"])
    assert a.voxel_size == 0.05 and a.voxel_min_points == 3 and not a.unique_fusion
    d = pipeline.arg_parser().parse_args(["folder"])
    assert d.voxel_size is None and d.voxel_min_points == 1
