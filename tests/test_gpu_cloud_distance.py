"""Nearest-neighbour cloud distances on the GPU (acmmp_fusion_cloud_distance, include/acmmp.h), bit for bit against the
exhaustive restatement (cloud_distance_support): d2, nearest and every word of the summary."""
import numpy as np
import pytest

import cloud_distance_support as cd
import visibility_support as vis
from acmmp import capi
from conftest import assert_bitwise_equal
from fusion_scene_support import fill

pytestmark = pytest.mark.gpu

F32 = np.float32
CAM = np.zeros(1, capi.CAMERA_DTYPE)
CAM["width"], CAM["height"] = 8, 8


def _fusion():
    """A fusion object that needs no view: the clouds come through set_scene / set_mesh / set_reference_cloud."""
    return capi.Fusion(0, CAM)


def _assert_distance(fu, source, direction, want, max_dist=cd.MAX_DIST, taus=cd.TAUS, what=""):
    """One cloud_distance, every output against (d2, nearest, summary) of the restatement.  Returns the bytes read."""
    r = fu.cloud_distance(source, direction, max_dist, taus)
    d2, nn = fu.distance_results(squared=True)
    grid = fu.distance_grid(fu._forced if hasattr(fu, "_forced") else 0.0)
    print(what, source, direction, "queries", r.n_query, "valid", r.n_valid, "matched", r.n_matched, "mean", r.mean, grid)
    assert d2.dtype == F32 and nn.dtype == np.int32
    assert_bitwise_equal(d2, want[0], f"{what}: d2")
    assert np.array_equal(nn, want[1]), f"{what}: nearest"
    assert cd.summary_of(r) == want[2], f"{what}: summary"
    dist, nn2 = fu.distance_results(0, len(nn))
    assert_bitwise_equal(dist, np.sqrt(want[0]), f"{what}: dist")
    return d2.tobytes() + nn.tobytes() + np.array(cd.summary_of(r), np.int64).tobytes()


def _force(fu, cell):
    fu._forced = cell
    fu.distance_grid(cell)


def _scene_pair(offset=0.0):
    Q, T = (c + F32(offset) for c in cd.clouds())
    fu = _fusion()
    assert fu.set_scene(cd.as_points(Q)) == len(Q) and fu.set_reference_cloud(T) == len(T)
    return fu


@pytest.mark.parametrize("direction", cd.DIRECTIONS)
def test_scene_both_directions_twice(direction):
    fu = _scene_pair()
    want = cd.restated(direction)
    first = _assert_distance(fu, "scene", direction, want, what="scene")
    assert _assert_distance(fu, "scene", direction, want, what="again") == first          # two runs: identical bytes
    s = want[2]
    assert 0 < s[2] < s[1] < s[0]
    fu.close()


@pytest.mark.parametrize("direction", cd.DIRECTIONS)
def test_forced_cells(direction):
    """A tiny cell (many rings, the coarse level and the cap end the search), a huge one (every target in one cell) and
    the automatic one: the same bits."""
    fu = _scene_pair()
    want = cd.restated(direction)
    seen = {}
    for name, cell in (("auto", 0.0), ("tiny", cd.MAX_DIST / 12), ("huge", 1e6)):
        _force(fu, cell)
        seen[name] = (_assert_distance(fu, "scene", direction, want, what=name), fu.distance_grid(cell))
    assert seen["auto"][0] == seen["tiny"][0] == seen["huge"][0]
    assert seen["huge"][1]["cells"] == 1 and seen["huge"][1]["rings"] == 0 and seen["huge"][1]["cell"] == F32(1e6)
    assert seen["huge"][1]["max_list"] == int(cd.valid(cd.clouds()[1 if direction == "data_to_ref" else 0]).sum())
    assert seen["tiny"][1]["rings"] >= 12 and seen["tiny"][1]["cells"] > seen["auto"][1]["cells"] > 1
    assert seen["auto"][1]["cell"] == F32(cd.MAX_DIST)                     # the outliers stretch the box: the cap decides
    fu.close()


@pytest.mark.parametrize("direction", cd.DIRECTIONS)
def test_offset_clouds(direction):
    """The same clouds moved by 1e4 on every axis: coordinates 1e-3 apart in float32, ties and duplicates everywhere."""
    fu = _scene_pair(1e4)
    want = cd.restated(direction, 1e4)
    a = _assert_distance(fu, "scene", direction, want, what="offset")
    _force(fu, 0.004)
    assert _assert_distance(fu, "scene", direction, want, what="offset, cell 0.004") == a
    fu.close()


@pytest.mark.parametrize("direction", cd.DIRECTIONS)
def test_cell_indices_near_the_limit(direction):
    """A forced cell of a millionth of the extent: indices near 2^20, where the cell is enlarged to fit; queries beside
    the far target that spans the extent."""
    fu = _scene_pair()
    md = 0.02                                                              # rings of up to 21 cells, not 42
    taus = cd.TAUS[:6]
    want = cd.restated(direction, taus=taus, max_dist=md)
    T = cd.clouds()[1 if direction == "data_to_ref" else 0]
    ext = float((T[cd.valid(T)].max(0).astype(np.float64) - T[cd.valid(T)].min(0)).max())
    _force(fu, ext / 1.04e6)
    _assert_distance(fu, "scene", direction, want, md, taus, what="cell ext / 1.04e6")
    assert fu.distance_grid(0.0)["cell"] == F32(ext / 1.04e6)
    _force(fu, ext / 4e6)                                                  # would need 4e6 cells: enlarged to ext / 2^20
    _assert_distance(fu, "scene", direction, want, md, taus, what="cell ext / 4e6")
    assert fu.distance_grid(0.0)["cell"] == F32(ext / 1048576.0)
    if direction == "data_to_ref":
        beside = np.nonzero((np.abs(cd.clouds()[0] - F32(1000)) < 1).all(1))[0]
        far = int(np.nonzero((cd.clouds()[1] == F32(1000)).all(1))[0][0])
        assert len(beside) == 8 and (want[1][beside] == far).any()         # matched at the top of the index range
    fu.close()


def test_small_and_empty_inputs():
    Q, T = cd.clouds()
    fu = _fusion()
    fu.set_scene(cd.as_points(Q))
    for name, ref in (("single target", T[:1]), ("single far target", np.array([[1000, 1000, 1000]], F32)),
                      ("no target", T[:0]), ("no valid target", np.full((3, 3), np.nan, F32))):
        assert fu.set_reference_cloud(ref) == len(ref)
        for n_tau in (0, 8):
            taus = cd.TAUS[:n_tau]
            _assert_distance(fu, "scene", "data_to_ref", cd.distances(Q, ref, cd.MAX_DIST, taus), taus=taus, what=name)
            _assert_distance(fu, "scene", "ref_to_data", cd.distances(ref, Q, cd.MAX_DIST, taus), taus=taus, what=name)
    fu.set_reference_cloud(T)
    fu.set_scene(np.zeros((0, 9), F32))                                    # no query one way, no target the other
    r = fu.cloud_distance("scene", "data_to_ref", cd.MAX_DIST, cd.TAUS)
    assert cd.summary_of(r) == [0] * cd.SUMMARY_WORDS and len(fu.distance_results()[0]) == 0
    _assert_distance(fu, "scene", "ref_to_data", cd.distances(T, T[:0], cd.MAX_DIST, cd.TAUS), what="empty scene")
    fu.close()


def _chain():
    """A fusion object holding a voxel, a clean and a visible result of the constructed sphere rig."""
    cams, depths, normals, colours, cloud, size = vis.constructed("sphere")
    fu = fill(capi.Fusion(0, cams), cams, depths, normals, colours)
    fu.set_scene(cloud)
    nv = fu.voxelize(size)[0]
    nc = fu.voxel_clean(26, 1, 2, 1)[0]
    nk = fu.voxel_visibility(list(range(len(cams))), 0.01, 1, 1, 0, source="clean")[0]
    assert 0 < nk <= nc < nv
    return fu, size, {"voxels": fu.voxel_points(0, nv), "clean": fu.clean_points(0, nc), "visible": fu.visible_points(0, nk)}


@pytest.mark.parametrize("source", ["voxels", "clean", "visible", "mesh"])
def test_sources(source):
    """Every resident cloud as the data cloud, both directions, against a reference cloud made from the voxel cloud:
    every third voxel moved by about a voxel, every fourth copied."""
    fu, size, data = _chain()
    rng = np.random.default_rng(5)
    V = data["voxels"][:, :3]
    ref = np.concatenate([V[::3] + (F32(size) * rng.standard_normal((len(V[::3]), 3))).astype(F32), V[::4]]).astype(F32)
    fu.set_reference_cloud(ref)
    if source == "mesh":
        data["mesh"] = cd.as_points(cd.clouds()[0])[:1500]
        data["mesh"][:700, :3] = V[:700]
        assert fu.set_mesh(data["mesh"], np.zeros((0, 3), np.int32)) == (1500, 0)
    max_dist = 1.5 * size
    taus = (0.0, 0.5 * size, size)
    for direction in cd.DIRECTIONS:
        q, t = (data[source], ref) if direction == "data_to_ref" else (ref, data[source])
        want = cd.distances(q, t, max_dist, taus)
        assert 0 < want[2][2] < want[2][1]                                 # matched and unmatched queries
        _assert_distance(fu, source, direction, want, max_dist, taus, what=source)
    for name, read in (("voxels", fu.voxel_points), ("clean", fu.clean_points), ("visible", fu.visible_points)):
        assert_bitwise_equal(read(0, len(data[name])), data[name], f"{name} after the distance calls")   # sources untouched
    fu.close()


def _state(fu, n):
    return fu.distance_results(0, n, squared=True)


def test_invalid_arguments_leave_everything():
    Q, T = cd.clouds()
    fu = _scene_pair()
    want = cd.restated("data_to_ref")
    _assert_distance(fu, "scene", "data_to_ref", want, what="before")
    L, h = fu.L, fu.h
    tau = np.array(cd.TAUS, F32)
    p = lambda a: a.ctypes.data
    out = np.zeros(cd.SUMMARY_WORDS, np.int64)

    def call(source=0, direction=0, max_dist=cd.MAX_DIST, n_tau=8, taus=tau):
        return L.acmmp_fusion_cloud_distance(h, source, direction, max_dist, n_tau, None if taus is None else p(taus), p(out))
    bad_tau = lambda v: np.array([0.01, v], F32)
    cases = {"source 5": dict(source=5), "source -1": dict(source=-1), "direction 2": dict(direction=2),
             "no voxel result": dict(source=1), "no clean result": dict(source=2), "no visible result": dict(source=3),
             "no mesh result": dict(source=4), "max_dist 0": dict(max_dist=0.0), "max_dist < 0": dict(max_dist=-1.0),
             "max_dist nan": dict(max_dist=float("nan")), "max_dist inf": dict(max_dist=float("inf")),
             "n_tau 9": dict(n_tau=9), "n_tau -1": dict(n_tau=-1), "tau NULL": dict(n_tau=1, taus=None),
             "tau nan": dict(n_tau=2, taus=bad_tau(np.nan)), "tau < 0": dict(n_tau=2, taus=bad_tau(-0.01)),
             "tau inf": dict(n_tau=2, taus=bad_tau(np.inf)), "tau > max_dist": dict(n_tau=2, taus=bad_tau(0.0401))}

    def unchanged(what):
        d2, nn = _state(fu, len(Q))
        assert_bitwise_equal(d2, want[0], f"after {what}: d2")
        assert np.array_equal(nn, want[1]), f"after {what}: nearest"
        assert_bitwise_equal(fu.scene_points(0, len(Q)), cd.as_points(Q), f"after {what}: scene")
    for what, kw in cases.items():
        assert call(**kw) == 1, what                                       # ACMMP_ERR_INVALID_ARGUMENT
        unchanged(what)
    for cell in (-1.0, float("nan"), float("inf")):                        # a forced cell that is not finite and > 0
        fu.distance_grid(cell)
        assert call() == 1
        unchanged(f"forced cell {cell}")
    fu.distance_grid(0.0)
    # the reference cloud's own arguments
    assert L.acmmp_fusion_set_reference_cloud(h, -1, p(T)) == 1 and L.acmmp_fusion_set_reference_cloud(h, 3, None) == 1
    assert L.acmmp_fusion_set_reference_cloud(h, 2 ** 31, p(T)) == 1
    unchanged("set_reference_cloud")
    for first, n in ((0, len(Q) + 1), (len(Q), 1), (-1, 1), (0, -1)):
        assert L.acmmp_fusion_distance_results(h, first, n, None, None) == 1
    assert L.acmmp_fusion_distance_results(h, len(Q), 0, None, None) == 0
    assert call() == 0 and out.tolist() == want[2]                         # and the call still works
    # no reference cloud at all
    fresh = _fusion()
    fresh.set_scene(cd.as_points(Q[:10]))
    with pytest.raises(capi.AcmmpError):
        fresh.cloud_distance("scene", "data_to_ref", 1.0)
    with pytest.raises(capi.AcmmpError):
        fresh.distance_results(0, 1)
    fresh.close()
    fu.close()


def test_lifetimes():
    fu, size, data = _chain()
    ref = data["voxels"][::2, :3] + F32(0.25 * size)
    fu.set_reference_cloud(ref)
    gone = lambda: fu.L.acmmp_fusion_distance_results(fu.h, 0, 1, None, None) == 1
    run = lambda source: fu.cloud_distance(source, "data_to_ref", size, (size,))
    cams, depths, normals, colours = vis.constructed("sphere")[:4]
    r = run("voxels")
    assert r.n_query == len(data["voxels"]) and not gone()
    fu.set_view(0, depths[0], normals[0], colours[0])                      # kept across set_view
    assert not gone()
    fu.voxel_clean(26, 1, 2, 1)                                            # a clean leaves a result of the voxel cloud alone
    assert not gone()
    fu.set_reference_cloud(ref)                                            # discarded with the reference cloud
    assert gone()
    run("voxels")
    fu.voxelize(size)                                                      # discarded when voxelize replaces its source
    assert gone()
    fu.voxel_clean(26, 1, 2, 1)
    run("clean")
    fu.voxel_clean(26, 1, 2, 1)                                            # a clean replaces the clean cloud
    assert gone()
    fu.voxel_visibility([0, 1], 0.01, 1, 1, 0, source="clean")
    run("visible")
    fu.voxel_visibility([0, 1], 0.01, 1, 1, 0, source="clean")
    assert gone()
    run("visible")
    fu.voxel_clean(26, 1, 2, 1)                                            # the visible cloud goes with the clean cloud
    assert gone()
    fu.set_mesh(data["voxels"][:100], np.zeros((0, 3), np.int32))
    run("mesh")
    scene = fu.scene_points(0, 50)
    fu.set_scene(scene)                                                    # a set mesh outlives the scene, and so does its result
    assert not gone()
    fu.set_mesh(data["voxels"][:100], np.zeros((0, 3), np.int32))
    assert gone()
    run("scene")
    fu.set_mesh(data["voxels"][:10], np.zeros((0, 3), np.int32))           # another source's replacement does not touch it
    assert not gone()
    fu.set_scene(scene)
    assert gone()
    fu.close()
