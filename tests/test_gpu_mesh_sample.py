"""Area-uniform samples of the mesh on the GPU (acmmp_fusion_mesh_sample, include/acmmp.h), bit for bit against the numpy
restatement (mesh_sample_support): all 9 floats of every sample, face, n_samples and n_skipped; then the samples as the
source "samples" of cloud_distance, cloud_align and cloud_align_plane against those calls' restatements fed with the
restated samples; the refusals and the lifetimes."""
import functools

import numpy as np
import pytest

import cloud_align_plane_support as cap
import cloud_align_support as ca
import cloud_distance_support as cd
import mesh_sample_support as mss
import surface_distance_support as sd
import visibility_support as vis
from acmmp import capi
from conftest import assert_bitwise_equal
from fusion_scene_support import fill

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
CAM = np.zeros(1, capi.CAMERA_DTYPE)
CAM["width"], CAM["height"] = 8, 8
TOP = 2 ** 64 - 1
TINY_SEED = 3                                                      # see test_case_properties


def _fusion():
    return capi.Fusion(0, CAM)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(vertices, faces, spacing) of a named case."""
    tiny = mss.spacing_for(*mss.tiny_faces(), 0.3)
    if name == "empty":
        return sd.cube()[0], sd.cube()[1][:0], 0.1
    if name == "all invalid":
        return (*mss.all_invalid(), 0.1)
    if name == "tiny":
        return (*mss.tiny_faces(), tiny)
    if name == "square":
        return (*mss.square(), float(F32(np.sqrt(1.0 / 200000))))
    if name.startswith("embedded "):
        return (*mss.embedded(name.split()[1]), tiny)
    if name == "bad faces":
        return (*mss.with_bad_faces(), 0.05)
    if name == "cube + 1e4":
        return (*mss.moved_cube(), 0.05)
    v, f, size = sd.rig_mesh()
    return v, f, {"rig half voxel": 0.5 * size, "rig two voxels": 2.0 * size}[name]


CASES = [("empty", 0), ("all invalid", 0), ("tiny", TINY_SEED), ("square", 0), ("square", TOP), ("embedded front", 0),
         ("embedded middle", TOP), ("embedded end", 3), ("bad faces", 0), ("bad faces", TOP), ("cube + 1e4", 0),
         ("rig half voxel", 0), ("rig two voxels", TOP)]


@functools.lru_cache(maxsize=None)
def _want(name, seed):
    v, f, spacing = _case(name)
    return mss.sample(v, f, spacing, seed)


def test_case_properties():
    """What the cases are there for, checked on the restatement."""
    v, f, spacing = _case("tiny")
    n, _ = mss.counts(v, f, spacing, TINY_SEED)
    assert n[0] == 0 and n[-1] == 0 and 200 < n.sum() < 400 and n.max() >= 1      # runs of faces without samples
    gaps = np.diff(np.nonzero(n)[0])
    assert gaps.max() >= 8 and (gaps == 1).any()
    pts, face, _ = _want("square", 0)
    assert 199000 < len(pts) < 201000 and (np.bincount(face) > 256 * 300).all()   # a face spans hundreds of workgroups
    for where, seed in (("front", 0), ("middle", TOP), ("end", 3)):
        n, _ = mss.counts(*_case("embedded " + where), seed)
        at = {"front": 0, "middle": 500, "end": 1000}[where]
        assert (n[at:at + 2] > 500).all() and n.sum() - n[at:at + 2].sum() < 400
    for name in ("rig half voxel", "rig two voxels"):
        v, f, spacing = _case(name)
        ok, e = mss.expected(v, f, spacing)
        print(name, "faces", len(f), "mean e", e.mean())
        assert (0.5 < e.mean() < 8) if "half" in name else (e.mean() < 0.5)


def _assert_samples(fu, want, spacing, seed, what):
    r = fu.mesh_sample(spacing, seed)
    pts, face = fu.sample_points()
    print(what, "samples", r.n_samples, "skipped", r.n_skipped)
    assert (r.n_samples, r.n_skipped) == (len(want[0]), want[2]), what
    assert pts.dtype == F32 and face.dtype == np.int32 and pts.shape == (len(want[0]), 9)
    assert np.array_equal(face, want[1]), f"{what}: face"
    assert_bitwise_equal(pts, want[0], f"{what}: points")
    return pts.tobytes() + face.tobytes()


def _reference(pts, md):
    """About 300 reference points: samples moved by md / 8, a few uniform ones in the box, one that is not finite."""
    rng = np.random.default_rng(len(pts))
    ok = np.isfinite(pts[:, :3]).all(1)
    if not ok.any():
        return rng.random((50, 3), dtype=F32)
    p = pts[ok, :3]
    sub = p[:: max(1, len(p) // 280)][:280] + F32(md / 8)
    lo, hi = p.min(0), p.max(0)
    box = (lo + (hi - lo) * rng.random((20, 3), dtype=F32)).astype(F32)
    return np.ascontiguousarray(np.concatenate([sub, box, [[np.nan, 0, 0]]]).astype(F32))


def _assert_consumers(fu, pts, what):
    """The sample result held by fu as the source "samples", against the restatements fed with the restated samples."""
    ok = np.isfinite(pts[:, :3]).all(1)
    ext = float((pts[ok, :3].max(0) - pts[ok, :3].min(0)).max()) if ok.any() else 1.0
    md = float(F32(0.1 * ext))
    taus = tuple(float(F32(t * md)) for t in (0.0, 0.125, 0.5, 1.0))
    ref = _reference(pts, md)
    fu.set_reference_cloud(ref)
    for direction in cd.DIRECTIONS:
        q, t = (pts, ref) if direction == "data_to_ref" else (ref, pts)
        want = cd.distances(q, t, md, taus, rows=32)
        r = fu.cloud_distance("samples", direction, md, taus)
        d2, nn = fu.distance_results(squared=True)
        assert_bitwise_equal(d2, want[0], f"{what} {direction}: d2")
        assert np.array_equal(nn, want[1]), f"{what} {direction}: nearest"
        assert cd.summary_of(r) == want[2], f"{what} {direction}: summary"
        if len(pts):
            assert want[2][2] > 0, f"{what} {direction}: nothing matched"
    stride = max(1, len(pts) // 1500)
    r = fu.cloud_align("samples", "rigid", md, 2, stride)
    assert 1 <= r.iterations <= 2
    for k, rec in enumerate(r.records):
        want = ca.iteration_record(rec.M, pts, ref, md, stride)            # under the device's own M_k
        assert [int(x) for x in rec.words] == want, f"{what}: align iteration {k}"
    p = fu.cloud_align_plane("samples", md, 1, stride)
    rec = p.records[0]
    assert [int(x) for x in rec.words] == cap.iteration_record(rec.M, rec.pivot, pts, ref, md, stride), f"{what}: plane record"
    if len(pts) > 100:
        assert rec.n_pairs > 0 and rec.n_no_normal == 0


@pytest.mark.parametrize("name,seed", CASES)
def test_samples_and_consumers(name, seed):
    v, f, spacing = _case(name)
    want = _want(name, seed)
    fu = _fusion()
    fu.set_mesh(v, f)
    first = _assert_samples(fu, want, spacing, seed, name)
    _assert_consumers(fu, want[0], name)
    assert _assert_samples(fu, want, spacing, seed, name + " again") == first     # two runs: identical bytes
    if len(want[0]) and seed != 1:
        other = fu.mesh_sample(spacing, 1)
        assert abs(other.n_samples - len(want[0])) < 6 * np.sqrt(len(f)) + 1
        assert fu.sample_points()[0].tobytes() != first[:36 * len(want[0])]
    # ranges
    n = len(want[0])
    fu.mesh_sample(spacing, seed)
    if n > 3:
        part, pf = fu.sample_points(n - 3, 3)
        assert_bitwise_equal(part, want[0][-3:], "a range")
        assert np.array_equal(pf, want[1][-3:])
    assert fu.L.acmmp_fusion_sample_points(fu.h, n, 0, None, None) == 0
    for first_, count in ((0, n + 1), (n, 1), (-1, 1), (0, -1)):
        assert fu.L.acmmp_fusion_sample_points(fu.h, first_, count, None, None) == 1
    fu.close()


def test_refusals_leave_the_previous_result():
    fresh = _fusion()                                                      # no mesh result
    assert fresh.L.acmmp_fusion_mesh_sample(fresh.h, 0.1, 0, None, None) == 1
    with pytest.raises(capi.AcmmpError):
        fresh.mesh_sample(0.1)
    assert fresh.L.acmmp_fusion_sample_points(fresh.h, 0, 1, None, None) == 1
    assert fresh.L.acmmp_fusion_mesh_sample(None, 0.1, 0, None, None) == 1
    fresh.close()
    v, f = mss.square(1000.0)                                              # two large triangles
    want = mss.sample(v, f, 20.0, 9)
    fu = _fusion()
    fu.set_mesh(v, f)
    kept = _assert_samples(fu, want, 20.0, 9, "large square")
    assert len(want[0]) > 2000
    out = np.full(2, -7, np.int64)

    def unchanged(what):
        pts, face = fu.sample_points()
        assert pts.tobytes() + face.tobytes() == kept, what
        assert out.tolist() == [-7, -7], what                               # a refusal writes no count
    for spacing in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert fu.L.acmmp_fusion_mesh_sample(fu.h, spacing, 0, out[0:1].ctypes.data, out[1:2].ctypes.data) == 1, spacing
        unchanged(f"spacing {spacing}")
    with pytest.raises(OverflowError):
        mss.sample(v, f, 0.01, 0)
    assert fu.L.acmmp_fusion_mesh_sample(fu.h, 0.01, 0, out[0:1].ctypes.data, out[1:2].ctypes.data) == 5     # ACMMP_ERR_UNSUPPORTED
    assert b"4294967296 samples" in fu.L.acmmp_fusion_last_error(fu.h)      # refused on the total: 2^32 samples would be 160 GiB
    unchanged("too many samples")
    assert fu.mesh_sample(20.0, 9).n_samples == len(want[0])               # and the call still works
    fu.close()


def _chain():
    """A fusion object holding a scene, a voxel, a clean and a visible result of the constructed sphere rig and, as its
    mesh, the first 1500 faces of the rig's restated mesh."""
    cams, depths, normals, colours, cloud, size = vis.constructed("sphere")
    fu = fill(capi.Fusion(0, cams), cams, depths, normals, colours)
    scene = cloud[::4]
    fu.set_scene(scene)
    fu.voxelize(size)
    fu.voxel_clean(26, 1, 2, 1)
    fu.voxel_visibility(list(range(len(cams))), 0.01, 1, 1, 0, source="clean")
    fu.set_mesh(*sd.rig_part())
    return fu, size, scene, (cams, depths, normals, colours)


def test_lifetimes():
    fu, size, scene, (cams, depths, normals, colours) = _chain()
    mesh = sd.rig_part()
    have = lambda: fu.L.acmmp_fusion_sample_points(fu.h, 0, 1, None, None) == 0
    dist_have = lambda: fu.L.acmmp_fusion_distance_results(fu.h, 0, 1, None, None) == 0
    align_have = lambda: fu.L.acmmp_fusion_align_records(fu.h, 0, 1, None, None, None) == 0
    sample = lambda: fu.mesh_sample(size, 0)
    ref = (scene[::3, :3] + F32(0.25 * size)).astype(F32)
    assert not have()
    assert sample().n_samples > 100 and have()
    before = fu.sample_points()
    fu.set_view(0, depths[0], normals[0], colours[0])                      # set_view, the reference cloud, a distance, a surface
    fu.set_reference_cloud(ref)                                            # and a render call leave the samples alone
    fu.cloud_distance("voxels", "data_to_ref", size, (size,))
    fu.surface_distance("reference", size, (size,))
    fu.render_mesh(0)
    fu.cloud_align("voxels", "rigid", size, 1)
    after = fu.sample_points()
    assert have() and after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
    fu.set_scene(scene)                                                    # the samples of a set mesh survive the scene
    assert have()
    fu.run_scene([0], [[1, 2]])
    assert have()
    fu.cloud_distance("samples", "data_to_ref", size, (size,))             # a distance result of the samples
    fu.cloud_align("samples", "rigid", size, 1)
    assert dist_have() and align_have()
    sample()                                                               # goes when the samples are replaced
    assert not dist_have() and not align_have() and have()
    fu.cloud_distance("samples", "ref_to_data", size, (size,))
    fu.set_reference_cloud(ref)                                            # and with the reference cloud, which leaves the samples
    assert not dist_have() and have()
    fu.cloud_distance("samples", "data_to_ref", size, (size,))
    fu.set_mesh(*mesh)                                                     # the samples go with set_mesh, and their distances with them
    assert not have() and not dist_have()
    with pytest.raises(capi.AcmmpError):
        fu.cloud_distance("samples", "data_to_ref", size, (size,))
    fu.set_scene(scene)
    fu.voxelize(size)
    sample()
    fu.voxel_mesh([0, 1, 2], 3 * size)                                     # with voxel_mesh
    assert not have()
    assert sample().n_samples > 0 and have()
    fu.voxelize(size)                                                      # and with what discards the mesh upstream
    assert not have()
    with pytest.raises(capi.AcmmpError):
        sample()
    fu.close()
