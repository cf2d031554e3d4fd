"""The point-to-plane device ICP on the GPU (acmmp_fusion_cloud_align_plane, include/acmmp.h) against the numpy
restatement (cloud_align_plane_support): the 70 words of every iteration bit for bit from the device's own M_k and g_k,
the fit within the bound two float64 solvers meet on well-conditioned systems, recovery, edges, arguments, lifetimes."""
import functools

import numpy as np
import pytest

import cloud_align_plane_support as cp
import cloud_align_support as ca
import cloud_distance_support as cd
import visibility_support as vis
from acmmp import capi
from conftest import assert_bitwise_equal
from fusion_scene_support import fill

pytestmark = pytest.mark.gpu

F32 = np.float32
CAM = np.zeros(1, capi.CAMERA_DTYPE)
CAM["width"], CAM["height"] = 8, 8


def _scene_pair(data, ref):
    fu = capi.Fusion(0, CAM)
    assert fu.set_scene(data) == len(data) and fu.set_reference_cloud(ref) == len(ref)
    return fu


def _record_bytes(r):
    return b"".join(rec.words.tobytes() + rec.M.tobytes() + np.float64(rec.shift).tobytes() for rec in r.records) + r.M.tobytes()


def _check_records(r, M0, data, ref, max_dist, stride, what):
    """Every record of the device run r against the restatement under the device's own M_k and g_k, and the pivots'
    chain: g_0 from the point pass under M_0, g_{k+1} from iteration k's words."""
    assert r.iterations == len(r.records) >= 1, what
    assert r.records[0].M.tobytes() == ca.as_matrix(M0).tobytes(), what
    assert r.records[0].pivot == cp.point_pivot(M0, data, ref, max_dist, stride), f"{what}: g_0"
    wants = []
    for k, rec in enumerate(r.records):
        want = cp.iteration_record(rec.M, rec.pivot, data, ref, max_dist, stride)
        assert [int(x) for x in rec.words] == want, f"{what}: iteration {k}: record"
        if k + 1 < len(r.records):
            assert r.records[k + 1].pivot == cp.pivot(want[cp.SUM_Q3:cp.SUM_Q3 + 3], want[cp.N_PAIRS]), f"{what}: g_{k + 1}"
        wants.append(want)
    return wants


# ---- all five sources

def _chain():
    """test_gpu_cloud_distance's rig: a fusion object holding a voxel, a clean and a visible result, and a mesh (whose
    vertices here carry random normals)."""
    cams, depths, normals, colours, cloud, size = vis.constructed("sphere")
    fu = fill(capi.Fusion(0, cams), cams, depths, normals, colours)
    fu.set_scene(cloud)
    nv = fu.voxelize(size)[0]
    nc = fu.voxel_clean(26, 1, 2, 1)[0]
    nk = fu.voxel_visibility(list(range(len(cams))), 0.01, 1, 1, 0, source="clean")[0]
    data = {"scene": np.asarray(cloud, F32), "voxels": fu.voxel_points(0, nv), "clean": fu.clean_points(0, nc),
            "visible": fu.visible_points(0, nk)}
    data["mesh"] = cd.as_points(cd.clouds()[0])[:1500]
    data["mesh"][:700, :3] = data["voxels"][:700, :3]
    data["mesh"][:, 3:6] = np.random.default_rng(8).standard_normal((1500, 3)).astype(F32)
    assert fu.set_mesh(data["mesh"], np.zeros((0, 3), np.int32)) == (1500, 0)
    return fu, size, data


def test_records_of_all_sources():
    fu, size, data = _chain()
    V = data["voxels"][:, :3]
    centre = V.astype(np.float64).mean(0)
    M = ca.about(ca.rotation((2, -1, 1), 2.0), centre, (0.3 * size, -0.2 * size, 0.1 * size))
    ref = ca.transform_points(M, V)[::2]
    fu.set_reference_cloud(ref)
    max_dist = 2.5 * size
    scaled = ca.about(ca.rotation((0, 1, 1), 1.0), centre, (0, 0.2 * size, 0), 1.01)
    for source in cd.SOURCES:
        for stride, init in ((1, None), (3, scaled)):
            r = fu.cloud_align_plane(source, max_dist, 2, stride, 0.0, init)
            wants = _check_records(r, ca.IDENTITY if init is None else init, data[source], ref, max_dist, stride, f"{source} stride {stride}")
            print(source, stride, "iterations", r.iterations, r.stop_reason, "N", [w[cp.N_PAIRS] for w in wants],
                  "no normal", [w[cp.N_NO_NORMAL] for w in wants], "rms", [rec.rms_plane for rec in r.records])
            assert wants[0][cp.N_PAIRS] >= 6, source
    for name, read in (("voxels", fu.voxel_points), ("clean", fu.clean_points), ("visible", fu.visible_points)):
        assert_bitwise_equal(read(0, len(data[name])), data[name], f"{name} after the align calls")
    fu.close()


# ---- records and fit on the condition-checked clouds

@functools.lru_cache(maxsize=None)
def _device_run(name, cell=0.0):
    clouds, max_dist, init, stride, iterations = cp.FIT_CASES[name]
    data, ref = clouds()
    fu = _scene_pair(data, ref)
    fu.distance_grid(cell)
    r = fu.cloud_align_plane("scene", max_dist, iterations, stride, 0.0, init)
    grid = fu.distance_grid(cell)
    again = fu.cloud_align_plane("scene", max_dist, iterations, stride, 0.0, init)
    assert _record_bytes(again) == _record_bytes(r), "a second run gives the same bytes"
    fu.close()
    return r, grid


@pytest.mark.parametrize("name", list(cp.FIT_CASES))
def test_records_and_fit(name):
    clouds, max_dist, init, stride, iterations = cp.FIT_CASES[name]
    data, ref = clouds()
    r, grid = _device_run(name)
    restated = cp.restated_fit_case(name)
    lo, hi = ca.target_box(ref)
    wants = _check_records(r, ca.IDENTITY if init is None else init, data, ref, max_dist, stride, name)
    assert (r.stop_reason, r.iterations) == (restated.stop_reason, restated.iterations) == ("max_iterations", iterations)
    for k, (rec, want) in enumerate(zip(r.records, wants)):
        cond = cp.condition(want)
        D = cp.fit(want, lo, max_dist)
        nxt = r.records[k + 1].M if k + 1 < len(r.records) else r.M
        got = ca.compose(nxt, ca.inverse(rec.M))                           # the device's D: M_{k+1} o M_k^-1
        err = np.abs(got - D) / np.maximum(1.0, np.abs(D))
        print(name, k, "N", rec.n_pairs, "no normal", rec.n_no_normal, "out of range", rec.n_out_of_range, "condition", cond,
              "D error", err.max(), "shift", rec.shift, "rms", rec.rms_plane)
        assert cond < 1e4
        assert err.max() <= 1e-9, f"{name}: iteration {k}: D"
        assert abs(rec.shift - ca.corner_shift(D, lo, hi)) <= 1e-9 * (1 + max(np.abs(lo).max(), np.abs(hi).max())) * 4
    if name == "records":
        assert wants[0][cp.N_NO_NORMAL] == 4                               # the edge normals: zero, NaN, inf, -inf
        assert wants[0][cp.N_OUT_OF_RANGE] > 0                             # the queries beside the target at 1000
        assert grid["cell"] == F32(max_dist) and grid["cells"] > 1         # the grid outputs describe the align call


def test_forced_cells_give_the_same_bytes():
    name = "records rotated"
    auto, tiny, huge = _device_run(name), _device_run(name, cd.MAX_DIST / 12), _device_run(name, 1e6)
    assert _record_bytes(auto[0]) == _record_bytes(tiny[0]) == _record_bytes(huge[0])
    assert huge[1]["cells"] == 1 and huge[1]["rings"] == 0 and tiny[1]["rings"] >= 12 and tiny[1]["cells"] > auto[1]["cells"]


def test_recovers_the_known_motion_as_the_restatement_does():
    data, ref, known = cp.two_samplings()
    full = cp.restated_fit_case("two samplings")
    min_shift = 1e-5                                                       # between the restated shifts 2.6e-4 and 2.4e-6
    stop = next(i for i, rec in enumerate(full.records) if rec.shift <= min_shift)
    assert all(abs(rec.shift - min_shift) > 1e-6 for rec in full.records)  # no shift near enough to decide otherwise
    fu = _scene_pair(data, ref)
    r = fu.cloud_align_plane("scene", cp.CLAIM_MAX_DIST, cp.CLAIM_ITERATIONS, min_shift=min_shift)
    point = fu.cloud_align("scene", "rigid", cp.CLAIM_MAX_DIST, stop + 1)
    ep, eq = cp.corner_error(r.M, known), cp.corner_error(point.M, known)
    print("iterations", r.iterations, "corner error: plane", ep, "point", eq, "restated plane", cp.corner_error(full.records[stop + 1].M, known))
    assert (r.stop_reason, r.iterations) == ("converged", stop + 1)
    assert np.abs(r.M - full.records[stop + 1].M).max() <= 1e-9 and ep < eq
    assert fu.cloud_transform() is None                                    # the call installs nothing
    assert_bitwise_equal(fu.scene_points(0, len(data)), data, "the scene is not transformed")
    fu.close()


def test_a_sphere_at_its_correspondences_is_degenerate():
    """The noise-floor rule on the host: the eigenvalue rule passes this record (condition 1.2e3), the floor does not."""
    rng = np.random.default_rng(2)
    v = rng.standard_normal((2000, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    xyz = (v + 0.5).astype(F32)
    data = cp.with_normals(xyz, v.astype(F32))
    fu = _scene_pair(data, xyz)
    r = fu.cloud_align_plane("scene", 0.06, 5)
    want = _check_records(r, ca.IDENTITY, data, xyz, 0.06, 1, "sphere")[0]
    assert want[cp.N_PAIRS] == 2000 and cp.condition(want) < 1e4 and cp.rotation_over_noise(want) < 2.0
    assert r.stop_reason == "degenerate" and r.iterations == 1 and np.array_equal(r.M, ca.IDENTITY) and r.records[0].shift == 0.0
    fu.close()


# ---- edges

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_partial_waves_and_workgroups(n):
    data, ref, _ = cp.two_samplings()
    fu = _scene_pair(data[:n], ref)
    for stride in (1, 2, n + 3):
        r = fu.cloud_align_plane("scene", cp.CLAIM_MAX_DIST, 1, stride)
        want = _check_records(r, ca.IDENTITY, data[:n], ref, cp.CLAIM_MAX_DIST, stride, (n, stride))[0]
        assert r.records[0].n_query == -(-n // stride)
        D = cp.fit(want, ca.target_box(ref)[0], cp.CLAIM_MAX_DIST)
        assert r.stop_reason == ("degenerate" if D is None else "max_iterations")
        if D is None:
            assert np.array_equal(r.M, ca.IDENTITY) and r.records[0].shift == 0.0
    fu.close()


def test_no_target_no_match_no_data():
    data, T = cp.record_clouds()
    init = ca.SMALL_ROTATION
    fu = _scene_pair(data, T)
    for name, ref in (("no target", T[:0]), ("no valid target", np.full((3, 3), np.nan, F32)),
                      ("every query too far", (T[cd.valid(T)][:500] + F32(5000)).astype(F32))):
        fu.set_reference_cloud(ref)
        r = fu.cloud_align_plane("scene", cd.MAX_DIST, 5, 1, 0.0, init)
        assert r.stop_reason == "degenerate" and r.iterations == 1, name
        assert r.M.tobytes() == init.tobytes(), name                       # M_out == init bit for bit
        assert [int(x) for x in r.records[0].words] == cp.iteration_record(init, [0, 0, 0], data, ref, cd.MAX_DIST), name
        assert r.records[0].n_pairs == 0 and r.records[0].n_matched == 0 and r.records[0].n_valid > 0 and r.records[0].shift == 0.0
    fu.set_reference_cloud(T)
    fu.set_scene(np.zeros((0, 9), F32))                                    # an empty data result is valid, and degenerate
    r = fu.cloud_align_plane("scene", cd.MAX_DIST, 5)
    assert r.stop_reason == "degenerate" and r.iterations == 1 and r.records[0].words.tolist() == [0] * cp.RECORD_WORDS
    assert np.array_equal(r.M, ca.IDENTITY)
    fu.close()


# ---- arguments and lifetimes

def test_invalid_arguments_leave_everything():
    data, T = cp.record_clouds()
    Q = data[:, :3]
    fu = _scene_pair(data, T)
    M = ca.about(ca.rotation((1, 0, 0), 1.0), (0.5, 0.5, 0.5))
    fu.set_cloud_transform(M)
    want = cd.distances(ca.transform_points(M, Q), T, cd.MAX_DIST, cd.TAUS)
    fu.cloud_distance("scene", "data_to_ref", cd.MAX_DIST, cd.TAUS)
    kept = fu.cloud_align_plane("scene", cd.MAX_DIST, 2)
    L, h = fu.L, fu.h
    p = lambda a: a.ctypes.data
    out, it, stop = np.zeros(12), np.zeros(1, np.int32), np.zeros(1, np.int32)
    bad = lambda v: np.array([1, 0, 0, 0, 0, 1, 0, v, 0, 0, 1, 0], np.float64)

    def call(source=0, max_dist=cd.MAX_DIST, iterations=2, stride=1, min_shift=0.0, init=None):
        return L.acmmp_fusion_cloud_align_plane(h, source, max_dist, iterations, stride, min_shift,
                                                None if init is None else p(init), p(out), p(it), p(stop))

    def unchanged(what):
        d2, nn = fu.distance_results(0, len(Q), squared=True)
        assert_bitwise_equal(d2, want[0], f"after {what}: d2")
        assert np.array_equal(nn, want[1]), f"after {what}: nearest"
        assert np.array_equal(fu.cloud_transform(), M), f"after {what}: transform"
        assert _record_bytes(dataclass_of(fu.align_plane_records(0, 2, cd.MAX_DIST), kept.M)) == _record_bytes(kept), f"after {what}: records"
        assert_bitwise_equal(fu.scene_points(0, len(Q)), data, f"after {what}: scene")

    def dataclass_of(records, M):
        return capi.CloudAlignment(M=M, iterations=len(records), stop_reason="", records=records)
    cases = {"source 5": dict(source=5), "source -1": dict(source=-1), "no voxel result": dict(source=1),
             "no mesh result": dict(source=4), "max_dist 0": dict(max_dist=0.0), "max_dist nan": dict(max_dist=float("nan")),
             "max_dist inf": dict(max_dist=float("inf")), "max_dist < 0": dict(max_dist=-1.0), "iterations 0": dict(iterations=0),
             "iterations 1025": dict(iterations=1025), "stride 0": dict(stride=0), "stride -1": dict(stride=-1),
             "min_shift nan": dict(min_shift=float("nan")), "min_shift inf": dict(min_shift=float("inf")),
             "min_shift < 0": dict(min_shift=-1e-9), "init nan": dict(init=bad(np.nan)), "init inf": dict(init=bad(np.inf))}
    for what, kw in cases.items():
        assert call(**kw) == 1, what                                       # ACMMP_ERR_INVALID_ARGUMENT
        unchanged(what)
    for cell in (-1.0, float("nan"), float("inf")):
        fu.distance_grid(cell)
        assert call() == 1
        unchanged(f"forced cell {cell}")
    fu.distance_grid(0.0)
    for first, n in ((0, 3), (2, 1), (-1, 1), (0, -1)):
        assert L.acmmp_fusion_align_plane_records(h, first, n, None, None, None) == 1
    assert L.acmmp_fusion_align_plane_records(h, 2, 0, None, None, None) == 0
    assert call() == 0 and it[0] == 2 and np.array_equal(out.reshape(3, 4), kept.M)     # and the call still works
    unchanged("a successful align")                                        # which touches neither the distance result nor the transform
    fresh = capi.Fusion(0, CAM)                                            # no reference cloud at all
    fresh.set_scene(data[:10])
    with pytest.raises(capi.AcmmpError):
        fresh.cloud_align_plane("scene", 1.0)
    with pytest.raises(capi.AcmmpError):
        fresh.align_plane_records(0, 1)
    with pytest.raises(ValueError):
        fresh.cloud_align_plane("cloud", 1.0)
    fresh.close()
    fu.close()


def test_lifetimes():
    fu, size, data = _chain()
    ref = data["voxels"][::2, :3] + F32(0.25 * size)
    fu.set_reference_cloud(ref)
    M = ca.about(ca.rotation((0, 1, 0), 1.0), (0, 0, 0), (size, 0, 0))
    fu.set_cloud_transform(M)
    gone = lambda: fu.L.acmmp_fusion_align_plane_records(fu.h, 0, 1, None, None, None) == 1
    point_gone = lambda: fu.L.acmmp_fusion_align_records(fu.h, 0, 1, None, None, None) == 1
    run = lambda source: fu.cloud_align_plane(source, 2 * size, 1)
    same = lambda: np.array_equal(fu.cloud_transform(), M)
    cams, depths, normals, colours = vis.constructed("sphere")[:4]
    run("voxels")
    assert not gone() and point_gone()
    fu.cloud_align("voxels", "rigid", 2 * size, 1)                         # a point call discards the plane records
    assert gone() and not point_gone()
    run("voxels")                                                          # and a plane call the point records
    assert not gone() and point_gone()
    fu.set_view(0, depths[0], normals[0], colours[0])                      # set_view touches nothing
    assert not gone() and same()
    before = fu.cloud_distance("voxels", "data_to_ref", size)              # nor does a distance call, a set or a clear
    d2 = fu.distance_results(squared=True)[0]
    run("voxels")                                                          # and the plane call leaves the distance result
    assert_bitwise_equal(fu.distance_results(squared=True)[0], d2, "the distance result after a plane call")
    assert before.n_matched > 0
    fu.set_cloud_transform(None)
    fu.set_cloud_transform(M)
    assert not gone()
    fu.set_reference_cloud(ref)                                            # the records go with the reference cloud
    assert gone() and same()
    run("voxels")
    fu.voxelize(size)                                                      # and with their source
    assert gone() and same()
    run("scene")
    fu.voxel_clean(26, 1, 2, 1)                                            # another source's replacement does not touch them
    assert not gone()
    fu.set_scene(fu.scene_points(0, 50))
    assert gone() and same()                                               # the transform survives set_scene
    fu.set_mesh(data["voxels"][:100], np.zeros((0, 3), np.int32))
    run("mesh")
    fu.set_mesh(data["voxels"][:100], np.zeros((0, 3), np.int32))
    assert gone() and same()
    fu.close()
