"""The cloud transform and the device ICP on the GPU (acmmp_fusion_set_cloud_transform / acmmp_fusion_cloud_align,
include/acmmp.h) against the numpy restatement (cloud_align_support): transformed distances and the records of every
iteration bit for bit, the fit within the bound a float64 solver meets, recovery of a known motion, edges, lifetimes."""
import functools

import numpy as np
import pytest

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
ITERATIONS = 4                                     # of the record tests: each is checked against an exhaustive restatement


def _fusion():
    return capi.Fusion(0, CAM)


def _scene_pair(Q=None, T=None):
    Q0, T0 = cd.clouds()
    Q, T = Q0 if Q is None else Q, T0 if T is None else T
    fu = _fusion()
    assert fu.set_scene(cd.as_points(Q)) == len(Q) and fu.set_reference_cloud(T) == len(T)
    return fu


def _distance_bytes(fu, source, direction, max_dist, taus, want=None, what=""):
    r = fu.cloud_distance(source, direction, max_dist, taus)
    d2, nn = fu.distance_results(squared=True)
    if want is not None:
        assert_bitwise_equal(d2, want[0], f"{what}: d2")
        assert np.array_equal(nn, want[1]), f"{what}: nearest"
        assert cd.summary_of(r) == want[2], f"{what}: summary"
    return d2.tobytes() + nn.tobytes() + np.array(cd.summary_of(r), np.int64).tobytes()


# ---- transformed distances

def _chain():
    """test_gpu_cloud_distance's rig: a fusion object holding a voxel, a clean and a visible result, and a mesh."""
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
    assert fu.set_mesh(data["mesh"], np.zeros((0, 3), np.int32)) == (1500, 0)
    return fu, size, data


def test_transformed_distances_all_sources():
    fu, size, data = _chain()
    rng = np.random.default_rng(5)
    V = data["voxels"][:, :3]
    centre = V.astype(np.float64).mean(0)
    M = ca.about(ca.rotation((2, -1, 1), 3.0), centre, (0.3 * size, -0.2 * size, 0.1 * size), 1.01)
    moved = ca.transform_points(M, V)
    ref = np.concatenate([moved[::3] + (F32(0.5 * size) * rng.standard_normal((len(V[::3]), 3))).astype(F32), moved[::4]])
    fu.set_reference_cloud(ref.astype(F32))
    max_dist, taus = 1.5 * size, (0.0, 0.5 * size, size)
    for source in cd.SOURCES:
        for direction in cd.DIRECTIONS:
            plain = _distance_bytes(fu, source, direction, max_dist, taus)
            fu.set_cloud_transform(ca.IDENTITY)
            assert fu.L.acmmp_fusion_distance_results(fu.h, 0, 1, None, None) == 1     # a set discards the result
            assert _distance_bytes(fu, source, direction, max_dist, taus) == plain, "the identity gives the bits of none"
            fu.set_cloud_transform(M)
            assert np.array_equal(fu.cloud_transform(), M)
            x = ca.transform_points(M, data[source])
            q, t = (x, ref) if direction == "data_to_ref" else (ref, x)
            want = cd.distances(q, t, max_dist, taus)
            assert 0 < want[2][2] < want[2][1]
            under = _distance_bytes(fu, source, direction, max_dist, taus, want, f"{source} {direction} under M")
            assert under != plain
            fu.set_cloud_transform(None)
            assert fu.cloud_transform() is None
            assert fu.L.acmmp_fusion_distance_results(fu.h, 0, 1, None, None) == 1     # and so does a clear
            assert _distance_bytes(fu, source, direction, max_dist, taus) == plain, "clearing restores the bits"
    for name, read in (("voxels", fu.voxel_points), ("clean", fu.clean_points), ("visible", fu.visible_points)):
        assert_bitwise_equal(read(0, len(data[name])), data[name], f"{name} after the transformed calls")
    fu.close()


def test_transform_that_leaves_float32_makes_points_invalid():
    Q, T = cd.clouds()
    fu = _scene_pair()
    M = ca.IDENTITY.copy()
    M[0, 0] = 1e39                                                         # x' is infinite wherever x is not 0
    fu.set_cloud_transform(M)
    for direction in cd.DIRECTIONS:
        x = ca.transform_points(M, Q)
        want = cd.distances(x, T, cd.MAX_DIST, cd.TAUS) if direction == "data_to_ref" else cd.distances(T, x, cd.MAX_DIST, cd.TAUS)
        _distance_bytes(fu, "scene", direction, cd.MAX_DIST, cd.TAUS, want, "overflowing transform")
    fu.close()


# ---- records

def _record_bytes(r):
    return b"".join(rec.words.tobytes() + rec.M.tobytes() + np.float64(rec.shift).tobytes() for rec in r.records) + r.M.tobytes()


@functools.lru_cache(maxsize=None)
def _device_run(mode, stride, rotated, cell=0.0):
    fu = _scene_pair()
    fu.distance_grid(cell)
    r = fu.cloud_align("scene", mode, cd.MAX_DIST, ITERATIONS, stride, 0.0, ca.SMALL_ROTATION if rotated else None)
    grid = fu.distance_grid(cell)
    again = fu.cloud_align("scene", mode, cd.MAX_DIST, ITERATIONS, stride, 0.0, ca.SMALL_ROTATION if rotated else None)
    assert _record_bytes(again) == _record_bytes(r), "a second run gives the same bytes"
    fu.close()
    return r, grid


@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("mode", ca.MODES)
def test_records_and_fit(mode, stride, rotated):
    Q, T = cd.clouds()
    r, grid = _device_run(mode, stride, rotated)
    lo, hi = ca.target_box(T)
    assert r.iterations == len(r.records) == ITERATIONS and r.stop_reason == "max_iterations"
    assert np.array_equal(r.records[0].M, ca.SMALL_ROTATION if rotated else ca.IDENTITY)
    out_of_range = 0
    for k, rec in enumerate(r.records):
        want = ca.iteration_record(rec.M, Q, T, cd.MAX_DIST, stride)       # under the device's own M_k
        assert [int(x) for x in rec.words] == want, f"iteration {k}: record"
        out_of_range += rec.n_out_of_range
        d = ca.svd_parts(want)[2]
        print(mode, stride, rotated, k, "matched", rec.n_matched, "N", rec.n_pairs, "mean", rec.mean, "d1/d0", d[1] / d[0],
              "shift", rec.shift)
        assert d[1] / d[0] >= 0.4                                          # well-conditioned: the bound below applies
        D = ca.fit(want, lo, cd.MAX_DIST, mode)
        nxt = ca.compose(D, rec.M)
        got = r.records[k + 1].M if k + 1 < len(r.records) else r.M
        assert np.abs(got[:, :3] - nxt[:, :3]).max() <= 1e-10, f"iteration {k}: rotation and scale"
        assert np.abs(got[:, 3] - nxt[:, 3]).max() <= 1e-10 * (1 + max(np.abs(lo).max(), np.abs(hi).max())), f"iteration {k}: translation"
        assert abs(rec.shift - ca.corner_shift(D, lo, hi)) <= 1e-10 * (1 + max(np.abs(lo).max(), np.abs(hi).max())) * 4
        assert rec.shift > 0.0
    if stride == 1 and not rotated:
        assert out_of_range > 0                                            # the queries beside the target at 1000
    assert grid["cell"] == F32(cd.MAX_DIST) and grid["cells"] > 1          # the grid outputs describe the align call


@pytest.mark.parametrize("mode", ca.MODES)
def test_forced_cells_give_the_same_bytes(mode):
    auto = _device_run(mode, 1, True)
    tiny = _device_run(mode, 1, True, cd.MAX_DIST / 12)
    huge = _device_run(mode, 1, True, 1e6)
    assert _record_bytes(auto[0]) == _record_bytes(tiny[0]) == _record_bytes(huge[0])
    assert huge[1]["cells"] == 1 and huge[1]["rings"] == 0 and tiny[1]["rings"] >= 12 and tiny[1]["cells"] > auto[1]["cells"]


def test_stop_reason_follows_shift_and_min_shift():
    fu = _scene_pair()
    full = fu.cloud_align("scene", "rigid", cd.MAX_DIST, ITERATIONS)
    shifts = [rec.shift for rec in full.records]
    k = int(np.argmin(shifts[:-1]))                                        # stop there: the first shift at or below it
    stop = next(i for i, s in enumerate(shifts) if s <= shifts[k])
    r = fu.cloud_align("scene", "rigid", cd.MAX_DIST, ITERATIONS, min_shift=shifts[k])
    assert r.stop_reason == "converged" and r.iterations == stop + 1 and r.records[-1].shift <= shifts[k]
    assert all(rec.shift > shifts[k] for rec in r.records[:-1])
    assert _record_bytes(r)[:-96] == _record_bytes(full)[:(stop + 1) * (32 * 8 + 96 + 8)]
    assert np.array_equal(r.M, full.records[stop + 1].M)
    one = fu.cloud_align("scene", "rigid", cd.MAX_DIST, 1)
    assert one.stop_reason == "max_iterations" and one.iterations == 1 and np.array_equal(one.M, full.records[1].M)
    fu.close()


# ---- recovery

@pytest.mark.parametrize("mode", ca.MODES)
def test_recovers_a_known_transform(mode):
    data, ref, known = ca.recovery_clouds(mode)
    restated = ca.restated_recovery(mode)
    fu = _scene_pair(data, ref)
    before = fu.cloud_distance("scene", "data_to_ref", cd.MAX_DIST)
    r = fu.cloud_align("scene", mode, cd.MAX_DIST, 10)
    own = np.abs(restated.M - known).max()
    err = np.abs(r.M - known).max()
    print(mode, "device error", err, "restatement error", own, "means", [rec.mean for rec in r.records])
    assert all(rec.n_matched >= 0.85 * rec.n_valid for rec in r.records)
    assert err <= 2 * own
    assert fu.cloud_transform() is None                                    # the call installs nothing
    fu.set_cloud_transform(r.M)
    after = fu.cloud_distance("scene", "data_to_ref", cd.MAX_DIST)
    print(mode, "accuracy mean", before.mean, "->", after.mean, "matched", before.n_matched, "->", after.n_matched)
    assert after.mean < before.mean                                        # accuracy under M improves on the identity's
    assert_bitwise_equal(fu.scene_points(0, len(data)), cd.as_points(data), "the scene is not transformed")
    fu.close()


# ---- edges

@pytest.mark.parametrize("n", [1, 63, 257])
def test_partial_wave_partial_workgroup_two_workgroups(n):
    data, ref, _ = ca.recovery_clouds("rigid")
    fu = _scene_pair(data[:n], ref)
    for stride in (1, 2, n + 3):
        r = fu.cloud_align("scene", "rigid", cd.MAX_DIST, 1, stride)
        want = ca.iteration_record(ca.IDENTITY, data[:n], ref, cd.MAX_DIST, stride)
        assert [int(x) for x in r.records[0].words] == want, (n, stride)
        assert r.records[0].n_query == -(-n // stride)
        D = ca.fit(want, ca.target_box(ref)[0], cd.MAX_DIST, "rigid")
        assert r.stop_reason == ("degenerate" if D is None else "max_iterations")
        if D is None:
            assert np.array_equal(r.M, ca.IDENTITY)
    fu.close()


def test_no_target_no_match_no_data():
    Q, T = cd.clouds()
    init = ca.SMALL_ROTATION
    fu = _scene_pair()
    for name, ref in (("no target", T[:0]), ("no valid target", np.full((3, 3), np.nan, F32)),
                      ("every query too far", (T[cd.valid(T)][:500] + F32(5000)).astype(F32))):
        fu.set_reference_cloud(ref)
        r = fu.cloud_align("scene", "similarity", cd.MAX_DIST, 5, 1, 0.0, init)
        assert r.stop_reason == "degenerate" and r.iterations == 1, name
        assert r.M.tobytes() == init.tobytes(), name                       # M_out == init bit for bit
        assert [int(x) for x in r.records[0].words] == ca.iteration_record(init, Q, ref, cd.MAX_DIST), name
        assert r.records[0].n_pairs == 0 and r.records[0].n_matched == 0 and r.records[0].n_valid > 0 and r.records[0].shift == 0.0
    fu.set_reference_cloud(T)
    fu.set_scene(np.zeros((0, 9), F32))                                    # an empty data result is valid, and degenerate
    r = fu.cloud_align("scene", "rigid", cd.MAX_DIST, 5)
    assert r.stop_reason == "degenerate" and r.iterations == 1 and r.records[0].words.tolist() == [0] * 32
    assert np.array_equal(r.M, ca.IDENTITY)
    fu.close()


# ---- arguments and lifetimes

def test_invalid_arguments_leave_everything():
    Q, T = cd.clouds()
    fu = _scene_pair()
    M = ca.about(ca.rotation((1, 0, 0), 1.0), (0.5, 0.5, 0.5))
    fu.set_cloud_transform(M)
    want = cd.distances(ca.transform_points(M, Q), T, cd.MAX_DIST, cd.TAUS)
    _distance_bytes(fu, "scene", "data_to_ref", cd.MAX_DIST, cd.TAUS, want, "before")
    kept = fu.cloud_align("scene", "rigid", cd.MAX_DIST, 2)
    L, h = fu.L, fu.h
    p = lambda a: a.ctypes.data
    out, it, stop = np.zeros(12), np.zeros(1, np.int32), np.zeros(1, np.int32)
    bad = lambda v: np.array([1, 0, 0, 0, 0, 1, 0, v, 0, 0, 1, 0], np.float64)

    def call(source=0, mode=0, max_dist=cd.MAX_DIST, iterations=2, stride=1, min_shift=0.0, init=None):
        return L.acmmp_fusion_cloud_align(h, source, mode, max_dist, iterations, stride, min_shift,
                                          None if init is None else p(init), p(out), p(it), p(stop))

    def unchanged(what):
        d2, nn = fu.distance_results(0, len(Q), squared=True)
        assert_bitwise_equal(d2, want[0], f"after {what}: d2")
        assert np.array_equal(nn, want[1]), f"after {what}: nearest"
        assert np.array_equal(fu.cloud_transform(), M), f"after {what}: transform"
        recs = fu.align_records(0, 2, cd.MAX_DIST)
        assert b"".join(r.words.tobytes() + r.M.tobytes() for r in recs) == \
            b"".join(r.words.tobytes() + r.M.tobytes() for r in kept.records), f"after {what}: records"
        assert_bitwise_equal(fu.scene_points(0, len(Q)), cd.as_points(Q), f"after {what}: scene")
    cases = {"source 5": dict(source=5), "source -1": dict(source=-1), "mode 2": dict(mode=2), "mode -1": dict(mode=-1),
             "no voxel result": dict(source=1), "no mesh result": dict(source=4), "max_dist 0": dict(max_dist=0.0),
             "max_dist nan": dict(max_dist=float("nan")), "max_dist inf": dict(max_dist=float("inf")),
             "max_dist < 0": dict(max_dist=-1.0), "iterations 0": dict(iterations=0), "iterations 1025": dict(iterations=1025),
             "stride 0": dict(stride=0), "stride -1": dict(stride=-1), "min_shift nan": dict(min_shift=float("nan")),
             "min_shift inf": dict(min_shift=float("inf")), "min_shift < 0": dict(min_shift=-1e-9),
             "init nan": dict(init=bad(np.nan)), "init inf": dict(init=bad(np.inf))}
    for what, kw in cases.items():
        assert call(**kw) == 1, what                                       # ACMMP_ERR_INVALID_ARGUMENT
        unchanged(what)
    for cell in (-1.0, float("nan"), float("inf")):
        fu.distance_grid(cell)
        assert call() == 1
        unchanged(f"forced cell {cell}")
    fu.distance_grid(0.0)
    for v in (np.nan, np.inf, -np.inf):
        assert L.acmmp_fusion_set_cloud_transform(h, p(bad(v))) == 1
        unchanged(f"transform {v}")
    for first, n in ((0, 3), (2, 1), (-1, 1), (0, -1)):
        assert L.acmmp_fusion_align_records(h, first, n, None, None, None) == 1
    assert L.acmmp_fusion_align_records(h, 2, 0, None, None, None) == 0
    assert call() == 0 and it[0] == 2 and np.array_equal(out.reshape(3, 4), kept.M)     # and the call still works
    unchanged("a successful align")                                        # which touches neither the distance result nor the transform
    fresh = _fusion()                                                      # no reference cloud at all
    fresh.set_scene(cd.as_points(Q[:10]))
    with pytest.raises(capi.AcmmpError):
        fresh.cloud_align("scene", "rigid", 1.0)
    with pytest.raises(capi.AcmmpError):
        fresh.align_records(0, 1)
    fresh.close()
    fu.close()


def test_lifetimes():
    fu, size, data = _chain()
    ref = data["voxels"][::2, :3] + F32(0.25 * size)
    fu.set_reference_cloud(ref)
    M = ca.about(ca.rotation((0, 1, 0), 1.0), (0, 0, 0), (size, 0, 0))
    fu.set_cloud_transform(M)
    gone = lambda: fu.L.acmmp_fusion_align_records(fu.h, 0, 1, None, None, None) == 1
    run = lambda source: fu.cloud_align(source, "rigid", 2 * size, 1)
    same = lambda: np.array_equal(fu.cloud_transform(), M)
    cams, depths, normals, colours = vis.constructed("sphere")[:4]
    run("voxels")
    assert not gone()
    fu.set_view(0, depths[0], normals[0], colours[0])                      # set_view touches nothing
    assert not gone() and same()
    fu.cloud_distance("voxels", "data_to_ref", size)                       # nor does a distance call, a set or a clear
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
