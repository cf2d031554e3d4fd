"""Evaluation regions on the GPU (acmmp_fusion_set_region / acmmp_fusion_region_classify, include/acmmp.h) against the
numpy restatement (eval_region_support): the class bytes and counts byte for byte, and for each of the four measuring
calls the substitution equivalence -- a run with a region equals, bit for bit, a run without one on the same cloud with
x replaced by NaN where the restatement's class is not 0."""
import ctypes as C

import numpy as np
import pytest

import cloud_align_support as ca
import cloud_distance_support as cd
import eval_region_support as er
from acmmp import capi
from conftest import assert_bitwise_equal

pytestmark = pytest.mark.gpu

F32 = np.float32
CAM = np.zeros(1, capi.CAMERA_DTYPE)
CAM["width"], CAM["height"] = 8, 8
MAX_DIST, TAUS = 0.05, (0.0, 0.005, 0.01, 0.02, 0.05)
ALL = dict(planes=True, prism=True, grid=True)
DATA_REGION, REF_REGION = er.region(prism=True, grid=True), er.region(planes=True, prism=True, polygon=er.TRIANGLE)


def _fusion(Q=None, T=None):
    fu = capi.Fusion(0, CAM)
    Q = er.cloud() if Q is None else Q
    T = er.reference_cloud() if T is None else T
    assert fu.set_scene(er.as_points(Q)) == len(Q) and fu.set_reference_cloud(T) == len(T)
    return fu


def _classes(fu, source):
    n = fu.region_classify(source)
    return n, fu.region_classes()


# ---- 1. classes and counts

@pytest.mark.parametrize("parts", [dict(planes=True), dict(prism=True), dict(grid=True), ALL,
                                   dict(prism=True, axis=0), dict(prism=True, axis=1), dict(prism=True, polygon=er.TRIANGLE)],
                         ids=["planes", "prism", "grid", "all", "axis0", "axis1", "triangle"])
def test_classes_and_counts(parts):
    fu = _fusion()
    r = er.region(**parts)
    Q, T = er.cloud(), er.reference_cloud()
    for M in (None, er.MOTION):
        fu.set_cloud_transform(M)
        fu.set_region("data", r)
        fu.set_region("reference", r)
        for source, pts, under in (("scene", Q, M), ("reference", T, None)):      # stride 9 and stride 3; no transform for the reference
            want = er.classify(pts, r, under)
            n, cls = _classes(fu, source)
            assert cls.dtype == np.uint8 and cls.tobytes() == want.tobytes(), (source, M is not None)
            assert n == er.counts(want)
        assert 0 < er.counts(er.classify(Q, r, M))["inside"] < len(Q)
    fu.close()


def test_no_region_every_valid_point_is_inside():
    fu = _fusion()
    for source, pts in (("scene", er.cloud()), ("reference", er.reference_cloud())):
        n, cls = _classes(fu, source)
        assert cls.tobytes() == er.classify(pts, None).tobytes() and n == er.counts(er.classify(pts, None))
        assert n["inside"] == n["points"] - n["invalid"] and n["planes"] == n["prism"] == n["grid"] == 0
    # a range, and the empty cloud
    fu.set_region("data", er.region(**ALL))
    want = er.classify(er.cloud(), er.region(**ALL))
    fu.region_classify("scene")
    assert fu.region_classes(700, 300).tobytes() == want[700:1000].tobytes() and len(fu.region_classes(er.N_CLOUD, 0)) == 0
    assert fu.L.acmmp_fusion_region_classes(fu.h, er.N_CLOUD - 1, 2, None) == 1
    fu.set_scene(np.zeros((0, 9), F32))
    assert fu.region_classify("scene") == dict.fromkeys(er.COUNTS, 0) and len(fu.region_classes()) == 0
    fu.close()


# ---- 2. substitution equivalence

def _distance(fu, source, direction):
    r = fu.cloud_distance(source, direction, MAX_DIST, TAUS)
    d2, nn = fu.distance_results(squared=True)
    return d2, nn, cd.summary_of(r)


def _same(a, b, what):
    assert_bitwise_equal(a[0], b[0], f"{what}: d2")
    assert np.array_equal(a[1], b[1]), f"{what}: nearest"
    assert a[2] == b[2] and len(a[2]) == 268, f"{what}: summary"


@pytest.mark.parametrize("M", [None, er.MOTION], ids=["plain", "transformed"])
def test_cloud_distance_substitution(M):
    Q, T = er.cloud(), er.reference_cloud()
    cq, ct = er.classify(Q, DATA_REGION, M), er.classify(T, REF_REGION)
    a = _fusion()
    a.set_cloud_transform(M)
    a.set_region("data", DATA_REGION)
    a.set_region("reference", REF_REGION)
    b = _fusion(er.substituted(Q, cq), er.substituted(T, ct))
    b.set_cloud_transform(M)
    plain = _fusion()
    plain.set_cloud_transform(M)
    for direction in cd.DIRECTIONS:
        ra, rb = _distance(a, "scene", direction), _distance(b, "scene", direction)
        _same(ra, rb, direction)
        nv = (cq == 0).sum() if direction == "data_to_ref" else (ct == 0).sum()
        assert ra[2][0] == (len(Q) if direction == "data_to_ref" else len(T)) and ra[2][1] == nv and 0 < ra[2][2] < nv
        assert ra[2] != _distance(plain, "scene", direction)[2]
        # against the restatement of the distance itself, so that both runs are not wrong together
        x = ca.transform_points(M, Q) if M is not None else Q
        qs, ts = er.substituted(x, cq), er.substituted(T, ct)
        want = cd.distances(qs, ts, MAX_DIST, TAUS) if direction == "data_to_ref" else cd.distances(ts, qs, MAX_DIST, TAUS)
        _same(ra, want, direction + " restated")
    # one side only: the other side's points all remain
    a.set_region("reference", None)
    half = _fusion(er.substituted(Q, cq), T)
    half.set_cloud_transform(M)
    for direction in cd.DIRECTIONS:
        _same(_distance(a, "scene", direction), _distance(half, "scene", direction), "data region only, " + direction)
    for fu in (a, b, plain, half):
        fu.close()


def _mesh():
    """A 9 x 9 vertex sheet over [0, 1]^2 at z = 0.25, two faces per square."""
    g = np.linspace(0, 1, 9, dtype=F32)
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    v = cd.as_points(np.column_stack([xy, np.full(len(xy), 0.25, F32)]))
    idx = np.arange(81).reshape(9, 9)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    return v, np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32)


def _surface(fu, query):
    r = fu.surface_distance(query, 0.2, (0.01, 0.05, 0.2))
    d2, nf = fu.surface_results(squared=True)
    return d2, nf, cd.summary_of(r)


@pytest.mark.parametrize("M", [None, er.MOTION], ids=["plain", "transformed"])
def test_surface_distance_substitution(M):
    Q, T = er.cloud(), er.reference_cloud()
    cq, ct = er.classify(Q, DATA_REGION, M), er.classify(T, REF_REGION)          # the data queries: where the region lives
    v, faces = _mesh()
    a, b = _fusion(), _fusion(er.substituted(Q, cq), er.substituted(T, ct))
    for fu in (a, b):
        fu.set_cloud_transform(M)
        assert fu.set_mesh(v, faces) == (81, 128)
    a.set_region("data", DATA_REGION)
    a.set_region("reference", REF_REGION)
    for query, cls in (("scene", cq), ("reference", ct)):
        ra, rb = _surface(a, query), _surface(b, query)
        _same(ra, rb, query)
        assert ra[2][1] == (cls == 0).sum() and 0 < ra[2][2] <= ra[2][1]
        assert (ra[1][cls != 0] == -1).all() and np.isinf(ra[0][cls != 0]).all() and (ra[1][cls == 0] >= 0).any()
    a.close()
    b.close()


def _align(fu, plane, iterations, init=None):
    if plane:
        r = fu.cloud_align_plane("scene", 0.1, iterations, 1, 0.0, init)
    else:
        r = fu.cloud_align("scene", "rigid", 0.1, iterations, 1, 0.0, init)
    return r, [rec.words.tobytes() + rec.M.tobytes() + np.float64(rec.shift).tobytes() for rec in r.records]


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_align_substitution_reference_region(plane):
    """The reference side is never transformed, so one host substitution serves every iteration."""
    Q, T = er.cloud(), er.reference_cloud()
    ct = er.classify(T, REF_REGION)
    a, b = _fusion(), _fusion(Q, er.substituted(T, ct))
    a.set_region("reference", REF_REGION)
    (ra, reca), (rb, recb) = _align(a, plane, 3, er.MOTION), _align(b, plane, 3, er.MOTION)
    assert ra.iterations == rb.iterations == 3 and reca == recb and ra.M.tobytes() == rb.M.tobytes()
    assert ra.stop_reason == rb.stop_reason
    plain = _fusion()
    assert _align(plain, plane, 3, er.MOTION)[1] != reca
    # a queries-only reference region leaves an align call's targets whole: the bits of no region
    a.set_region("reference", REF_REGION, queries_only=True)
    assert _align(a, plane, 3, er.MOTION)[1] == _align(plain, plane, 3, er.MOTION)[1]
    for fu in (a, b, plain):
        fu.close()


def test_align_substitution_data_region_follows_the_transform():
    """The data side is classified under every M_k.  The point call is followed step by step: run B substitutes under
    M_k on the host and runs iteration k alone from M_k, which gives record k and M_{k+1}."""
    Q, T = er.cloud(), er.reference_cloud()
    ct = er.classify(T, REF_REGION)
    a = _fusion()
    a.set_region("data", DATA_REGION)
    a.set_region("reference", REF_REGION)
    ra, reca = _align(a, False, 3, er.MOTION)
    assert ra.iterations == 3
    M, changed = er.MOTION, 0
    prev = None
    for k in range(3):
        assert ra.records[k].M.tobytes() == np.asarray(M, np.float64).tobytes()
        cq = er.classify(Q, DATA_REGION, M)
        changed += prev is not None and not np.array_equal(prev, cq)
        prev = cq
        b = _fusion(er.substituted(Q, cq), er.substituted(T, ct))
        rb, recb = _align(b, False, 1, M)
        assert recb[0] == reca[k], f"iteration {k}"
        assert ra.records[k].words[1] == (cq[np.isfinite(ca.transform_points(M, Q)).all(1)] == 0).sum()      # n_valid
        M = rb.M
        b.close()
    assert ra.M.tobytes() == np.asarray(M, np.float64).tobytes()
    assert changed, "the classes must move with the transform, or the test shows nothing"
    assert _align(a, False, 3, er.MOTION)[1] == reca                                  # and the whole call reproduces
    a.close()


def test_align_plane_data_region_iteration_0_and_reproduces():
    Q, T = er.cloud(), er.reference_cloud()
    cq, ct = er.classify(Q, DATA_REGION, er.MOTION), er.classify(T, REF_REGION)
    a, b = _fusion(), _fusion(er.substituted(Q, cq), er.substituted(T, ct))
    a.set_region("data", DATA_REGION)
    a.set_region("reference", REF_REGION)
    (ra, reca), (rb, recb) = _align(a, True, 3, er.MOTION), _align(b, True, 3, er.MOTION)
    assert reca[0] == recb[0] and ra.records[0].words[1] == (cq == 0).sum()
    assert _align(a, True, 3, er.MOTION)[1] == reca
    a.close()
    b.close()


# ---- 3. queries only

def test_queries_only_keeps_the_targets():
    """DTU's completeness: reference queries against the whole reconstruction; and its accuracy: only observed data points
    are queries."""
    Q, T = er.cloud(), er.reference_cloud()
    cq = er.classify(Q, DATA_REGION)
    a = _fusion()
    a.set_region("data", DATA_REGION, queries_only=True)
    assert a.region("data") == {"queries_only": True, "n_planes": 0, "n_vertices": 9, "dims": er.GRID_DIMS}
    sub, whole = _fusion(er.substituted(Q, cq), T), _fusion()
    _same(_distance(a, "scene", "data_to_ref"), _distance(sub, "scene", "data_to_ref"), "accuracy: queries are cropped")
    _same(_distance(a, "scene", "ref_to_data"), _distance(whole, "scene", "ref_to_data"), "completeness: targets are whole")
    assert _distance(sub, "scene", "ref_to_data")[2] != _distance(whole, "scene", "ref_to_data")[2]
    for fu in (a, sub, whole):
        fu.close()


# ---- 4. forced cells

def test_forced_cells_do_not_change_regioned_results():
    a = _fusion()
    a.set_region("data", DATA_REGION)
    a.set_region("reference", REF_REGION)
    want = {d: _distance(a, "scene", d) for d in cd.DIRECTIONS}
    for cell in (0.011, 0.37):
        a.distance_grid(cell)
        for d in cd.DIRECTIONS:
            _same(_distance(a, "scene", d), want[d], f"cell {cell} {d}")
        assert a.distance_grid(cell)["cell"] == F32(cell)
    a.close()


# ---- 5. errors and lifetimes

def _gone(fu):
    """Which of the distance, surface, point-align, plane-align and class results refuse a one-element read."""
    L, h = fu.L, fu.h
    return {"distance": L.acmmp_fusion_distance_results(h, 0, 1, None, None) == 1,
            "surface": L.acmmp_fusion_surface_results(h, 0, 1, None, None) == 1,
            "align": L.acmmp_fusion_align_records(h, 0, 1, None, None, None) == 1,
            "align_plane": L.acmmp_fusion_align_plane_records(h, 0, 1, None, None, None) == 1,
            "classes": L.acmmp_fusion_region_classes(h, 0, 1, None) == 1}


def _measure(fu, plane=False):
    fu.cloud_distance("scene", "data_to_ref", MAX_DIST, TAUS)
    fu.surface_distance("scene", 0.2, ())
    _align(fu, plane, 1)
    fu.region_classify("scene")


def test_invalid_arguments_leave_the_object_as_it_was():
    fu = _fusion()
    fu.set_mesh(*_mesh())
    fu.set_region("data", DATA_REGION)
    _measure(fu)
    before = (fu.region("data"), fu.region("reference"), fu.region_classes().tobytes(), _gone(fu))
    good, keep = capi.region_struct(er.region(**ALL))
    nan, inf = float("nan"), float("inf")

    def bad(**kw):
        st = capi.RegionStruct.from_buffer_copy(good)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(st, k)[v[0]] = v[1]
            else:
                setattr(st, k, v)
        return st
    cases = [bad(n_planes=9), bad(n_planes=-1), bad(n_vertices=2), bad(n_vertices=257), bad(n_vertices=-3), bad(axis=3),
             bad(axis=-1), bad(dims=(0, 0)), bad(dims=(1, 4097)), bad(dims=(2, -1)), bad(planes=(5, nan)), bad(planes=(31, inf)),
             bad(axis_min=nan), bad(axis_max=-inf), bad(axis_min=1.0, axis_max=0.5), bad(origin=(1, nan)), bad(cell=nan),
             bad(cell=inf), bad(cell=0.0), bad(cell=-0.125), bad(polygon=None), bad(bits=None)]
    poly = np.array(er.POLYGON)
    poly[4, 1] = np.inf
    cases.append(bad(polygon=poly.ctypes.data))
    for st in cases:
        for side in (0, 1):
            assert fu.L.acmmp_fusion_set_region(fu.h, side, C.byref(st), 0) == 1
    for side, flags in ((2, 0), (-1, 0), (0, 2), (1, -1), (0, 3)):
        assert fu.L.acmmp_fusion_set_region(fu.h, side, C.byref(good), flags) == 1
        assert fu.L.acmmp_fusion_set_region(fu.h, side, None, flags) == 1
    assert fu.L.acmmp_fusion_get_region(fu.h, 2, None, None, None, None, None) == 1
    assert fu.L.acmmp_fusion_region_classify(fu.h, 7, None) == 1 and fu.L.acmmp_fusion_region_classify(fu.h, 1, None) == 1
    assert (fu.region("data"), fu.region("reference"), fu.region_classes().tobytes(), _gone(fu)) == before
    assert before[3] == {"distance": False, "surface": False, "align": False, "align_plane": True, "classes": False}
    # absent parts are not looked at: non-finite numbers and NULL arrays there are no error
    absent = capi.RegionStruct()
    absent.n_planes, absent.planes[7], absent.axis_min, absent.cell, absent.axis = 1, nan, nan, -1.0, 9
    assert fu.L.acmmp_fusion_set_region(fu.h, 1, C.byref(absent), 0) == 0
    assert fu.region("reference") == {"queries_only": False, "n_planes": 1, "n_vertices": 0, "dims": (0, 0, 0)}
    del keep
    fu.close()


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_set_and_clear_discard_what_was_measured_and_keep_the_rest(plane):
    fu = _fusion()
    fu.set_mesh(*_mesh())
    fu.set_cloud_transform(er.MOTION)
    held = "align_plane" if plane else "align"
    for change in (lambda: fu.set_region("data", DATA_REGION), lambda: fu.set_region("data", None),
                   lambda: fu.set_region("reference", REF_REGION, queries_only=True), lambda: fu.set_region("reference", None)):
        _measure(fu, plane)
        assert not any(v for k, v in _gone(fu).items() if k in ("distance", "surface", held, "classes"))
        change()
        assert all(_gone(fu).values())
        # the sources, the reference cloud and the transform stay
        assert np.array_equal(fu.cloud_transform(), er.MOTION)
        assert np.asarray(fu.scene_points(0, er.N_CLOUD)).tobytes() == er.as_points(er.cloud()).tobytes()
        assert fu.cloud_distance("scene", "ref_to_data", MAX_DIST, ()).n_query == len(er.reference_cloud())
    fu.close()


def test_class_result_and_region_lifetimes():
    fu = _fusion()
    fu.set_region("data", DATA_REGION)
    fu.set_region("reference", REF_REGION)
    # the classes of a data cloud go with the cloud and with the transform; the reference's only with the reference
    fu.region_classify("scene")
    fu.set_cloud_transform(er.MOTION)
    assert _gone(fu)["classes"]
    fu.region_classify("scene")
    fu.set_reference_cloud(er.reference_cloud())
    assert not _gone(fu)["classes"]
    fu.set_scene(er.as_points(er.cloud()[::-1]))
    assert _gone(fu)["classes"]
    fu.region_classify("reference")
    fu.set_cloud_transform(None)
    fu.set_scene(er.as_points(er.cloud()))
    assert not _gone(fu)["classes"]
    fu.set_reference_cloud(er.reference_cloud())
    assert _gone(fu)["classes"]
    # the regions survive all of it
    assert fu.region("data") == {"queries_only": False, "n_planes": 0, "n_vertices": 9, "dims": er.GRID_DIMS}
    assert fu.region("reference") == {"queries_only": False, "n_planes": 8, "n_vertices": 3, "dims": (0, 0, 0)}
    n, cls = _classes(fu, "scene")
    assert cls.tobytes() == er.classify(er.cloud(), DATA_REGION).tobytes()
    r = fu.cloud_distance("scene", "data_to_ref", MAX_DIST, TAUS)
    assert r.n_valid == n["inside"] and r.n_query == n["points"]
    # the measuring calls write a scratch of their own: the class result is as it was
    assert fu.region_classes().tobytes() == cls.tobytes()
    fu.close()
