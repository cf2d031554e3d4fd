"""The numpy restatement of the cloud alignment (cloud_align_support) checked against itself and against the constants of
capi: the split sums, the reflection guard, the degenerate cases, the stride, the composition order, convergence."""
import numpy as np
import pytest

import cloud_align_support as ca
import cloud_distance_support as cd
from acmmp import capi

F32 = np.float32


def test_constants_match_capi():
    assert tuple(capi.ALIGN_MODES) == ca.MODES and list(capi.ALIGN_MODES.values()) == [0, 1]
    assert capi.ALIGN_STOP_REASONS == ca.STOP_REASONS and capi.ALIGN_RECORD_WORDS == ca.RECORD_WORDS
    for name in ("acmmp_fusion_set_cloud_transform", "acmmp_fusion_get_cloud_transform", "acmmp_fusion_cloud_align",
                 "acmmp_fusion_align_records"):
        assert name in capi.EXPORTS
    for method in ("set_cloud_transform", "cloud_transform", "cloud_align", "align_records"):
        assert callable(getattr(capi.Fusion, method)) and callable(getattr(ca.RestatedAlignFusion, method))
    r = capi.AlignRecord(words=np.arange(32, dtype=np.int64), M=ca.IDENTITY, shift=0.0, max_dist=0.5)
    s = ca.Record(np.arange(32, dtype=np.int64), ca.IDENTITY, 0.0, 0.5)
    for field in ("n_query", "n_valid", "n_matched", "sum_q", "n_out_of_range", "n_pairs", "mean"):
        assert getattr(r, field) == getattr(s, field)


def test_transform_association_and_rounding():
    M = np.array([[0.1, 0.7, -0.3, 1e-3], [1e8, -1e8, 1.0, 0.5], [0.0, 0.0, 1e39, 0.0]])
    X = np.array([[1.0, 2.0, 3.0], [0.1, 0.1, 0.25], [np.nan, 0.0, 0.0], [1.0, 1.0, 1.0]], F32)
    got = ca.transform_points(M, X)
    assert got.dtype == F32
    x = X.astype(np.float64)
    assert got[0, 0] == F32(((0.1 * x[0, 0] + 0.7 * x[0, 1]) + -0.3 * x[0, 2]) + 1e-3)
    assert got[1, 1] == F32(((1e8 * x[1, 0] + -1e8 * x[1, 1]) + x[1, 2]) + 0.5) == F32(0.75)     # the sum of the first two first
    assert np.isinf(got[3, 2]) and np.isnan(got[2]).all()                   # 1e39 leaves float32; 0 * nan is nan
    assert np.array_equal(ca.transform_points(ca.IDENTITY, X[:2]), X[:2])


def test_split_sums_equal_direct_sums():
    rng = np.random.default_rng(1)
    lim = 2 ** 30 - 1
    P = [tuple(int(v) for v in row) for row in rng.integers(-lim, lim, (500, 3), endpoint=True)]
    Q = [tuple(int(v) for v in row) for row in rng.integers(-lim, lim, (500, 3), endpoint=True)]
    P[0], Q[0], P[1], Q[1] = (lim,) * 3, (-lim,) * 3, (-lim,) * 3, (-lim,) * 3
    w = ca.pair_moments(P, Q)
    assert w[ca.N_PAIRS] == 500
    for a in range(3):
        assert w[ca.SUM_P + a] == sum(p[a] for p in P) and w[ca.SUM_Q3 + a] == sum(q[a] for q in Q)
        for b in range(3):
            at = ca.PQ + 2 * (3 * a + b)
            assert ca.join(w, at) == sum(p[a] * q[b] for p, q in zip(P, Q))
            assert 0 <= w[at + 1] < 500 * 2 ** 32
    assert ca.join(w, ca.PP) == sum(p[0] ** 2 + p[1] ** 2 + p[2] ** 2 for p in P)
    # the header's bounds: one pair's words at the edge of the range, times 2^31 - 1 pairs, inside int64
    worst = 3 * lim * lim
    assert (worst >> 32) * (2 ** 31 - 1) < 2 ** 63 and 0xffffffff * (2 ** 31 - 1) < 2 ** 63 and lim * (2 ** 31 - 1) < 2 ** 63


def _record_of_pairs(X, Y, c, max_dist):
    """The record of the given correspondences (no matching): the points quantised as step 2 does."""
    kq = 65536.0 / float(F32(max_dist))
    P = [tuple(int(v) for v in row) for row in ca.quantise(X, c, kq)]
    Q = [tuple(int(v) for v in row) for row in ca.quantise(Y, c, kq)]
    return ca.pair_moments(P, Q)


@pytest.mark.parametrize("mode", ca.MODES)
def test_fit_recovers_a_known_motion_and_guards_against_reflection(mode):
    rng = np.random.default_rng(2)
    known = ca.known_transform(mode)
    c = np.zeros(3)
    for name, X in (("volume", rng.random((400, 3), dtype=F32)),
                    ("nearly planar", np.concatenate([rng.random((400, 2), dtype=F32),
                                                      (1e-4 * rng.standard_normal((400, 1))).astype(F32)], 1)),
                    ("planar", np.concatenate([rng.random((400, 2), dtype=F32), np.zeros((400, 1), F32)], 1))):
        Y = ca.transform_points(known, X)
        noise = (2e-4 * rng.standard_normal(Y.shape)).astype(F32)           # enough to turn the smallest singular pair
        D = ca.fit(_record_of_pairs(X, Y + noise, c, 0.04), c, 0.04, mode)
        R = D[:, :3] / np.cbrt(np.linalg.det(D[:, :3]))
        print(name, mode, "det", np.linalg.det(D[:, :3]), "error", np.abs(D - known).max())
        assert np.linalg.det(D[:, :3]) > 0 and np.allclose(R @ R.T, np.eye(3), atol=1e-12), name
        assert np.abs(D[:, :2] - known[:, :2]).max() < 2e-3, name          # the in-plane part is determined in every case
    # a mirrored cloud: the best orthogonal map is a reflection, the fit returns a rotation all the same
    X = rng.random((400, 3), dtype=F32)
    D = ca.fit(_record_of_pairs(X, X * np.array([1, 1, -1], F32), c, 0.04), c, 0.04, "rigid")
    assert np.isclose(np.linalg.det(D[:, :3]), 1.0)


def test_degenerate_cases():
    c = np.zeros(3)
    t = np.linspace(0, 1, 50, dtype=F32)[:, None]
    line = t * np.array([[1.0, 2.0, 0.5]], F32)
    assert ca.fit(_record_of_pairs(line, line, c, 0.04), c, 0.04, "rigid") is None          # collinear
    one = np.repeat(np.array([[0.25, 0.5, 0.75]], F32), 10, 0)
    assert ca.fit(_record_of_pairs(one, one, c, 0.04), c, 0.04, "rigid") is None            # var = 0
    X = np.random.default_rng(0).random((2, 3), dtype=F32)
    assert ca.fit(_record_of_pairs(X, X, c, 0.04), c, 0.04, "rigid") is None                # N < 3
    assert ca.fit(_record_of_pairs(X[:0], X[:0], c, 0.04), c, 0.04, "similarity") is None
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32)
    assert ca.fit(_record_of_pairs(tri, tri, c, 0.04), c, 0.04, "rigid") is not None        # three points in a plane do
    far = np.full((5, 3), 100.0, F32)                                       # nothing within max_dist: N = 0
    r = ca.align(far, tri, "rigid", 0.04, 5, init=ca.SMALL_ROTATION)
    assert r.stop_reason == "degenerate" and r.iterations == 1 and np.array_equal(r.M, ca.SMALL_ROTATION)
    assert r.records[0].n_pairs == 0 and r.records[0].n_valid == 5 and r.records[0].shift == 0.0


def test_stride_picks_every_nth_point():
    Q, T = cd.clouds()
    for stride in (1, 3, 7, len(Q) + 5):
        w = ca.iteration_record(ca.IDENTITY, Q, T, cd.MAX_DIST, stride)
        want = cd.distances(Q[np.arange(0, len(Q), stride)], T, cd.MAX_DIST)[2]
        assert w[:4] == want[:4] and w[ca.N_QUERY] == -(-len(Q) // stride)
    marked = np.full((10, 3), 100.0, F32)                                   # only the indices 0, 4, 8 can match
    marked[[0, 4, 8]] = [[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.3, 0.3, 0.3]]
    w = ca.iteration_record(ca.IDENTITY, marked, marked[[0, 4, 8]], 0.04, 4)
    assert w[ca.N_QUERY] == 3 and w[ca.N_MATCHED] == 3
    assert ca.iteration_record(ca.IDENTITY, marked, marked[[0, 4, 8]], 0.04, 3)[ca.N_MATCHED] == 1


def test_out_of_range_pairs_enter_no_moment():
    Q, T = cd.clouds()
    w = ca.iteration_record(ca.IDENTITY, Q, T, cd.MAX_DIST)
    assert w[ca.N_OUT_OF_RANGE] >= 1 and w[ca.N_PAIRS] + w[ca.N_OUT_OF_RANGE] == w[ca.N_MATCHED]
    assert max(abs(w[ca.SUM_P + a]) for a in range(3)) < w[ca.N_PAIRS] * 2 ** 30


def test_composition_order():
    A = ca.about(ca.rotation((0, 0, 1), 90.0), (0, 0, 0), (1, 0, 0))        # turn about z, then move along x
    B = ca.about(np.eye(3), (0, 0, 0), (0, 2, 0), 2.0)                      # scale by 2, then move along y
    x = np.array([[1.0, 0.0, 0.0]], F32)
    AB = ca.compose(A, B)                                                   # B first
    assert np.allclose(ca.transform_points(AB, x), ca.transform_points(A, ca.transform_points(B, x)))
    assert np.allclose(ca.transform_points(AB, x), [[-1.0, 2.0, 0.0]]) and not np.allclose(AB, ca.compose(B, A))
    assert np.allclose(ca.compose(ca.inverse(A), A), ca.IDENTITY) and ca.corner_shift(ca.IDENTITY, np.zeros(3), np.ones(3)) == 0.0
    assert np.isclose(ca.corner_shift(ca.about(np.eye(3), (0, 0, 0), (3, 4, 0)), np.zeros(3), np.ones(3)), 5.0)


@pytest.mark.parametrize("mode", ca.MODES)
def test_convergence_on_the_recovery_clouds(mode):
    data, ref, known = ca.recovery_clouds(mode)
    r = ca.restated_recovery(mode)
    means = [rec.mean for rec in r.records]
    share = [rec.n_matched / rec.n_valid for rec in r.records]
    err = np.abs(r.M - known).max()
    print(mode, "means", means, "matched share", share, "error", err, "stop", r.stop_reason)
    assert r.iterations == 10 and r.stop_reason == "max_iterations"
    assert min(share) >= 0.85
    assert means[0] > 1e-2 and means[-1] < 2.5e-3 and err < 2e-3
    last, before = r.records[-1], r.records[-2]                             # the record has all but stopped changing
    assert last.n_matched == before.n_matched and abs(last.mean - before.mean) < 1e-6 * before.mean and last.shift < 1e-4
    for rec in r.records:                                                   # well-conditioned throughout
        d = ca.svd_parts(rec.words)[2]
        assert d[1] / d[0] >= 0.4
    again = ca.align(data, ref, mode, cd.MAX_DIST, 10, min_shift=1e-4)      # and with a min_shift it stops early
    assert again.stop_reason == "converged" and again.iterations < 10 and again.records[-1].shift <= 1e-4
