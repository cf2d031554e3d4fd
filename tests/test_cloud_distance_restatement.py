"""The numpy restatement of acmmp_fusion_cloud_distance (cloud_distance_support), pinned by properties of the definition
in include/acmmp.h; and the condition on the clouds that the GPU tests measure."""
import numpy as np
import pytest

import cloud_distance_support as cd

F32 = np.float32


def test_a_cloud_against_itself():
    rng = np.random.default_rng(1)
    P = rng.random((300, 3), dtype=F32)
    P[[50, 120, 299]] = P[7]                                              # exact duplicates: the lowest index wins
    d2, nn, s = cd.distances(P, P, 0.5, (0.0, 0.5))
    assert (d2 == 0).all() and d2.dtype == F32 and nn.dtype == np.int32
    want = np.arange(300)
    want[[50, 120, 299]] = 7
    assert np.array_equal(nn, want)
    assert s[:4] == [300, 300, 300, 0] and s[4:6] == [300, 300] and s[12] == 300 and sum(s[12:]) == 300


def test_rigid_shift_of_a_lattice():
    g = np.arange(6, dtype=F32)
    T = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)  # spacing 1: well separated for a shift of 0.125
    s = F32(0.125)
    Q = T + np.array([s, 0, 0], F32)
    d2, nn, summ = cd.distances(Q, T, 0.5, (0.125, 0.1))
    assert (d2 == s * s).all() and np.array_equal(nn, np.arange(len(T)))
    k = 1048576.0 / 0.5
    assert summ[3] == len(T) * int(np.rint(0.125 * k)) and summ[4:6] == [len(T), 0]
    # a shift that is not exact in float32: d2 is the float32 square of the float32 difference, whatever that is
    Q = (T + np.array([F32(0.1), 0, 0], F32)).astype(F32)
    d2, nn, _ = cd.distances(Q, T, 0.5)
    dx = Q[:, 0] - T[:, 0]
    assert np.array_equal(d2, dx * dx) and np.array_equal(nn, np.arange(len(T)))


def test_exact_tie_goes_to_the_lower_index():
    T = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, -1]], F32)
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1]):
        d2, nn, _ = cd.distances(np.zeros((1, 3), F32), T[order], 2.0)
        assert d2[0] == 1 and nn[0] == 0
    d2, nn, _ = cd.distances(np.zeros((1, 3), F32), np.concatenate([T * F32(1.5), T[2:3]]), 2.0)
    assert d2[0] == 1 and nn[0] == 4                                      # a strictly nearer target wins whatever its index


def test_the_cap_is_inclusive():
    md = F32(0.5)
    m2 = md * md
    # (0.5 - 2^-25)^2 rounds to 0.25 - 2^-25 and 2^-24 on top of it is 0.25 + 2^-25: one float32 step beyond m2
    Q = np.array([[0.5, 0, 0], [0.5 - 2.0 ** -25, 2.0 ** -12, 0]], F32)
    T = np.zeros((1, 3), F32)
    assert cd.pair_d2(Q, T)[:, 0].tolist() == [m2, np.nextafter(m2, F32(1))]
    d2, nn, s = cd.distances(Q, T, md, (md,))
    assert d2[0] == m2 and nn[0] == 0 and np.isinf(d2[1]) and nn[1] == -1
    assert s[:3] == [2, 2, 1] and s[4] == 1 and s[12 + 255] == 1          # q = 2^20: the last bin


def test_non_finite_points():
    T = np.array([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0.25, 0, 0], [0, 0, -np.inf]], F32)
    Q = np.array([[0.2, 0, 0], [np.nan, 0, 0], [0, 0, np.inf], [5, 5, 5]], F32)
    d2, nn, s = cd.distances(Q, T, 1.0, (1.0,))
    assert nn.tolist() == [3, -1, -1, -1] and np.isinf(d2[1:]).all()      # target indices count the invalid targets too
    assert s[:3] == [4, 2, 1]
    d2, nn, s = cd.distances(Q, T[[1, 2, 4]], 1.0)                        # no valid target: nothing is matched
    assert (nn == -1).all() and np.isinf(d2).all() and s[:4] == [4, 2, 0, 0] and sum(s[4:]) == 0
    d2, nn, s = cd.distances(np.zeros((0, 3), F32), T, 1.0)
    assert len(d2) == 0 and s == [0] * cd.SUMMARY_WORDS
    big = np.array([[3e38, 3e38, 3e38]], F32)
    d2, nn, s = cd.distances(big, -big, 1.0)                              # the pair distance overflows: +inf, never NaN
    assert np.isinf(d2[0]) and nn[0] == -1 and s[:3] == [1, 1, 0]


def test_arguments():
    P = np.zeros((1, 3), F32)
    for md, taus in ((0.0, ()), (-1.0, ()), (np.nan, ()), (np.inf, ()), (1.0, (2.0,)), (1.0, (-0.5,)), (1.0, (np.nan,)),
                     (1.0, (0.1,) * 9)):
        with pytest.raises(ValueError):
            cd.distances(P, P, md, taus)


@pytest.mark.parametrize("direction", cd.DIRECTIONS)
def test_summary_properties(direction):
    d2, nn, s = cd.restated(direction)
    matched = nn >= 0
    assert s[2] == matched.sum() and sum(s[12:]) == s[2]                  # sum(hist) == n_matched
    within = s[4:12]
    assert list(cd.TAUS) == sorted(cd.TAUS) and within == sorted(within)  # monotone in tau
    assert within[-1] == s[2] and 0 < within[0] < within[3] < within[-1]  # tau = max_dist counts every match; 0 the duplicates
    assert np.isinf(d2[~matched]).all() and (d2[matched] <= F32(cd.MAX_DIST) * F32(cd.MAX_DIST)).all()


@pytest.mark.parametrize("offset", [0.0, 1e4])
@pytest.mark.parametrize("direction", cd.DIRECTIONS)
def test_generator_matched_share(direction, offset):
    """The clouds of the GPU tests keep the matched share of the valid queries between 20% and 80%, so both branches of
    step 4 are exercised; they hold duplicates, ties, outliers and non-finite points on both sides."""
    d2, nn, s = cd.restated(direction, offset)
    assert 0.2 <= s[2] / s[1] <= 0.8
    assert s[1] < s[0]                                                    # invalid queries
    Q, T = cd.clouds()
    assert 2900 <= len(Q) <= 3100 and 3900 <= len(T) <= 4100
    for P in (Q, T):
        assert len(np.unique(P[cd.valid(P)], axis=0)) < cd.valid(P).sum() and np.abs(P[cd.valid(P)]).max() > 50
    if offset == 0.0 and direction == "data_to_ref":
        q = int(np.nonzero((Q == np.array([0.5, 0.25, -0.5], F32)).all(1))[0][0])
        tied = np.nonzero(cd.pair_d2(Q[q:q + 1], T)[0] == d2[q])[0]
        assert len(tied) == 4 and nn[q] == tied.min()                     # a four-way tie, resolved to the lowest index
