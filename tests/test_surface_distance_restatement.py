"""The numpy restatement of acmmp_fusion_surface_distance (surface_distance_support), pinned by properties that do not
depend on it: distances to one triangle known in closed form, a bracket from a dense sample of the face, the unit cube's
analytic surface distance, the claim the call exists for, ties, the cap, invalid and degenerate input, and the
inequality the device's skips rest on."""
import numpy as np
import pytest

import cloud_distance_support as cd
import mesh_render_support as rs
import surface_distance_support as sd

F32, F64 = np.float32, np.float64
TRI = rs.as_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]])


def _d2(queries, mesh=TRI, max_dist=100.0):
    return sd.distances(np.asarray(queries, F32), *mesh, max_dist)


def test_one_triangle_regions():
    """Every coordinate is a small dyadic number, so every operation of step 3 is exact and so is the comparison."""
    cases = [((0.25, 0.25, 0.5), 0.25), ((0.25, 0.5, -2.0), 4.0),                     # above and below the interior
             ((0.5, -1.0, 0.0), 1.0), ((-1.0, 0.5, 0.0), 1.0), ((1.0, 1.0, 0.0), 0.5),   # beyond AB, AC, BC
             ((0.5, -1.0, 1.0), 2.0), ((1.0, 1.0, 0.5), 0.75),
             ((-1.0, -1.0, 0.0), 2.0), ((2.0, -1.0, 0.0), 2.0), ((-1.0, 2.0, 0.0), 2.0),  # beyond A, B, C
             ((3.0, 0.0, 0.0), 4.0), ((0.0, 3.0, 2.0), 8.0), ((-2.0, 0.0, 0.0), 4.0),
             ((0.25, 0.25, 0.0), 0.0), ((0.5, 0.0, 0.0), 0.0), ((0.5, 0.5, 0.0), 0.0),    # on the face, two edges
             ((0.0, 0.0, 0.0), 0.0), ((1.0, 0.0, 0.0), 0.0), ((0.0, 1.0, 0.0), 0.0)]     # the vertices
    d2, nn, summary, skipped = _d2([c[0] for c in cases])
    assert d2.tolist() == [c[1] for c in cases] and (nn == 0).all() and skipped == 0
    assert summary[:3] == [len(cases)] * 3
    # the same under every order of the corners
    for order in ([1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0], [1, 0, 2]):
        assert _d2([c[0] for c in cases], (TRI[0], np.array([order], np.int32)))[0].tolist() == [c[1] for c in cases]


def test_dense_sample_bracket():
    """For random triangles and queries the true distance t satisfies lattice_min - spacing <= t <= lattice_min: the
    lattice points (iA + jB + kC) / N lie on the face, and every point of the face is within one lattice cell --
    longest edge / N -- of one.  The restated float32 D2 is t^2 up to its one float32 rounding (2^-24, so 2^-25 on the
    root) and float64 noise far below it for coordinates of order 1 and distances above 0.01; 2^-23 covers both."""
    rng = np.random.default_rng(11)
    N = 64
    i, j = np.meshgrid(np.arange(N + 1), np.arange(N + 1), indexing="ij")
    keep = i + j <= N
    w = np.stack([i[keep], j[keep], N - i[keep] - j[keep]], 1).astype(F64) / N
    checked = 0
    for _ in range(60):
        tri = rng.standard_normal((3, 3)).astype(F32)
        Q = (2.0 * rng.standard_normal((40, 3))).astype(F32)
        d2 = _d2(Q, rs.as_mesh(tri, [[0, 1, 2]]))[0].astype(F64)
        lattice = w @ tri.astype(F64)
        dmin = np.sqrt(((Q.astype(F64)[:, None, :] - lattice[None]) ** 2).sum(2)).min(1)
        edges = tri.astype(F64) - np.roll(tri.astype(F64), 1, 0)
        spacing = np.sqrt((edges ** 2).sum(1)).max() / N
        far = dmin > 0.01 + spacing
        got = np.sqrt(d2[far])
        assert (got <= dmin[far] * (1 + 2.0 ** -23)).all()
        assert (got >= (dmin[far] - spacing) * (1 - 2.0 ** -23)).all()
        checked += int(far.sum())
    assert checked > 2000


def test_unit_cube_lattice():
    """Queries on a lattice inside and outside the 12-face cube: sqrt(d2) within one float32 ulp of the box-surface
    distance (the bound test_mesh_render_restatement.py uses for its ray-box depths)."""
    g = np.linspace(-1.0, 1.0, 9)
    shifted = g + 0.0625
    Q = np.concatenate([np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3) for a in (g, shifted)]).astype(F32)
    d2, nn, summary, _ = _d2(Q, sd.cube())
    want = sd.cube_surface_distance(Q)
    got = np.sqrt(d2.astype(F64))
    assert (nn >= 0).all() and summary[2] == len(Q)
    assert (np.abs(got - want) <= np.spacing(want.astype(F32)).astype(F64)).all()
    inside = (np.abs(Q) < 0.5).all(1)
    assert inside.sum() > 50 and (~inside).sum() > 500 and (want[inside] > 0).all()


def test_the_claim():
    """Reference points on the cube's faces lie on the surface -- up to the float32 rounding of coordinates below 1 --
    and a long way from its eight vertices."""
    P = sd.cube_surface_points(2000)
    v, f = sd.cube()
    d2, nn, summary, _ = sd.distances(P, v, f, 0.25)
    assert summary[2] == len(P) and (nn >= 0).all()
    assert (d2.astype(F64) <= (2.0 ** -22) ** 2).all()
    words = cd.distances(P, v, 2.0)[2]
    vertex_only = cd.Summary(words, 2.0, 0)
    assert vertex_only.n_matched == len(P) and vertex_only.mean > 0.3


def test_ties_cap_and_invalid_input():
    v, f = TRI
    twice = np.concatenate([f, f, f])
    Q = np.array([[0.25, 0.25, 0.5], [2, 2, 2], [0.5, 0.5, 0]], F32)
    assert (_d2(Q, (v, twice))[1] == 0).all()                              # a duplicated face loses to its lower index
    assert (_d2(Q, (v, np.concatenate([f[:, ::-1], f])))[1] == 0).all()
    # the cap is inclusive; one float32 step beyond it is unmatched
    step = np.nextafter(F32(0.5), F32(1))
    d2, nn, summary, _ = sd.distances(np.array([[0.25, 0.25, 0.5], [0.25, 0.25, step]], F32), v, f, 0.5, (0.5,))
    assert nn.tolist() == [0, -1] and d2.tolist() == [0.25, np.inf] and summary[:5] == [2, 2, 1, 1048576, 1]
    assert sd.distances(Q[:1], v, f, np.nextafter(F32(0.5), F32(0)))[1].tolist() == [-1]
    # a non-finite query is skipped, a non-finite vertex makes its face invalid
    bad_q = np.array([[np.nan, 0, 0], [0.25, 0.25, 1], [0, np.inf, 0], [0.25, 0.25, -1]], F32)
    d2, nn, summary, skipped = _d2(bad_q)
    assert nn.tolist() == [-1, 0, -1, 0] and d2.tolist() == [np.inf, 1.0, np.inf, 1.0] and summary[:3] == [4, 2, 2]
    v2, f2 = rs.as_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, np.nan], [np.inf, 0, 5]], [[0, 1, 3], [0, 1, 2], [4, 1, 2], [2, 1, 0]])
    d2, nn, summary, skipped = _d2(bad_q, (v2, f2))
    assert skipped == 2 and nn.tolist() == [-1, 1, -1, 1] and d2.tolist() == [np.inf, 1.0, np.inf, 1.0]
    d2, nn, summary, skipped = _d2(bad_q, (v2, f2[[0, 2]]))                # no valid face at all
    assert skipped == 2 and (nn == -1).all() and np.isinf(d2).all() and summary[:3] == [4, 2, 0]
    assert _d2(bad_q, (v2, f2[:0]))[2][:3] == [4, 2, 0] and _d2(bad_q[:0])[2][:3] == [0, 0, 0]


def test_degenerate_faces():
    """What the restatement does with degenerate faces.  A == B == C: every dot is 0, the first case applies and the
    face is the point A.  A == B: d1 = d3 = vc = 0; a query with dot(ac, ap) <= 0 takes the first case (the point A); any
    other reaches the third case, v = 0 / 0, and the face is no candidate for it -- the query goes to whatever other
    face there is, or stays unmatched.  No NaN reaches a result."""
    rng = np.random.default_rng(2)
    Q = rng.standard_normal((200, 3)).astype(F32)
    A = np.array([0.25, -0.5, 0.125], F32)
    d2, nn, _, skipped = _d2(Q, rs.as_mesh([A, A, A], [[0, 1, 2]]))
    e = A.astype(F64) - Q.astype(F64)
    assert skipped == 0 and (nn == 0).all()
    assert np.array_equal(d2, ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]).astype(F32))
    C = np.array([1.25, -0.5, 0.125], F32)
    needle = rs.as_mesh([A, A, C], [[0, 1, 2]])
    d2, nn, summary, _ = _d2(Q, needle)
    behind = ((C.astype(F64) - A) * (Q.astype(F64) - A)).sum(1) <= 0
    assert 20 < behind.sum() < 180
    assert (nn[behind] == 0).all() and (nn[~behind] == -1).all() and np.isinf(d2[~behind]).all()
    assert not np.isnan(d2).any() and summary[2] == behind.sum()
    assert np.isnan(sd.pair_d2(Q[~behind], A[None], A[None], C[None])).all()
    # with a proper face beside it the other queries go there
    v = np.concatenate([needle[0], TRI[0]])
    d2, nn, _, _ = _d2(Q, (v, np.array([[0, 1, 2], [3, 4, 5]], np.int32)))
    assert (nn[~behind] == 1).all() and not np.isnan(d2).any() and np.isfinite(d2).all()


@pytest.mark.parametrize("name", list(sd.gpu_test_meshes()))
def test_conservativeness(name):
    """The inequality the device's skips rest on, on every mesh of the GPU test, its vertices as float32 after step 1:
    a valid face whose vertex box is at least L from the query on an axis has D2 >= L * L * (1 - 2^-20) when
    L * L >= 2^-120.  A pair whose D2 is NaN is no candidate for any query, so a skip cannot lose it."""
    v, f, M = sd.gpu_test_meshes()[name]
    A, B, C, ok = sd.corners(v, f, M)
    A, B, C = A[ok], B[ok], C[ok]
    assert ok.any() and (ok.all() or name == "invalid and degenerate")
    X = np.stack([A, B, C], 1).astype(F64)
    lo, hi = X.min(1), X.max(1)
    rng = np.random.default_rng(4)
    centre, ext = (lo.min(0) + hi.max(0)) / 2, (hi.max(0) - lo.min(0)).max()
    near = sd.near_queries(np.concatenate([A, B, C]), np.arange(3 * len(A)).reshape(3, -1).T, 150, ext / 50, seed=9)
    Q = np.concatenate([near, (centre + ext * (rng.random((100, 3)) - 0.5) * 1.5).astype(F32), A[:25], C[:25]])
    checked = nans = 0
    for a in range(0, len(Q), 25):
        q = Q[a:a + 25]
        d2 = sd.pair_d2(q, A, B, C).astype(F64)
        p = q.astype(F64)[:, None, :]
        L = np.maximum(lo[None] - p, p - hi[None]).max(2)
        claim = (L > 0) & (L * L >= 2.0 ** -120) & ~np.isnan(d2)
        assert (d2[claim] >= (L * L * (1 - 2.0 ** -20))[claim]).all()
        checked += int(claim.sum())
        nans += int(np.isnan(d2).sum())
    assert checked > 500 and (nans > 0) == (name == "invalid and degenerate")
