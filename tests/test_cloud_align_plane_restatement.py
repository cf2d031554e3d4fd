"""The numpy restatement of acmmp_fusion_cloud_align_plane (cloud_align_plane_support) against what it must mean: the
split sums, the integer budget, the pivot, the normals, the degenerate cases, first-order recovery, pivot invariance, the
point-to-plane claim on two samplings of one surface, and the conditioning of the clouds the GPU fit test uses."""
import numpy as np
import pytest

import cloud_align_plane_support as cp
import cloud_align_support as ca
import cloud_distance_support as cd

F32 = np.float32
SOLVER_TOL = 1e-9                                  # per entry, times max(1, |entry|): the GPU fit test's bound


def _close(D, E):
    return (np.abs(D - E) <= SOLVER_TOL * np.maximum(1.0, np.abs(E))).all()


def test_split_sums_against_direct_sums():
    rng = np.random.default_rng(0)
    rows = []
    for _ in range(300):
        L = [int(v) for v in rng.integers(-2 ** 18, 2 ** 18, 3)]
        n = rng.standard_normal(3)
        Nn = [int(v) for v in np.rint(n / np.linalg.norm(n) * 4096.0)]
        D = [int(v) for v in rng.integers(-2 ** 17 + 1, 2 ** 17, 3)]
        rows.append(cp.row(L, Nn, D))
    w = cp.row_moments(rows)
    for k, (a, b) in enumerate(cp.CC_PAIRS):
        assert cp.join(w, cp.CC + 2 * k) == sum(c[a] * c[b] for c, _ in rows)
        assert 0 <= w[cp.CC + 2 * k + 1] < len(rows) * 2 ** 32
    for a in range(6):
        assert cp.join(w, cp.CR + 2 * a) == sum(c[a] * r for c, r in rows)
    assert cp.join(w, cp.RR) == sum(r * r for _, r in rows)
    assert any(cp.join(w, cp.CR + 2 * a) < 0 for a in range(6))            # negative products go through the split too
    assert cp.CC + 2 * len(cp.CC_PAIRS) == cp.CR and cp.CR + 12 == cp.RR and cp.RR + 2 == cp.RECORD_WORDS
    S, b = cp.system(w)
    assert np.array_equal(S, S.T) and S[0, 5] == float(sum(c[0] * c[5] for c, _ in rows)) and b[2] == -float(sum(c[2] * r for c, r in rows))


def test_extreme_rows_stay_inside_the_budget():
    """L = -2^18 on every axis, the quantised unit normals with the largest |Nn_1| + |Nn_2| and the largest single
    component, D at its bound: |c_a| < 2^31, |r| < 2^31, every product < 2^62, and 2^31 - 1 such pairs fit int64."""
    worst = 0
    d = 2 ** 17 - 1
    normals = [(0, 2896, 2896), (0, 2897, 2896), (0, -2897, 2896), (4096, 0, 0), (0, 0, -4096), (2365, 2365, 2365), (1, 4096, 1)]
    for Nn in normals:
        assert abs(np.linalg.norm(Nn) - 4096.0) <= np.sqrt(3) / 2                # something rint(unit * 4096) can give
        for L in ([-2 ** 18] * 3, [-2 ** 18, 2 ** 18 - 1, -2 ** 18], [2 ** 18 - 1, -2 ** 18, 2 ** 18 - 1]):
            for D in ([d, d, d], [-d, d, -d], [d, -d, -d]):
                c, r = cp.row(L, list(Nn), D)
                assert all(abs(v) < 2 ** 31 for v in c) and abs(r) < 2 ** 31
                worst = max(worst, max(abs(x * y) for x in c + [r] for y in c + [r]))
    assert worst < 2 ** 62
    n = 2 ** 31 - 1
    assert n * (worst >> 32) < 2 ** 63 and n * 0xffffffff < 2 ** 63
    assert (-2 ** 30 + 1) >> 12 == -2 ** 18 and (2 ** 30 - 1) >> 12 == 2 ** 18 - 1   # the lever of an in-range pair


def test_pivot_rounds_to_nearest_with_floor_division():
    assert cp.pivot([0, 0, 0], 0) == [0, 0, 0] and cp.pivot([5, -5, 7], 0) == [0, 0, 0]
    assert cp.pivot([10, 11, 12], 4) == [3, 3, 3]                          # 2.5 -> 3, 2.75 -> 3, 3 -> 3
    assert cp.pivot([-10, -11, -9], 4) == [-2, -3, -2]                     # -2.5 -> -2 (half up), -2.75 -> -3, -2.25 -> -2
    assert cp.pivot([-1, 1, 0], 2) == [0, 1, 0]                            # -0.5 -> 0, 0.5 -> 1
    big = 2 ** 61 - 3
    assert cp.pivot([big, -big, 1], 2 ** 31 - 1) == [(2 * big + 2 ** 31 - 1) // (2 ** 32 - 2), (-2 * big + 2 ** 31 - 1) // (2 ** 32 - 2), 0]
    for s, n in ((7, 3), (-7, 3), (-8, 3), (100, 7), (-100, 7)):
        assert cp.pivot([s, s, s], n)[0] == int(np.floor(s / n + 0.5))


def test_usable_unusable_and_unnormalised_normals():
    usable, Nn = cp.quantised_normals(ca.IDENTITY, cp.EDGE_NORMALS)
    # zero, NaN, inf, -inf: unusable; denormals, lengths 1e-3 and 1e3, 1e19, 3e38 (float64 holds their l2), 1e-30: usable
    assert usable.tolist() == [False] * 4 + [True] * 9
    assert Nn[4].tolist() == [4096, 0, 0] and Nn[6].tolist() == [4096, 0, 0] and Nn[8].tolist() == [4096, 0, 0]
    assert Nn[5].tolist() == [0, -3664, 1832]                              # two and one float32 denormal steps: (0, -2, 1) / sqrt(5)
    assert np.abs(Nn[7] - [0, 2457.6, -3276.8]).max() <= 0.5 + 1e-3 and np.abs(Nn[9] - [0, 2457.6, 3276.8]).max() <= 0.5 + 1e-3
    assert Nn[10].tolist() == Nn[11].tolist() == [2365, 2365, 2365] and Nn[12].tolist() == [2896, 2896, 0]
    assert (Nn[~usable] == 0).all()
    # an init that overflows l2 or flushes it to 0 makes the normal unusable
    huge, tiny = ca.IDENTITY * 1e300, ca.IDENTITY * 1e-150
    assert not cp.quantised_normals(huge, cp.EDGE_NORMALS[10:12])[0].any()
    assert not cp.quantised_normals(tiny, cp.EDGE_NORMALS[4:6])[0].any() and cp.quantised_normals(tiny, cp.EDGE_NORMALS[8:10])[0].all()
    # and one of scale 2 changes nothing: the normal is normalised after the transform
    rng = np.random.default_rng(3)
    n = rng.standard_normal((200, 3)).astype(F32)
    u1, N1 = cp.quantised_normals(ca.SMALL_ROTATION, n)
    M2 = ca.SMALL_ROTATION.copy()
    M2[:, :3] *= 2.0
    u2, N2 = cp.quantised_normals(M2, n)
    assert u1.all() and u2.all() and np.array_equal(N1, N2)
    R = ca.SMALL_ROTATION[:, :3]
    unit = (n / np.linalg.norm(n.astype(np.float64), axis=1)[:, None]) @ R.T
    assert np.abs(N1 - unit * 4096.0).max() <= 0.5 + 1e-6 and np.abs(N1).max() <= 4096
    # the counts of a record: an in-range pair with an unusable normal is n_no_normal, and enters nothing
    data, ref = cp.record_clouds()
    g = cp.point_pivot(ca.IDENTITY, data, ref, cd.MAX_DIST)
    w = cp.iteration_record(ca.IDENTITY, g, data, ref, cd.MAX_DIST)
    assert w[cp.N_NO_NORMAL] == 4 and w[cp.N_OUT_OF_RANGE] > 0 and w[cp.ZERO] == 0 and w[cp.PIVOT:cp.PIVOT + 3] == g
    assert w[cp.N_MATCHED] == w[cp.N_OUT_OF_RANGE] + w[cp.N_NO_NORMAL] + w[cp.N_PAIRS]
    assert w[:4] == ca.iteration_record(ca.IDENTITY, data[:, :3], ref, cd.MAX_DIST)[:4]


def _self_pairs(xyz, normals, max_dist, M=ca.IDENTITY):
    data, ref = cp.with_normals(xyz, normals), np.ascontiguousarray(xyz, F32)
    g = cp.point_pivot(M, data, ref, max_dist)
    return cp.iteration_record(M, g, data, ref, max_dist), ca.target_box(ref)[0]


def test_single_plane_and_too_few_pairs_are_degenerate():
    rng = np.random.default_rng(5)
    flat = np.zeros((400, 3), F32)
    flat[:, :2] = rng.random((400, 2), dtype=F32)
    w, c = _self_pairs(flat, [0, 0, 1], 0.05)
    assert w[cp.N_PAIRS] == 400 and cp.fit(w, c, 0.05) is None             # S_33 = S_44 = 0
    tilt = ca.rotation((1, 2, 0), 25.0)
    w, c = _self_pairs((flat.astype(np.float64) @ tilt.T).astype(F32), tilt[:, 2].astype(F32), 0.05)
    assert w[cp.N_PAIRS] == 400 and cp.fit(w, c, 0.05) is None             # a constant Nn: rank 3, exactly in integers
    print("tilted plane: lambda_max / lambda_min", cp.condition(w))
    cube, nrm = cp.cube_surface(5, rng)
    w, c = _self_pairs(cube, nrm, 0.05)
    assert w[cp.N_PAIRS] == 5 and cp.fit(w, c, 0.05) is None               # N < 6
    r = cp.align_plane(cp.with_normals(flat, [0, 0, 1]), flat, 0.05, 5, init=ca.SMALL_ROTATION)
    assert r.stop_reason == "degenerate" and r.iterations == 1 and r.M.tobytes() == ca.SMALL_ROTATION.tobytes()
    assert r.records[0].shift == 0.0


def test_a_sphere_is_degenerate():
    """A sphere's rotation columns (q - G) x n vanish up to the lever's rounding (one step is max_dist / 16), and the Jacobi
    scaling normalises that rounding to unit diagonal like any other column, so the eigenvalue rule alone does not see
    it: lambda_max / lambda_min is 1.2e3 on 2000 points of the unit sphere at max_dist 0.06, 39 at 0.5, 21 at 16, 2.1e3
    for 500 points of radius 0.25 at 0.02.  The noise-floor rule does: what the translation columns leave of the rotation
    block is 0.93 to 1.02 of the floor the rounding alone predicts on all four, and the rule asks for more than 4; the
    clouds of every other test are above 8 (a cube of a sixth of max_dist) and the GPU fit clouds above 6e4."""
    rng = np.random.default_rng(2)
    for n, radius, max_dist in ((2000, 1.0, 0.06), (2000, 1.0, 0.5), (500, 0.25, 0.02), (2000, 1.0, 16.0)):
        v = rng.standard_normal((n, 3))
        v /= np.linalg.norm(v, axis=1)[:, None]
        w, c = _self_pairs((radius * v + 0.5).astype(F32), v.astype(F32), max_dist)
        ratio = cp.rotation_over_noise(w)
        print("sphere", n, radius, max_dist, "N", w[cp.N_PAIRS], "lambda_max / lambda_min", cp.condition(w), "over the floor", ratio)
        assert w[cp.N_PAIRS] == n and cp.condition(w) < 2.0 ** 40 and 0.5 < ratio < 2.0   # the floor is the rounding's, as derived
        assert cp.fit(w, c, max_dist) is None
    # a cube a sixth of max_dist across still has levers above the floor: the rule does not take small objects
    xyz, nrm = cp.cube_surface(2000, rng)
    w, c = _self_pairs((xyz * F32(0.01)).astype(F32), nrm, 0.06)
    print("cube of 0.01 at max_dist 0.06: over the floor", cp.rotation_over_noise(w))
    assert cp.rotation_over_noise(w) > 8.0 and cp.fit(w, c, 0.06) is not None


def test_one_iteration_recovers_a_small_motion_to_first_order():
    """Exact correspondences, exact normals.  What is left after one step is second order: theta^2 |x| ~ (3.5e-3)^2 * 0.87
    = 1.1e-5 from the linearisation, theta * max_dist / 16 = 1.1e-5 from the lever's quantisation, |d| / 4096 ~ 1e-6 from
    the normal's: under 3e-5 in all, 1% of the 4e-3 the motion moves a corner."""
    rng = np.random.default_rng(7)
    cell = (np.stack(np.meshgrid(np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 2) + 0.5) / 10
    ref, nrm = np.zeros((600, 3), F32), np.zeros((600, 3), F32)            # a jittered 10 x 10 grid per face: no close pairs
    for f in range(6):
        part = slice(100 * f, 100 * f + 100)
        ref[part, f // 2] = f % 2
        ref[part, [a for a in range(3) if a != f // 2]] = cell + 0.04 * (rng.random((100, 2)) - 0.5)
        nrm[part, f // 2] = 2 * (f % 2) - 1
    known =ca.about(ca.rotation((2, -1, 3), 0.2), (0.5, 0.5, 0.5), (0.0008, -0.0006, 0.0005))
    inv = ca.inverse(known)
    data = cp.with_normals(ca.transform_points(inv, ref), (nrm.astype(np.float64) @ inv[:, :3].T).astype(F32))
    r = cp.align_plane(data, ref, 0.05, 1)
    d2, nn, _ = cd.distances(ca.transform_points(ca.IDENTITY, data[:, :3]), ref, 0.05)
    assert np.array_equal(nn, np.arange(len(ref)))                         # every pair is the true one
    before, after = cp.corner_error(ca.IDENTITY, known), cp.corner_error(r.M, known)
    print("corner error", before, "->", after, "rms plane residual", r.records[0].rms_plane)
    assert r.stop_reason == "max_iterations" and 3e-3 < before < 5e-3 and after <= 3e-5
    R = r.M[:, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(R) - 1.0) <= 1e-14   # rigid


def test_pivots_a_multiple_of_the_lever_step_apart_give_the_same_fit():
    """g and g' = g + 4096 m give every pair the levers L and L - m: the same least-squares problem with tau about another
    point, omega' = omega and tau' = tau + omega x (G' - G), so the two fits agree within the solver's tolerance.  The two
    D then differ in the second order only, by (R - I - [omega]x)(G' - G) ~ theta^2 |G' - G| / 2, because the exact
    rotation of a linearised omega is taken about another point.  (Pivots that differ by a fraction of a lever step round
    the levers differently and agree only to the lever's resolution.)"""
    data, ref, _ = cp.two_samplings()
    lo = ca.target_box(ref)[0]
    kq = 65536.0 / float(F32(cp.CLAIM_MAX_DIST))
    g = cp.point_pivot(ca.IDENTITY, data, ref, cp.CLAIM_MAX_DIST)
    far = [g[0] + 4096 * 37, g[1] - 4096 * 120, g[2] + 4096 * 5]
    w1, w2 = (cp.iteration_record(ca.IDENTITY, p, data, ref, cp.CLAIM_MAX_DIST) for p in (g, far))
    assert w1[cp.N_PAIRS] == w2[cp.N_PAIRS] > 2500 and w1[cp.CC:] != w2[cp.CC:] and w1[cp.RR:] == w2[cp.RR:]
    assert max(cp.condition(w1), cp.condition(w2)) < 1e4
    x1, x2 = cp.solve(w1), cp.solve(w2)
    om1, om2, tau1, tau2 = x1[:3] / 4096.0, x2[:3] / 4096.0, x1[3:] / kq, x2[3:] / kq
    dG = (np.array(far, np.float64) - np.array(g, np.float64)) / kq
    print("conditions", cp.condition(w1), cp.condition(w2), "omega", om1, "difference", np.abs(om1 - om2).max(),
          "tau", tau2, "difference", np.abs(tau2 - (tau1 + np.cross(om1, dG))).max())
    assert _close(om2, om1) and _close(tau2, tau1 + np.cross(om1, dG))
    D1, D2 = cp.fit(w1, lo, cp.CLAIM_MAX_DIST), cp.fit(w2, lo, cp.CLAIM_MAX_DIST)
    K = np.array([[0, -om1[2], om1[1]], [om1[2], 0, -om1[0]], [-om1[1], om1[0], 0]])
    second = (D1[:, :3] - np.eye(3) - K) @ dG
    print("translations differ by", np.abs(D2[:, 3] - D1[:, 3]).max(), "of which unexplained", np.abs(D2[:, 3] - D1[:, 3] + second).max())
    assert _close(D2[:, :3], D1[:, :3]) and _close(D2[:, 3], D1[:, 3] - second)
    assert 1e-5 < np.abs(second).max() < (om1 @ om1) * np.linalg.norm(dG)
    w3 =cp.iteration_record(ca.IDENTITY, [g[0] + 2048, g[1], g[2] - 1000], data, ref, cp.CLAIM_MAX_DIST)
    D3 = cp.fit(w3, lo, cp.CLAIM_MAX_DIST)
    # the third range rule: a pivot 2^30 steps off puts every pair out of range, and one nearer splits them
    w4 = cp.iteration_record(ca.IDENTITY, [g[0] + 2 ** 30 + 2 ** 20, g[1], g[2]], data, ref, cp.CLAIM_MAX_DIST)
    assert w4[cp.N_OUT_OF_RANGE] == w4[cp.N_MATCHED] == w1[cp.N_MATCHED] and w4[cp.N_PAIRS] == 0 and not any(w4[cp.CC:])
    w5 = cp.iteration_record(ca.IDENTITY, [g[0] + 2 ** 30, g[1], g[2]], data, ref, cp.CLAIM_MAX_DIST)
    assert 0 < w5[cp.N_OUT_OF_RANGE] < w5[cp.N_MATCHED] and w5[cp.N_PAIRS] == w5[cp.N_MATCHED] - w5[cp.N_OUT_OF_RANGE]
    # the lever's resolution, not the solver's: the rotation (1.5 degrees) times a lever step (max_dist / 16) is 1e-4
    print("pivots half a lever step apart: largest difference", np.abs(D3 - D1).max())
    assert not _close(D3, D1) and np.abs(D3 - D1).max() <= 2e-4


def test_point_to_plane_is_closer_than_point_to_point_on_two_samplings():
    """The claim the call exists for: two independent samplings of the unit cube's surface, 3000 points each, the data
    cloud moved by a known rigid motion; after the same 8 iterations from the identity with the same cap the plane run is
    strictly closer to the true motion than the point run (largest corner displacement: 9.4e-4 against 3.1e-3, from
    3.4e-2; the plane run is there after three iterations)."""
    data, ref, known = cp.two_samplings()
    plane, point = cp.restated_claim()
    start, ep, eq = cp.corner_error(ca.IDENTITY, known), cp.corner_error(plane.M, known), cp.corner_error(point.M, known)
    print("corner error: start", start, "plane", ep, "point", eq, "plane per iteration",
          [cp.corner_error(r.M, known) for r in plane.records], "point per iteration", [cp.corner_error(r.M, known) for r in point.records])
    assert plane.iterations == point.iterations == cp.CLAIM_ITERATIONS
    assert plane.stop_reason == point.stop_reason == "max_iterations"
    assert ep < eq < start and ep < 0.5 * eq
    assert plane.records[-1].rms_plane < plane.records[0].rms_plane
    assert all(r.n_no_normal == 0 and r.n_out_of_range == 0 and r.n_pairs == r.n_matched for r in plane.records)


def test_every_cloud_of_the_gpu_fit_test_is_well_conditioned():
    """A condition on the inputs: with lambda_max / lambda_min below 1e4 the two float64 solvers agree to about
    1e4 * 2^-52 = 2e-12, and the GPU test's 1e-9 leaves a factor 500 for their different operation orders."""
    for name in cp.FIT_CASES:
        r = cp.restated_fit_case(name)
        assert r.iterations >= 1, name
        for k, rec in enumerate(r.records):
            cond = cp.condition(rec.words)
            print(name, k, "N", rec.n_pairs, "condition", cond, "shift", rec.shift)
            assert cond < 1e4, (name, k)


def test_loop_stride_and_stop_reasons():
    data, ref, known = cp.two_samplings()
    full = cp.restated_claim()[0]
    shifts = [r.shift for r in full.records]
    assert all(s > 0 for s in shifts) and shifts[3] < 1e-2 * shifts[0]
    stop = next(i for i, s in enumerate(shifts) if s <= shifts[3])
    r = cp.align_plane(data, ref, cp.CLAIM_MAX_DIST, cp.CLAIM_ITERATIONS, min_shift=shifts[3])
    assert r.stop_reason == "converged" and r.iterations == stop + 1 and np.array_equal(r.M, full.records[stop + 1].M)
    assert [x.pivot for x in r.records] == [x.pivot for x in full.records[:stop + 1]]
    assert full.records[1].pivot == cp.pivot(full.records[0].words[cp.SUM_Q3:cp.SUM_Q3 + 3], full.records[0].n_pairs)
    assert full.records[0].pivot == cp.point_pivot(ca.IDENTITY, data, ref, cp.CLAIM_MAX_DIST)
    s3 = cp.align_plane(data, ref, cp.CLAIM_MAX_DIST, 1, stride=3)
    assert s3.records[0].n_query == 1000 and s3.records[0].words.tolist() == cp.iteration_record(
        ca.IDENTITY, cp.point_pivot(ca.IDENTITY, data[::3], ref, cp.CLAIM_MAX_DIST), data[::3], ref, cp.CLAIM_MAX_DIST)
    for bad in (dict(max_dist=0.0), dict(max_iterations=0), dict(max_iterations=1025), dict(stride=0), dict(min_shift=-1.0),
                dict(init=np.full((3, 4), np.nan))):
        with pytest.raises(ValueError):
            cp.align_plane(data, ref, **{"max_dist": 0.05, **bad})
    with pytest.raises(ValueError):
        cp.align_plane(data[:, :3], ref, 0.05)                             # a data cloud without normals
