"""The numpy restatement of acmmp_fusion_mesh_sample (mesh_sample_support) pinned by properties of the definition; no
device is involved."""
import numpy as np
import pytest

import mesh_render_support as rs
import mesh_sample_support as mss
import surface_distance_support as sd

F32, F64, U64 = np.float32, np.float64, np.uint64
SEEDS = (0, 1, 2 ** 64 - 1)


def test_mix_is_splitmix64():
    # the first outputs of splitmix64 seeded with 0: its state after k steps is k * golden, which mix() adds itself
    golden = 0x9e3779b97f4a7c15
    state = np.array([(k * golden) % 2 ** 64 for k in range(3)], U64)
    assert [int(x) for x in mss.mix(state)] == [0xe220a8397b1dcdaf, 0x6e789e6aa1b965f4, 0x06c45d188009454f]


def test_lattice_constants_are_the_plastic_number():
    # p^3 = p + 1; G1 = floor(2^64 / p) and G2 = 2^64 / p^2 rounded up to odd, checked in integers: x = G / 2^64 solves
    # x^3 + x^2 = 1 for 1 / p, and 1 / p^2 = (1 / p)^2
    one = 1 << 64
    g1, g2 = int(mss.G1), int(mss.G2)
    f = lambda g: g ** 3 + g ** 2 * one - one ** 3
    assert f(g1) < 0 < f(g1 + 1)
    assert g2 % 2 == 1 and abs(g2 * one - g1 * g1) < 2 * one


@pytest.mark.parametrize("seed", SEEDS)
def test_counts_follow_the_floor_ceil_rule(seed):
    v, f = mss.with_bad_faces()
    for spacing in (0.05, 0.3, 1.7):
        ok, e = mss.expected(v, f, spacing)
        n, skipped = mss.counts(v, f, spacing, seed)
        assert skipped == 2 and list(np.nonzero(~ok)[0]) == [7, 10]
        assert (n[~ok] == 0).all()
        assert ((n == np.floor(e)) | (n == np.floor(e) + 1))[ok].all()
        assert e[3] == 0.0 and n[3] == 0 and ok[3]                        # the degenerate face: valid, no samples
    v, f = mss.all_invalid()
    n, skipped = mss.counts(v, f, 0.1, seed)
    assert skipped == 3 and (n == 0).all()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("r", (0.3, 0.5, 0.9))
def test_rounding_is_unbiased(seed, r):
    """F faces of one area, e = 2 + r each: the total is 2 F plus F Bernoulli(r) terms, so it deviates from F e by at
    most 6 standard deviations sqrt(F r (1 - r)) (the bound is the binomial's, not a measurement)."""
    F = 4096
    v, _ = mss.square(1.0)
    f = np.tile(np.array([[0, 1, 2]], np.int32), (F, 1))                  # area 0.5 each
    spacing = F32(np.sqrt(0.5 / (2 + r)))
    ok, e = mss.expected(v, f, spacing)
    assert (e == e[0]).all() and abs(e[0] - (2 + r)) < 1e-5
    n, _ = mss.counts(v, f, spacing, seed)
    frac = e[0] - 2.0
    assert set(np.unique(n)) == {2, 3}
    assert abs(int(n.sum()) - F * e[0]) <= 6 * np.sqrt(F * frac * (1 - frac))


@pytest.mark.parametrize("seed", SEEDS)
def test_weights_are_exact_and_samples_stay_in_the_box(seed):
    h = mss.face_hash(seed, 64)
    j = np.arange(2000, dtype=U64)
    i0, i1, i2 = mss.weights(np.repeat(h, len(j)), np.tile(j, len(h)))
    with np.errstate(over="ignore"):
        o1 = mss.mix(np.repeat(h, len(j)))
        raw1 = (o1 + np.tile(j, len(h)) * mss.G1) >> U64(11)
        raw2 = (mss.mix(o1) + np.tile(j, len(h)) * mss.G2) >> U64(11)
    folded = raw1 + raw2 > mss.ONE
    assert 0.3 < folded.mean() < 0.7                                      # both branches are taken
    w = [i.astype(F64) * 2.0 ** -53 for i in (i0, i1, i2)]
    for x, i in zip(w, (i0, i1, i2)):
        assert (i <= mss.ONE).all() and (x >= 0).all() and (x * 2.0 ** 53 == i.astype(F64)).all()
    assert ((w[0] + w[1]) + w[2] == 1.0).all() and (i0 + i1 + i2 == mss.ONE).all()
    v, f = sd.rig_part()
    pts, face, _ = mss.sample(v, f, mss.spacing_for(v, f, 1.5), seed)
    corner = v[f[face]][:, :, :3]
    assert (pts[:, :3] >= corner.min(1)).all() and (pts[:, :3] <= corner.max(1)).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_unit_cube(seed):
    v, f = sd.cube()
    spacing = 0.02
    pts, face, skipped = mss.sample(v, f, spacing, seed)
    n = np.bincount(face, minlength=12)
    e = 0.5 / (float(F32(spacing)) ** 2)                                  # every face is half a unit square
    assert skipped == 0 and ((n == int(np.floor(e))) | (n == int(np.floor(e)) + 1)).all()
    assert (np.diff(face) >= 0).all()
    assert sd.cube_surface_distance(pts[:, :3]).max() <= 2.0 ** -22
    d2, nearest, _, _ = sd.distances(pts[::7, :3], v, f, 0.5)
    assert (nearest >= 0).all() and np.sqrt(d2.astype(F64)).max() <= 2.0 ** -22
    length = np.linalg.norm(pts[:, 3:6].astype(F64), axis=1)
    assert np.abs(length - 1).max() < 1e-6


@pytest.mark.parametrize("seed", SEEDS)
def test_lattice_covers_the_triangle(seed):
    """4096 samples of one triangle: each mean barycentric weight within 0.01 of 1 / 3 (the unhashed lattice gives
    0.3338 for w0 and 0.3331 for w1 and w2), and no quarter of the triangle is starved."""
    j = np.arange(4096, dtype=U64)
    plain = [float((i.astype(F64) * 2.0 ** -53).mean()) for i in mss.weights(np.zeros(4096, U64), j, hashed=False)]
    assert [round(x, 4) for x in plain] == [0.3338, 0.3331, 0.3331]
    h = mss.face_hash(seed, 1)
    w = np.stack([i.astype(F64) * 2.0 ** -53 for i in mss.weights(np.repeat(h, 4096), j)], 1)
    assert np.abs(w.mean(0) - 1 / 3).max() <= 0.01
    # the four congruent sub-triangles (three corners, the middle) hold a quarter of the samples each, within 6 sigma
    # of a binomial -- a lattice does better
    part = np.where(w[:, 0] >= 0.5, 0, np.where(w[:, 1] >= 0.5, 1, np.where(w[:, 2] >= 0.5, 2, 3)))
    assert np.abs(np.bincount(part, minlength=4) - 1024).max() <= 6 * np.sqrt(4096 * 0.25 * 0.75)


def test_determinism_and_seeds():
    v, f = mss.embedded("middle")
    spacing = mss.spacing_for(*mss.tiny_faces(), 0.3)
    a, b = mss.sample(v, f, spacing, 5), mss.sample(v, f, spacing, 5)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    c = mss.sample(v, f, spacing, 6)
    ok, e = mss.expected(v, f, spacing)
    for pts, face, _ in (a, c):
        n = np.bincount(face, minlength=len(f))
        assert ((n == np.floor(e)) | (n == np.floor(e) + 1)).all()
    big = len(f) // 2                                                     # the square's first face: other points
    pa, pc = a[0][a[1] == big], c[0][c[1] == big]
    m = min(len(pa), len(pc))
    assert m > 500 and abs(len(pa) - len(pc)) <= 1 and not (pa[:m, :3] == pc[:m, :3]).all(1).any()


def test_too_many_samples_is_refused_before_allocation():
    v, f = mss.square(1000.0)
    with pytest.raises(OverflowError):
        mss.sample(v, f, 0.01)
    with pytest.raises(ValueError):
        mss.sample(v, f, 0.0)
    n, _ = mss.counts(rs.as_mesh([[0, 0, 0], [1e6, 0, 0], [0, 1e6, 0]], [[0, 1, 2]])[0], [[0, 1, 2]], 1e-3)
    assert int(n[0]) == 2 ** 31                                           # e >= 2^31 counts as 2^31
