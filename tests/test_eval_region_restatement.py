"""The numpy restatement of the evaluation regions (eval_region_support) against independent statements: the prism's
parity against an exact-rational winding number off the edges and against a literal table on them, the grid's indexing
against Python integers, and io.read_region on both JSON forms (tests/golden/eval_region_*)."""
import os
from fractions import Fraction

import numpy as np
import pytest

import eval_region_support as er
from acmmp import io

F32 = np.float32


def _is_left(a, b, p):
    return (b[0] - a[0]) * (p[1] - a[1]) - (p[0] - a[0]) * (b[1] - a[1])


def winding(polygon, p):
    """(winding number, on an edge) of point p about the polygon, in exact rationals."""
    poly = [(Fraction(float(u)), Fraction(float(v))) for u, v in polygon]
    p = (Fraction(float(p[0])), Fraction(float(p[1])))
    wn, on = 0, False
    for i, a in enumerate(poly):
        b = poly[(i + 1) % len(poly)]
        side = _is_left(a, b, p)
        if side == 0 and min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1]):
            on = True
        if a[1] <= p[1]:
            if b[1] > p[1] and side > 0:
                wn += 1
        elif b[1] <= p[1] and side < 0:
            wn -= 1
    return wn, on


@pytest.mark.parametrize("polygon", [er.POLYGON, er.TRIANGLE, er.POLYGON[::-1]], ids=["concave", "triangle", "clockwise"])
def test_parity_is_the_winding_number_off_the_edges(polygon):
    rng = np.random.default_rng(3)
    uv = np.concatenate([rng.random((1500, 2)) * 1.5 - 0.25, rng.integers(-2, 11, (500, 2)) / 8.0,
                         np.array([q for q, _ in er.ON_BOUNDARY + er.COLLINEAR])]).astype(F32).astype(np.float64)
    got = er.crossing_parity(polygon, uv[:, 0], uv[:, 1])
    checked = 0
    for k, p in enumerate(uv):
        wn, on = winding(polygon, p)
        if not on:
            assert got[k] == (wn != 0), (p, wn)
            checked += 1
    assert checked > 1800 and 0 < got.sum() < len(got)


def test_boundary_points_fall_where_the_rule_puts_them():
    """A point counts the edges whose one end is above it (v > p_v), the other not, and that pass strictly to its right
    (p_u < the crossing).  So a point on a left or a bottom edge of the interior is inside -- the edge itself is not to its
    right, the far side is -- and one on a right or a top edge is outside; at v = 1 nothing is above, so the whole top
    is outside; a vertex follows the edges it ends.  The table is written out, not computed."""
    table = er.ON_BOUNDARY + er.COLLINEAR
    uv = np.array([q for q, _ in table], np.float64)
    assert len({q for q, _ in table}) == len(table) == 26
    for (q, _), on in zip(table, [winding(er.POLYGON, q)[1] for q, _ in table]):
        assert on == (q in {b for b, _ in er.ON_BOUNDARY}), q
    got = er.crossing_parity(er.POLYGON, uv[:, 0], uv[:, 1])
    assert [bool(g) for g in got] == [w for _, w in table]
    # the prism's bit: the same at axis_min and axis_max, which belong to it, and set one float32 step beyond them
    q = er.prism_queries()
    cls = er.classify(q, er.region(prism=True))
    want = [w for _, w in table]
    assert [c == 0 for c in cls[:3 * len(table)]] == want * 3
    assert list(cls[3 * len(table):]) == [er.PRISM, er.PRISM, 0, 0]


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_prism_axes_take_the_other_two_coordinates_in_increasing_order(axis):
    u, v = [k for k in range(3) if k != axis]
    q = er.prism_queries()
    turned = np.zeros_like(q)
    turned[:, u], turned[:, v], turned[:, axis] = q[:, 0], q[:, 1], q[:, 2]
    assert np.array_equal(er.classify(turned, er.region(prism=True, axis=axis)), er.classify(q, er.region(prism=True)))


def test_grid_indexing_in_python_integers():
    r = er.region(grid=True)
    q = np.concatenate([er.grid_queries(), (np.random.default_rng(4).integers(-400, 1500, (600, 3)) / 1024.0).astype(F32)])
    cls = er.classify(q, r)
    o, c = [Fraction(x) for x in er.GRID_ORIGIN], Fraction(er.GRID_CELL)
    ties = {0: 0, 1: 0}
    for p, got in zip(q, cls):
        exact = [(Fraction(float(p[a])) - o[a]) / c for a in range(3)]
        idx = [round(e) for e in exact]                            # Fraction.__round__: half to even
        for e, i in zip(exact, idx):
            if e.denominator == 2:
                ties[i & 1] += 1
                assert i % 2 == 0
        inside = all(0 <= idx[a] < er.GRID_DIMS[a] for a in range(3)) and er.grid_cell_set(*idx)
        assert (got == 0) == inside and got in (0, er.GRID), (p, idx)
    assert ties[0] > 20
    # both parities are met: a tie below an odd index goes down, one above it goes up
    lo = er.classify(np.array([[0.125 * 0.5, 0.125 + 0.125 * 3, -0.25 + 0.125 * 4]], F32), r)     # i_x = 0.5 -> 0
    hi = er.classify(np.array([[0.125 * 1.5, 0.125 + 0.125 * 3, -0.25 + 0.125 * 4]], F32), r)     # i_x = 1.5 -> 2
    assert (lo[0] == 0) == er.grid_cell_set(0, 3, 4) and (hi[0] == 0) == er.grid_cell_set(2, 3, 4)
    # the bytes: cells straddle byte boundaries (no dimension is a multiple of 8), bit k & 7 of byte k >> 3, x fastest
    bits = er.grid_bits()
    assert len(bits) == 40 and all(n % 8 for n in er.GRID_DIMS)
    flat = np.unpackbits(bits, bitorder="little")[:315].reshape(9, 7, 5)                          # [iz, iy, ix]
    assert all(bool(flat[iz, iy, ix]) == er.grid_cell_set(ix, iy, iz) for ix in range(5) for iy in range(7) for iz in range(9))
    assert not np.unpackbits(bits, bitorder="little")[315:].any()


def test_planes_zero_and_minus_zero_pass():
    q = er.plane_queries()
    cls = er.classify(q, er.region(planes=True))
    assert list(cls) == [0, 0, 0, 0, 0, er.PLANES, 0, er.PLANES, er.PLANES, er.PLANES, 0]
    assert np.signbit(q[3]).all() and not np.signbit(q[4]).any()


def test_every_part_is_evaluated_and_invalid_points_carry_bit_0_alone():
    c = er.cloud()
    parts = [er.classify(c, er.region(**{k: True})) for k in ("planes", "prism", "grid")]
    both = er.classify(c, er.region(planes=True, prism=True, grid=True))
    assert np.array_equal(both, parts[0] | parts[1] | parts[2])
    bad = ~np.isfinite(c).all(1)
    assert bad.sum() == len(er.INVALID_ROWS) and (both[bad] == er.INVALID).all() and not (both[~bad] & er.INVALID).any()
    # the planes bound a box around the polygon, so what fails them fails the prism too; the other bits come alone as well
    assert set(np.unique(both)) >= {0, er.PRISM, er.GRID, er.PRISM | er.GRID, er.PLANES | er.PRISM | er.GRID}
    n = er.counts(both)
    assert n["points"] == er.N_CLOUD and n["inside"] > 100 and n["inside"] + n["invalid"] < n["points"]
    assert er.counts(er.classify(c, None)) == {"points": er.N_CLOUD, "invalid": 6, "inside": er.N_CLOUD - 6, "planes": 0,
                                               "prism": 0, "grid": 0}
    assert not np.array_equal(er.classify(c, er.region(prism=True), er.MOTION), parts[1])
    assert len(er.classify(np.zeros((0, 3), F32), er.region(prism=True, grid=True))) == 0


def test_read_region_round_trips_both_forms(tmp_path):
    crop = io.read_region(os.path.join(er.GOLDEN, "eval_region_crop.json"))
    assert crop.planes is None and crop.dims is None and crop.bits is None
    assert (crop.axis, crop.axis_min, crop.axis_max) == (2, er.AXIS_MIN, er.AXIS_MAX)
    assert crop.polygon.dtype == np.float64 and np.array_equal(crop.polygon, er.POLYGON)
    own = io.read_region(os.path.join(er.GOLDEN, "eval_region_own.json"))
    assert np.array_equal(own.planes, er.PLANE_ROWS) and np.signbit(own.planes[7, 3])
    assert (own.axis, own.axis_min, own.axis_max) == (1, er.AXIS_MIN, er.AXIS_MAX) and np.array_equal(own.polygon, er.TRIANGLE)
    assert own.dims == er.GRID_DIMS and own.cell == er.GRID_CELL and np.array_equal(own.origin, er.GRID_ORIGIN)
    assert own.bits.dtype == np.uint8 and np.array_equal(own.bits, er.grid_bits())
    want = er.region(planes=True, prism=True, grid=True, axis=1, polygon=er.TRIANGLE)
    assert np.array_equal(er.classify(er.cloud(), own), er.classify(er.cloud(), want))
    # a crop volume about X or Y takes the other two coordinates in increasing index order
    import json
    d = json.load(open(os.path.join(er.GOLDEN, "eval_region_crop.json")))
    d["orthogonal_axis"] = "Y"
    d["bounding_polygon"] = [[u, 7.0, v] for u, v in er.TRIANGLE]
    (tmp_path / "y.json").write_text(json.dumps(d))
    y = io.read_region(str(tmp_path / "y.json"))
    assert y.axis == 1 and np.array_equal(y.polygon, er.TRIANGLE)
    # refusals
    for bad in ({"class_name": "Box"}, {"sphere": 1}, {"grid": {"origin": [0, 0, 0], "cell": 1, "dims": [5, 7, 9], "bits": "short.bin"}}):
        (tmp_path / "short.bin").write_bytes(b"\0" * 39)
        (tmp_path / "bad.json").write_text(json.dumps(bad))
        with pytest.raises((ValueError, KeyError)):
            io.read_region(str(tmp_path / "bad.json"))
