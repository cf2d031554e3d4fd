"""The camera rigs of tests/rig_support.py, checked without a GPU, so that tests/test_gpu_rigs.py can only fail
because of the engine: each rig exercises what it is there for (computed in float64 with plain numpy), every gated
set has enough valid (query, view) pairs, and -- the precondition of the fast gates -- the CPU oracle, which IS the
exact mode, stays as close to float64 on the rig as on scene.py's rig of the same model, views and texel format:
class agreement >= 0.99, and the share of valid pairs within 1e-4 of float64 no more than 2 points below the base
rig's own share (rigid moves of the world frame spread that share by 0.4 points; the allowance adds room for the new
source geometry).  A rig that misses this has its offsets shrunk; the gate stays.

With ACMMP_TEST_REPORT_DIR set, the fractions go to rig_inputs.json (profiles/rigs/).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fastmath_support as fs
import np_reference as npr
import rig_support as rs

GATED = ("interior", "border", "source_edge")


def _record(name, entry):
    print(name, json.dumps(entry))
    out_dir = os.environ.get("ACMMP_TEST_REPORT_DIR")
    if not out_dir:
        return
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "rig_inputs.json")
    report = {}
    if os.path.exists(path):
        with open(path) as fh:
            report = json.load(fh)
    report[name] = entry
    with open(path, "w") as fh:
        json.dump(report, fh, indent=1, sort_keys=True)


def _shares(orc, ref):
    fr = fs.t1_fractions(orc, orc, ref)
    return {"valid": int(((orc < 2.0) & (ref < 2.0)).sum()), "class_agree": fr["class_agree_exact_f64"],
            "within_1e-4": fr["frac_exact_within_1e-4_of_f64"], "worst": fr["worst_exact_vs_f64"]}


@pytest.mark.parametrize("name", list(rs.RIGS) + list(rs.DEGENERATE))
def test_rig_sets_and_fast_precondition(oracle_mod, name):
    kind, V, tex = rs.RIGS[name] if name in rs.RIGS else (rs.DEGENERATE[name], 3, "f16")
    sc, p = rs.make_rig(name)
    W, H = rs.SIZES[kind]
    assert len(sc.images) == V + 1 and all(im.shape == (H, W) for im in sc.images)
    assert len(sc.extra["gt_depths"]) == V + 1 and all(d.shape == (H, W) for d in sc.extra["gt_depths"])
    assert np.allclose(sc.extra["gt_depths"][0], sc.gt_depth, rtol=1e-5, atol=0) and (sc.gt_depth > 0).all()
    exact16 = all(np.array_equal(im, im.astype(np.float16).astype(np.float32)) for im in sc.images)
    assert exact16 == (tex == "f16")
    sets = rs.rig_sets(name)
    assert tuple(sets) == fs.SETS
    entry = {}
    for set_name in fs.SETS:
        px, py, planes = sets[set_name]
        assert px.shape == py.shape == (fs.PIXELS[V],) and planes.shape == (fs.PIXELS[V], fs.PLANES, 4)
        assert np.isfinite(planes).all()
        ref, _ = rs.rig_f64(name, set_name)
        orc = rs.rig_oracle(oracle_mod, name, set_name)
        base = _shares(fs.oracle_costs(oracle_mod, kind, V, tex, set_name), fs.f64_costs(kind, V, tex, set_name)[0])
        mine = _shares(orc, ref)
        entry[set_name] = dict(mine, base_within=base["within_1e-4"], base_class_agree=base["class_agree"])
    _record(name + "/sets" if name in rs.DEGENERATE else name, entry)
    gated = GATED + (("wild",) if "behind" in name else ())
    for set_name in gated:
        e = entry[set_name]
        assert e["valid"] >= fs.MIN_VALID, (set_name, e)
        assert e["class_agree"] >= 0.99, (set_name, e)
        if set_name in GATED:
            assert e["within_1e-4"] >= e["base_within"] - 0.02, (set_name, e)


@pytest.mark.parametrize("name", ["pinhole-moved", "sphere-moved"])
def test_moved_rig_is_the_base_rig(name):
    """R' = R G^T, t' = t - R' g: the moved cameras are rigid, far from the identity and the origin, and the float64
    costs of the base case's own queries equal the base rig's.  The only difference is the binary32 rounding of R' and
    t': |t'| < 64, so a centre moves by at most sqrt(3) * 2^-19 = 3.3e-6 units -- below 1e-4 source pixels at these focal
    lengths and depths (>= 1.5); with textures of wavelength >= 6 pixels an NCC moves by far less than 1e-3."""
    kind, V, tex = rs.RIGS[name]
    sc, p = rs.make_rig(name)
    base, _ = fs.make_case(kind, V, tex)
    G, g = sc.extra["G"], sc.extra["g"]
    assert np.allclose(G @ G.T, np.eye(3), atol=1e-12) and np.arccos((np.trace(G) - 1) / 2) == pytest.approx(2.1)
    assert np.array_equal(g, (30.0, -40.0, 20.0))
    for k in range(V + 1):
        R = sc.cameras[k]["R"].astype(np.float64).reshape(3, 3)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-6)
        assert np.abs(R - np.eye(3)).max() > 0.5                       # no view is near the identity
        Cm = -R.T @ sc.cameras[k]["t"].astype(np.float64)
        Rb = base.cameras[k]["R"].astype(np.float64).reshape(3, 3)
        Cb = -Rb.T @ base.cameras[k]["t"].astype(np.float64)
        assert np.allclose(Cm, G @ Cb + g, atol=2e-5) and np.linalg.norm(Cm) > 50
        assert np.array_equal(sc.images[k], base.images[k])
    for set_name in fs.SETS:
        q, qb = rs.rig_sets(name)[set_name], fs.query_sets(kind, V, tex)[set_name]
        assert all(np.array_equal(a, b) for a, b in zip(q, qb)), set_name      # the same queries
        mine, theirs = rs.rig_f64(name, set_name)[0], fs.f64_costs(kind, V, tex, set_name)[0]
        both = (mine < 2.0) & (theirs < 2.0)
        assert np.mean((mine >= 2.0) == (theirs >= 2.0)) >= 0.999, set_name
        worst = float(np.abs(mine - theirs)[both].max())
        print(name, set_name, "worst |moved - base| in float64:", worst)
        assert worst <= 1e-3, (set_name, worst)


def test_intrinsics_rig_has_the_terms():
    """The reference: fx != fy, off-centre principal point, no skew.  The sources: K[1] = 0.04 fx, -0.03 fx, 0, one
    K[3] = 0.01 fy, focal lengths +-15%, principal points of their own -- and the skew moves the projections by pixels, so
    a dropped K[1] or K[3] term cannot hide below the costs' noise."""
    for name in ("pinhole-intrinsics", "pinhole-intrinsics-v5"):
        sc, p = rs.make_rig(name)
        W, H = rs.SIZES["pinhole"]
        K = [c["K"].astype(np.float64).reshape(3, 3) for c in sc.cameras]
        assert K[0][0, 0] == pytest.approx(0.8 * W) and K[0][1, 1] == pytest.approx(0.65 * W)
        assert K[0][0, 2] == pytest.approx(0.42 * W) and K[0][1, 2] == pytest.approx(0.57 * H)
        assert K[0][0, 1] == 0 and K[0][1, 0] == 0
        for k, Kv in enumerate(K[1:]):
            assert Kv[0, 1] == pytest.approx(rs.SRC_SKEW[k % 3] * Kv[0, 0], abs=1e-4)
            assert Kv[1, 0] == pytest.approx(rs.SRC_K3[k % 3] * Kv[1, 1], abs=1e-4)
            assert Kv[0, 0] / K[0][0, 0] == pytest.approx(rs.SRC_F[k % 3]) and Kv[1, 1] / K[0][1, 1] == pytest.approx(rs.SRC_F[k % 3])
            assert (Kv[0, 2], Kv[1, 2]) != (K[0][0, 2], K[0][1, 2])
        assert [round(float(Kv[0, 1] / Kv[0, 0]), 4) for Kv in K[1:4]] == [0.04, -0.03, 0.0]
        assert sum(Kv[1, 0] != 0 for Kv in K[1:4]) == 1 and K[2][1, 0] / K[2][1, 1] == pytest.approx(0.01)
        # what the two terms are worth in source pixels on the surface
        xs, ys = np.meshgrid(np.arange(6, W - 6, 4), np.arange(6, H - 6, 4))
        P = npr.world_point(sc.cameras[0], xs.ravel(), ys.ravel(), sc.gt_depth[ys.ravel(), xs.ravel()].astype(np.float64))
        for v, field, idx in ((1, "K[1]", 1), (2, "K[1]", 1), (2, "K[3]", 3)):
            cam = sc.cameras[v].copy()
            x0, y0, _ = npr.project(cam, P)
            cam["K"][idx] = 0.0
            x1, y1, _ = npr.project(cam, P)
            shift = np.hypot(x1 - x0, y1 - y0)
            print(name, "source", v, field, "moves projections by up to", float(shift.max()), "pixels")
            assert shift.max() > 0.25, (v, field, shift.max())
        # and the rendered sources are consistent with the full K: the texture matches at the surface
        ref, _ = rs.rig_f64(name, "interior")
        assert np.median(ref[ref < 2.0]) < 0.2


def test_turned_rig_has_interior_seams_and_poles():
    """At least 16 pixels inside the image (the base rig's seams and poles lie within a few pixels of its border: its
    sources turn by < 0.05 rad), >= 20 pixels of the turned rig have samples across a source's seam and >= 20 a
    sample row clamped at a source's pole; the base rig has none."""
    base, bp = rs.make_rig("sphere-base")
    _, _, diag = rs.surface_diagnostics(base, bp, margin=16)
    assert not diag["seam"].any() and not diag["pole"].any()
    for name in ("sphere-turned", "sphere-turned-v5", "sphere-turned-fp32"):
        sc, p = rs.make_rig(name)
        c0 = sc.cameras[0]
        assert (c0["params"][1], c0["params"][2]) == (np.float32(0.37 * 128), np.float32(0.55 * 64))
        assert all((c["params"][1], c["params"][2]) != (64.0, 32.0) for c in sc.cameras)
        _, _, diag = rs.surface_diagnostics(sc, p, margin=16)
        seam, pole = int(diag["seam"].any(axis=1).sum()), int(diag["pole"].any(axis=1).sum())
        print(name, "interior pixels at a source seam:", seam, "at a source pole:", pole)
        assert seam >= 20 and pole >= 20
        # per source: the yawed ones bring their seam in, the pitched one its pole
        assert diag["seam"][:, 0].sum() >= 10 and diag["seam"][:, 1].sum() >= 10 and diag["pole"][:, 2].sum() >= 20


def test_interpolation_rig_has_an_interior_source_pole():
    """The two-source turned rig of tests/test_gpu_rigs.py's interpolation case (turns = INTERP_TURNS: the 90 degree yaw
    and the pitched, rolled source), at 128x64 and 250x125 standing in for 2000x1000 (the geometry scales with the
    image): the yawed source brings a seam, the pitched one a pole, at least 16 pixels inside the reference image."""
    assert rs.INTERP_TURNS == (0, 2)
    for W, H in ((128, 64), (250, 125)):
        sc = rs.turned(W, H, V=2, seed=1234, n_waves=12, turns=rs.INTERP_TURNS)
        assert len(sc.images) == 3
        assert np.allclose(sc.cameras[2]["R"].reshape(3, 3), rs.TURNS[2], atol=1e-6)
        _, _, diag = rs.surface_diagnostics(sc, fs.params_for(sc), margin=16)
        seam, pole = diag["seam"].sum(axis=0), diag["pole"].sum(axis=0)
        print(f"{W}x{H}", "interior seam pixels per source:", seam.tolist(), "pole pixels per source:", pole.tolist())
        assert seam[0] >= 20 and pole[1] >= 20


def test_behind_rig_puts_samples_behind_a_source():
    name = "pinhole-behind"
    sc, p = rs.make_rig(name)
    c1 = sc.cameras[1]
    assert np.array_equal(c1["R"], np.eye(3, dtype=np.float32).ravel()) and np.array_equal(c1["t"], (0, 0, -4))
    px, py, planes = rs.rig_sets(name)["wild"]
    P = rs.sample_points(sc, p, *fs.flat_queries(px, py, planes))
    tz = P @ c1["R"].astype(np.float64).reshape(3, 3)[2] + float(c1["t"][2])
    _, diag = rs.rig_f64(name, "wild")
    behind = int((tz <= 0).sum())
    mixed = int(((tz <= 0).any(axis=1) & (tz > 0).any(axis=1)).sum())
    print(name, "samples with tz <= 0:", behind, "queries with samples on both sides:", mixed,
          "sign_flip queries:", int(diag["sign_flip"].sum()))
    assert behind >= 50 and mixed >= 1 and diag["sign_flip"].any()


def _oracle_point_and_projection(oracle_mod, cams, x, y, depth, src):
    L = oracle_mod.lib()
    cb = np.frombuffer(np.ascontiguousarray(cams).tobytes(), dtype=oracle_mod.CAMERA_DTYPE).copy()
    X, pt, d = np.zeros(3, np.float32), np.zeros(2, np.float32), np.zeros(1, np.float32)
    L.or_world_point(cb[0:1].ctypes.data, C.c_float(x), C.c_float(y), C.c_float(depth), X.ctypes.data)
    L.or_project(cb[src:src + 1].ctypes.data, X.ctypes.data, pt.ctypes.data, d.ctypes.data)
    return X, pt, float(d[0])


@pytest.mark.parametrize("name", list(rs.DEGENERATE))
def test_degenerate_queries_reach_the_centre_in_binary32(oracle_mod, name):
    """The degenerate point is exact by construction, shown here on the rig's own binary32 numbers: every product of the
    chain is exact (so fused and unfused orders agree) and the camera-frame point of source 1 is (0, 0, 0) -- SPHERE
    d = 0 < 1e-6, pinhole tz == 0.  The oracle's binary32 functions say the same."""
    sc, p = rs.make_rig(name)
    sphere = rs.DEGENERATE[name] == "sphere"
    px, py, planes = rs.degenerate_queries(sc)
    c0, c1 = sc.cameras[0], sc.cameras[1]
    assert np.array_equal(c0["R"], np.eye(3, dtype=np.float32).ravel()) and not c0["t"].any()
    x0, y0 = int(px[0]), int(py[0])
    ray = np.zeros(3, np.float32)
    oracle_mod.lib().or_pixel_to_dir(np.frombuffer(np.ascontiguousarray(c0).tobytes(), dtype=oracle_mod.CAMERA_DTYPE).copy().ctypes.data,
                                     x0, y0, ray.ctypes.data)
    assert np.array_equal(ray, (0, 0, 1))                               # binary32 PixelToDir of the principal point
    assert np.array_equal(planes[0, 0], (0, 0, -1, 2))
    R1, t1 = c1["R"].reshape(3, 3), c1["t"]
    for q in range(len(px)):
        # the sample (or, for query 0, the patch centre) at the principal point, every plane
        assert (x0 - px[q]) % 2 == (0 if q == 0 else 1) and abs(x0 - px[q]) <= 5 and abs(y0 - py[q]) <= 5
        for h in range(fs.PLANES):
            n, w = planes[q, h, :3], planes[q, h, 3]
            den = np.float32(n[2] * ray[2])                              # n . (0, 0, 1): the other products are 0
            assert den == n[2] and abs(den) >= 1e-6
            depth = np.float32(-w) / den
            assert depth == np.float32(2.0)                              # 2 n_z / n_z
    # R1 (0, 0, 2) + t1: 2 R1[:, 2] is exact in binary32, and t1 = -2 R1[:, 2]
    assert all(np.float32(2.0) * R1[r, 2] + t1[r] == 0 for r in range(3)) and np.abs(t1).min() > 0.05
    X, pt, d = _oracle_point_and_projection(oracle_mod, sc.cameras, x0, y0, 2.0, 1)
    assert np.array_equal(X, (0, 0, 2))
    if sphere:
        assert d == 0.0 and np.array_equal(pt, (c1["params"][1], c1["params"][2]))      # the d < 1e-6 select
    else:
        assert d == 0.0 and not np.isfinite(pt).any()                                   # 1 / tz at tz == 0
    # the queries' float64 and oracle costs exist (recorded; the GPU test gates the classes)
    ref, _ = rs.rig_f64(name, "degenerate")
    orc = rs.rig_oracle(oracle_mod, name, "degenerate")
    _record(name, {"degenerate": {"queries": int(orc.size), "oracle_nan": int(np.isnan(orc).sum()),
                                  "f64_nan": int(np.isnan(ref).sum()), "oracle_valid": int((orc < 2.0).sum()),
                                  "oracle_valid_first_source": int((orc[..., 0] < 2.0).sum())}})
    assert not np.isnan(orc).any()
