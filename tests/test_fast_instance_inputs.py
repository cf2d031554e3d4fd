"""The inputs of the small-shape fast-mode instance matrix (tests/test_gpu_fast_instances.py), checked without a
GPU, so that the GPU test can only fail because of the engine: for every case and query set, with the CPU oracle
(binary32) standing in for the engine, the set has its size and its intended pixels, the source-edge and
wild-plane sets contain what they are there to exercise (computed in float64), enough (query, view) pairs are
valid for T1's percentages to mean something, and the oracle's {valid, 2.0} classes agree with float64's.
"""
import numpy as np
import pytest

import fastmath_support as fs
import np_reference as npr


@pytest.mark.parametrize("kind,V,tex", fs.CASES, ids=[fs.case_id(*c) for c in fs.CASES])
def test_query_sets(oracle_mod, kind, V, tex):
    sc, p = fs.make_case(kind, V, tex)
    W, H = fs.MODELS[kind]
    assert sc.images[0].shape == (H, W) and len(sc.images) == V + 1
    # the texel format the engine will take: 8-bit images are binary16-exact, the unquantised ones are not
    exact16 = all(np.array_equal(im, im.astype(np.float16).astype(np.float32)) for im in sc.images)
    assert exact16 == (tex == "f16")
    sets = fs.query_sets(kind, V, tex)
    assert tuple(sets) == fs.SETS
    for name, (px, py, planes) in sets.items():
        n = fs.PIXELS[V]
        assert px.shape == py.shape == (n,) and planes.shape == (n, fs.PLANES, 4), name
        assert px.dtype == np.int32 and py.dtype == np.int32 and planes.dtype == np.float32, name
        assert np.isfinite(planes).all(), name
        assert px.min() >= 0 and px.max() < W and py.min() >= 0 and py.max() < H, name
        inside = (px >= 6) & (px < W - 6) & (py >= 6) & (py < H - 6)
        if name == "border":
            assert not inside.any()
            assert {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)} <= set(zip(px.tolist(), py.tolist()))
        else:
            assert inside.all(), name
        ref, diag = fs.f64_costs(kind, V, tex, name)
        orc = fs.oracle_costs(oracle_mod, kind, V, tex, name)
        valid = (orc < 2.0) & (ref < 2.0)
        assert valid.sum() >= fs.MIN_VALID, (name, int(valid.sum()))
        agree = np.mean((orc >= 2.0) == (ref >= 2.0))
        assert agree >= 0.99, (name, agree)
        if name == "source_edge":
            hit = diag["out_of_image"] | diag["seam"] | diag["pole"]
            assert hit.mean() >= 0.25, (name, hit.mean())
            if kind == "sphere":
                assert diag["seam"].any() and diag["pole"].any()
        if name == "wild":
            assert diag["clamp"].any() and diag["sign_flip"].any(), name
            # the planes built to contain a sample's ray (fastmath_support.grazing_plane) are what hits the clamp
            clamp = diag["clamp"].reshape(n, fs.PLANES)
            assert all(clamp[q, q % 5] for q in range(4))
            if kind == "pinhole":
                assert diag["centre_out"].any()


@pytest.mark.parametrize("kind,V,tex", [("pinhole", 3, "f16"), ("sphere", 2, "fp32")])
def test_vectorised_float64_ncc_is_the_scalar_one(kind, V, tex):
    sc, p = fs.make_case(kind, V, tex)
    for name in fs.SETS:
        px, py, planes = fs.query_sets(kind, V, tex)[name]
        ref, _ = fs.f64_costs(kind, V, tex, name)
        for q in range(0, len(px), 7):
            for h in range(fs.PLANES):
                for v in range(V):
                    want = npr.bilateral_ncc(sc.images, sc.cameras, p, v + 1, int(px[q]), int(py[q]),
                                             planes[q, h].astype(np.float64))
                    got = ref[q, h, v]
                    assert (np.isnan(want) and np.isnan(got)) or abs(got - want) <= 1e-12, (name, q, h, v, got, want)


def test_t1_gates_reject_a_shifted_fast_mode():
    """The shared gates on made-up costs: equal fast and exact costs pass; 2% of valid queries moved by 3e-4
    fail the pinhole gate (99.5% within 1e-4), 8% fail SPHERE's (exact's own share + 5 pt), a NaN fails, and
    2% of class flips fail."""
    rng = np.random.default_rng(0)
    ref = rng.uniform(0.05, 1.5, 4000)
    ref[::10] = 2.0
    e = ref + rng.normal(0, 1e-5, ref.size)
    e[::10] = 2.0
    fs.t1_gates(e.copy(), e, ref, sphere=False)
    fs.t1_gates(e.copy(), e, ref, sphere=True)
    valid = np.nonzero(e < 2.0)[0]
    f = e.copy()
    f[valid[: len(valid) // 50]] += 3e-4
    with pytest.raises(AssertionError):
        fs.t1_gates(f, e, ref, sphere=False)
    f = e.copy()
    f[valid[: len(valid) * 8 // 100]] += 3e-4
    with pytest.raises(AssertionError):
        fs.t1_gates(f, e, ref, sphere=True)
    f = e.copy()
    f[3] = np.nan
    with pytest.raises(AssertionError):
        fs.t1_gates(f, e, ref, sphere=True)
    f = e.copy()
    f[valid[: len(valid) // 50]] = 2.0
    with pytest.raises(AssertionError):
        fs.t1_gates(f, e, ref, sphere=False)


@pytest.mark.parametrize("kind,V,tex", [("pinhole", 3, "f16"), ("sphere", 5, "fp32"), ("sphere", 1, "f16")])
def test_reformed_initial_cost_is_the_oracles(oracle_mod, kind, V, tex):
    """fastmath_support.reform_initial_cost on the oracle's per-view costs of RandomInitialization's planes gives
    the oracle's initial costs bit for bit (the GPU test re-forms the fast k_init's costs with it), and enough of
    those pixels have a valid view for that comparison to mean something."""
    sc, p = fs.make_case(kind, V, tex)
    H, W = sc.images[0].shape
    prob = oracle_mod.Problem(sc.images, sc.cameras, p)
    o = oracle_mod.run_patchmatch(prob, seed=17 + V, n_half_sweeps=0, do_post=False)
    per_view = np.array([[oracle_mod.ncc(prob, v + 1, x, y, o["planes"][y, x]) for v in range(V)]
                         for y in range(H) for x in range(W)], np.float32)
    want = fs.reform_initial_cost(per_view, p["top_k"]).reshape(H, W)
    assert np.array_equal(want.view(np.uint32), o["costs"].view(np.uint32))
    assert np.mean(want < 2.0) > 0.3
