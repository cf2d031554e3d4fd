"""The per-pixel negligible-sample mask in the fast SPHERE k_init at V <= 4 (ncc_chunk's PNEG through
initial_cost), read after the initialisation alone: acmmp_band_begin over the whole view runs k_init and nothing else,
acmmp_band_get_rows returns its planes (in the kernel's own form), costs and selected views, and
acmmp_debug_band_cvec the cost cache it filled.

Shapes: 2000x1000 V = 2 and 2000x1500 V = 4, the smallest at which the gate holds (tests/test_gpu_ref_neg_skip.py's).
Query pixels: test_gpu_neg_skip.py's sets (rows at the dead band's edges, seam columns, rows next to both poles, mixed
dead / live runs, random, pole and seam pixels) and 1500 seeded pixels more; the whole-view comparisons take every
pixel.

  * Mask on against off.  ACMMP_REF_NEG_SKIP=0 launches the instance without the mask; a threshold no weight reaches
    (ACMMP_REF_NEG_TAU=1e-45: the masked instance, empty mask) gives the same planes, costs, selected views and cached
    vectors, bit for bit, over the whole view.  At 2000x1000 V = 2 the unmasked instance equals the parent commit's
    library on a seeded sample of 2000 pixels per colour (tests/golden/init_neg_parent_2000x1000-v2.npy: plane, cost and
    selected views after k_init, recorded on an MI355X).
  * Threshold of 1: every sample masked, so every cached cost and every cost is 2.0.
  * Consistency.  For k_init's own planes its cached vector equals the refinement's masked arithmetic
    (acmmp_debug_ncc_ref: k_eval_ref's staging and instance, all 5 lanes) bit for bit: with the mask off, at the product
    threshold, and at a threshold that moves costs (BIG_TAU) -- where the cache must also differ from the unmasked one.
    The cost and the selected views are initial_cost's fold of that vector (restated in binary32).
  * Cut independence: a 6-half-sweep run is bit-identical on 1, 2 and 4 strips and as two row bands, at the product
    threshold and at BIG_TAU.
  * Bound on the change.  Per query |on - off| within the pixel's own dropped share plus one binary32 spacing per
    operation, propagated through the NCC (np_neg_skip.on_off_bound over np_ref_neg_skip's per-sample restatement);
    excluded: costs of 2.0 and source variances too small for the bound's first-order form, capped as in
    test_gpu_ref_neg_skip.py.  At BIG_TAU the kernel is within 1e-4 of the float64 restatement with that threshold's
    per-pixel mask as often as the unmasked kernel is of the unmasked restatement, to 3 points.
"""
import os

import numpy as np
import pytest

import np_neg_skip as ns
import np_ref_neg_skip as rn
from acmmp import band, capi, scene
from test_gpu_neg_skip import BIG_TAU, SHAPES, _params, _queries

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KNOBS = ("ACMMP_REF_NEG_SKIP", "ACMMP_REF_NEG_TAU", "ACMMP_STRIPS", "ACMMP_STRIP_STREAMS")
SEED = 9
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731


@pytest.fixture(scope="module", params=list(SHAPES))
def rig(request):
    name = request.param
    W, H, V, seed = SHAPES[name]
    sc = scene.sphere_scene(W, H, n_src=V, seed=seed, n_waves=16)
    with capi.Context(0) as ctx:
        ctx.set_params(_params(sc))
        ctx.upload_views(sc.images, sc.cameras)
        ctx.set_math("fast")
        yield name, sc, ctx


def _env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def init_state(ctx, monkeypatch, **env):
    """k_init alone with the given knobs -> per colour: (Pc, 6) words (plane, cost, selected views) and (V, Pc) cache
    words, colour-grid pixel y * ceil(W / 2) + x // 2."""
    _env(monkeypatch, env)
    ctx.band_begin(SEED, 0, ctx.H)
    rows = [ctx.band_get_rows(c, 0, ctx.H) for c in (0, 1)]
    cvec = [bits(ctx.debug_band_cvec(c, 0, ctx.H)) for c in (0, 1)]
    ctx.band_end(do_post=False)
    _env(monkeypatch, {})
    return rows, cvec


def golden_sample(rows):
    """The recorded sample of a 2000x1000 initialisation: 2000 seeded colour-grid pixels per colour -> (2, 2000, 6)."""
    idx = np.random.default_rng(2025).choice(rows[0].shape[0], 2000, replace=False)
    return np.stack([rows[0][idx], rows[1][idx]])


def query_pixels(sc, W, H):
    px, py = _queries(sc, W, H)
    rng = np.random.default_rng(W * 3 + H)
    return (np.concatenate([px, rng.integers(0, W, 1500)]).astype(np.int32),
            np.concatenate([py, rng.integers(0, H, 1500)]).astype(np.int32))


def at_pixels(state, W, px, py):
    """k_init's planes (n, 4) float32, costs, selected views and cached vectors (n, V) words at the pixels."""
    rows, cvec = state
    colour, ci = (px + py) & 1, py.astype(np.int64) * ((W + 1) // 2) + px // 2
    r = np.where(colour[:, None] == 0, rows[0][ci], rows[1][ci])
    cv = np.where(colour[:, None] == 0, cvec[0][:, ci].T, cvec[1][:, ci].T)
    return np.ascontiguousarray(r[:, :4]).view(np.float32), r[:, 4].copy(), r[:, 5].copy(), np.ascontiguousarray(cv)


def fold(cv, top_k):
    """initial_cost's fold of a cost vector (ACMMP.cu:519-556), binary32: cv (n, V) -> cost words, selected views."""
    n, V = cv.shape
    s = np.sort(cv, axis=1)
    k = np.minimum((cv < 2.0).sum(axis=1), top_k)
    acc = np.zeros(n, np.float32)
    for i in range(V):
        acc = np.where(i < k, acc + s[:, i], acc).astype(np.float32)
    cost = np.where(k > 0, acc / np.maximum(k, 1).astype(np.float32), np.float32(2.0)).astype(np.float32)
    thr = s[np.arange(n), np.maximum(k, 1) - 1]
    sel = np.zeros(n, np.uint32)
    for i in range(V):
        sel |= ((cv[:, i] <= thr) & (k > 0)).astype(np.uint32) << np.uint32(i)
    return bits(cost), sel


def test_on_against_off_whole_view(rig, monkeypatch):
    name, sc, ctx = rig
    off = init_state(ctx, monkeypatch, ACMMP_REF_NEG_SKIP="0")
    empty = init_state(ctx, monkeypatch, ACMMP_REF_NEG_TAU="1e-45")
    for c in (0, 1):
        assert np.array_equal(off[0][c], empty[0][c]), c
        assert np.array_equal(off[1][c], empty[1][c]), c
    live = off[1][0].view(np.float32) < 2.0
    assert live.mean() > 0.1, live.mean()
    if name == "2000x1000-v2":
        # the unmasked instance against the parent commit's library
        want = np.load(os.path.join(GOLDEN, "init_neg_parent_2000x1000-v2.npy"))
        assert np.array_equal(golden_sample(off[0]), want)
    # every sample masked: no source sums anywhere
    gone = init_state(ctx, monkeypatch, ACMMP_REF_NEG_TAU="1.0")
    for c in (0, 1):
        assert np.all(gone[1][c].view(np.float32) == 2.0)
        assert np.all(gone[0][c][:, 4].view(np.float32) == 2.0) and np.all(gone[0][c][:, 5] == 0)
        assert np.array_equal(gone[0][c][:, :4], off[0][c][:, :4])      # the planes are drawn before any cost


def test_cache_equals_masked_refinement(rig, monkeypatch):
    name, sc, ctx = rig
    W, H, V, _ = SHAPES[name]
    px, py = query_pixels(sc, W, H)
    top_k = int(_params(sc)["top_k"])
    got = {}
    for which, env in (("off", {"ACMMP_REF_NEG_SKIP": "0"}), ("product", {}),
                       ("big", {"ACMMP_REF_NEG_TAU": repr(BIG_TAU[H])})):
        planes, cost, sel, cv = at_pixels(init_state(ctx, monkeypatch, **env), W, px, py)
        _env(monkeypatch, env)
        ref = ctx.debug_ncc_ref(px, py, np.repeat(planes[:, None, :], 5, axis=1))
        _env(monkeypatch, {})
        for h in range(5):
            differ = bits(ref[:, h, :]) != cv
            assert not differ.any(), (which, h, float(differ.mean()))
        want_cost, want_sel = fold(cv.view(np.float32), top_k)
        assert np.array_equal(cost, want_cost), (which, float(np.mean(cost != want_cost)))
        assert np.array_equal(sel, want_sel), (which, float(np.mean(sel != want_sel)))
        got[which] = (planes, cv.view(np.float32))
    for which in ("product", "big"):
        assert np.array_equal(bits(got[which][0]), bits(got["off"][0]))      # the same planes
    off, on, big = got["off"][1], got["product"][1], got["big"][1]
    live = off < 2.0
    assert live.mean() > 0.1, live.mean()
    assert np.array_equal(on >= 2.0, off >= 2.0)
    changed = float(np.mean(bits(on)[live] != bits(off)[live]))
    moved = float(np.mean(np.abs(big - off)[live] > 1e-3))
    print(f"{name}: {off.size} cached costs, {live.mean():.3f} live; the product threshold changes the bits of {changed:.5f} "
          f"of them, worst |on - off| {np.abs(on - off)[live].max():.3g}; the large threshold moves {moved:.3f} by more "
          f"than 1e-3")
    # the large threshold reaches k_init's loop (its cache equals the masked refinement above, not the unmasked one)
    assert moved >= 0.1, moved


@pytest.mark.parametrize("which", ["big", "product"])
def test_cut_independence(rig, monkeypatch, which):
    name, sc, ctx = rig
    W, H, V, _ = SHAPES[name]
    tau = {} if which == "product" else {"ACMMP_REF_NEG_TAU": repr(BIG_TAU[H])}

    def outputs(c):
        planes, costs = c.download()
        sel, _ = c.download_aux()
        return [bits(planes).copy(), bits(costs).copy(), bits(sel).copy()]

    def run(**env):
        _env(monkeypatch, env)
        ctx.run_patchmatch(SEED, n_half_sweeps=6)
        return outputs(ctx)

    off = run(ACMMP_REF_NEG_SKIP="0", ACMMP_STRIPS="1")
    base = run(ACMMP_STRIPS="1", **tau)
    if which == "big":
        assert not np.array_equal(base[0], off[0]) and not np.array_equal(base[1], off[1])
    for strips in ("2", "4"):
        got = run(ACMMP_STRIPS=strips, **tau)
        for a, b, what in zip(base, got, ("planes", "costs", "views")):
            assert np.array_equal(a, b), (strips, what, float(np.mean(a != b)))
    # two row bands (each initialises its rows and a halo only): the default parameters' run is these 6 half-sweeps
    assert 2 * int(_params(sc)["max_iterations"]) == 6
    _env(monkeypatch, tau)
    others = [capi.Context(0) for _ in range(2)]
    try:
        for c in others:
            c.set_params(_params(sc))
            c.upload_views(sc.images, sc.cameras)
            c.set_math("fast")
        bands = band.split_rows(H, 2)
        band.run_local(others, SEED, bands)
        for c, (lo, hi) in zip(others, bands):
            for a, b, what in zip(base, outputs(c), ("planes", "costs", "views")):
                assert np.array_equal(a[lo:hi], b[lo:hi]), ("band", lo, hi, what, float(np.mean(a[lo:hi] != b[lo:hi])))
    finally:
        for c in others:
            c.close()
        _env(monkeypatch, {})


def test_change_within_its_bound(rig, monkeypatch):
    name, sc, ctx = rig
    W, H, V, _ = SHAPES[name]
    px, py = _queries(sc, W, H)
    p = _params(sc)
    planes, _, _, cv_off = at_pixels(init_state(ctx, monkeypatch, ACMMP_REF_NEG_SKIP="0"), W, px, py)
    cv_on = at_pixels(init_state(ctx, monkeypatch), W, px, py)[3]
    cv_big = at_pixels(init_state(ctx, monkeypatch, ACMMP_REF_NEG_TAU=repr(BIG_TAU[H])), W, px, py)[3]
    off, on, big = (a.view(np.float32) for a in (cv_off, cv_on, cv_big))
    none = np.zeros(36, bool)
    n = n_class = n_f64_class = n_lin = 0
    worst_ratio, near_on, near_off, near_big, big_moves = 0.0, [], [], [], []
    for q in range(0, len(px), 2):
        x, y = int(px[q]), int(py[q])
        w = ns.weights(sc.images, sc.cameras, p, x, y)
        m_tau, m_big = rn.pixel_mask(w), rn.pixel_mask(w, tau=BIG_TAU[H])
        own = float((w * m_tau).sum() / w.sum())
        assert own <= 36 * rn.TAU
        plane = planes[q].astype(np.float64)
        for v in range(V):
            a = (sc.images, sc.cameras, p, v + 1, x, y, plane)
            c, t = rn.masked_ncc(*a, none, terms=True)
            n += 1
            n_f64_class += t is None
            if t is None or on[q, v] >= 2.0 or off[q, v] >= 2.0:
                n_class += 1
                continue
            b = ns.on_off_bound(t, drop=own)
            if b is None:
                n_lin += 1
                continue
            dq = abs(float(on[q, v]) - float(off[q, v]))
            worst_ratio = max(worst_ratio, dq / b)
            assert dq <= b, (q, v, dq, b)
            near_on.append(abs(float(on[q, v]) - rn.masked_ncc(*a, m_tau)) <= 1e-4)
            near_off.append(abs(float(off[q, v]) - c) <= 1e-4)
            c_big = rn.masked_ncc(*a, m_big)
            if c_big < 2.0 and big[q, v] < 2.0:
                near_big.append(abs(float(big[q, v]) - c_big) <= 1e-4)
                big_moves.append(abs(c_big - c))
    f_on, f_off, f_big = float(np.mean(near_on)), float(np.mean(near_off)), float(np.mean(near_big))
    big_moves = np.array(big_moves)
    print(f"{name}: {n} cached costs against float64: excluded {n_class / n:.3f} (cost class 2.0; in float64 alone "
          f"{n_f64_class / n:.3f}) + {n_lin / n:.4f} (variance too small for the bound), worst |on - off| / bound "
          f"{worst_ratio:.3g}; within 1e-4 of float64: on {f_on:.3f}, off {f_off:.3f}, large tau {f_big:.3f} (it moves "
          f"{np.mean(big_moves > 1e-3):.3f} of the float64 costs by more than 1e-3)")
    assert len(near_on) >= 100 and n_lin / n <= 0.02
    assert n_class / n <= n_f64_class / n + 0.02
    assert f_on >= f_off - 0.01
    assert np.mean(big_moves > 1e-3) >= 0.1, np.mean(big_moves > 1e-3)
    assert f_big >= f_off - 0.03, (f_big, f_off)
