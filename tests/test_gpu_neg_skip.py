"""The fast SPHERE k_eval_nb's negligible-sample mask (kernels.hip stage_neg_mask) through the
per-query hook acmmp_debug_ncc_nb, which runs k_eval_nb's staging and NCC instance (a wave = 8 consecutive
queries), and through short whole runs.

Query sets per shape (2000x1000 V = 2 and 2000x1500 V = 4, the smallest that interpolate): the pole, seam and
random sets of test_gpu_interp.py, rows at the edge of the dead band, rows next to both poles, seam columns,
and waves that mix dead (patch sum below 1e-6) and live pixels.

  * ACMMP_NEG_SKIP=0 launches the instance without the mask: its costs equal the parent commit's on the same
    queries bit for bit (tests/golden/neg_skip_parent_*.npy).  A threshold so small that no sample qualifies
    (ACMMP_NEG_TAU=1e-45: the masked instance with an empty mask) must give the same bits.
  * With every sample masked (ACMMP_NEG_TAU=1) the interpolated costs become 2.0 and the fallbacks keep the
    per-sample bits: the mask reaches the loop and only the loop.
  * At the product threshold, on against off: the same cost class everywhere, and per query |on - off| within the
    36 tau dropped mass plus one binary32 spacing per operation, propagated through the NCC
    (np_neg_skip.on_off_bound).  Both are within 1e-4 of the float64 interpolated restatement as often as the
    per-sample fast arithmetic is of its own restatement.  The excluded share is printed and capped.
  * At a large threshold (2^-10, 2^-3 at 1500 rows), where the mask moves costs visibly, the kernel stays as close to the float64
    restatement with that threshold's mask as the unmasked kernel to the unmasked restatement: the mask is
    folded over the right pixels and samples.
  * The fallback set is the same on and off: the entries k_nb_fix recomputed (the ones that keep a cost with
    every sample masked) equal the per-sample hook bit for bit in both runs.
"""
import os

import numpy as np
import pytest

import np_interp as ni
import np_neg_skip as ns
from acmmp import capi, scene, types

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# a threshold at which the mask moves costs visibly: at 1500 rows a pixel of vertical offset costs 9.55 in the exponent, so
# only the |j| = 1 samples carry weight and it takes 2^-3 to reach into them; at 1000 rows (6.37) 2^-10 does
BIG_TAU = {1000: 2.0 ** -10, 1500: 2.0 ** -3}
SHAPES = {"2000x1000-v2": (2000, 1000, 2, 77), "2000x1500-v4": (2000, 1500, 4, 1234)}


def _params(sc):
    c0 = sc.cameras[0]
    return types.default_params(num_images=len(sc.images), depth_min=float(c0["depth_min"]) * 0.6,
                                depth_max=float(c0["depth_max"]) * 1.2)


def _queries(sc, W, H):
    """-> px, py: whole waves of 8 queries."""
    rng = np.random.default_rng(W + H)
    xs, ys = [], []
    for kind, n in (("random", 40), ("pole", 32), ("seam", 32)):
        px, py, _ = ni.special_pixels(sc, kind, n, seed=len(kind) + 17)
        px, py = px[:len(px) // 8 * 8], py[:len(py) // 8 * 8]
        xs.append(px)
        ys.append(py)
    # rows around the dead band's edges (|latitude| 38 .. 50 degrees), next to both poles, at the seam columns
    band = [int(H * (0.5 + s * d / 180.0)) for s in (-1, 1) for d in (38, 41, 44, 47, 50)]
    poles = [6, 7, 9, 14, H - 15, H - 10, H - 8, H - 7]
    for row in band + poles:
        x0 = int(rng.integers(8, W - 24)) & ~1
        xs.append(np.arange(x0, x0 + 16, 2))                    # 8 consecutive pixels of one colour: a real wave
        ys.append(np.full(8, row))
        xs.append(np.array([0, 2, 4, 6, W - 8, W - 6, W - 4, W - 2]))
        ys.append(np.full(8, row))
    # mixed waves: 4 pixels on the equator (dead: patch sum below 1e-6) beside 4 live ones
    for row in (band[0], band[-1], poles[0]):
        x0 = int(rng.integers(8, W - 24))
        xs.append(np.array([x0, x0 + 1, x0 + 2, x0 + 3] * 2))
        ys.append(np.array([H // 2, row, H // 2 + 1, row, row, H // 2, row, H // 2 - 1]))
    return np.concatenate(xs).astype(np.int32), np.concatenate(ys).astype(np.int32)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _setup(name):
    """-> scene, params, query pixels and their 8 planes each (6 near the surface, 2 far off it)."""
    W, H, V, seed = SHAPES[name]
    sc = scene.sphere_scene(W, H, n_src=V, seed=seed, n_waves=16)
    px, py = _queries(sc, W, H)
    assert 200 <= len(px) <= 600 and len(px) % 8 == 0
    planes = ni.near_surface_planes(sc, px, py, 8, seed=31)
    planes[:, 6:] = ni.near_surface_planes(sc, px, py, 2, seed=33, spread=1.5, depth_jitter=0.4)
    return sc, _params(sc), px, py, planes


@pytest.mark.parametrize("name", list(SHAPES))
def test_mask_per_query(ctx, name, monkeypatch):
    W, H, V, seed = SHAPES[name]
    sc, p, px, py, planes = _setup(name)
    ctx.set_params(p)
    ctx.upload_views(sc.images, sc.cameras)
    ctx.set_math("fast")

    def run(**env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = ctx.debug_ncc_nb(px, py, planes)
        for k in env:
            monkeypatch.delenv(k)
        return out

    on = run()
    off = run(ACMMP_NEG_SKIP="0")
    empty = run(ACMMP_NEG_TAU="1e-45")
    ps = ctx.debug_ncc(np.repeat(px, 8), np.repeat(py, 8), planes.reshape(-1, 4)).reshape(on.shape)
    bits = lambda a: a.view(np.uint32)  # noqa: E731
    # the masked instance with an empty mask against the instance without the mask: the same bits
    assert np.array_equal(bits(empty), bits(off))
    # (a dropped term is below the sums' rounding, so few bits change: `changed` is printed, not gated)
    live = off < 2.0
    assert live.mean() > 0.1, live.mean()
    if H == 1500:                                   # (2000x1000 has no dead band: its mixed waves are all live)
        assert (~live).mean() > 0.05, live.mean()
    changed = float(np.mean(bits(on)[live] != bits(off)[live]))
    # class and distance
    assert np.array_equal(on >= 2.0, off >= 2.0)
    d = np.abs(on - off)[live]
    # The fallback set.  With every sample masked (tau = 1) an interpolated view has no source sums, so its cost is
    # 2.0; an entry that still has a cost below 2.0 was recomputed by k_nb_fix, which keeps all 36 samples.  Those
    # entries carry the per-sample hook's bits with the mask on and off alike, and no other live entry is left
    # (equal bits alone do not mark a fallback: costs a rounding apart often coincide).
    gone = run(ACMMP_NEG_TAU="1.0")
    fell = (gone < 2.0) & live
    print(f"{name}: {on.size} queries, {live.mean():.3f} live, {changed:.5f} of the live ones changed bits, "
          f"worst |on - off| {d.max():.3g}, fallbacks {int(fell.sum())}")
    assert np.array_equal(bits(gone)[fell], bits(ps)[fell])
    assert np.array_equal(bits(on)[fell], bits(ps)[fell]) and np.array_equal(bits(off)[fell], bits(ps)[fell])
    assert np.all(gone[live & ~fell] >= 2.0) and (live & ~fell).sum() > 0.5 * live.sum()
    # ACMMP_NEG_SKIP=0 against the parent commit's library on the same queries (tests/golden, recorded on an MI355X)
    want = np.load(os.path.join(GOLDEN, f"neg_skip_parent_{name}.npy"))
    assert np.array_equal(bits(off), want)
    # A threshold large enough to matter (BIG_TAU: the masked terms now move costs by more than the fast mode's noise)
    # against the float64 restatement with the same threshold and the hook's own waves (8 consecutive queries):
    # a mask folded over the wrong pixels or samples, or a threshold scaled wrongly, parts the two.
    big = run(ACMMP_NEG_TAU=repr(BIG_TAU[H]))
    ctx.set_math("exact")
    exact = ctx.debug_ncc_nb(px, py, planes)
    ctx.set_math("fast")
    # On against off, per query, within the 36 tau bound propagated through the NCC with one binary32 spacing per
    # operation (np_neg_skip.on_off_bound: what the arithmetic can need, whatever the number of steps), from the
    # float64 terms of the interpolated restatement: a near-surface and a far plane of every 2nd query, every view
    # (every wave of the sets).  Excluded: entries with a cost of 2.0 in a run or in float64 -- held against what
    # test_gpu_interp.py's rule (exact, fast or float64 per-sample cost of 2.0) excludes on the same entries -- and
    # those whose source variance is too small for the bound's first-order form, capped at 2%.
    none = np.zeros(36, bool)
    n = n_class = n_lin = n_interp_rule = 0
    worst_ratio, near, near_ps, big_near, big_moves = 0.0, [], [], [], []
    for q in range(0, len(px), 2):
        w0 = q // 8 * 8
        wts = np.stack([ns.weights(sc.images, sc.cameras, p, int(px[k]), int(py[k])) for k in range(w0, w0 + 8)])
        m_big, m_tau = ns.wave_mask(wts, tau=BIG_TAU[H]), ns.wave_mask(wts)
        own = float((wts[q - w0] * m_tau).sum() / wts[q - w0].sum())
        assert own <= 36 * ns.TAU or wts[q - w0].sum() < 1e-6      # (a pixel below the patch-sum floor has no say)
        for h in (0, 7):
            plane = planes[q, h].astype(np.float64)
            for v in range(V):
                n += 1
                a = (sc.images, sc.cameras, p, v + 1, int(px[q]), int(py[q]), plane)
                c, _, t = ns.masked_ncc(*a, none, terms=True)
                ref = ni.ncc(*a, False)[0]
                n_interp_rule += bool(exact[q, h, v] >= 2.0 or off[q, h, v] >= 2.0 or ref >= 2.0)
                if t is None or on[q, h, v] >= 2.0 or off[q, h, v] >= 2.0:
                    n_class += 1
                    continue
                b = ns.on_off_bound(t)
                if b is None:
                    n_lin += 1
                    continue
                dq = abs(float(on[q, h, v]) - float(off[q, h, v]))
                worst_ratio = max(worst_ratio, dq / b)
                assert dq <= b, (q, h, v, dq, b)
                near.append((abs(float(on[q, h, v]) - c) <= 1e-4, abs(float(off[q, h, v]) - c) <= 1e-4))
                if ref < 2.0 and ps[q, h, v] < 2.0:
                    near_ps.append(abs(float(ps[q, h, v]) - ref) <= 1e-4)
                cb = ns.masked_ncc(*a, m_big)[0]
                if cb < 2.0 and big[q, h, v] < 2.0 and not fell[q, h, v]:
                    big_near.append(abs(float(big[q, h, v]) - cb) <= 1e-4)
                    big_moves.append(abs(cb - c))
    near, big_near, big_moves = np.array(near), np.array(big_near), np.array(big_moves)
    f_on, f_off, f_ps, f_big = near[:, 0].mean(), near[:, 1].mean(), float(np.mean(near_ps)), big_near.mean()
    print(f"{name}: {n} entries against float64: excluded {n_class / n:.3f} (cost class 2.0; test_gpu_interp's rule "
          f"{n_interp_rule / n:.3f}) + {n_lin / n:.4f} (variance too small for the bound), worst |on - off| / bound "
          f"{worst_ratio:.3g}; within 1e-4 of float64: on {f_on:.3f}, off {f_off:.3f}, per-sample fast {f_ps:.3f}, "
          f"large tau {f_big:.3f} (it moves {np.mean(big_moves > 1e-3):.3f} of the float64 costs by more than 1e-3)")
    assert len(near) >= 100 and n_lin / n <= 0.02
    assert (n_class + n_lin) / n <= n_interp_rule / n + 0.02
    # both within the existing tolerance of float64: as often within 1e-4 of the interpolated restatement as the
    # per-sample fast arithmetic is of the per-sample one, to 3 points (test_gpu_interp.py's gate), and alike
    assert f_on >= f_ps - 0.03 and f_off >= f_ps - 0.03, (f_on, f_off, f_ps)
    assert f_on >= f_off - 0.01
    # the large threshold: its mask matters on these sets, and the kernel follows the restatement's mask as closely
    assert np.mean(big_moves > 1e-3) >= 0.1, np.mean(big_moves > 1e-3)
    assert f_big >= f_off - 0.03, (f_big, f_off)
    ctx.set_math("exact")


def _run(ctx, seed):
    ctx.run_patchmatch(seed, n_half_sweeps=2)
    planes, costs = ctx.download()
    sel, _ = ctx.download_aux()
    return [np.ascontiguousarray(a).view(np.uint32) for a in (planes, costs, sel)]


def test_whole_run_strips_and_exact_mode(monkeypatch):
    """One iteration at 2000x1000, V = 2.  Two strips against one with the mask on: a wave's 8 pixels are fixed by
    the 8 x 4 tile geometry, which strips preserve, so the bits of planes, costs and selected views are the same.
    The exact mode with the knob set against unset: the knob does not reach it."""
    sc = scene.sphere_scene(2000, 1000, n_src=2, seed=77)
    with capi.Context(0) as ctx:
        ctx.set_params(_params(sc))
        ctx.upload_views(sc.images, sc.cameras)
        ctx.set_math("fast")
        monkeypatch.setenv("ACMMP_STRIPS", "1")
        one = _run(ctx, 9)
        monkeypatch.setenv("ACMMP_STRIPS", "2")
        two = _run(ctx, 9)
        for a, b in zip(one, two):
            assert np.array_equal(a, b)
        assert np.isfinite(one[1].view(np.float32)).any()
        ctx.set_math("exact")
        monkeypatch.delenv("ACMMP_STRIPS")
        unset = _run(ctx, 9)
        monkeypatch.setenv("ACMMP_NEG_TAU", "1.0")
        knob = _run(ctx, 9)
        for a, b in zip(unset, knob):
            assert np.array_equal(a, b)
