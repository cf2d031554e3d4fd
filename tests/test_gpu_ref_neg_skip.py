"""The per-pixel negligible-sample mask of the fast SPHERE refinement at V <= 4 (ncc_chunk's PNEG
instances in k_eval_ref, k_eval_ref_tail and k_select's cache-miss evaluation), through the per-query hook
acmmp_debug_ncc_ref (k_eval_ref's staging and NCC instance) and through short whole runs.

Shapes: 2000x1000 V = 2 and 2000x1500 V = 4, the smallest at which the gate holds; query sets and the large
thresholds (BIG_TAU) are test_gpu_neg_skip.py's.

  * ACMMP_REF_NEG_SKIP=0 launches the instances without the mask.  A threshold so small that no sample with a
    weight qualifies (ACMMP_REF_NEG_TAU=1e-45: the masked instances, empty mask) gives the same bits, per query and
    over a 2-half-sweep run's planes, costs and selected views.
  * ACMMP_REF_NEG_SKIP=0 against the parent commit's library: planes and costs of the 2-half-sweep run at 2000x1000
    V = 2 on a fixed seeded sample of pixels (tests/golden/ref_neg_parent_2000x1000-v2.npy, recorded on an MI355X),
    bit for bit.
  * With every sample masked (ACMMP_REF_NEG_TAU=1) every cost of the hook is 2.0: the mask reaches the loop.
  * Cut invariance.  Which of the three kernels evaluates a (pixel, plane, view), and beside which other pixels,
    depends on the strip cut and the refinement's split point; a mask that depended on the wave would show as
    differing bits between cuts -- but only at a threshold that moves costs, so the set runs at BIG_TAU (where each
    run must also differ from the unmasked one) and at the product threshold.
  * Product threshold, hook on against off: the same cost class everywhere, and per query |on - off| within the pixel's
    own dropped share (at most 36 tau) plus one binary32 spacing per operation, propagated through the NCC
    (np_neg_skip.on_off_bound) from the float64 terms of the per-sample restatement (np_ref_neg_skip).  Excluded:
    entries with a cost of 2.0 in a run or in float64, and those whose source variance is too small for the bound's
    first-order form; both shares are printed and capped -- the second at the 2% tests/test_ref_neg_mask_design.py
    holds the restatement to on the same sets, the first at float64's own share of 2.0 costs plus 2 points.
  * At the large threshold the hook is within 1e-4 of the float64 restatement with that threshold's per-pixel mask as
    often as the unmasked hook is of the unmasked restatement, to 3 points (test_gpu_neg_skip.py's gate): a threshold
    scaled wrongly, held against another sum or folded over the wrong samples parts the two.
"""
import os

import numpy as np
import pytest

import np_neg_skip as ns
import np_ref_neg_skip as rn
from acmmp import capi, scene
from test_gpu_neg_skip import BIG_TAU, SHAPES, _params

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KNOBS = ("ACMMP_REF_NEG_SKIP", "ACMMP_REF_NEG_TAU", "ACMMP_STRIPS", "ACMMP_REF_SPLIT", "ACMMP_REF_SPLIT_AT")
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731


def _scene(name):
    W, H, V, seed = SHAPES[name]
    return scene.sphere_scene(W, H, n_src=V, seed=seed, n_waves=16)


@pytest.fixture(scope="module", params=list(SHAPES))
def rig(request):
    name = request.param
    sc = _scene(name)
    with capi.Context(0) as ctx:
        ctx.set_params(_params(sc))
        ctx.upload_views(sc.images, sc.cameras)
        ctx.set_math("fast")
        yield name, sc, ctx


def _run(ctx, monkeypatch, n_half_sweeps, **env):
    """-> [planes, costs, selected views] as words, of a run with the given knobs (every other knob unset)."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx.run_patchmatch(9, n_half_sweeps=n_half_sweeps)
    planes, costs = ctx.download()
    sel, _ = ctx.download_aux()
    for k in env:
        monkeypatch.delenv(k)
    return [bits(planes).copy(), bits(costs).copy(), bits(sel).copy()]


def golden_sample(planes_w, costs_w):
    """The recorded sample of a 2000x1000 run: 4000 seeded pixels -> (4000, 5) words (plane, cost)."""
    H, W = costs_w.shape
    idx = np.random.default_rng(2024).choice(H * W, 4000, replace=False)
    return np.concatenate([planes_w.reshape(H * W, 4)[idx], costs_w.reshape(H * W, 1)[idx]], axis=1)


def test_hook(rig, monkeypatch):
    name, sc, ctx = rig
    W, H, V, _ = SHAPES[name]
    px, py, planes = rn.hook_queries(sc, W, H)

    def hook(**env):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = ctx.debug_ncc_ref(px, py, planes)
        for k in env:
            monkeypatch.delenv(k)
        return out

    on = hook()
    off = hook(ACMMP_REF_NEG_SKIP="0")
    empty = hook(ACMMP_REF_NEG_TAU="1e-45")
    gone = hook(ACMMP_REF_NEG_TAU="1.0")
    big = hook(ACMMP_REF_NEG_TAU=repr(BIG_TAU[H]))
    live = off < 2.0
    assert live.mean() > 0.1, live.mean()
    # the masked instance with an empty mask against the instance without one
    assert np.array_equal(bits(empty), bits(off))
    # every sample masked: no source sums, every cost 2.0
    assert np.all(gone == 2.0)
    # the product threshold: the same class everywhere
    assert np.array_equal(on >= 2.0, off >= 2.0)
    d = np.abs(on - off)[live]
    changed = float(np.mean(bits(on)[live] != bits(off)[live]))
    moved = float(np.mean(np.abs(big - off)[live] > 1e-3))
    print(f"{name}: {on.size} costs, {live.mean():.3f} live, {changed:.5f} of them change bits at the product "
          f"threshold, worst |on - off| {d.max():.3g}; the large threshold moves {moved:.3f} of them by more than 1e-3")
    # the large threshold reaches into samples that carry weight (else the cut-invariance test below shows nothing)
    assert moved >= 0.1, moved
    # Against float64 (np_ref_neg_skip.float64_study: every 5th query, a near-surface and the far plane, every view).
    n = n_class = n_f64_class = n_lin = 0
    worst_ratio, near_on, near_off, near_big, big_moves = 0.0, [], [], [], []
    for q, h, v, c, t, c_tau, c_big, own in rn.float64_study(sc, _params(sc), px, py, planes, BIG_TAU[H]):
        n += 1
        n_f64_class += t is None
        if t is None or on[q, h, v] >= 2.0 or off[q, h, v] >= 2.0:
            n_class += 1
            continue
        assert own <= 36 * rn.TAU
        b = ns.on_off_bound(t, drop=own)
        if b is None:
            n_lin += 1
            continue
        dq = abs(float(on[q, h, v]) - float(off[q, h, v]))
        worst_ratio = max(worst_ratio, dq / b)
        assert dq <= b, (q, h, v, dq, b)
        near_on.append(abs(float(on[q, h, v]) - c_tau) <= 1e-4)
        near_off.append(abs(float(off[q, h, v]) - c) <= 1e-4)
        if c_big < 2.0 and big[q, h, v] < 2.0:
            near_big.append(abs(float(big[q, h, v]) - c_big) <= 1e-4)
            big_moves.append(abs(c_big - c))
    f_on, f_off, f_big = float(np.mean(near_on)), float(np.mean(near_off)), float(np.mean(near_big))
    big_moves = np.array(big_moves)
    print(f"{name}: {n} entries against float64: excluded {n_class / n:.3f} (cost class 2.0; in float64 alone "
          f"{n_f64_class / n:.3f}) + {n_lin / n:.4f} (variance too small for the bound), worst |on - off| / bound "
          f"{worst_ratio:.3g}; within 1e-4 of float64: on {f_on:.3f}, off {f_off:.3f}, large tau {f_big:.3f} (it moves "
          f"{np.mean(big_moves > 1e-3):.3f} of the float64 costs by more than 1e-3)")
    assert len(near_on) >= 100 and n_lin / n <= 0.02
    assert n_class / n <= n_f64_class / n + 0.02
    assert f_on >= f_off - 0.01
    # the large threshold: its mask matters on these sets, and the kernel follows the restatement's mask as closely
    assert np.mean(big_moves > 1e-3) >= 0.1, np.mean(big_moves > 1e-3)
    assert f_big >= f_off - 0.03, (f_big, f_off)


def test_empty_mask_run(rig, monkeypatch):
    name, sc, ctx = rig
    off = _run(ctx, monkeypatch, 2, ACMMP_REF_NEG_SKIP="0")
    empty = _run(ctx, monkeypatch, 2, ACMMP_REF_NEG_TAU="1e-45")
    for a, b in zip(off, empty):
        assert np.array_equal(a, b)
    assert np.isfinite(off[1].view(np.float32)).any()
    if name == "2000x1000-v2":
        # the unmasked instances against the parent commit's library
        want = np.load(os.path.join(GOLDEN, "ref_neg_parent_2000x1000-v2.npy"))
        assert np.array_equal(golden_sample(off[0], off[1]), want)


@pytest.mark.parametrize("which", ["big", "product"])
def test_cut_invariance(rig, monkeypatch, which):
    name, sc, ctx = rig
    W, H, V, _ = SHAPES[name]
    tau = {} if which == "product" else {"ACMMP_REF_NEG_TAU": repr(BIG_TAU[H])}
    cuts = [{"ACMMP_STRIPS": "1"}, {"ACMMP_STRIPS": "2"}, {"ACMMP_STRIPS": "4"}, {"ACMMP_REF_SPLIT": "0"},
            {"ACMMP_REF_SPLIT_AT": "1"}]
    if V == 4:
        cuts += [{"ACMMP_REF_SPLIT_AT": "2"}, {"ACMMP_REF_SPLIT_AT": "3"}]
    off = _run(ctx, monkeypatch, 6, ACMMP_REF_NEG_SKIP="0")
    base = _run(ctx, monkeypatch, 6, **tau)
    differ = [float(np.mean(a != b)) for a, b in zip(base, off)]
    print(f"{name} {which}: against the unmasked run {differ[0]:.5f} of plane words, {differ[1]:.5f} of costs, "
          f"{differ[2]:.5f} of selected views differ")
    if which == "big":
        assert differ[0] > 0 and differ[1] > 0
    for cut in cuts:
        got = _run(ctx, monkeypatch, 6, **tau, **cut)
        for a, b, what in zip(base, got, ("planes", "costs", "views")):
            assert np.array_equal(a, b), (cut, what, float(np.mean(a != b)))
        if which == "big":
            assert not np.array_equal(got[1], off[1]), cut
