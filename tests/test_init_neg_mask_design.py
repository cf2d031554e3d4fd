"""The per-pixel negligible-sample mask in k_init, CPU, float64: on the pixel sets
tests/test_gpu_init_neg_skip.py queries -- rows at the dead band's edges, seam columns, rows next to both poles, mixed
dead / live runs -- every live pixel drops at most 36 tau of its own weight sum, at the product threshold and at the
large thresholds the GPU test moves costs with (tests/test_ref_neg_mask_design.py's argument: each dropped weight is
at most tau x the sum, and there are 36 samples); a pixel below the patch-sum floor has no mask; and the sets hold
enough live pixels, with masked samples among them, for the GPU test to mean something.  Also held: the binary32
restatement of initial_cost's fold the GPU test compares k_init's cost and selected views with."""
import numpy as np
import pytest

import np_neg_skip as ns
import np_ref_neg_skip as rn
from acmmp import scene
from test_gpu_init_neg_skip import fold
from test_gpu_neg_skip import BIG_TAU, SHAPES, _params, _queries


@pytest.mark.parametrize("name", list(SHAPES))
def test_dropped_share_on_the_init_queries(name):
    W, H, V, seed = SHAPES[name]
    sc = scene.sphere_scene(W, H, n_src=V, seed=seed, n_waves=16)
    p = _params(sc)
    px, py = _queries(sc, W, H)
    n_live = n_masked = n_big = 0
    worst = {rn.TAU: 0.0, BIG_TAU[H]: 0.0}
    for x, y in zip(px.tolist(), py.tolist()):
        w = ns.weights(sc.images, sc.cameras, p, x, y)
        sbw = w.sum()
        if sbw < 1e-6:
            assert not rn.pixel_mask(w).any() and not rn.pixel_mask(w, tau=BIG_TAU[H]).any()
            continue
        n_live += 1
        for tau in worst:
            m = rn.pixel_mask(w, tau=tau)
            share = float((w * m).sum() / sbw)
            assert share <= 36 * tau, (x, y, tau, share)
            assert not np.any(m & (w > tau * sbw))
            worst[tau] = max(worst[tau], share / (36 * tau))
        n_masked += int(rn.pixel_mask(w).sum())
        n_big += int(rn.pixel_mask(w, tau=BIG_TAU[H]).sum())
    print(f"{name}: {len(px)} pixels, {n_live} live, {n_masked / n_live:.1f} of 36 samples masked at 2^-35, "
          f"{n_big / n_live:.1f} at {BIG_TAU[H]:g}; largest dropped share / (36 tau): "
          + ", ".join(f"{v:.3g}" for v in worst.values()))
    assert n_live >= 100 and n_masked > 0 and n_big > n_masked


def test_fold_restates_initial_cost():
    """ACMMP.cu:519-556 in binary32, one vector at a time, against the vectorised fold."""
    rng = np.random.default_rng(3)
    for V, top_k in ((1, 4), (2, 4), (4, 4), (4, 2)):
        cv = rng.uniform(0, 2.2, (300, V)).astype(np.float32)
        cv[cv > 2.0] = 2.0
        cv[::7, 0] = cv[::7, V - 1]                               # ties
        cost, sel = fold(cv, top_k)
        for q in range(len(cv)):
            c = sorted(cv[q].tolist())
            k = min(sum(1 for a in cv[q] if a < 2.0), top_k)
            if k == 0:
                assert cost[q] == np.float32(2.0).view(np.uint32) and sel[q] == 0
                continue
            acc = np.float32(0.0)
            for a in c[:k]:
                acc = np.float32(acc + np.float32(a))
            assert cost[q] == np.float32(acc / np.float32(k)).view(np.uint32)
            assert sel[q] == sum(1 << i for i in range(V) if cv[q, i] <= np.float32(c[k - 1]))
