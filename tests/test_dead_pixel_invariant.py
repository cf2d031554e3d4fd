"""A SPHERE pixel whose bilateral weight sum is below 1e-6 (every NCC 2.0, ACMMP.cu:501-503) leaves each of its
half-sweeps exactly as DESIGN.md §4 says: plane and selected views unchanged, cost 0/0, 15 draws, nothing
accepted.  The engine's dead-pixel mask relies on that; this pins it on the oracle itself (CPU only).

Shape: SPHERE 128x512, V = 2, 2 iterations (4 half-sweeps), a plain pass and a planar-prior pass whose mask
covers the band.  The dead set is read off the oracle: the pixels whose initial per-view costs are all 2.0
(initial cost 2.0 with no selected view, ACMMP.cu:519-556) under the plain pass's random planes -- and, in the
prior pass, under that pass's starting planes too.  One plane field alone is not enough there: a live pixel
whose starting plane fails on every view (variance or image bounds) also starts at 2.0, and such a pixel does
move (2 of 65536 in the prior pass).  The oracle's trace holds a pixel's last update only, so the state after
every half-sweep comes from one run per half-sweep count.  Tolerance: none."""
import numpy as np
import pytest

from acmmp import scene, types

W, H, V, ITERS = 128, 512, 2, 2


def _params(sc, **kw):
    c0 = sc.cameras[0]
    return types.default_params(num_images=len(sc.images), depth_min=float(c0["depth_min"]) * 0.6,
                                depth_max=float(c0["depth_max"]) * 1.2, max_iterations=ITERS, **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _all_two(oracle_mod, prob, seed, **state):
    """The pass's initial state, and the pixels whose initial costs are 2.0 on every view."""
    init = oracle_mod.run_patchmatch(prob, seed, n_half_sweeps=0, do_post=False, **state)
    return init, (init["costs"] == 2.0) & (init["selected_views"] == 0)


def _check_pass(oracle_mod, prob, seed, within=None, **state):
    """Runs the pass for 0 .. 2 * ITERS half-sweeps and checks the dead pixels after each."""
    init, dead = _all_two(oracle_mod, prob, seed, **state)
    if within is not None:
        dead &= within
    frac = float(dead.mean())
    print(f"dead fraction {frac:.3f}")
    assert 0.3 < frac < 0.9, frac
    yy, xx = np.mgrid[0:H, 0:W]
    # rows the reference's checkerboard grid covers (the rest is never updated)
    covered = yy < min(H, 32 * ((H // 2 + 15) // 16))
    for n in range(1, 2 * ITERS + 1):
        out = oracle_mod.run_patchmatch_traced(prob, seed, n_half_sweeps=n, do_post=False, **state)
        colour = (n - 1) & 1
        upd = dead & covered & (((xx + yy) & 1) == colour)       # updated by half-sweep n - 1
        assert upd.any()
        seen = dead & covered & ((n > 1) | (((xx + yy) & 1) == 0))  # updated at least once so far
        assert np.array_equal(_bits(out["planes"])[dead], _bits(init["planes"])[dead]), f"planes, {n} half-sweeps"
        assert np.array_equal(out["selected_views"][dead], init["selected_views"][dead]), f"views, {n} half-sweeps"
        assert np.isnan(out["costs"][seen]).all(), f"costs, {n} half-sweeps"
        tr = out["trace"][upd]
        assert np.all(tr["draws_after"] - tr["draws_before"] == 15), f"draws, {n} half-sweeps"
        assert np.all(tr["accepted"] == 8), f"accepted, {n} half-sweeps"
        assert not tr["view_weights"].any() and not tr["temp_selected_views"].any()
    return dead


@pytest.fixture(scope="module")
def band_scene():
    return scene.sphere_scene(W, H, n_src=V, seed=5)


def test_plain_pass(oracle_mod, band_scene):
    sc = band_scene
    _check_pass(oracle_mod, oracle_mod.Problem(sc.images, sc.cameras, _params(sc)), seed=77)


def test_planar_prior_pass(oracle_mod, band_scene):
    """Prior-restricted propagation (ACMMP.cu:1247-1299): the restricted costs of a dead pixel are NaN too, so
    no neighbour and no candidate is taken, with the prior's label set over the whole band."""
    sc = band_scene
    first = oracle_mod.run_patchmatch(oracle_mod.Problem(sc.images, sc.cameras, _params(sc)), seed=77, do_post=True)
    rng = np.random.default_rng(2)
    prior = np.zeros((H, W, 4), np.float32)
    prior[..., 2] = -1.0
    prior[..., 3] = rng.uniform(4.0, 6.0, (H, W)).astype(np.float32)
    prior[..., :3] += rng.normal(0, 0.1, (H, W, 3)).astype(np.float32)
    mask = np.ones((H, W), np.uint32)
    mask[:, ::7] = 0                                             # some pixels of every row keep the plain branch
    prob = oracle_mod.Problem(sc.images, sc.cameras, _params(sc, planar_prior=1), prior_planes=prior,
                              plane_masks=mask)
    _, dead0 = _all_two(oracle_mod, oracle_mod.Problem(sc.images, sc.cameras, _params(sc)), seed=77)
    dead = _check_pass(oracle_mod, prob, seed=78, within=dead0, planes=first["planes"], costs=first["costs"])
    assert (mask[dead] > 0).any() and (mask[dead] == 0).any()
