"""Parity on general camera rigs (tests/rig_support.py; their contents are checked without a GPU in
tests/test_rig_inputs.py): a posed reference far from the origin (`moved`), per-view intrinsics with skew
(`intrinsics`), sources rolled by quarter turns on a wide convergent baseline (`rolled`), samples behind a source
(`behind`), SPHERE sources whose seams and poles cross the reference image (`turned`), and queries whose point is a
source's centre (`degenerate`).  DESIGN.md "Camera rigs under test" says which statement each one reaches.

Exact mode, per rig, bit for bit against the CPU oracle, no tolerance: the three NCC hooks on the four query sets
(and the degenerate queries), acmmp_debug_geom on jittered rendered depth maps, a full default run, and a
geometric-consistency pass from that run's state.

Fast mode, per rig: the hook-against-hook bit equalities of tests/test_gpu_fast_instances.py (b), T1's gates
(fastmath_support.t1_gates) against float64 on the interior, border and source-edge sets, and the k_init identity of
test_fast_k_init_is_the_debug_hook.  On `behind`'s wild planes and on the degenerate queries: no NaN and T1's class
gate (a); the other fractions are recorded.  With ACMMP_TEST_REPORT_DIR set, rig_<name>.json (profiles/rigs/).

One interpolation case: a `turned` rig at 2000x1000 under test_gpu_interp.test_interpolated_k_eval_nb_per_query's own
assertions, then a full fast run that must not overflow the interpolation fallback queue.
"""
import json
import os

import numpy as np
import pytest

import fastmath_support as fs
import rig_support as rs
import test_gpu_interp as interp_tests
from acmmp import capi
from conftest import assert_bitwise_equal

pytestmark = pytest.mark.gpu

ALL = list(rs.RIGS) + list(rs.DEGENERATE)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.set_math("exact")
    c.close()


def _clean_env(monkeypatch):
    for name in ("ACMMP_PIN_HOMOG", "ACMMP_TEX16", "ACMMP_INTERP", "ACMMP_SPREAD_MAX"):
        monkeypatch.delenv(name, raising=False)


def _texel_bytes(name):
    return 2 if name in rs.DEGENERATE or rs.RIGS[name][2] == "f16" else 4


def _query_sets(name):
    """The rig's four sets, and the degenerate queries on a degenerate rig."""
    sets = dict(rs.rig_sets(name))
    if name in rs.DEGENERATE:
        sets["degenerate"] = rs.degenerate_queries(rs.make_rig(name)[0])
    return sets


@pytest.mark.parametrize("name", ALL)
def test_exact_hooks_are_the_oracle(ctx, oracle_mod, monkeypatch, name):
    sc, p = rs.make_rig(name)
    V = len(sc.images) - 1
    _clean_env(monkeypatch)
    ctx.set_math("exact")
    ctx.set_params(p)
    ctx.upload_views(sc.images, sc.cameras)
    assert ctx.texel_bytes() == _texel_bytes(name)
    for set_name, (px, py, planes) in _query_sets(name).items():
        what = f"{name}/{set_name}"
        orc = rs.rig_oracle(oracle_mod, name, set_name)
        fx, fy, fpl = fs.flat_queries(px, py, planes)
        e = ctx.debug_ncc(fx, fy, fpl).reshape(len(px), fs.PLANES, V)
        assert_bitwise_equal(e, orc, f"{what}: exact debug_ncc vs oracle")
        assert_bitwise_equal(ctx.debug_ncc_nb(px, py, planes), orc, f"{what}: exact debug_ncc_nb vs oracle")
        assert_bitwise_equal(ctx.debug_ncc_ref(px, py, np.ascontiguousarray(planes[:, :5])), orc[:, :5],
                             f"{what}: exact debug_ncc_ref vs oracle")


@pytest.mark.parametrize("name", ALL)
def test_geom_cost_is_the_oracle(ctx, oracle_mod, monkeypatch, name):
    """acmmp_debug_geom: reference pixel -> world -> source pixel -> the source's depth there -> world -> back into
    the reference, so the source's R, C and K are used in both directions.  Depth maps are each view's rendered depth
    times a (0.97, 1.03) jitter with a lattice of zeros; two planes of every query of every set."""
    sc, p = rs.make_rig(name)
    V = len(sc.images) - 1
    _clean_env(monkeypatch)
    depths = rs.geom_depths(sc, seed=5)
    ctx.set_math("exact")
    ctx.set_params(p)
    ctx.upload_views(sc.images, sc.cameras)
    ctx.upload_depths(depths)
    prob = oracle_mod.Problem(sc.images, sc.cameras, p, depths=depths)
    close = 0
    for set_name, (px, py, planes) in _query_sets(name).items():
        fx, fy, fpl = fs.flat_queries(px, py, planes[:, :2])
        g = ctx.debug_geom(fx, fy, fpl)
        o = np.array([[oracle_mod.geom_cost(prob, v + 1, int(fx[k]), int(fy[k]), fpl[k]) for v in range(V)]
                      for k in range(len(fx))], np.float32)
        assert_bitwise_equal(g, o, f"{name}/{set_name}: geom")
        close += int((o < 3.0).sum())
    assert close >= 100, close                                  # the comparison is not one of 3.0 with 3.0


_first_pass = {}


def _oracle_first_pass(oracle_mod, name):
    if name not in _first_pass:
        sc, p = rs.make_rig(name)
        _first_pass[name] = oracle_mod.run_patchmatch(oracle_mod.Problem(sc.images, sc.cameras, p), seed=4321)
    return _first_pass[name]


def _gpu_run(ctx, sc, p, seed, planes=None, costs=None, depths=None):
    ctx.set_params(p)
    ctx.upload_views(sc.images, sc.cameras)
    if depths is not None:
        ctx.upload_depths(depths)
    if planes is not None:
        ctx.set_state(planes, costs)
    ctx.run_patchmatch(seed)
    pl, co = ctx.download()
    return {"planes": pl, "costs": co, "selected_views": ctx.download_aux()[0]}


@pytest.mark.parametrize("name", ALL)
def test_full_run_bitexact(ctx, oracle_mod, monkeypatch, name):
    sc, p = rs.make_rig(name)
    _clean_env(monkeypatch)
    ctx.set_math("exact")
    g = _gpu_run(ctx, sc, p, seed=4321)
    o = _oracle_first_pass(oracle_mod, name)
    for k in ("planes", "costs", "selected_views"):
        assert_bitwise_equal(g[k], o[k], f"{name}: {k}")
    assert np.mean(o["costs"] < 2.0) > 0.5


@pytest.mark.parametrize("name", ALL)
def test_geom_consistency_pass_bitexact(ctx, oracle_mod, monkeypatch, name):
    """Pass 2 of the reference schedule from the first pass's state; the sources' depth maps are their rendered
    depths, jittered."""
    sc, p = rs.make_rig(name)
    _clean_env(monkeypatch)
    first = _oracle_first_pass(oracle_mod, name)
    depths = [first["planes"][..., 3]] + rs.geom_depths(sc, seed=9)[1:]
    pg = fs.params_for(sc, geom_consistency=1, max_iterations=2)
    ctx.set_math("exact")
    g = _gpu_run(ctx, sc, pg, seed=2, planes=first["planes"], costs=first["costs"], depths=depths)
    o = oracle_mod.run_patchmatch(oracle_mod.Problem(sc.images, sc.cameras, pg, depths=depths), seed=2,
                                  planes=first["planes"], costs=first["costs"])
    for k in ("planes", "costs", "selected_views"):
        assert_bitwise_equal(g[k], o[k], f"{name}: {k}")


def _class_gate(f, e, ref, what):
    """T1 (a) alone, as fastmath_support.t1_gates states it, and no NaN -> t1_fractions."""
    fr = fs.t1_fractions(f, e, ref)
    assert fr["fast_nan"] == 0, (what, fr["fast_nan"])
    agree_fe, agree_ef = fr["class_agree_fast_exact"], fr["class_agree_exact_f64"]
    assert agree_fe >= agree_ef - 0.002 and agree_fe >= 0.99, (what, agree_fe, agree_ef)
    return fr


@pytest.mark.parametrize("name", ALL)
def test_fast_hooks_per_query(ctx, oracle_mod, monkeypatch, name):
    sc, p = rs.make_rig(name)
    V = len(sc.images) - 1
    sphere = sc.kind == "sphere"
    _clean_env(monkeypatch)
    ctx.set_math("fast")
    ctx.set_params(p)
    ctx.upload_views(sc.images, sc.cameras)
    assert ctx.texel_bytes() == _texel_bytes(name)
    report, gates = {}, []
    try:
        for set_name, (px, py, planes) in _query_sets(name).items():
            what = f"{name}/{set_name}"
            e = rs.rig_oracle(oracle_mod, name, set_name)          # exact mode = the oracle (test_exact_hooks_...)
            f64, _ = rs.rig_f64(name, set_name)
            hooks = rs.fast_hook_costs(ctx, monkeypatch, px, py, planes, V, sphere, what)
            report[set_name] = {"pixels": len(px)}
            for hook, f in hooks.items():
                k = f.shape[1]
                fr = fs.t1_fractions(f, e[:, :k], f64[:, :k])
                print(what, hook, json.dumps(fr))
                report[set_name][hook] = fr
                gates.append((set_name, hook, f, e[:, :k], f64[:, :k]))
        for set_name, hook, f, e, f64 in gates:                    # (every set is measured before any is judged)
            what = f"{name}/{set_name}: {hook}"
            if set_name in ("interior", "border", "source_edge"):
                fr = fs.t1_gates(f, e, f64, sphere, what=what)
                assert fr["valid"] >= fs.MIN_VALID, (what, fr["valid"])
            elif set_name == "wild" and "behind" in name:
                _class_gate(f, e, f64, what)
            elif set_name == "degenerate":
                continue                                            # judged in test_fast_degenerate_queries
            else:
                assert not np.isnan(f).any(), what
    finally:
        ctx.set_math("exact")
        out_dir = os.environ.get("ACMMP_TEST_REPORT_DIR")
        if out_dir:                                                 # (a failing rig records what it measured too)
            os.makedirs(out_dir, exist_ok=True)
            with open(os.path.join(out_dir, f"rig_{name}.json"), "w") as fh:
                json.dump(report, fh, indent=1)


@pytest.mark.parametrize("name", list(rs.DEGENERATE))
def test_fast_degenerate_queries(ctx, oracle_mod, monkeypatch, name):
    """Queries with a sample (or the patch centre) on the first source's centre: no NaN, and T1's class gate (a).
    The fast SPHERE projection's atan divisors are floored (camera_dev.h max_abs_nt / max_abs_h), so the point projects
    to the principal point as ProjectonCamera_cu's `d < 1e-6` branch does; unfloored it was NaN, the view's cost 2.0,
    and fast agreed with exact on the class of 0.74 of the pairs.  Pinhole: tz == 0 is an out-of-image sample in both
    modes."""
    sc, p = rs.make_rig(name)
    V = len(sc.images) - 1
    _clean_env(monkeypatch)
    px, py, planes = rs.degenerate_queries(sc)
    e = rs.rig_oracle(oracle_mod, name, "degenerate")
    f64, _ = rs.rig_f64(name, "degenerate")
    try:
        ctx.set_math("fast")
        ctx.set_params(p)
        ctx.upload_views(sc.images, sc.cameras)
        hooks = rs.fast_hook_costs(ctx, monkeypatch, px, py, planes, V, sc.kind == "sphere", name)
    finally:
        ctx.set_math("exact")
    for hook, f in hooks.items():
        k = f.shape[1]
        print(name, hook, json.dumps(fs.t1_fractions(f, e[:, :k], f64[:, :k])))
    for hook, f in hooks.items():
        k = f.shape[1]
        _class_gate(f, e[:, :k], f64[:, :k], f"{name}/degenerate: {hook}")


@pytest.mark.parametrize("name", ALL)
def test_fast_k_init_is_the_debug_hook(ctx, monkeypatch, name):
    """As tests/test_gpu_fast_instances.py: the fast k_init's planes equal the exact run's (the RNG alone decides
    them) and its costs equal the initial cost re-formed in binary32 from acmmp_debug_ncc's per-view fast costs."""
    sc, p = rs.make_rig(name)
    V = len(sc.images) - 1
    _clean_env(monkeypatch)
    H, W = sc.images[0].shape
    got = {}
    try:
        for mode in ("exact", "fast"):
            ctx.set_math(mode)
            ctx.set_params(p)
            ctx.upload_views(sc.images, sc.cameras)
            ctx.run_patchmatch(17 + V, n_half_sweeps=0, do_post=False)
            got[mode] = ctx.download()
        fp, fc = got["fast"]
        assert_bitwise_equal(fp, got["exact"][0], "planes after k_init, fast vs exact")        # RNG only
        ys, xs = np.mgrid[0:H, 0:W]
        per_view = ctx.debug_ncc(xs.ravel().astype(np.int32), ys.ravel().astype(np.int32), fp.reshape(-1, 4))
    finally:
        ctx.set_math("exact")
    assert not np.isnan(per_view).any()
    want = fs.reform_initial_cost(per_view, p["top_k"]).reshape(H, W)
    assert np.mean(want < 2.0) > 0.3                         # the comparison is not one of 2.0 with 2.0
    assert_bitwise_equal(fc, want, "fast k_init cost vs the cost re-formed from debug_ncc")


INTERP_RIG = "turned-2000x1000-v2"


def test_turned_rig_interpolation(ctx, monkeypatch):
    """The fast SPHERE k_eval_nb's interpolated coordinates on a turned rig at the interpolation's smallest size:
    tests/test_gpu_interp.py's per-query test itself, run on this rig (its pole, seam and random sets, its assertions
    and its report, interp_queries_<rig>.json).  Then one full fast run: a source pole inside the image queues more
    per-sample fallbacks than any other rig under test, and the run must return ACMMP_OK -- an overflowed fallback
    queue is an error status (run_plan.h sizes plan.fix_cap for every entry a launch can queue)."""
    _clean_env(monkeypatch)
    made = {}

    def make():
        made.setdefault("sc", rs.turned(2000, 1000, V=2, seed=1234, n_waves=12, turns=rs.INTERP_TURNS))
        return made["sc"]

    monkeypatch.setitem(interp_tests.CONFIGS, INTERP_RIG, (make, 8))
    try:
        interp_tests.test_interpolated_k_eval_nb_per_query(ctx, INTERP_RIG)
        sc = make()
        p = fs.params_for(sc)
        ctx.set_math("fast")
        ctx.set_params(p)
        ctx.upload_views(sc.images, sc.cameras)
        ctx.run_patchmatch(4321)                              # raises capi.AcmmpError on any status but ACMMP_OK
        planes, costs = ctx.download()
        assert np.isfinite(planes).all()      # (a cost may be NaN as in the exact mode and the oracle: no view weighted)
        ok = np.abs(planes[..., 3] - sc.gt_depth) < 0.02 * sc.gt_depth
        print(INTERP_RIG, "fast run: depth within 2% of the surface on", float(ok.mean()), "of the pixels; valid cost on",
              float(np.mean(costs < 2.0)))
    finally:
        ctx.set_math("exact")
