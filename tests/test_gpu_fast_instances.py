"""Every fast-math NCC instance against float64, at small shapes.

The workload's own shapes (tests/test_gpu_fastmath.py, tests/test_gpu_interp.py) reach the fast mode only with
binary16 texels, V in {4, 6, 10, 15, 20, 32}, interior pixels and -- for the refinement hook -- SPHERE above 4
views.  The per-sample fast arithmetic runs at any size, so this matrix (tests/fastmath_support.py: pinhole 96x64
and SPHERE 128x64, V in {1, 2, 3, 5, 9}, 8-bit and float images) reaches the other instances of ncc_chunk:
TEX = 0 with FM = 1 (fetch_tap_pin_p<0>, lerp_tap<0>, for_all_views_tf<.., TF = 0> with kp.fast), view chunks
of 1 and 2 (pick_vb), a partial last chunk (V = 3: 2 + 1 through the has(v) guards of the fast pinhole chunks,
nb_vb's cap of 2; V = 5, 9), the fast pinhole k_eval_ref and the SPHERE k_eval_ref at V <= 4 (coop_patch_sep).
Four query sets per case -- interior, border, source edge, wild planes (fastmath_support.query_sets; their
contents are checked without a GPU in tests/test_fast_instance_inputs.py) -- and per case AND per set:

  a. exact mode: acmmp_debug_ncc, acmmp_debug_ncc_nb and acmmp_debug_ncc_ref equal the CPU oracle bit for bit;
  b. fast mode, hook against hook, bit for bit wherever ncc_chunk folds the same values in the same order:
       SPHERE   debug_ncc_nb == debug_ncc and debug_ncc_ref == debug_ncc at every V and both texel formats.
                Below 2000x1000 kp.interp is 0, so every instance takes the per-sample loop (`if (!interp_done)`);
                the staged layouts hold patch_sample's own values (coop_patch_nb stores them, coop_patch_sep
                stores (w, texel) and the ray tables' entries, from which the loop forms ray_at's two products),
                and the patch sums are folded in patch_sums' order.
       pinhole  with ACMMP_PIN_HOMOG=0, debug_ncc_nb == debug_ncc and debug_ncc_ref == debug_ncc: the same
                per-sample loop on coop_patch_nb's copies of patch_sample's values.
                The product path (ACMMP_PIN_HOMOG unset) is NOT bit-identical to debug_ncc: `if constexpr (kHomog)
                if (kp.homog)` forms a sample's source point as `pk_fma(nn, splat2(rcp(tz)), xy0[v])` from the
                per-view homogeneous vector affine in the patch offsets, where the per-sample loop runs
                project_fast(cam_point_fast(depth_from_plane_fast(..))) -- the same point up to rounding.  Its two
                hooks are therefore held to (c) directly; between themselves (k_eval_nb's and k_eval_ref's
                instances of that loop: other view chunks, the same per-view statements) they are bit-identical.
  c. fast mode against float64 (np_reference.bilateral_ncc, vectorised in fastmath_support.f64_ncc) under T1's
     gates (fastmath_support.t1_gates, the function tests/test_gpu_fastmath.py uses): debug_ncc, and for pinhole
     the product path's debug_ncc_nb and debug_ncc_ref;
  d. at least 300 (query, view) pairs valid in exact, fast and float64 for every gated hook;
  e. with ACMMP_TEST_REPORT_DIR set, fast_instances_<case>.json: per set every fraction the gates use and the
     worst |fast - float64| and |exact - float64| (recorded, not gated; profiles/fast_instances/).

k_init in the fast mode (V in {1, 2, 3, 5}): planes equal the exact run's bit for bit (the RNG alone decides
them), and the costs equal the initial cost re-formed in binary32 from acmmp_debug_ncc's per-view fast costs of
those planes, bit for bit: k_init's initial_cost and k_debug both evaluate the unstaged patch (make_patch,
STAGED 0) through the same ncc_chunk<MODEL, VB, 0, true, TEX, 1> statements -- only the view-chunk width differs
(kInitVB = 4 against pick_vb(V)), and a view's sums never mix with another's.
"""
import json
import os

import numpy as np
import pytest

import fastmath_support as fs
from acmmp import capi
from conftest import assert_bitwise_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("kind,V,tex", fs.CASES, ids=[fs.case_id(*c) for c in fs.CASES])
def test_fast_instances_per_query(ctx, oracle_mod, monkeypatch, kind, V, tex):
    sc, p = fs.make_case(kind, V, tex)
    sphere = kind == "sphere"
    for name in ("ACMMP_PIN_HOMOG", "ACMMP_TEX16", "ACMMP_INTERP"):
        monkeypatch.delenv(name, raising=False)
    ctx.set_math("exact")
    ctx.set_params(p)
    ctx.upload_views(sc.images, sc.cameras)
    assert ctx.texel_bytes() == (2 if tex == "f16" else 4)
    report = {}
    try:
        for name, (px, py, planes) in fs.query_sets(kind, V, tex).items():
            what = f"{fs.case_id(kind, V, tex)}/{name}"
            n = len(px)
            fx, fy, fpl = fs.flat_queries(px, py, planes)
            ref5 = np.ascontiguousarray(planes[:, :5])
            orc = fs.oracle_costs(oracle_mod, kind, V, tex, name)
            f64, _ = fs.f64_costs(kind, V, tex, name)
            # (a) the exact hooks are the oracle
            ctx.set_math("exact")
            e = ctx.debug_ncc(fx, fy, fpl).reshape(n, fs.PLANES, V)
            assert_bitwise_equal(e, orc, f"{what}: exact debug_ncc vs oracle")
            assert_bitwise_equal(ctx.debug_ncc_nb(px, py, planes), orc, f"{what}: exact debug_ncc_nb vs oracle")
            assert_bitwise_equal(ctx.debug_ncc_ref(px, py, ref5), orc[:, :5], f"{what}: exact debug_ncc_ref vs oracle")
            # (b) the fast hooks against each other
            ctx.set_math("fast")
            f = ctx.debug_ncc(fx, fy, fpl).reshape(n, fs.PLANES, V)
            f_nb = ctx.debug_ncc_nb(px, py, planes)
            f_ref = ctx.debug_ncc_ref(px, py, ref5)
            gated = {"debug_ncc": (f, e, f64)}
            if sphere:
                assert_bitwise_equal(f_nb, f, f"{what}: fast debug_ncc_nb vs debug_ncc")
                assert_bitwise_equal(f_ref, f[:, :5], f"{what}: fast debug_ncc_ref vs debug_ncc")
            else:
                monkeypatch.setenv("ACMMP_PIN_HOMOG", "0")
                ps_nb = ctx.debug_ncc_nb(px, py, planes)
                ps_ref = ctx.debug_ncc_ref(px, py, ref5)
                monkeypatch.delenv("ACMMP_PIN_HOMOG")
                assert_bitwise_equal(ps_nb, f, f"{what}: fast per-sample debug_ncc_nb vs debug_ncc")
                assert_bitwise_equal(ps_ref, f[:, :5], f"{what}: fast per-sample debug_ncc_ref vs debug_ncc")
                assert np.any(f_nb.view(np.uint32) != ps_nb.view(np.uint32)), what      # the homogeneous loop ran
                assert_bitwise_equal(f_ref, f_nb[:, :5], f"{what}: fast homogeneous debug_ncc_ref vs debug_ncc_nb")
                gated["debug_ncc_nb_homog"] = (f_nb, e, f64)
                gated["debug_ncc_ref_homog"] = (f_ref, e[:, :5], f64[:, :5])
            # (c), (d): T1 against float64, per hook not tied to debug_ncc by (b)
            report[name] = {"pixels": n}
            for hook, (ff, ee, rr) in gated.items():
                fr = fs.t1_fractions(ff, ee, rr)
                print(what, hook, json.dumps(fr))
                report[name][hook] = fr
            for hook, (ff, ee, rr) in gated.items():
                fr = fs.t1_gates(ff, ee, rr, sphere, what=f"{what}: {hook}")
                assert fr["valid"] >= fs.MIN_VALID, (what, hook, fr["valid"])
    finally:
        ctx.set_math("exact")
        out_dir = os.environ.get("ACMMP_TEST_REPORT_DIR")
        if out_dir:                                             # (a failing case records what it measured too)
            os.makedirs(out_dir, exist_ok=True)
            with open(os.path.join(out_dir, f"fast_instances_{fs.case_id(kind, V, tex)}.json"), "w") as fh:
                json.dump(report, fh, indent=1)


INIT_CASES = [c for c in fs.CASES if c[1] in (1, 2, 3, 5)]


@pytest.mark.parametrize("kind,V,tex", INIT_CASES, ids=[fs.case_id(*c) for c in INIT_CASES])
def test_fast_k_init_is_the_debug_hook(ctx, monkeypatch, kind, V, tex):
    sc, p = fs.make_case(kind, V, tex)
    for name in ("ACMMP_PIN_HOMOG", "ACMMP_TEX16", "ACMMP_INTERP"):
        monkeypatch.delenv(name, raising=False)
    H, W = sc.images[0].shape
    got = {}
    try:
        for mode in ("exact", "fast"):
            ctx.set_math(mode)
            ctx.set_params(p)
            ctx.upload_views(sc.images, sc.cameras)
            ctx.run_patchmatch(17 + V, n_half_sweeps=0, do_post=False)
            got[mode] = ctx.download()
        assert ctx.texel_bytes() == (2 if tex == "f16" else 4)
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
