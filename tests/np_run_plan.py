"""An independent restatement of the run-time gates of a PatchMatch run: which variant of the engine a view's shape and
the environment knobs select.  Written from build_kparams and the host launchers as they stood before csrc/run_plan.h
existed (one gate per paragraph there) and from DESIGN.md §2.4 / §4; tests/test_run_plan.py holds plan_run to it.

plan(shape, env) returns a dict of plain ints and floats (binary32 values as Python floats).  `shape`: model (11 =
SPHERE, 0 = pinhole), W, H, V, patch_size, radius_increment, fast, tex16, geom, want_strips (0: the default and
ACMMP_STRIPS decide).  `env`: the ACMMP_* knobs that are set, name -> string.
"""
import numpy as np

SPHERE, PINHOLE = 11, 0
HALO = 23                       # ACMMP_BAND_HALO
NB_PIX, REF_PIX, REF_SLOTS, REGIONS, MAX_STRIPS = 32, 51, 255, 256, 64
TAU = 2.0 ** -35
NEG = {"none": 0, "test": 1, "word": 2, "publish": 3}


def f32(s):
    return float(np.float32(float(s)))


def strip_bounds(rows, want):
    """4-row units dealt evenly, strips of at least 24 rows, at most 64 of them."""
    units, per = rows // 4, (HALO + 3) // 4
    ns = max(1, min(want, MAX_STRIPS))
    ns = max(1, min(ns, units // per))
    bounds, at = [], 0
    for i in range(ns):
        bounds.append(4 * at)
        at += units // ns + (1 if i < units % ns else 0)
    bounds[0] = 0
    return bounds + [rows]


def plan(shape, env):
    model, W, H, V = shape["model"], shape["W"], shape["H"], shape["V"]
    fast, tex16, geom = bool(shape["fast"]), bool(shape["tex16"]), bool(shape["geom"])
    sphere = model == SPHERE
    on = lambda name, default=True: (int(env[name]) != 0) if name in env else default

    R = shape["patch_size"] // 2
    if R > 64:
        return {"status": 1, "error": "patch radius > 64"}
    nside = len(range(-R, R + 1, shape["radius_increment"]))
    S = nside * nside
    if S > 64:
        return {"status": 2, "error": "more than 64 patch samples (patch_size / radius_increment)"}
    Wh = (W + 1) // 2
    Pc = H * Wh
    rows = min(H, 32 * ((H // 2 + 15) // 16))
    p = {"status": 0, "R": R, "nside": nside, "S": S, "Wh": Wh, "Pc": Pc, "rows": rows}

    # §2.4: 6 x 6 samples whose radius spans at most 5 pixels of 2 pi / 2000 rad, SPHERE only
    geometry = sphere and nside == 6 and 2000 * R <= 5 * W and 1000 * R <= 5 * H
    # the refinement's per-pixel mask: the geometry alone (not ACMMP_INTERP), fast, binary16, V <= 4
    ref_tau = -1.0
    if geometry and fast and tex16 and V <= 4:
        ref_tau = f32(env.get("ACMMP_REF_NEG_TAU", TAU))
        if not on("ACMMP_REF_NEG_SKIP"):
            ref_tau = -1.0
    keep = ref_tau >= 0.0 and not geom and on("ACMMP_KEEP_MASK")
    interp = geometry and on("ACMMP_INTERP")
    # the fallback queue keys a colour-grid pixel in 24 bits; without it the fast binary16 run does not interpolate
    max_pc = min(1 << 24, int(env["ACMMP_NBFIX_MAX_PC"])) if "ACMMP_NBFIX_MAX_PC" in env else 1 << 24
    fast16 = sphere and fast and tex16
    queue = fast16 and interp and Pc < max_pc
    if fast16 and interp and not queue:
        interp = False
    tile = on("ACMMP_NB_TILE")
    neg_tau = f32(env.get("ACMMP_NEG_TAU", TAU))
    if not on("ACMMP_NEG_SKIP") or not interp or not tile:
        neg_tau = -1.0

    # view chunks of k_eval_nb: 8 views once the sources' texels outgrow the cache
    if "ACMMP_NB_VIEW_CHUNK" in env:
        chunk = int(env["ACMMP_NB_VIEW_CHUNK"])
    else:
        chunk = 8 if (V > 8 and 4.0 * (W + 2) * (H + 2) * V > 160e6) else 0
    if chunk <= 0 or chunk >= V:
        chunk = V

    # split point of the refinement
    ref_interp_views = fast16 and interp and V > 4
    at = int(env.get("ACMMP_REF_SPLIT_AT", 0))
    if not on("ACMMP_REF_SPLIT") or V < 2 or Pc >= 1 << 29:
        split = 0
    elif at > 0:
        split = at if at < V else 0
    elif ref_interp_views and V > 8:
        split = 8
    else:
        split = V // 2 if V <= 4 else 4

    # strips
    want = shape.get("want_strips", 0)
    if want <= 0:
        want = 2 if (sphere and V <= 4 and W * H >= 2000000) else 1
        if int(env.get("ACMMP_STRIPS", 0)) > 0:
            want = int(env["ACMMP_STRIPS"])
    if fast and (not sphere or (interp and V > 4)):
        want = 1
    bounds = strip_bounds(rows, want)
    ns = len(bounds) - 1
    ref_blocks, fix_cap = [], []
    for i in range(ns):
        srows = bounds[i + 1] - bounds[i]
        nb_blocks = ((srows + 3) // 4) * ((Wh + 7) // 8) if tile else (srows * Wh + 31) // 32
        rb = (srows * Wh + REF_PIX - 1) // REF_PIX
        ref_blocks.append(rb)
        fix_cap.append(0 if not queue else max(-(-nb_blocks // REGIONS) * NB_PIX * 8 * chunk,
                                               -(-rb // REGIONS) * REF_SLOTS * max(split, 0)))
    ref_total, fix_total = sum(ref_blocks), sum(fix_cap)

    p.update(interp=int(interp), ref_interp=int(interp and split > 0), homog=int(on("ACMMP_PIN_HOMOG")),
             spread_max=f32(env.get("ACMMP_SPREAD_MAX", 256.0)), neg_tau=neg_tau, ref_neg_tau=ref_tau, keep=int(keep),
             fix_queue=int(queue), ref_fix=int(queue and V > 4 and split > 0), ref_split=split, nb_chunk=chunk,
             nb_tile=int(tile), dead_skip=int(sphere and on("ACMMP_DEAD_SKIP")), ns=ns, bounds=bounds,
             ref_blocks=ref_blocks, fix_cap=fix_cap,
             # slab pieces whose size follows the plan
             surv_n=max(5 * Pc + 256, ref_total * REF_SLOTS), surv_count_n=max(Pc // 51 + 2, ref_total),
             surv_pre_n=max(Pc // 51 + 3, ref_total + ns), psum_n=3 * Pc if keep else Pc,
             nbfix_n=REGIONS * fix_total, nbfix_count_n=REGIONS * ns)
    p["keep_mask_bytes"] = 16 * (p["psum_n"] - Pc)

    # instances.  The masked per-sample loops exist for fast SPHERE, binary16, V <= 4 -- where ref_tau can be >= 0
    masked = ref_tau >= 0.0
    p["init_inst"] = NEG["none"] if not masked else (NEG["publish"] if keep else NEG["test"])
    p["ref_inst"] = NEG["none"] if not masked else (NEG["word"] if keep and not geom else NEG["test"])
    p["nb_tex"], p["nb_fm"] = int(tex16), int(fast)
    p["nb_masked"] = int(fast and tex16 and neg_tau >= 0.0)
    p["sel_mv"] = (1 if V <= 1 else 2 if V <= 2 else 4) if V <= 4 else (8 if V <= 8 else 16 if V <= 16 else 32)
    p["sel_masked"] = int(sphere and masked and p["sel_mv"] <= 4)
    # the knobs that are no gate
    p["strip_streams"] = int(env["ACMMP_STRIP_STREAMS"]) if int(env.get("ACMMP_STRIP_STREAMS", 0)) > 0 else 4
    p["time_all"] = int(env.get("ACMMP_KERNEL_TIMING") == "all")
    return p


def check_properties(p, shape):
    """What must hold of any plan, whatever the equalities say."""
    if p["status"]:
        return
    V, Wh = shape["V"], p["Wh"]
    assert not p["keep"] or (p["ref_neg_tau"] >= 0.0 and not shape["geom"])
    assert not p["neg_tau"] >= 0.0 or (p["interp"] and p["nb_tile"])
    assert not p["ref_fix"] or p["fix_queue"]
    assert not p["ref_interp"] or p["interp"]
    assert p["bounds"][0] == 0 and p["bounds"][-1] == p["rows"] and len(p["bounds"]) == p["ns"] + 1
    for i in range(p["ns"]):
        srows = p["bounds"][i + 1] - p["bounds"][i]
        assert srows > 0
        if p["fix_queue"]:
            nb_blocks = ((srows + 3) // 4) * ((Wh + 7) // 8) if p["nb_tile"] else (srows * Wh + 31) // 32
            assert p["fix_cap"][i] >= -(-nb_blocks // REGIONS) * NB_PIX * 8 * p["nb_chunk"]
            assert p["fix_cap"][i] >= -(-p["ref_blocks"][i] // REGIONS) * REF_SLOTS * p["ref_split"]
        else:
            assert p["fix_cap"][i] == 0
    if shape["fast"] and (shape["model"] != SPHERE or (p["interp"] and V > 4)):
        assert p["ns"] == 1
    assert p["init_inst"] in (0, 1, 3) and p["ref_inst"] in (0, 1, 2)
    assert (p["init_inst"] == NEG["publish"]) == bool(p["keep"]) == (p["ref_inst"] == NEG["word"])
