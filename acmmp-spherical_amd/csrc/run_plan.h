// run_plan.h -- which variant of the PatchMatch engine a run takes: one pure host function of the run's shape and the
// environment knobs ("the run plan").  No HIP type: build_kparams copies the plan into KParams, the
// host launchers and the test hooks pick their kernel instances from it, and tests/run_plan_walk.cpp compiles it with
// the host compiler alone.  Each gate is written once, in dependency order; KParams (engine.h) says what the kernels
// do with a field, this header says when it is set.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>

#include "acmmp.h"

namespace acmmp {

constexpr int kPinhole = 0;
constexpr int kSphere = 11;
constexpr int kMaxViews = 32;       // cost_vector[32], uint32 view bitmask (ACMMP.cu:522,1153)
constexpr int kNbPix = 32;          // k_eval_nb: pixels per 256-lane block (8 lanes each)
constexpr int kNbFixRegions = 256;  // the queue's regions, one counter each (block % regions)
constexpr int kRefLanes = 5;        // k_eval_ref: refinement candidates (ACMMP.cu:870)
constexpr int kRefPix = 51;         // k_eval_ref: pixels per 256-lane block (255 lanes used)
constexpr int kRefSlots = kRefPix * kRefLanes;  // survivor slots per k_eval_ref block
constexpr unsigned kStatusFixOverflow = 1u;   // KParams::status: k_nb_fix found a region's queue overfull

// Strip schedule of a run's half-sweeps: the checkerboard rows [0, rows) cut into contiguous
// strips, each running its own k_pick .. k_finish chain on one of a few streams.
constexpr int kMaxStrips = 64;
constexpr int kMaxStripStreams = 4;  // the context's stream included: the runtime's default hardware queues

// Grid size of a launch: ceil(a / b).
inline int cdiv(long long a, int b) { return static_cast<int>((a + b - 1) / b); }

// View-chunk width: the per-view accumulators live in registers (6 per view).
inline int pick_vb(int V) { return V <= 1 ? 1 : (V <= 2 ? 2 : (V <= 4 ? 4 : 8)); }
// Texel and arithmetic form of the per-sample NCC instances: 0 fp32 texels, 1 binary16 exact, 2 binary16 fast.
inline int tf_of(bool tex16, bool fast) { return tex16 ? (fast ? 2 : 1) : 0; }

// The psum piece of the scratch slab (build_kparams), in float4 entries: one colour's sums, or with the kept-sample
// mask both colours' and behind them the 2 Pc mask words (two words per entry).
inline size_t psum_count(size_t Pc, bool keep) { return keep ? 3 * Pc : Pc; }

// k_eval_nb's block count over colour-grid rows [0, rows) of width Wh: 32-pixel row runs, or 8 x 4 tiles
inline long long nb_block_count(long long rows, long long Wh, int tile) {
    return tile ? ((rows + 3) / 4) * ((Wh + 7) / 8) : (rows * Wh + 31) / 32;
}

// Strip boundaries: `want` strips clamped so that every boundary but the last is a multiple of 4 rows
// (k_eval_nb's 8 x 4 tiles keep their shape) and every strip is at least ACMMP_BAND_HALO rows tall (24, the
// next multiple of 4), so a half-sweep reads no strip beyond its two neighbours.  The 4-row units are dealt
// evenly, the first strips one more; the last strip takes the rows past the last whole unit.  Returns the
// strip count NS >= 1 and writes bounds[0 .. NS].
inline int strip_plan(int rows, int want, int* bounds) {
    const int units = rows / 4, per = (ACMMP_BAND_HALO + 3) / 4;
    int ns = want < 1 ? 1 : (want > kMaxStrips ? kMaxStrips : want);
    if (ns > units / per) ns = units / per;
    if (ns < 1) ns = 1;
    int at = 0;
    for (int i = 0; i < ns; ++i) {
        bounds[i] = 4 * at;
        at += units / ns + (i < units % ns ? 1 : 0);
    }
    bounds[0] = 0;
    bounds[ns] = rows;
    return ns;
}

// Strips whose half-sweep n must be complete before strip i's half-sweep n + 1 starts: i - 1, i and i + 1
// where they exist (-1 otherwise); none with a single strip, whose one stream orders its launches.
inline void strip_waits(int ns, int i, int waits[3]) {
    waits[0] = (ns > 1 && i > 0) ? i - 1 : -1;
    waits[1] = ns > 1 ? i : -1;
    waits[2] = (ns > 1 && i + 1 < ns) ? i + 1 : -1;
}

// ------------------------------------------------------------------ knobs
//
// Every run-time knob of the engine with its default (DESIGN.md §4 has the table: what each switches and the test
// that flips it).  read_knobs() is called once per run, per acmmp_band_begin and per test-hook call, so a test can
// flip a knob inside one process.
constexpr int kKnobAuto = INT_MIN;
struct RunKnobs {
    bool interp = true;             // ACMMP_INTERP=0 projects every sample in the fast mode too (the per-sample fast
                                    // arithmetic the interpolation is gated against, tests/test_gpu_fastmath.py T2)
    bool pin_homog = true;          // ACMMP_PIN_HOMOG=0: fast pinhole projects each sample through depth and point
                                    // instead of the per-view homogeneous affine form (ncc_chunk; A/B, tests)
    float spread_max = 256.0f;      // ACMMP_SPREAD_MAX: the interpolation's corner-spread fallback threshold (ncc_chunk;
                                    // tests force fallbacks with a small one, A/B without any with a huge one)
    float neg_tau = 0x1p-35f;       // ACMMP_NEG_TAU: the interpolated loop's negligible-sample threshold (stage_neg_mask,
                                    // DESIGN.md §2.4): 36 dropped terms of at most tau x the patch sum each move a source
                                    // sum by 36 tau = 2^-29.8 of its scale, 1 / 57 of one binary32 rounding (2^-24) of it
    bool neg_skip = true;           // ACMMP_NEG_SKIP=0 keeps every sample in k_eval_nb
    float ref_neg_tau = 0x1p-35f;   // ACMMP_REF_NEG_TAU: the per-sample refinement loops' threshold (tests)
    bool ref_neg_skip = true;       // ACMMP_REF_NEG_SKIP=0 launches the instances without the per-pixel mask
    bool keep_mask = true;          // ACMMP_KEEP_MASK=0 launches the instances that recompute the test, with the same
                                    // bits (A/B, tests/test_gpu_keep_mask.py)
    size_t nbfix_max_pc = static_cast<size_t>(1) << 24;   // ACMMP_NBFIX_MAX_PC lowers the colour-grid size from which a
                                    // run has no fallback queue (a test forces that branch at a small size)
    bool dead_skip = true;          // ACMMP_DEAD_SKIP=0 keeps no SPHERE dead mask: every pixel takes the long paths, with
                                    // the same result (A/B, tests/test_gpu_dead_skip.py)
    bool ref_split = true;          // ACMMP_REF_SPLIT=0: the refinement in one part (A/B switch)
    int ref_split_at = 0;           // ACMMP_REF_SPLIT_AT=S: fixed split point (A/B); 0: the rule's
    int nb_view_chunk = kKnobAuto;  // ACMMP_NB_VIEW_CHUNK=c: views per k_eval_nb launch (c <= 0: one launch over all)
    bool nb_tile = true;            // ACMMP_NB_TILE=0: k_eval_nb blocks as 32-pixel row runs, not 8 x 4 tiles
    int strips = 0;                 // ACMMP_STRIPS: strips of a run; 0: default_strips (they change no result,
                                    // tests/test_gpu_strips.py)
    int strip_streams = kMaxStripStreams;   // ACMMP_STRIP_STREAMS: streams the strips are dealt to
    bool time_all = false;          // ACMMP_KERNEL_TIMING=all: events around all four kernel buckets of a half-sweep, not
                                    // k_eval_nb's alone -- an event record between two kernels leaves the GPU idle ~6 us,
                                    // 3 x 6 per half-sweep (0.45% of the metric's RunPatchMatch,
                                    // profiles/r06_ab9_events_ab.txt)
};

// get(name): the knob's text or null (std::getenv, or a test's table).
template <typename Get>
RunKnobs read_knobs(Get get) {
    RunKnobs k;
    auto flag = [&](const char* name, bool& v) { if (const char* e = get(name)) v = std::atoi(e) != 0; };
    auto real = [&](const char* name, float& v) { if (const char* e = get(name)) v = std::strtof(e, nullptr); };
    auto whole = [&](const char* name, int& v) { if (const char* e = get(name)) v = std::atoi(e); };
    flag("ACMMP_INTERP", k.interp);
    flag("ACMMP_PIN_HOMOG", k.pin_homog);
    real("ACMMP_SPREAD_MAX", k.spread_max);
    real("ACMMP_NEG_TAU", k.neg_tau);
    flag("ACMMP_NEG_SKIP", k.neg_skip);
    real("ACMMP_REF_NEG_TAU", k.ref_neg_tau);
    flag("ACMMP_REF_NEG_SKIP", k.ref_neg_skip);
    flag("ACMMP_KEEP_MASK", k.keep_mask);
    if (const char* e = get("ACMMP_NBFIX_MAX_PC")) k.nbfix_max_pc = std::min<size_t>(k.nbfix_max_pc, std::strtoull(e, nullptr, 10));
    flag("ACMMP_DEAD_SKIP", k.dead_skip);
    flag("ACMMP_REF_SPLIT", k.ref_split);
    whole("ACMMP_REF_SPLIT_AT", k.ref_split_at);
    whole("ACMMP_NB_VIEW_CHUNK", k.nb_view_chunk);
    flag("ACMMP_NB_TILE", k.nb_tile);
    if (const char* e = get("ACMMP_STRIPS")) { if (std::atoi(e) > 0) k.strips = std::atoi(e); }
    if (const char* e = get("ACMMP_STRIP_STREAMS")) { if (std::atoi(e) > 0) k.strip_streams = std::atoi(e); }
    if (const char* e = get("ACMMP_KERNEL_TIMING")) k.time_all = std::strcmp(e, "all") == 0;
    return k;
}
// The process environment as it is now: the engine's only getenv calls for a run.
inline RunKnobs read_knobs() { return read_knobs([](const char* name) { return std::getenv(name); }); }

// ------------------------------------------------------------------ shape and plan

struct RunShape {
    int model = kSphere;            // kPinhole / kSphere, uniform over all views
    int W = 0, H = 0, V = 0;        // reference size, source views
    int patch_size = 11, radius_increment = 2;
    bool fast = false;              // acmmp_set_math(ACMMP_MATH_FAST)
    bool tex16 = false;             // every view has an exact binary16 copy
    bool geom = false;              // geom_consistency
    int want_strips = 0;            // > 0: the caller's strip count (band runs and hooks: 1); 0: knob or default
};

// The per-pixel mask form of a per-sample kernel's instance (the values of kernels.hip's NegMode).
enum MaskInst { kInstNone = 0, kInstTest = 1, kInstWord = 2, kInstPublish = 3 };

enum PlanStatus { kPlanOk = 0, kPlanRadius = 1, kPlanSamples = 2 };
inline const char* plan_error(int status) {
    return status == kPlanRadius ? "patch radius > 64"
         : status == kPlanSamples ? "more than 64 patch samples (patch_size / radius_increment)" : "";
}

struct RunPlan {
    int status = kPlanOk;           // not kPlanOk: an unsupported shape, nothing else is set
    int R = 0, nside = 0, S = 0;    // patch radius, offsets per axis, samples
    int Wh = 0, rows = 0;           // colour row width ceil(W / 2), rows the reference's checkerboard grid covers
    size_t Pc = 0;                  // H * Wh
    // KParams fields of the same names
    int interp = 0;                 // as every kernel but the refinement's sees it
    int ref_interp = 0;             // as k_eval_ref, its fallbacks and its tail see it
    int homog = 1;
    float spread_max = 256.0f;
    float neg_tau = -1.0f, ref_neg_tau = -1.0f;
    int keep = 0;
    int ref_split = 0, nb_chunk = 0, nb_tile = 1;
    bool dead_skip = false;         // the run keeps the SPHERE dead mask (KParams::dead)
    bool fix_queue = false;         // k_eval_nb defers interpolation fallbacks to KParams::nbfix (else null)
    bool ref_fix = false;           // the refinement's interpolated instance queues there too
    // strips: rows [bounds[i], bounds[i + 1]), their k_eval_ref blocks and fallback-queue entries per region
    int ns = 1;
    int bounds[kMaxStrips + 1] = {};
    size_t ref_blocks[kMaxStrips] = {}, fix_cap[kMaxStrips] = {};
    // pieces of the scratch slab whose size follows from the above (elements)
    size_t surv_n = 0, surv_count_n = 0, surv_pre_n = 0, psum_n = 0, nbfix_n = 0, nbfix_count_n = 0;
    // instances
    MaskInst init_inst = kInstNone; // k_init: none / test / publish
    MaskInst ref_inst = kInstNone;  // k_eval_ref, its tail, the refinement hook: none / test / word
    bool nb_tex = false, nb_fm = false, nb_masked = false;   // k_eval_nb and its hook: TEX, FM, stage_neg_mask
    int sel_mv = 1;                 // k_select's MV
    bool sel_masked = false;        // its masked per-sample loop
};

// Split point of the refinement evaluation: half the views up to 4 views, one 4-view NCC
// chunk above (r03 sweep, profiles/r03_ref_split_sweep.txt / r03_ref_split_v20.txt: at V = 10, 15 and 20
// S = 4 beats 6 / 8 / 12 by 1-4%); 0 (no split) for one view, for colour grids too large for the 32-bit
// queue entries, or with ACMMP_REF_SPLIT=0.
// interp_ref: the refinement's first part interpolates SPHERE sample coordinates (fast mode, V > 4, views
// of the interpolation's size), which makes its views cheaper than the tail's per-sample ones: S = 8 there
// from V = 9 up (C3 V = 15: 88.9 -> 90.4 Mpix-it/s against S = 4; S = 10 / 12 lose, and the exact mode
// loses 5% at S = 8, profiles/r04_split_ab.txt, r04_split2_ab.txt)
inline int ref_split_point(int V, size_t Pc, bool interp_ref, const RunKnobs& k) {
    if (!k.ref_split || V < 2 || Pc >= (static_cast<size_t>(1) << 29)) return 0;
    if (k.ref_split_at > 0) return k.ref_split_at < V ? k.ref_split_at : 0;
    if (interp_ref && V > 8) return 8;
    return V <= 4 ? V / 2 : 4;
}

// Strips of a run when ACMMP_STRIPS does not say (profiles/strips_ab.txt).
// Two strips for SPHERE views of 2 Mpixel and up (metric -4.5%, 2000x1000 -2.7% per step; four and more lose
// again); smaller views, where a strip's launches no longer fill the chip, pinhole and more than 4 source views
// (not measured; the fast mode's interpolating runs with V > 4 ignore the knob too, plan_run) stay at one.
inline int default_strips(int model, int W, int H, int V) {
    return (model == kSphere && V <= 4 && static_cast<long long>(W) * H >= 2000000LL) ? 2 : 1;
}

// The geometric part of the interpolation gate.  Interpolated SPHERE sample coordinates in the fast k_eval_nb
// (DESIGN.md §2.4): 6x6 patches whose radius spans at most 5 pixels of 2 pi / 2000 rad (patch_size 11,
// radius_increment 2 from 2000x1000 up) -- a wider patch angle makes the interpolation's NCC error exceed 1e-4 in
// the tail near source poles, where the 256-pixel corner-spread fallback no longer catches it (1600x800: 3.7e-3 at a
// spread of 65 px; scripts/interp_feasibility.py, tests/test_interp_design.py).  patch_size 21 / increment 4
// also gives 6x6 samples but spans twice the angle: it projects every sample below 4000x2000.
inline bool interp_geometry(int model, int nside, int R, int W, int H) {
    return model == kSphere && nside == 6 && 2000LL * R <= 5LL * W && 1000LL * R <= 5LL * H;
}

// The per-sample refinement loops' negligible-sample threshold (ncc_chunk's PNEG instances):
// fast SPHERE with binary16 texels, V <= 4, in k_init, k_eval_ref, k_eval_ref_tail and k_select's cache misses
// (without the binary16 images these run the TF = 0 instances, which have no masked form), so the cost cache holds
// one arithmetic from the first vector on.  A sample whose weight is at most tau x its own pixel's patch sum
// adds nothing to the source sums: a function of the pixel alone, so whichever kernel and wave evaluates a
// (pixel, plane, view) forms the same bits.  Gated by the geometry only, not by ACMMP_INTERP, and by none of
// ACMMP_SPREAD_MAX / ACMMP_NBFIX_MAX_PC / ACMMP_NEG_*: the runs the tests compare across those knobs share
// one refinement.
inline float ref_neg_tau_of(bool interp_geom, bool fast, bool tex16, int V, const RunKnobs& k) {
    return (interp_geom && fast && tex16 && V <= 4 && k.ref_neg_skip) ? k.ref_neg_tau : -1.0f;
}

// The kept-sample mask (KParams::keep): the drop test above is the same in every half-sweep of a run, so a masked
// run's k_init publishes it once per pixel, with the patch sums, and k_eval_ref and its tail read it instead of
// forming every weight again to test it; without the mask there is nothing to publish.  Not in a geom run:
// k_eval_ref's geom form would go from 80 to 81 VGPRs and from 6 waves to 5 with the word, and it and the tail must
// agree on who fills psum.
inline bool keep_mask_of(float ref_neg_tau, bool geom, const RunKnobs& k) {
    return ref_neg_tau >= 0.0f && !geom && k.keep_mask;
}

// View-chunked k_eval_nb: one launch per chunk of 8 source views when the sources' texels outgrow the
// 256 MB Infinity Cache, so all waves in flight sample the same few images (r02 A/B
// profiles/r02_view_chunk_ab.txt: SPHERE V = 15 at 3200x1600 +3.7%, at 4096x2048 +6.4%; pinhole V = 10
// at 1600x1200, 77 MB of texels, -1% -- not chunked; round 4 with the deferred fallbacks, C3: 8 views 90.2,
// 5 89.6, one launch 89.4 Mpix-it/s, profiles/r04_chunk_ab.txt).  ACMMP_NB_VIEW_CHUNK=c overrides (c <= 0: one
// launch over all views).
inline int nb_view_chunk(int W, int H, int V, const RunKnobs& k) {
    int c = k.nb_view_chunk;
    if (c == kKnobAuto) {
        // texel bytes of the sources at the reference's size (row-pair binary16 or fp32: 4 B per texel)
        const double bytes = 4.0 * (W + 2) * (H + 2) * V;
        c = (V > 8 && bytes > 160e6) ? 8 : 0;
    }
    return (c <= 0 || c >= V) ? V : c;
}

// k_eval_nb's block shape (KParams::nb_tile): 8 x 4 tiles of the colour grid (a block's 32 pixels then span
// 4 rows, so their patches and source footprints overlap in the CU's L1): k_eval_nb -3% at C2 (3.17 -> 3.07 ms),
// -2.5% at C3, neutral at the metric against 32-pixel row runs (profiles/r05_ab7_ab.txt).  ACMMP_NB_TILE=0: row runs.
inline int nb_tile_order(const RunKnobs& k) { return k.nb_tile ? 1 : 0; }

inline RunPlan plan_run(const RunShape& sh, const RunKnobs& k) {
    RunPlan p;
    const int V = sh.V;
    p.R = sh.patch_size / 2;
    if (p.R > 64) { p.status = kPlanRadius; return p; }
    for (int i = -p.R; i <= p.R; i += sh.radius_increment) ++p.nside;
    p.S = p.nside * p.nside;
    if (p.S > 64) { p.status = kPlanSamples; return p; }
    p.Wh = (sh.W + 1) / 2;
    p.rows = std::min(sh.H, 32 * (((sh.H / 2) + 15) / 16));
    p.Pc = static_cast<size_t>(sh.H) * p.Wh;

    const bool geometry = interp_geometry(sh.model, p.nside, p.R, sh.W, sh.H);
    p.ref_neg_tau = ref_neg_tau_of(geometry, sh.fast, sh.tex16, V, k);
    p.keep = keep_mask_of(p.ref_neg_tau, sh.geom, k) ? 1 : 0;
    p.homog = k.pin_homog ? 1 : 0;
    p.spread_max = k.spread_max;
    p.nb_chunk = nb_view_chunk(sh.W, sh.H, V, k);
    p.nb_tile = nb_tile_order(k);

    // Queue of k_eval_nb's deferred interpolation fallbacks (pixel << 8 | hypothesis << 5 | view), where the fast mode
    // interpolates SPHERE sample coordinates on binary16 texels -- the one place that condition is written.  The key
    // holds the colour-grid pixel in 24 bits: a larger grid (views of 8192x4096 and up) has no queue, and then
    // k_eval_nb does not interpolate (ncc_chunk interpolates only with somewhere to put its fallbacks).
    const bool fast16_interp = geometry && k.interp && sh.fast && sh.tex16;
    p.fix_queue = fast16_interp && p.Pc < k.nbfix_max_pc;
    p.interp = (geometry && k.interp && (p.fix_queue || !fast16_interp)) ? 1 : 0;
    // k_eval_nb's negligible-sample mask: only where it interpolates (the exact mode never reads it), and the mask is
    // per wave: only the 8 x 4 tile order keeps a wave's 8 pixels the same under every strip and band cut -- with row
    // runs, ACMMP_NB_TILE=0, a cut regroups them -- so no mask there
    p.neg_tau = (k.neg_skip && p.interp && p.nb_tile) ? k.neg_tau : -1.0f;

    // The refinement's interpolated instance (fast SPHERE, V > 4) leaves its rough views to k_eval_ref_tail: none
    // without a split, and then k_eval_ref sees no interpolation at all.
    p.ref_split = ref_split_point(V, p.Pc, p.fix_queue && V > 4, k);
    p.ref_interp = (p.interp && p.ref_split > 0) ? 1 : 0;
    p.ref_fix = p.fix_queue && V > 4 && p.ref_split > 0;
    p.dead_skip = sh.model == kSphere && k.dead_skip;

    // One strip where the fast mode's refinement has two arithmetic forms for the same cost: pinhole (k_eval_ref's
    // homogeneous sample points against the per-sample projection of k_eval_ref_tail and k_select's cache misses)
    // and SPHERE with interpolated coordinates and V > 4 (k_eval_ref's interpolated instance against the same two).
    // Which of a candidate's views the tail evaluates, and so which form a cached cost has, depends on the views
    // the other lanes of its wave selected; a strip start regroups the waves, and the low bits of some costs follow
    // (two strips run one after the other on one stream already differ from one).  A knob changes no
    // result, so these runs ignore ACMMP_STRIPS.  Everywhere else every form of a cost has the same bits.
    int want = sh.want_strips > 0 ? sh.want_strips : (k.strips > 0 ? k.strips : default_strips(sh.model, sh.W, sh.H, V));
    if (sh.fast && (sh.model != kSphere || (p.interp && V > 4))) want = 1;
    p.ns = strip_plan(p.rows, want, p.bounds);
    // Per strip, by its own share of blocks (its launches number their blocks from 0).  The queue has, per region
    // (blocks b with b % kNbFixRegions equal), room for every entry its blocks can queue, so none is ever dropped
    // (metric 193 MB, C3 656 MB): kNbPix x 8 hypotheses x the launch's views each for k_eval_nb; for the refinement,
    // which queues its survivors' fallback views of [0, ref_split) into the same regions after k_eval_nb's queue is
    // drained, a region's k_eval_ref blocks x kRefSlots survivors x ref_split views.  The room is the larger of the
    // two producers' worst cases (the split can exceed the view chunk: ACMMP_REF_SPLIT_AT / ACMMP_NB_VIEW_CHUNK).
    size_t ref_total = 0, fix_total = 0;
    for (int i = 0; i < p.ns; ++i) {
        const size_t srows = static_cast<size_t>(p.bounds[i + 1] - p.bounds[i]);
        const size_t nb_blocks = static_cast<size_t>(nb_block_count(static_cast<long long>(srows), p.Wh, p.nb_tile));
        p.ref_blocks[i] = (srows * p.Wh + kRefPix - 1) / kRefPix;
        p.fix_cap[i] = !p.fix_queue ? 0 : std::max(
            (nb_blocks + kNbFixRegions - 1) / kNbFixRegions * kNbPix * 8 * static_cast<size_t>(p.nb_chunk),
            (p.ref_blocks[i] + kNbFixRegions - 1) / kNbFixRegions * kRefSlots * static_cast<size_t>(std::max(p.ref_split, 0)));
        ref_total += p.ref_blocks[i];
        fix_total += p.fix_cap[i];
    }
    p.surv_n = std::max(5 * p.Pc + 256, ref_total * kRefSlots);
    p.surv_count_n = std::max(p.Pc / 51 + 2, ref_total);
    p.surv_pre_n = std::max(p.Pc / 51 + 3, ref_total + p.ns);     // ref_blocks + 1 entries per strip
    p.psum_n = psum_count(p.Pc, p.keep != 0);
    p.nbfix_n = kNbFixRegions * fix_total;                        // (empty without a fallback queue)
    p.nbfix_count_n = static_cast<size_t>(kNbFixRegions) * p.ns;

    // Instances.  The ones with the per-pixel negligible-sample mask (ncc_chunk's PNEG; k_init and the refinement's
    // kernels) exist for fast SPHERE with binary16 texels up to 4 views (kernels.hip's ref_neg_inst) and are launched
    // where the run has the mask; every other launch, and ACMMP_REF_NEG_SKIP=0, takes the instance that has no code
    // for it.  A geom run publishes no word (keep_mask_of).
    const bool masked = p.ref_neg_tau >= 0.0f;
    p.init_inst = !masked ? kInstNone : (p.keep ? kInstPublish : kInstTest);
    p.ref_inst = !masked ? kInstNone : (p.keep ? kInstWord : kInstTest);
    // k_eval_nb: the instance with the negligible-sample mask (stage_neg_mask) where the run skips such samples;
    // without (ACMMP_NEG_SKIP=0, nothing interpolated) the instance that has no code for it
    p.nb_tex = sh.tex16;
    p.nb_fm = sh.fast;
    p.nb_masked = sh.fast && sh.tex16 && p.neg_tau >= 0.0f;
    // the per-view arrays of k_select are sized to the next power of two of V: a 32-entry bound for every V
    // above 4 kept C3's (V = 15) probabilities in 384 B of scratch per lane
    p.sel_mv = V <= 4 ? pick_vb(V) : (V <= 8 ? 8 : (V <= 16 ? 16 : 32));
    p.sel_masked = sh.model == kSphere && masked && p.sel_mv <= 4;
    return p;
}

}  // namespace acmmp
