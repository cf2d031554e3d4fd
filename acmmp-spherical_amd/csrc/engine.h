// engine.h -- internal device-side layout of the PatchMatch engine (not part of the ABI).
//
// HBM layout:
//  * source/reference images: one allocation, each view padded by one replicated
//    texel on every side so a bilinear footprint is always two 8-byte row pairs;
//  * reference ray table `dirs`: float4 per pixel of the reference view, padded by
//    the patch radius (PixelToDir, ACMMP.cu:119-134, evaluated once per view
//    instead of per sample);
//  * SPHERE rays are separable: per-row (sin, cos) of latitude and per-column (sin, cos)
//    of longitude (a few KB, cache resident) give PixelToDir's exact bits with two
//    multiplies; the bilateral spatial term per (row, sample) is a small table too, and
//    each lane keeps its pixel's 36 bilateral weights in LDS for the whole launch;
//  * working state colour-split (black = (x+y) even, red = odd), each colour
//    row-major over (H, ceil(W/2)); planes and costs double-buffered per colour so
//    a half-sweep reads the kernel-entry snapshot of its own colour;
//  * persistent state (what the reference keeps in plane_hypotheses_cuda /
//    costs_cuda between runs) row-major.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acmmp.h"
#include "run_plan.h"

namespace acmmp {

struct DevCam {
    // The fields the fast-math sample loop reads come first, contiguous and 16-byte aligned, so each
    // view's constants arrive in a few wide scalar loads (s_load_dwordx16 + x4 + x2 per sample and
    // view instead of nine narrow ones; r02 A/B profiles/r02_cam_layout_ab.txt: k_eval_nb -1.3%).
    // The fast projection works in the reference camera's frame: a source point is FR q + Ft for the
    // camera-frame point q = depth * ray of the reference pixel, FR = K R R0^T and Ft = K (R C0 + t)
    // (K = identity for SPHERE; R0, C0: the problem's reference camera, rounded once from doubles).
    float FRxy[6];                  // FR rows 0 and 1 interleaved: FR00 FR10 FR01 FR11 FR02 FR12
    float FRz[3];                   // FR row 2
    float Ft[3];
    float fkx, fky;                 // SPHERE: W / (2 pi), H / pi (fast mode)
    float cx, cy;                   // SPHERE params[1], params[2]
    // row-pair binary16 copy of the padded image (word (X, Y) = (t(X, Y), t(X, Y + 1))), present when
    // every texel of every view is exactly representable (8-bit images are): one 8-byte load per
    // bilinear footprint, same values
    const uint16_t* img16_base;
    int img16_bytes;
    float invW;                     // 1/W             (SPHERE longitude wrap)
    float Wf;
    float Hm1f;                     // H - 1 as float (SPHERE row clamp)
    int Wm1;                        // W - 1 (texel clamp)
    int pitch4;                     // bytes per padded row
    float Hf;                       // H as float (pinhole in-image test)
    int Hm1;                        // H - 1 (texel clamp)
    // the rest
    int model, W, H, img_pitch;     // img_pitch: floats per padded row (W + 2)
    float R[9];
    float t[3];
    float K[9];
    float inv_fx, inv_fy;           // 1/K[0], 1/K[4]  (pinhole world point)
    float C[3];                     // camera centre -(R^T t), computed like ACMMP.cu:592-594
    long long dep_off;              // float offset of the geom depth map (row-major)
    int dep_w, dep_h;
    int img_bytes;                  // bytes of the padded image (buffer descriptor range)
    const float* img_base;          // device address of padded texel (-1,-1) (buffer descriptor base)
};

// Per-pixel state handed from k_select to k_eval_ref / k_finish (80 bytes).
struct PixState {
    float4 plane_now;               // hypothesis entering PlaneHypothesisRefinement
    float4 cur_plane;               // plane_hypotheses[center] as of ACMMP.cu:1299
    uint4 vw;                       // view weights, 4-bit counts packed 8 per word
    float cost_now, depth_now, cur_cost, restricted_cost;
    uint32_t cur_sel, flags;        // flags: 1 = prior restricted, 2 = refinement runs
    float weight_norm;
    uint32_t src;                   // hypothesis ids of plane_now (bits 0-7) and cur_plane (8-15):
                                    // 0-7 neighbour direction, 8 current plane, 9+k candidate k
};

struct KParams {
    int model;                      // kPinhole / kSphere, uniform over all views
    int tex16;                      // 1: NCC fetches read the binary16 images (DevCam::img16_base)
    int fast;                       // 1: fast-math NCC sample projection (acmmp_set_math)
    int W, H, Wh, N, V;             // ref size, colour row width ceil(W/2), images, source views
    int R, inc, nside, S;           // patch radius, radius_increment, offsets per axis, samples
    int interp;                     // fast SPHERE k_eval_nb interpolates sample coordinates
    int homog;                      // fast pinhole staged chunks: homogeneous sample points
    float spread_max;               // interpolation fallback threshold, source pixels (ACMMP_SPREAD_MAX, 256)
    int rows;                       // rows the reference's checkerboard grid covers
    // row ranges (full image by default; a row band in the split latency mode, acmmp_band_*):
    int row_lo, row_hi;             // colour-grid rows the half-sweep kernels update, within [0, rows)
    int init_lo, init_hi;           // rows k_init initialises, within [0, H)
    int merge_lo, merge_hi;         // rows k_merge writes row-major, within [0, H)
    int filt_lo[2], filt_hi[2];     // rows k_filter updates per colour, within [0, rows)
    int dpitch;                     // dir table pitch (W + 2R)
    float depth_min, depth_max, sigma_spatial, sigma_color;
    int top_k;
    int geom, planar, hier, upsample;
    float scaled_cols, scaled_rows;
    int sw, sh;
    uint32_t seed_lo, seed_hi;
    const DevCam* cams;
    const float* dep;
    const float4* dirs;             // PINHOLE ray table, (W+2R) x (H+2R)
    const float2* sph_row;          // SPHERE (sin, cos) latitude, rows -R .. H+R-1
    const float2* sph_col;          // SPHERE (sin, cos) longitude, cols -R .. W+R-1
    const float* spatial;           // [(SPHERE ? H : 1)][S]: -dist / (2 sigma_s^2) (ACMMP.cu:398-403)
    float color_den;                // 2 * sigma_color^2
    float neg_tau;                  // k_eval_nb's interpolated loop skips a sample whose weight is <= neg_tau x the patch sum
                                    // in every live pixel of its wave (ACMMP_NEG_TAU, 2^-35); < 0: none (ACMMP_NEG_SKIP=0)
    float4* planes_rm;              // persistent row-major state
    float* w_rm;                    // planes_rm's .w (depth) as its own array: k_merge -> k_filter's taps (post only)
    float* costs_rm;
    float* pre_rm;
    uint32_t* sel_rm;
    const float4* scaled;           // hierarchy coarse planes (sw x sh)
    const float4* prior;            // planar prior planes (P)
    const uint32_t* mask;           // planar prior labels (P)
    float4* plane_cs[2];            // working state, current buffer per colour
    float* cost_cs[2];
    uint32_t* sel_cs[2];
    uint32_t* rng_cs[2];            // Philox draw counter per pixel
    // half-sweep scratch slab (one colour at a time)
    float* hyp_cost;                // [8][V][Pc] cost vectors of the 8 neighbour hypotheses
    float* cvec[2];                 // per colour [V][Pc]: NCC cost vector of the pixel's current plane
                                    // (NaN = view not evaluated for it yet)
    float* cand_vcost;              // [5][V][Pc] refinement candidates' cost vectors (NaN = not evaluated)
    int* nbpos;                     // [8][Pc] picked neighbour (x | y << 16) or -1
    float4* cand;                   // [5][Pc] refinement candidate planes
    float* cand_dep;                // [5][Pc] their depths (prior term, ACMMP.cu:912)
    float* cand_cost;               // [5][Pc] their aggregated costs
    PixState* pst;                  // [Pc]
    unsigned long long* work;       // [256] k_eval_nb pixels with NCC work (SPHERE patch sum >= 1e-6), per block % 256
    uint32_t nb_views;              // k_eval_nb: the source views this launch evaluates (all, or a chunk of them)
    int nb_chunk;                   // views per k_eval_nb launch (nb_view_chunk)
    int nb_tile;                    // k_eval_nb blocks as 8 x 4 tiles of the colour grid (nb_tile_order)
    int nb_count_work;              // k_eval_nb: this launch adds to `work` (the first launch of a half-sweep)
    long long Pc;                   // H * Wh
    // split refinement: k_eval_ref evaluates views [0, ref_split) of every candidate,
    // drops the ones whose partial aggregate already cannot beat cost_now, and queues the rest
    // (ci * 8 + candidate) for k_eval_ref_tail, which adds views [ref_split, V).  0 = no split.
    int ref_split;
    // (in the 4 bytes of padding before the next pointer: no field moves, so every kernel's argument offsets stay)
    float ref_neg_tau;              // the per-sample refinement loops (k_eval_ref, its tail, k_select's cache misses) drop a
                                    // sample whose weight is <= ref_neg_tau x its own pixel's patch sum
                                    // (ACMMP_REF_NEG_TAU, 2^-35); < 0: none (ACMMP_REF_NEG_SKIP=0, or outside the gate)
    uint32_t* surv;                 // queued candidates: kRefSlots (255) slots per k_eval_ref block
    unsigned* surv_count;           // [k_eval_ref blocks] slots used (zeroed before each k_eval_ref)
    unsigned* surv_pre;             // [k_eval_ref blocks + 1] their exclusive prefix (k_tail_scan)
    uint32_t* surv_dense;           // the survivors in block order (k_tail_compact)
    float4* psum;                   // [Pc] (patch sum w, sum w r, sum w r^2, centre texel) for the tail ([2][Pc] from
                                    // k_init with `keep`, below)
    // k_eval_nb's deferred interpolation fallbacks (ncc_chunk, k_nb_fix): pixel << 8 | hypothesis << 5 |
    // view; null = none (no interpolation, or ACMMP_SPREAD_MAX off)
    uint32_t* nbfix;                // kNbFixRegions regions of nbfix_cap entries (every entry a launch can queue)
    unsigned* nbfix_count;          // [kNbFixRegions]
    unsigned nbfix_cap;             // entries per region
    // (in the 4 bytes of padding before the next pointer: no field moves and the struct keeps its size, so every
    // kernel's argument offsets stay, the arguments behind the struct included)
    int keep;                       // 1: the run publishes the per-pixel kept-sample mask of the masked per-sample loops
                                    // (ref_neg_tau >= 0).  k_init then writes, for every pixel it
                                    // initialises, the patch sums into psum -- both colours, [2][Pc] colour-major -- and
                                    // behind them one 64-bit word per pixel (keep_words: bit s set = sample s is dropped,
                                    // its weight is <= ref_neg_tau x the pixel's patch sum), also [2][Pc]; k_eval_ref and
                                    // its tail read both and form no dropped weight again.  0: every kernel recomputes the
                                    // test from the weights (ACMMP_KEEP_MASK=0, a geom run, or outside the gate)
    // k_eval_ref's interpolated instance (SPHERE V > 4): per queued candidate, its selected views of
    // [0, ref_split) whose interpolation fell back -- k_eval_ref_tail recomputes them and restarts the chain
    uint32_t* cand_rough;           // [5][Pc]
    // SPHERE dead mask: per colour [Pc], 1 = the pixel's bilateral weight sum is below 1e-6, so
    // every NCC of it is 2.0 and its half-sweeps change nothing but its cost (0/0) and draw counter (+15).
    // k_init writes it where it forms the sum; the half-sweep kernels skip such pixels.  null = no skipping
    // (pinhole, ACMMP_DEAD_SKIP=0)
    uint8_t* dead[2];
    unsigned* dead_any;             // set by k_init when the view has a dead pixel at all (zeroed per run): a view
                                    // without one reads this word (a scalar load) and no mask byte
    unsigned* status;               // run status bits (kStatus*), zeroed per run, checked after it
};
static_assert(sizeof(KParams) == 568, "KParams is every kernel's first argument: a size change moves the ones behind it");

// The kept-sample words of a run with kp.keep, [2][Pc] colour-major.
__host__ __device__ inline unsigned long long* keep_words(const KParams& kp) {
    return reinterpret_cast<unsigned long long*>(kp.psum + 2 * kp.Pc);
}

// Per-half-sweep output buffers of the colour being updated.
struct SweepOut {
    float4* plane;
    float* cost;
};

// The queues of one strip's launches: everything a half-sweep indexes by block number or resets per launch
// (engine.h's KParams fields of the same names), carved per strip out of the scratch slab.
struct StripSlice {
    int row_lo, row_hi;
    uint32_t* surv;
    unsigned* surv_count;
    unsigned* surv_pre;
    uint32_t* surv_dense;
    uint32_t* nbfix;
    unsigned* nbfix_count;
    unsigned nbfix_cap;
};

// The plan-to-KParams step (run_plan.h): the fields the plan decides, as every kernel but the refinement's sees them
// (build_kparams sets the queue pointers with put_strip).
inline void put_plan(KParams& kp, const RunPlan& p) {
    kp.R = p.R; kp.nside = p.nside; kp.S = p.S;
    kp.Wh = p.Wh; kp.rows = p.rows; kp.Pc = static_cast<long long>(p.Pc);
    kp.interp = p.interp; kp.homog = p.homog; kp.spread_max = p.spread_max;
    kp.neg_tau = p.neg_tau; kp.ref_neg_tau = p.ref_neg_tau; kp.keep = p.keep;
    kp.nb_chunk = p.nb_chunk; kp.nb_tile = p.nb_tile; kp.ref_split = p.ref_split;
}
// One strip's rows and queues.
inline void put_strip(KParams& kp, const StripSlice& t) {
    kp.row_lo = t.row_lo; kp.row_hi = t.row_hi;
    kp.surv = t.surv; kp.surv_count = t.surv_count; kp.surv_pre = t.surv_pre; kp.surv_dense = t.surv_dense;
    kp.nbfix = t.nbfix; kp.nbfix_count = t.nbfix_count; kp.nbfix_cap = t.nbfix_cap;
}
// What k_eval_ref, its fallbacks and its tail see: the interpolated instance leaves its rough views to the tail, so
// without a split it does not interpolate.
inline KParams ref_stage(const KParams& kp, const RunPlan& p) {
    KParams r = kp;
    r.interp = p.ref_interp;
    if (!p.ref_fix) r.nbfix = nullptr;
    return r;
}
// A test hook whose queries the queue cannot hold or key: every sample projected instead.
inline KParams without_queue(const KParams& kp) {
    KParams r = kp;
    r.nbfix = nullptr;
    return r;
}

// Host-side launchers (kernels.hip; the fusion and voxel launchers are declared in fusion.h).  `plan` is the plan
// kp was built from: it names the kernel instances.
hipError_t launch_ray_tables(const KParams& kp, float4* dirs, float2* sph_row, float2* sph_col, hipStream_t s);
hipError_t launch_spatial_table(const KParams& kp, float* spatial, hipStream_t s);
hipError_t launch_init(const KParams& kp, const RunPlan& plan, hipStream_t s);
// ev: null, or 5 events recorded around the 4 kernels of the half-sweep (per-kernel timing); all_marks false
// records ev[0] and ev[1] only (the k_eval_nb bucket): each event record in the stream costs ~6 us of idle GPU
hipError_t launch_propagate(const KParams& kp, const RunPlan& plan, int colour, int iter, SweepOut out, hipStream_t s,
                            hipEvent_t* ev = nullptr, bool all_marks = true);
hipError_t launch_post(const KParams& kp, int do_post, hipStream_t s);
// Reference Camera -> device camera (derived constants computed as DESIGN.md §2.3 says), capi.cpp.
DevCam make_devcam(const acmmp_camera& cam);
void set_relative_frame(DevCam& d, const acmmp_camera& ref, const acmmp_camera& cam);   // DevCam::FR / Ft
// Current working-state buffers of one colour of a band run (capi.cpp; comm.cpp exchanges their rows).
struct BandBuffers {
    float4* plane;
    float* cost;
    uint32_t* sel;
    int Wh;
    hipStream_t stream;
    int device;
};
acmmp_status band_buffers(acmmp_ctx* c, int colour, BandBuffers* out);
// The context's device and engine stream (every kernel and copy of the context is queued there).
acmmp_status engine_stream(acmmp_ctx* c, int* device, hipStream_t* stream);

hipError_t launch_jbu(const float* ref, int W, int H, const float* coarse, int sw, int sh, int imagescale,
                      float* out, hipStream_t s);
// Launchers of aux_kernels.hip (with planar.h's).
hipError_t launch_export_depth(const float4* planes, long long P, float* dst, hipStream_t s);
hipError_t launch_copy(const void* src, void* dst, size_t bytes, hipStream_t s);  // bytes % 4 == 0
// Diagnostic clock probe (acmmp_clock_probe): per workgroup, shader cycles and 100 MHz ticks around a
// VALU-dense loop of `iters` steps on `rnd` (65536 floats); stamps may be null (warm-up launches).
struct ClockStamp {
    unsigned long long cycles, ticks;
};
hipError_t launch_clock_probe(const float* rnd, int iters, int blocks, ClockStamp* stamps, float* sink, hipStream_t s);
// acmmp_device_checksum: adds the checksum of `bytes` (multiple of 4) at ptr to *out (device, pre-zeroed)
hipError_t launch_checksum(const void* ptr, size_t bytes, unsigned long long* out, hipStream_t s);
hipError_t launch_debug(const KParams& kp, int which, int n, const int* px, const int* py, const float4* planes,
                        float* out, hipStream_t s);
// k_eval_nb's NCC instance on n pixels x 8 planes (planes[q * 8 + h]): out[(q * 8 + h) * V + v]
hipError_t launch_debug_nb(const KParams& kp, const RunPlan& plan, int n, const int* px, const int* py, const float4* planes, float* out,
                           hipStream_t s);
// k_eval_ref's NCC instance (+ the tail's per-sample fallbacks) on n pixels x 5 planes: out[(q * 5 + h) * V + v]
hipError_t launch_debug_ref(const KParams& kp, const RunPlan& plan, int n, const int* px, const int* py, const float4* planes, float* out,
                            hipStream_t s);
// Row-pair binary16 copy of one padded view (W + 2) x (H + 2) (DevCam::img16_base layout); *inexact
// (device int, pre-zeroed) is set when a texel is not exactly representable as a normal binary16
// number or zero.
hipError_t launch_to_f16_pairs(const float* src, int W, int H, uint32_t* dst, int* inexact, hipStream_t s);
hipError_t launch_pad_image(const float* src, size_t pitch_floats, int W, int H, float* dst, int dst_pitch,
                            hipStream_t s);

// Synchronous D2H into pageable caller memory.  Into destination pages that are not resident hipMemcpy
// crawled: 0.32 GB/s for a 800x600 view's planes + costs (30 ms) in heap memory freed and reused, against
// 14-50 GB/s into the same bytes once resident (profiles/r05_d2h_probe.json).  One store per 4 KiB page
// faults them in on the CPU first; the stores write bytes the copy overwrites.  (Heap pages never touched
// before stay slow to fault either way -- the Python binding gives large download arrays hugepage mappings of
// their own, capi.host_empty.)
inline hipError_t d2h(void* dst, const void* src, size_t bytes) {
    if (bytes >= (static_cast<size_t>(256) << 10)) {
        volatile unsigned char* p = static_cast<volatile unsigned char*>(dst);
        for (size_t o = 0; o < bytes; o += 4096) p[o] = 0;
        p[bytes - 1] = 0;
    }
    return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
}

}  // namespace acmmp
