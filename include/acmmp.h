/*
 * acmmp.h -- C ABI of the MI355X-native ACMMP-Spherical PatchMatch engine.
 *
 * Drop-in boundary for the depth/normal inference path of the reference
 * (/root/reference, contineu-ai/ACMMP-Spherical @ 2025-11-21).  The reference's only
 * caller of the hot path is ProcessProblem (main.cpp:73-210), which drives the
 * ACMMP class (ACMMP.h:57-111).  Every entry point below names the reference
 * member it replaces.  Plain C types only: pointers and sizes, no torch/HIP types.
 *
 * Threading: one context = one GPU = one host thread at a time (the reference is
 * single-threaded and not re-entrant either).  All host pointers are borrowed for
 * the duration of the call.  Errors are returned as acmmp_status codes; the C++
 * facade (acmmp-spherical_amd/host/ACMMP.hpp) maps them to the reference's
 * print-and-exit behaviour of CUDA_SAFE_CALL (ACMMP.cpp:64-72).
 */
#ifndef ACMMP_C_ABI_H
#define ACMMP_C_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACMMP_ABI_VERSION 1

/* CameraModel, main.h:35-38 */
#define ACMMP_PINHOLE 0
#define ACMMP_SPHERE 11

/* Camera, main.h:40-54 -- identical layout (120 bytes). */
typedef struct acmmp_camera {
    int32_t model;          /* ACMMP_PINHOLE or ACMMP_SPHERE */
    float params[4];        /* SPHERE: f, cx, cy, unused */
    float R[9];             /* world -> camera rotation, row-major */
    float t[3];             /* X_cam = R X_world + t */
    float K[9];             /* PINHOLE intrinsics, row-major */
    int32_t width, height;
    float depth_min, depth_max;
} acmmp_camera;

/* PatchMatchParams, ACMMP.h:32-55 -- identical layout (68 bytes). */
typedef struct acmmp_params {
    int32_t max_iterations;     /* 3; SetGeomConsistencyParams sets 2 (ACMMP.cpp:551) */
    int32_t patch_size;         /* 11 */
    int32_t num_images;         /* reference + sources, 2..33 */
    int32_t max_image_size;     /* 3200 */
    int32_t radius_increment;   /* 2 */
    float sigma_spatial;        /* 5 */
    float sigma_color;          /* 3 */
    int32_t top_k;              /* 4 */
    float baseline;             /* 0.54 (unused by the hot path) */
    float depth_min;            /* cams[0].depth_min * 0.6 (ACMMP.cpp:645) */
    float depth_max;            /* cams[0].depth_max * 1.2 (ACMMP.cpp:646) */
    float disparity_min;        /* unused by the hot path */
    float disparity_max;
    float scaled_cols;          /* hierarchy: coarse map size (ACMMP.cpp:810-811) */
    float scaled_rows;
    uint8_t geom_consistency;
    uint8_t planar_prior;
    uint8_t multi_geometry;
    uint8_t hierarchy;
    uint8_t upsample;
    uint8_t _pad[3];
} acmmp_params;

typedef enum acmmp_status {
    ACMMP_OK = 0,
    ACMMP_ERR_INVALID_ARGUMENT = 1,
    ACMMP_ERR_HIP = 2,
    ACMMP_ERR_OUT_OF_MEMORY = 3,
    ACMMP_ERR_STATE = 4,            /* call order violated (e.g. run before upload) */
    ACMMP_ERR_UNSUPPORTED = 5,      /* e.g. mixed camera models, > 32 source views */
    ACMMP_ERR_NO_DEVICE = 6,
    ACMMP_ERR_COMM = 7            /* RCCL failure */
} acmmp_status;

typedef struct acmmp_ctx acmmp_ctx;
typedef struct acmmp_image_cache acmmp_image_cache;
typedef struct acmmp_comm acmmp_comm;
typedef struct acmmp_fusion acmmp_fusion;
#define ACMMP_COMM_ID_BYTES 128

/* ACMMP::ACMMP() (ACMMP.cpp:99) + cudaSetDevice (main.cpp:77).  `device` is a HIP
 * ordinal; -1 keeps the calling thread's current device. */
acmmp_status acmmp_create(int device, acmmp_ctx **out);
/* ACMMP::~ACMMP() (ACMMP.cpp:101-143): frees every device buffer (no double free). */
void acmmp_destroy(acmmp_ctx *ctx);
const char *acmmp_status_str(acmmp_status s);
/* Message of the last error on this context (empty string if none). */
const char *acmmp_last_error(const acmmp_ctx *ctx);
int acmmp_abi_version(void);

/* Number of visible HIP devices (0 without a GPU); never fails. */
int acmmp_device_count(void);

/* Arithmetic of the NCC's per-sample projection (ComputeBilateralNCC, ACMMP.cu:456-476).
 * ACMMP_MATH_EXACT (default): the fixed IEEE definitions of DESIGN.md §2.3 -- results are
 * bit-identical to the CPU oracle.  ACMMP_MATH_FAST: what the reference's --use_fast_math build
 * (CMakeLists.txt:42) does to the same arithmetic -- hardware rsq/sqrt/rcp (<= 1 ulp), the
 * translation folded into the rotation, the asin/atan2 polynomials without special-argument paths
 * (DESIGN.md §2.4); results within the tolerances of DESIGN.md §2.4, not bit-identical.  Every new
 * context starts exact; callers choose fast explicitly.  No reference counterpart. */
enum { ACMMP_MATH_EXACT = 0, ACMMP_MATH_FAST = 1 };
acmmp_status acmmp_set_math(acmmp_ctx *ctx, int mode);
int acmmp_get_math(const acmmp_ctx *ctx);

/* The params member + Set{GeomConsistency,Hierarchy,PlanarPrior}Params
 * (ACMMP.cpp:548-565).  Copied; may be called again between runs. */
acmmp_status acmmp_set_params(acmmp_ctx *ctx, const acmmp_params *params);

/* Texture part of CudaSpaceInitialization (ACMMP.cpp:685-712): n = num_images
 * float grey images (0..255), images[i] is cams[i].height x cams[i].width,
 * row pitch `pitch_bytes[i]` (NULL -> tightly packed).  cams[0] is the reference. */
acmmp_status acmmp_upload_views(acmmp_ctx *ctx, int n, const float *const *images,
                                const size_t *pitch_bytes, const acmmp_camera *cams);

/* The same from device buffers of this context's GPU (in-memory pipeline: a view's image of one
 * scale is uploaded once and every problem of every pass that reads it copies it HBM to HBM).
 * images[i] are device pointers, otherwise as acmmp_upload_views.  No reference counterpart. */
acmmp_status acmmp_upload_views_device(acmmp_ctx *ctx, int n, const float *const *dev_images,
                                       const size_t *pitch_bytes, const acmmp_camera *cams);

/* Device-side cache of prepared source images (padded fp32 + binary16 copies), shared by the contexts
 * of one GPU.  The reference re-reads, re-converts and re-uploads every image of every problem
 * (InuputInitialization ACMMP.cpp:567-643 + CudaSpaceInitialization :685-712); a pipeline that keys its
 * (view, scale) images prepares each once.  budget_bytes: soft limit (least recently used entries no
 * current problem uses are freed beyond it), 0 = none.  Destroy after every context that used it. */
acmmp_status acmmp_image_cache_create(int device, size_t budget_bytes, acmmp_image_cache **out);
void acmmp_image_cache_destroy(acmmp_image_cache *cache);
/* out = {hits, misses, bytes held, entries, evictions} */
acmmp_status acmmp_image_cache_stats(acmmp_image_cache *cache, unsigned long long out[5]);

/* acmmp_upload_views (device_src = 0) / acmmp_upload_views_device (device_src = 1) with a content key
 * per view: keys[i] != 0 names the exact pixels of images[i] (the caller's promise -- e.g. view id and
 * scale); a view whose key and size are already in `cache` is not copied or converted again.  keys[i]
 * = 0 or cache = NULL: prepared privately, as acmmp_upload_views does.  No reference counterpart. */
acmmp_status acmmp_upload_views_keyed(acmmp_ctx *ctx, acmmp_image_cache *cache, int n, const uint64_t *keys,
                                      const float *const *images, const size_t *pitch_bytes,
                                      const acmmp_camera *cams, int device_src);

/* Geometric-consistency depth textures (ACMMP.cpp:653-678, 726-751): n depth maps,
 * depths[i] is h[i] x w[i] row-major (index 0 = reference, as the reference). */
acmmp_status acmmp_upload_depths(acmmp_ctx *ctx, int n, const float *const *depths,
                                 const int *w, const int *h);

/* The same from device buffers of this context's GPU (in-memory pipeline: the depth maps a geom
 * pass reads stay in HBM instead of the reference's depths*.dmb round trip). */
acmmp_status acmmp_upload_depths_device(acmmp_ctx *ctx, int n, const float *const *dev_depths,
                                        const int *w, const int *h);

/* The last run's depth map (.w of plane_hypotheses, ProcessProblem main.cpp:103-111) copied into a
 * device buffer of P floats on this context's GPU. */
acmmp_status acmmp_export_depth(acmmp_ctx *ctx, float *dev_dst);

/* Reference-view state for geom / hierarchy / planar reuse passes
 * (ACMMP.cpp:772-785, 833-843): planes = P float4 (nx, ny, nz, w) row-major,
 * costs = P floats (may be NULL -> unchanged).  P = cams[0].width*height. */
acmmp_status acmmp_set_state(acmmp_ctx *ctx, const float *planes, const float *costs);

/* The last run's planes (P float4) and costs (P floats) copied into device buffers of this context's GPU
 * (either may be NULL), and acmmp_set_state from such buffers: a geom pass restarts from the previous
 * pass's state without the host round trip of ProcessProblem's .dmb reload (ACMMP.cpp:772-785). */
acmmp_status acmmp_export_state(acmmp_ctx *ctx, float *dev_planes, float *dev_costs);
acmmp_status acmmp_set_state_device(acmmp_ctx *ctx, const float *dev_planes, const float *dev_costs);

/* Hierarchy coarse state scaled_plane_hypotheses (ACMMP.cpp:804-842):
 * sw*sh float4 row-major. */
acmmp_status acmmp_set_scaled_state(acmmp_ctx *ctx, const float *planes, int sw, int sh);

/* CudaPlanarPriorInitialization (ACMMP.cpp:847-867) after the host has expanded
 * labels: prior = P float4 plane params, mask = P labels (0 = no prior). */
acmmp_status acmmp_set_planar_prior(acmmp_ctx *ctx, const float *prior_planes, const uint32_t *masks);

/* ACMMP::RunPatchMatch (ACMMP.cu:1506-1556) minus the final D2H copy:
 * init, max_iterations x (black, red), GetDepthandNormal, black/red filter.
 * `seed` replaces curand_init(clock64(), ...) (ACMMP.cu:684).  Synchronous on
 * return, like the reference.  Results stay resident in HBM until downloaded. */
acmmp_status acmmp_run_patchmatch(acmmp_ctx *ctx, uint64_t seed);

/* Same with the schedule exposed (tests / profiling): n_half_sweeps < 0 means
 * 2*max_iterations; do_post = 0 leaves the raw working state (camera-frame
 * normal, w = plane distance) instead of (world normal, depth). */
acmmp_status acmmp_run_patchmatch_ex(acmmp_ctx *ctx, uint64_t seed, int n_half_sweeps, int do_post);

/* The D2H part of RunPatchMatch (ACMMP.cu:1553-1554) + GetPlaneHypothesis/GetCost
 * (ACMMP.cpp:884-892) in bulk: caller-allocated P float4 / P floats (either may be NULL). */
acmmp_status acmmp_download(acmmp_ctx *ctx, float *planes, float *costs);
/* Extra state readback for tests: selected_views bitmasks and pre_costs (either may be NULL). */
acmmp_status acmmp_download_aux(acmmp_ctx *ctx, uint32_t *selected_views, float *pre_costs);

/* Device-resident outputs (for in-process consumers such as an RCCL depth exchange):
 * returns device pointers to the row-major planes (float4[P]) and costs (float[P]). */
acmmp_status acmmp_device_outputs(acmmp_ctx *ctx, void **planes, void **costs);

/* Wait for all work of this context's device (hipDeviceSynchronize). */
acmmp_status acmmp_synchronize(acmmp_ctx *ctx);

/* Per-stage device time of the last run, measured with HIP events on the stream
 * the kernels run on: [init, propagation (all half-sweeps), post]. */
acmmp_status acmmp_last_timing(const acmmp_ctx *ctx, float ms[3]);

/* Per-kernel device time of the last run's half-sweeps (HIP events around the launches, on the
 * kernels' stream): summed ms and launch count for [k_eval_nb, k_select, k_eval_ref, k_finish]
 * (the stages one CheckerboardPropagation half-sweep is split into).  The k_eval_ref
 * bucket includes its tail launch (k_eval_ref_tail); the neighbour pick (k_pick) runs before the
 * k_eval_nb bucket opens and is in the propagation stage time only.  Only the k_eval_nb bucket is
 * timed unless ACMMP_KERNEL_TIMING=all was set in the environment for the run (each event record
 * idles the GPU a few microseconds); an untimed bucket reports 0 ms over 0 launches. */
acmmp_status acmmp_last_kernel_timing(const acmmp_ctx *ctx, float ms[4], int launches[4]);

/* Work accounting of the last run's k_eval_nb launches: pixels whose NCCs were evaluated, and all
 * pixels processed.  SPHERE pixels whose patch weight sum is below 1e-6 have every cost = 2.0
 * (ACMMP.cu:501-503) and are short-circuited; the roofline counts only evaluated pixels. */
acmmp_status acmmp_last_work(const acmmp_ctx *ctx, unsigned long long *evaluated, unsigned long long *total);

/* Host wall-clock breakdown of the last acmmp_set_planar_prior_from_state / _from_maps call, in ms:
 * [support points (device kernel + copy back; 0 for _from_maps, whose host scan is in the next entry),
 * Delaunay triangulation (host), the rest of the host half (labelled triangles, plane fits, step and trig
 * tables), device half (staging and enqueueing the table upload and the raster and mask kernels on the
 * context's stream -- they complete before its next run; see acmmp_set_planar_prior_from_maps)].
 * No reference counterpart (profiling of main.cpp:113-187's block). */
acmmp_status acmmp_last_planar_timing(const acmmp_ctx *ctx, float ms[4]);

/* Bytes per source texel the NCC fetches read: 2 when every texel of the uploaded views is exactly
 * a binary16 number (8-bit images are) and the engine keeps a binary16 copy of them, 4 for the fp32
 * images, 0 before acmmp_upload_views.  Results are identical either way; the
 * environment variable ACMMP_TEX16=0 at upload time forces 4.  No reference counterpart. */
int acmmp_texel_bytes(const acmmp_ctx *ctx);

/* ---- row-band split of one reference view (SURVEY.md §8e latency mode; no reference counterpart:
 * the reference runs a view on one GPU) -------------------------------------------------------------
 * Several contexts (one per GPU) holding the same uploaded problem each run RunPatchMatch on the image
 * rows [row0, row1) of one view; after every half-sweep each exchanges the updated colour's rows within
 * ACMMP_BAND_HALO of its band with the neighbouring bands.  Each band's output rows are bit-identical to
 * a whole-view acmmp_run_patchmatch with the same seed.  Bands must span >= ACMMP_BAND_HALO rows. */
#define ACMMP_BAND_HALO 23

/* The strip schedule of acmmp_run_patchmatch (no GPU needed): the checkerboard rows
 * [0, rows) cut into `want_strips` strips, clamped so that boundaries fall on multiples of 4 rows and every
 * strip spans >= ACMMP_BAND_HALO rows.  Returns the strip count NS (0: invalid arguments) and writes
 * bounds[0 .. NS] (room for 65) and, when `waits` is not null, for each strip i the three strips whose
 * previous half-sweep its next one waits for, waits[3 i .. 3 i + 2] = i - 1, i, i + 1, -1 where there is
 * none (room for 192).  The environment variables ACMMP_STRIPS and ACMMP_STRIP_STREAMS (read per run) set
 * the strip and stream counts of a run; neither changes a result.  Fast-math pinhole runs and fast-math
 * SPHERE runs with interpolated sample coordinates and more than 4 source views always run one strip. */
int acmmp_strip_plan(int rows, int want_strips, int *bounds, int *waits);

/* RandomInitialization of the band +- halo (the same per-pixel values every band computes). */
acmmp_status acmmp_band_begin(acmmp_ctx *ctx, uint64_t seed, int row0, int row1);
/* The next half-sweep (black, red, black, ...) on the band's rows; *colour = the colour updated. */
acmmp_status acmmp_band_sweep(acmmp_ctx *ctx, int *colour);
/* Half-sweeps of the band run still to do (0 when none is in progress). */
int acmmp_band_sweeps_left(const acmmp_ctx *ctx);
/* Row ranges [a, b) of the halo exchange after a half-sweep: send to the band above, receive from it,
 * send to the band below, receive from it (empty at the image edges).  A band's "send down" range is
 * the next band's "receive from above" range and vice versa. */
acmmp_status acmmp_band_halo_ranges(const acmmp_ctx *ctx, int ranges[8]);
/* In-process exchange: copy rows [row_a, row_b) of `colour`'s current plane / cost / selected-view
 * state from src to dst (same or peer device; waits for src's stream). */
acmmp_status acmmp_band_copy_rows(acmmp_ctx *dst, acmmp_ctx *src, int colour, int row_a, int row_b);
/* Host transport of the same exchange (ranks without a device-to-device path, e.g. a gloo or MPI run):
 * rows [row_a, row_b) of `colour`'s current state to / from host buffers of (row_b - row_a) * ceil(W / 2)
 * colour-grid pixels -- planes 4 floats, costs 1 float, selected-view masks 1 uint32 each.  get waits for the
 * context's half-sweep; set is complete on return. */
acmmp_status acmmp_band_get_rows(acmmp_ctx *ctx, int colour, int row_a, int row_b, float *planes, float *costs,
                                 uint32_t *selected_views);
acmmp_status acmmp_band_set_rows(acmmp_ctx *ctx, int colour, int row_a, int row_b, const float *planes,
                                 const float *costs, const uint32_t *selected_views);
/* Test hook: the cached NCC cost vectors of rows [row_a, row_b) of `colour` in a band run, out[v * n + k] for
 * source view v and colour-grid pixel k of the n = (row_b - row_a) * ceil(W / 2) -- straight after acmmp_band_begin,
 * what the initialisation evaluated for the planes acmmp_band_get_rows returns.  Waits for the context's stream. */
acmmp_status acmmp_debug_band_cvec(acmmp_ctx *ctx, int colour, int row_a, int row_b, float *out);
/* Test hook: the kept-sample mask words of the same rows, one per colour-grid pixel (bit s set: the initialisation
 * found patch sample s negligible for that pixel, and the refinement's per-sample loops skip it).  ACMMP_ERR_STATE
 * when the run publishes no mask (outside the fast SPHERE V <= 4 gate, ACMMP_REF_NEG_SKIP=0 or ACMMP_KEEP_MASK=0). */
acmmp_status acmmp_debug_band_keep_mask(acmmp_ctx *ctx, int colour, int row_a, int row_b, uint64_t *out);
/* Test hook: device memory the kept-sample mask adds to a run of a W x H view with these settings (model 0 pinhole / 11 sphere,
 * fast math, binary16 texels, source views, geom pass) under the environment as it is now: the run's own gates, no GPU
 * needed.  0 where the run publishes no mask, -1 on bad arguments. */
long long acmmp_keep_mask_bytes(int W, int H, int model, int patch_size, int radius_increment, int fast, int tex16,
                                int n_src, int geom);
/* GetDepthandNormal + the two filters on band +- 10 / 5 rows; synchronous.  Rows [row0, row1) of the
 * row-major outputs (acmmp_download / acmmp_device_outputs) are then final. */
acmmp_status acmmp_band_end(acmmp_ctx *ctx, int do_post);

/* ---- device buffers and the multi-GPU communicator (no reference counterpart:
 * the reference is single-GPU and exchanges depth maps through dmb files) ------------------- */

/* Plain device memory on `device` (pipeline depth store); kind: 0 = H2D, 1 = D2H, 2 = D2D. */
acmmp_status acmmp_device_alloc(int device, size_t bytes, void **ptr);
acmmp_status acmmp_device_free(int device, void *ptr);
acmmp_status acmmp_memcpy(int device, void *dst, const void *src, size_t bytes, int kind);

/* 64-bit checksum of `bytes` (a multiple of 4) of device memory on `device`: the sum mod 2^64 over its
 * 32-bit words w_i of splitmix64's finaliser applied to (i << 32) | w_i (position and value both enter).
 * The pipeline's depth exchange compares every rank's checksum of each broadcast map
 * (acmmp/pipeline.py RcclExchange); acmmp.capi.checksum_host is the same function on host arrays.
 * The caller must have completed every write to the buffer (acmmp_synchronize, or its own stream's
 * synchronize): the sum runs on the null stream, which the engine's non-blocking streams do not wait for. */
acmmp_status acmmp_device_checksum(int device, const void *ptr, size_t bytes, uint64_t *out);

/* Diagnostics for the performance record (bench.py `device`, `clock`); no reference counterpart.
 * acmmp_device_identity: the device's PCI bus id ("dddd:bb:dd.f") and its 16-byte UUID.
 * acmmp_clock_probe: the shader clock the device holds under a VALU-dense load on random operands
 * (MI355X_MICROARCH.md "DVFS give-back"): ~5 ms launches back to back for warm_ms, then one launch whose
 * workgroups read the shader-cycle and 100 MHz counters around their loop.  out = {median GHz over the
 * workgroups, min, max, ms of that launch}.  Synchronous; uses the device's null stream. */
acmmp_status acmmp_device_identity(int device, char *pci_bus_id, int len, uint8_t uuid[16]);
acmmp_status acmmp_clock_probe(int device, float warm_ms, double out[4]);

/* RCCL communicator, one rank per process / GPU.  Rank 0 creates the id and hands the 128 bytes
 * to the other ranks out of band (the Python driver uses the launcher's TCP store). */
acmmp_status acmmp_comm_unique_id(uint8_t id[ACMMP_COMM_ID_BYTES]);
acmmp_status acmmp_comm_create(int device, const uint8_t id[ACMMP_COMM_ID_BYTES], int nranks, int rank,
                               acmmp_comm **out);
void acmmp_comm_destroy(acmmp_comm *comm);

/* Orders every collective queued on comm after this call behind all the work ctx (a context of the
 * same GPU) has queued so far -- e.g. acmmp_export_depth into a buffer about to be broadcast: an event
 * recorded on the engine stream that the communicator's stream waits on, no host wait.  No reference
 * counterpart (the reference hands depth maps over through depths*.dmb files, ACMMP.cpp:653-678). */
acmmp_status acmmp_comm_after(acmmp_comm *comm, acmmp_ctx *ctx);

/* Grouped in-place broadcasts: device buffer bufs[i] (bytes[i]) from rank roots[i] to every rank.
 * Synchronous on return. */
acmmp_status acmmp_comm_broadcast(acmmp_comm *comm, int n, void *const *bufs, const size_t *bytes,
                                  const int *roots);

/* Element-wise max over ranks of n host doubles (timing reductions); synchronous. */
acmmp_status acmmp_comm_allreduce_max(acmmp_comm *comm, double *vals, int n);

/* Halo exchange of a band run over RCCL: after acmmp_band_sweep updated `colour`, grouped ncclSend /
 * ncclRecv of the acmmp_band_halo_ranges rows with rank_up / rank_down (-1 = none), queued on the
 * context's stream (ordered with its kernels, no host wait). */
acmmp_status acmmp_comm_band_exchange(acmmp_comm *comm, acmmp_ctx *ctx, int colour, int rank_up, int rank_down);

/* A whole band run: begin, every half-sweep followed by the RCCL halo exchange, end.  comm may be
 * NULL for a single band covering the view.  Synchronous on return. */
acmmp_status acmmp_run_patchmatch_band(acmmp_ctx *ctx, acmmp_comm *comm, uint64_t seed, int row0, int row1,
                                       int rank_up, int rank_down);

/* ---- GPU depth-map fusion (RunFusionCuda + SimpleFusionKernel, ACMMP.cu:1662-2105) -------------
 * One object per fusion run.  cams[i] is view i's camera already rescaled to its depth map
 * (RescaleImageAndCamera, ACMMP.cpp:213-246).  set_view uploads what the reference puts in textures:
 * the depth map (H x W), world-frame normals (3 floats per pixel, normals.dmb) and the colour image
 * rescaled to the depth size (3 bytes per pixel, OpenCV BGR order).  run fuses reference view `ref`
 * against src_views (indices into the set, -1 = missing, at most 32) and returns the consistent
 * points in pixel order, 9 floats each: x y z nx ny nz c0 c1 c2 (colour slots as the kernel stores them,
 * ACMMP.cu:1706-1708; StoreColorPlyFileBinaryPointCloud writes c2, c1, c0 as red, green, blue).
 * When `cap` is too small *n_points holds the count and ACMMP_ERR_INVALID_ARGUMENT is returned. */
acmmp_status acmmp_fusion_create(int device, int n_views, const acmmp_camera *cams, acmmp_fusion **out);
acmmp_status acmmp_fusion_set_view(acmmp_fusion *f, int view, const float *depth, const float *normals,
                                   const uint8_t *bgr);
acmmp_status acmmp_fusion_run(acmmp_fusion *f, int ref, int n_src, const int *src_views, float *points, int cap,
                              int *n_points);
const char *acmmp_fusion_last_error(const acmmp_fusion *f);
void acmmp_fusion_destroy(acmmp_fusion *f);

/* ---- whole-scene fusion (no reference counterpart: RunFusionCuda collects every view's points on the
 * host, ACMMP.cu:2064-2071) -------------------------------------------------------------------------
 * acmmp_fusion_run_scene fuses the reference views refs[0 .. n_refs) in that order in one call; view k
 * against src_views[32*k .. 32*k + n_src[k]) (indices into the set, -1 = missing, n_src[k] <= 32).  The
 * result stays in HBM, in the fusion object, until the next successful run replaces it: the points (9 floats
 * each, as acmmp_fusion_run) and per point its provenance -- the position k of its view in `refs`, its pixel
 * r*W + c in that view, and a source mask whose bit j says that src_views[32*k + j] was consistent.
 * counts[k] (may be NULL) = points of view k; *n_points = their 64-bit sum.  The chunk prefix sum runs on the
 * device; the host waits once per view, for that view's 4-byte count (the output buffer grows from it before
 * anything is written there; a growth, geometric, also waits for the device copy into the larger buffer),
 * and once at the end of the call.  No point crosses to the host before acmmp_fusion_scene_points.
 *
 * flags = 0, plain: the result is the concatenation of acmmp_fusion_run(refs[k], ...) over k, bit for bit
 * and in that order (every view emits every surface point it sees consistently: a point seen by V views
 * appears about V times).  The used masks are neither read nor written.
 *
 * flags = ACMMP_FUSE_UNIQUE, duplicate-free: every view carries a byte mask `used`, cleared by
 * acmmp_fusion_create, by acmmp_fusion_set_view of that view and by acmmp_fusion_reset_used.  View k is fused
 * exactly as above on depth maps in which every used pixel reads as depth 0 (a used reference pixel is
 * skipped, a used source sample is skipped; arithmetic, thresholds and the order of the sums are unchanged).
 * It sees the marks of the earlier views of the run and of earlier runs, never those of its own pixels.
 * After view k, for each point it emitted, its reference pixel is marked, and for each set source bit the
 * source pixel that was sampled.  So a depth sample that contributed to a point of an earlier reference view
 * contributes to no point of a later one.  Marks persist across calls until reset.
 *
 * Any error -- an out-of-memory part-way included -- leaves the object as it was before the call: the used
 * masks and the previous result are unchanged (the new result is built beside the previous one, so both are
 * held until the run ends). */
#define ACMMP_FUSE_UNIQUE 1
acmmp_status acmmp_fusion_run_scene(acmmp_fusion *f, int n_refs, const int *refs, const int *n_src,
                                    const int *src_views, int flags, int *counts, int64_t *n_points);
/* Points [first, first + n) of the scene result to host arrays, any of which may be NULL: points n x 9
 * floats, ref_index / pixel n int32, src_mask n uint32.  A caller streams a cloud larger than it wants to
 * hold by asking for one range after another. */
acmmp_status acmmp_fusion_scene_points(acmmp_fusion *f, int64_t first, int64_t n, float *points,
                                       int32_t *ref_index, int32_t *pixel, uint32_t *src_mask);
/* Clears every view's used mask. */
acmmp_status acmmp_fusion_reset_used(acmmp_fusion *f);
/* Test hook: view's used mask, H x W bytes (all 0 for a view that was never set). */
acmmp_status acmmp_fusion_download_used(acmmp_fusion *f, int view, uint8_t *mask);

/* ---- voxel-grid reduction of the scene result (no reference counterpart) -----------------------------
 * acmmp_fusion_voxelize reduces the resident scene result, points 0 .. N in their order, to one point per
 * occupied cell of a grid of `voxel_size` (finite, > 0): centroid, mean normal, mean colour and the number of
 * points.  The scene result is left untouched; the voxel result stays in HBM beside it until the next
 * successful voxelize replaces it or the next successful acmmp_fusion_run_scene / acmmp_fusion_set_scene discards it.
 *
 * The result is defined in integers, so that it is bit-reproducible and the same whatever order the device's
 * atomics land in.  With inv = 1.0f / voxel_size and plain IEEE float32 arithmetic (no contraction):
 *  1. a point is rejected when one of its nine floats is not finite or a normal / colour component exceeds
 *     2^20 in magnitude;
 *  2. per axis t = (x - o) * inv, g = floorf(t); the point is rejected too unless 0 <= g < 2^21 on every axis;
 *     its cell is key = gx | gy << 21 | gz << 42;
 *  3. per axis q = (int64) rintf((t - g) * 65536.0f), and q = (int64) rintf(v * 65536.0f) for each of the six
 *     normal and colour components v (round half to even; both products are exact);
 *  4. per cell: n = its points (at most 2^31 - 1), S = the nine int64 sums of q (wrapping), first = the
 *     smallest scene index among its points;
 *  5. a cell with n >= min_points (>= 1) gives, in float64 rounded once to float32,
 *     position = (float)((double)o + ((double)g + (double)S / ((double)n * 65536.0)) * (double)voxel_size) and
 *     normal, colour = (float)((double)S / ((double)n * 65536.0)) (normals are a plain mean, not renormalised);
 *  6. the kept cells are listed in ascending order of `first`: their order of first appearance in the scene.
 * origin = NULL takes for o the component-wise minimum of x, y, z over the points that pass step 1 (-0 orders
 * below +0), or (0, 0, 0) when there is none.
 *
 * *n_voxels = kept cells, *n_occupied = cells before the min_points cut, *n_rejected = rejected points,
 * origin_used[3] = o; any of the four may be NULL.  An empty scene gives 0 voxels.  ACMMP_ERR_INVALID_ARGUMENT:
 * a size that is not finite and > 0, min_points < 1, a non-finite origin, no scene result.  Any error -- an
 * out-of-memory part-way included -- leaves the previous voxel result and the scene result as they were.
 * Device memory while it runs: a hash table of 28 bytes per slot, with the smallest power of two
 * >= max(2 N, 1024) slots, and 72 bytes of sums per kept cell; the result holds 40 bytes per kept cell. */
acmmp_status acmmp_fusion_voxelize(acmmp_fusion *f, float voxel_size, const float *origin, int min_points,
                                   int64_t *n_voxels, int64_t *n_occupied, int64_t *n_rejected, float *origin_used);
/* Voxels [first, first + n) of the voxel result to host arrays, either of which may be NULL: points n x 9
 * floats (as the scene's), counts n int32.  Ranges as acmmp_fusion_scene_points. */
acmmp_status acmmp_fusion_voxel_points(acmmp_fusion *f, int64_t first, int64_t n, float *points, int32_t *counts);
/* Test hook.  force_slots = 0: automatic table size; otherwise the size of the next voxelize's table, a power of
 * two >= 64 and > the scene's point count then (so it is never full), else that voxelize returns
 * ACMMP_ERR_INVALID_ARGUMENT.  The outputs (any may be NULL) describe the last successful voxelize: slots,
 * occupied slots, the longest probe distance + 1 (depends on the order of arrival: informational) and the
 * number of cells stored at a slot index below their home slot (independent of it). */
acmmp_status acmmp_fusion_voxel_table(acmmp_fusion *f, int64_t force_slots, int64_t *slots, int64_t *occupied,
                                      int64_t *max_probe, int64_t *wrapped);

/* ---- a scene result from the host --------------------------------------------------------------------
 * acmmp_fusion_set_scene replaces the scene result with n >= 0 host points, 9 floats each, taken bit for bit (a
 * cloud of an earlier run, of another rank, or one built for a test).  ref_index / pixel / src_mask (n each) may
 * be NULL and are then stored as -1 / -1 / 0.  For lifetimes it is a successful acmmp_fusion_run_scene: the voxel
 * result, the clean result and the scratch sized for the previous scene are discarded; the used masks are not
 * touched.  n = 0 is an empty scene.  Any error leaves the object as it was. */
acmmp_status acmmp_fusion_set_scene(acmmp_fusion *f, int64_t n, const float *points, const int32_t *ref_index,
                                    const int32_t *pixel, const uint32_t *src_mask);

/* ---- cleaning the voxel result: support and connected components (no reference counterpart) -------------
 * acmmp_fusion_voxel_clean is defined over the resident voxel result V: voxels 0 .. nv in their order, each with
 * its cell (gx, gy, gz) of step 2 above and its point count c.
 *  1. Neighbours.  Voxel u is a neighbour of v when u is in V and the offset d = cell(u) - cell(v) has d != 0,
 *     |d_a| <= 1 on every axis and |dx| + |dy| + |dz| <= 1, 2 or 3 for connectivity 6, 18 or 26.  Offsets are
 *     applied per axis to the 21-bit indices, never to the packed key: a cell with an index outside [0, 2^21) does
 *     not exist.  Cells that min_points dropped at voxelize time are not in V.
 *  2. Support.  support(v) = the number of neighbours of v; S = { v : support(v) >= min_neighbours }, one pass,
 *     not iterated.  min_neighbours = 0 keeps every voxel.  *n_unsupported = nv - |S|.
 *  3. Labels.  The components are those of the neighbour graph induced on S; label(v) = the smallest voxel index
 *     of v's component, -1 for v outside S.
 *  4. Component table.  The components in ascending order of label, ids 0 .. *n_components; each entry holds
 *     root (the label), voxels, and points (the int64 sum of c).
 *  5. Kept voxels.  v is kept when it is in S and its component has voxels >= min_component_voxels and
 *     points >= min_component_points (both >= 1).  *n_components_kept = the components that pass.
 *  6. Clean result.  The kept voxels in ascending voxel index: their 9 floats and counts copied bit for bit from
 *     the voxel result, each with the id of its component in the table of step 4.  *n_kept = their number.
 * Every quantity is an integer and every device atomic a minimum or an integer add, so the result is the same
 * whatever order they land in.  *rounds = the labelling passes the host waited for (the last one changes
 * nothing); it depends on timing and is informational.  Any of the five outputs may be NULL.
 *
 * ACMMP_ERR_INVALID_ARGUMENT: a connectivity not in {6, 18, 26}, min_neighbours < 0, a threshold < 1, no voxel
 * result (an empty one gives 0 / 0 / 0).  The voxel result and the scene result are untouched.  The clean result
 * stays in HBM until the next successful clean replaces it or the next successful acmmp_fusion_voxelize,
 * acmmp_fusion_run_scene or acmmp_fusion_set_scene discards it.  Any error -- an out-of-memory part-way included,
 * or a labelling that exceeds its bound of nv + 2 rounds (ACMMP_ERR_HIP) -- leaves the object as it was.
 * Device memory: the voxel result keeps its hash table (28 bytes per slot) and 8 bytes per voxel for this call,
 * so a voxelize that replaces a voxel result fills a spare table and keeps both; the clean result holds 12 bytes per
 * voxel (label, neighbours), 48 per kept voxel and 24 per component; 24 bytes per voxel of scratch while it runs. */
acmmp_status acmmp_fusion_voxel_clean(acmmp_fusion *f, int connectivity, int min_neighbours,
                                      int64_t min_component_voxels, int64_t min_component_points, int64_t *n_kept,
                                      int64_t *n_components, int64_t *n_components_kept, int64_t *n_unsupported,
                                      int64_t *rounds);
/* Kept voxels [first, first + n) of the clean result to host arrays, any of which may be NULL: points n x 9
 * floats, counts n int32, component n int64.  Ranges as acmmp_fusion_voxel_points. */
acmmp_status acmmp_fusion_clean_points(acmmp_fusion *f, int64_t first, int64_t n, float *points, int32_t *counts,
                                       int64_t *component);
/* label and support of voxels [first, first + n) of the voxel result, as the last successful clean computed them
 * (no clean result: every range but an empty one at 0 is refused); either array may be NULL. */
acmmp_status acmmp_fusion_voxel_labels(acmmp_fusion *f, int64_t first, int64_t n, int64_t *label, int32_t *support);
/* Entries [first, first + n) of the component table; any array may be NULL. */
acmmp_status acmmp_fusion_component_table(acmmp_fusion *f, int64_t first, int64_t n, int64_t *root, int64_t *voxels,
                                          int64_t *points);

/* ---- visibility check of the voxel or clean result against the views' depth maps (no reference counterpart) ----
 * acmmp_fusion_voxel_visibility is defined over the entries e = 0 .. N of its source, in their order: the voxel result
 * (ACMMP_VIS_FROM_VOXELS) or the clean result's kept voxels (ACMMP_VIS_FROM_CLEAN), 9 floats and a count each.  X =
 * an entry's first three floats.  For list position j = 0 .. n_list, view i = views[j] (a view listed twice counts
 * twice), in plain IEEE float32 arithmetic with no contraction:
 *  1. Projection.  (px, py, pd) = the projection of X into camera i with its depth, exactly as the fusion projects a
 *     reference point into a source view (ProjectonCamera_cu, ACMMP.cu:602-644; SPHERE: pd = sqrtf of the squared
 *     camera-frame distance, pinhole: pd = the camera-frame z).
 *  2. Pixel.  The pair (e, j) is unobserved unless px, py and pd are finite and pd > 0.  Then c = (int)(px + 0.5f),
 *     r = (int)(py + 0.5f), saturated, and the pair is unobserved unless 0 <= c < W_i and 0 <= r < H_i.
 *  3. Samples.  The window is the pixels (c + dx, r + dy), |dx|, |dy| <= radius, that lie inside the image (no wrap
 *     across the SPHERE seam, as in the fusion).  A pixel whose raw depth sd -- as acmmp_fusion_set_view uploaded it;
 *     the used masks are never read -- is finite and > 0 is a sample.  With t = rel_tol * sd and d = pd - sd the sample
 *     agrees when fabsf(d) <= t, lies behind when d > t (the view's surface is nearer than the entry) and in front
 *     otherwise.
 *  4. Class of the pair.  No sample: unobserved.  Any sample that agrees: support.  Otherwise any sample behind:
 *     occluded.  Otherwise conflict: the entry lies in front of everything the view sees there, in the view's free
 *     space.  The class does not depend on the order of the samples.
 *  5. Tallies.  tallies[e] = (support, conflict, occluded): the int32 numbers of list positions of each class.  Entry e
 *     is kept when support >= min_support and conflict <= max_conflicts.
 *  6. Visible result.  The kept entries in ascending e: their 9 floats and counts copied bit for bit from the source,
 *     each with its tallies.  *n_kept = their number, *n_unsupported = the entries with support < min_support,
 *     *n_conflicting = those with conflict > max_conflicts (an entry may be in both), class_totals[4] = the int64 sums
 *     over the entries of support, conflict, occluded and unobserved.  Any of the four may be NULL.
 * Every quantity that is summed is an integer, so the result is the same whatever order the device's atomics land in.
 *
 * ACMMP_ERR_INVALID_ARGUMENT: a source that is neither constant, no such source result (an empty one gives zeros),
 * n_list outside [1, 4096], a view index outside the set or a view never given to acmmp_fusion_set_view, rel_tol not
 * finite or < 0, a radius not in {0, 1}, min_support < 0, max_conflicts < 0.  The source results, the scene result and
 * the used masks are never modified.  The visible result stays in HBM until the next successful visibility call
 * replaces it or its source is replaced or discarded: by a successful acmmp_fusion_voxelize, acmmp_fusion_run_scene or
 * acmmp_fusion_set_scene, and by a successful acmmp_fusion_voxel_clean when the source was the clean result (a clean
 * leaves a visible result of the voxel result alone).  acmmp_fusion_set_view does not touch it.  Any error -- an
 * out-of-memory part-way included -- leaves the object as it was (the new result is built beside the previous one).
 * Device memory: 12 bytes of tallies per entry of the source and 52 bytes per kept entry (point, count, tallies),
 * both held with the result; 4 bytes of flag per entry of a compaction segment (at most 2^30 entries) and 8 bytes per
 * 256 entries of one while it runs.  The host waits twice: for the counts, to size the result, and at the end. */
#define ACMMP_VIS_FROM_VOXELS 0   /* entries = the voxel result */
#define ACMMP_VIS_FROM_CLEAN 1    /* entries = the clean result's kept voxels */
acmmp_status acmmp_fusion_voxel_visibility(acmmp_fusion *f, int source, int n_list, const int *views, float rel_tol,
                                           int radius, int min_support, int max_conflicts, int64_t *n_kept,
                                           int64_t *n_unsupported, int64_t *n_conflicting, int64_t class_totals[4]);
/* Kept entries [first, first + n) of the visible result to host arrays, any of which may be NULL: points n x 9
 * floats, counts n int32, tallies n x 3 int32.  Ranges as acmmp_fusion_voxel_points. */
acmmp_status acmmp_fusion_visible_points(acmmp_fusion *f, int64_t first, int64_t n, float *points, int32_t *counts,
                                         int32_t *tallies);
/* tallies (n x 3 int32) of entries [first, first + n) of the source, as the last successful visibility call computed
 * them (no visible result: every range but an empty one at 0 is refused). */
acmmp_status acmmp_fusion_visibility_tallies(acmmp_fusion *f, int64_t first, int64_t n, int32_t *tallies);

/* ---- surface mesh of the voxel, clean or visible result: TSDF and surface nets (no reference counterpart) ----
 * acmmp_fusion_voxel_mesh is defined over the entries e = 0 .. ne of its source, in their order: the voxel result
 * (ACMMP_MESH_FROM_VOXELS), the clean result's kept voxels (ACMMP_MESH_FROM_CLEAN) or the visible result's kept
 * entries (ACMMP_MESH_FROM_VISIBLE).  An entry's cell (gx, gy, gz) is the cell step 2 of acmmp_fusion_voxelize gave
 * its voxel; it is carried with the entry (the clean and the visible result hold their entries' voxel indices), never
 * recomputed from the centroid.  o and voxel_size are the voxel result's.  Arithmetic is plain IEEE with no
 * contraction, float32 or float64 as said.
 *  1. Samples.  The sample cells are all g + d, d in {-1, 0, 1}^3, of all entries; offsets are applied per axis to the
 *     21-bit indices, and a cell with an index outside [0, 2^21) does not exist (as for acmmp_fusion_voxel_clean).  A
 *     sample's rank is the smallest e * 27 + (dz+1)*9 + (dy+1)*3 + (dx+1) over the pairs (e, d) that produce it;
 *     samples are numbered s = 0 .. ns in ascending rank.  A sample whose cell is an entry's own cell (d = 0)
 *     remembers that entry (at most one entry has that cell).  The dilation is one cell.
 *  2. TSDF.  X(s) = the cell centre, per axis (float)((double)o + ((double)g + 0.5) * (double)voxel_size).  For list
 *     position j, view i = views[j] (a view listed twice counts twice): (px, py, pd) and the pixel (c, r) exactly as
 *     steps 1-2 of acmmp_fusion_voxel_visibility, the pair being unobserved under the same conditions.  The only
 *     pixel read is (c, r) itself (radius 0, raw depth sd); a depth that is not finite and > 0 makes the pair
 *     unobserved.  With u = sd - pd in float32 the pair contributes nothing when u < -trunc (the sample is hidden
 *     behind that view's surface); otherwise it contributes q = (int32) rintf(fminf(u, trunc) * k), k = 1024.0f / trunc
 *     formed once in float32.  Per sample S = the int32 sum of q, n = the int32 number of contributions.  A sample is
 *     valid when n >= min_weight and inside when S < 0 (S == 0 is outside).  Only integers are summed.
 *  3. Cubes and vertices.  The cube of sample s with cell g has the corners g + (a, b, c), a, b, c in {0, 1}, corner
 *     index a + 2b + 4c.  It exists when all eight corners are valid samples and is active when it exists and its
 *     corners' inside flags differ.  Each active cube gives one vertex; vertices are numbered in ascending s.
 *     Position: over the 12 edges (p, q) in the order (0,1) (2,3) (4,5) (6,7), (0,2) (1,3) (4,6) (5,7), (0,4) (1,5)
 *     (2,6) (3,7), an edge whose flags differ has, in float64, t = (double)(Sp*nq) / ((double)(Sp*nq) - (double)(Sq*np))
 *     (products exact in int64) and the crossing = corner p's offset + t along the edge's axis; L = the float64 sum of
 *     the crossings in edge order, per axis, divided by their number; the position is per axis
 *     (float)((double)o + (((double)g + 0.5) + L) * (double)voxel_size).
 *     Normal: f = (double)S / (1024.0 * (double)n); G_axis = the float64 sum, in edge order over the axis's four
 *     edges, of f(q) - f(p); the normal is (float)(G / sqrt(Gx*Gx + Gy*Gy + Gz*Gz)), the sum taken left to right, and
 *     zero when G is zero.  It points into free space.
 *     Colour: over the corners that remember an entry, in corner order, the float64 sum of the entries' three colour
 *     floats divided by their number, rounded to float32; with no such corner (128, 128, 128), and the vertex counts in
 *     *n_uncoloured.
 *  4. Faces.  For each sample s in order and each axis a = 0, 1, 2, with s' the sample at g + e_a: s and s' must both be
 *     valid with differing inside flags, and with b = (a+1)%3, c = (a+2)%3 the four cubes at g - u e_b - v e_c, (u, v) =
 *     Q0 (0,0), Q1 (1,0), Q2 (1,1), Q3 (0,1), must all exist (they are then active).  The pair emits the triangles
 *     (Q0,Q1,Q2), (Q0,Q2,Q3) when s is inside and (Q0,Q3,Q2), (Q0,Q2,Q1) when s' is: counter-clockwise seen from free
 *     space.  Faces are int32 vertex indices, listed in ascending (s, a).
 * *n_vertices, *n_faces (triangles), *n_samples, *n_valid (valid samples), *n_cubes (cubes that exist) and
 * *n_uncoloured may each be NULL.  Every atomic of the device is an integer add or a minimum, and nothing a reader can
 * see depends on which slot of the sample table a cell got.
 *
 * ACMMP_ERR_INVALID_ARGUMENT: a source that is none of the three constants, no such source result (an empty one gives
 * an empty mesh), n_list outside [1, 4096], a view index outside the set or a view never given to
 * acmmp_fusion_set_view, trunc not finite or <= 0, min_weight < 1, more than 2^31 - 1 vertices.  The mesh result stays
 * in HBM until the next successful mesh call replaces it or its source is replaced or discarded (as the visible
 * result's; a successful acmmp_fusion_voxel_visibility discards a mesh of the visible result);
 * acmmp_fusion_set_view does not touch it.  The render, the surface and the sample result (acmmp_fusion_mesh_sample)
 * go with the mesh result they were computed on.  Any error -- an out-of-memory part-way and a full sample table
 * (ACMMP_ERR_HIP) included -- leaves the object as it was (the new result is built beside the previous one).
 * Device memory: 8 bytes per entry held with the clean and the visible result (the voxel index) and 8 per entry
 * while the call runs; the sample table, 32 bytes per slot with the smallest power of two >= max(54 ne, 1024) slots
 * (27 cells per entry, at most half full), while the call runs; 24 bytes per sample (cell, S, n, entry), 36 per vertex
 * and 12 per face held with the result; 6 bytes per sample, and 4 bytes of flag per lane of a compaction segment (at
 * most 2^30 lanes), while it runs.  The host waits three times: for the sample count, for the vertex and face counts,
 * and at the end. */
#define ACMMP_MESH_FROM_VOXELS 0    /* entries = the voxel result */
#define ACMMP_MESH_FROM_CLEAN 1     /* entries = the clean result's kept voxels */
#define ACMMP_MESH_FROM_VISIBLE 2   /* entries = the visible result's kept entries */
acmmp_status acmmp_fusion_voxel_mesh(acmmp_fusion *f, int source, int n_list, const int *views, float trunc,
                                     int min_weight, int64_t *n_vertices, int64_t *n_faces, int64_t *n_samples,
                                     int64_t *n_valid, int64_t *n_cubes, int64_t *n_uncoloured);
/* Vertices [first, first + n) of the mesh result: n x 9 floats (position, normal, colour: a cloud point's layout). */
acmmp_status acmmp_fusion_mesh_vertices(acmmp_fusion *f, int64_t first, int64_t n, float *vertices);
/* Triangles [first, first + n) of the mesh result: n x 3 int32 vertex indices. */
acmmp_status acmmp_fusion_mesh_faces(acmmp_fusion *f, int64_t first, int64_t n, int32_t *faces);
/* Test hook: samples [first, first + n) of the mesh result to host arrays, any of which may be NULL: cells n x 3 int32
 * (gx, gy, gz), tsdf n x 2 int32 (S, n), entry n int64 (the remembered entry, -1 = none). */
acmmp_status acmmp_fusion_mesh_samples(acmmp_fusion *f, int64_t first, int64_t n, int32_t *cells, int32_t *tsdf,
                                       int64_t *entry);
/* Test hook, as acmmp_fusion_voxel_table for the sample table.  force_slots = 0: automatic size; otherwise the size of
 * the next mesh call's table, a power of two >= 64 (else that call returns ACMMP_ERR_INVALID_ARGUMENT); one too small
 * for the samples makes that call fail with ACMMP_ERR_HIP.  The outputs describe the last successful mesh call. */
acmmp_status acmmp_fusion_mesh_table(acmmp_fusion *f, int64_t force_slots, int64_t *slots, int64_t *occupied,
                                     int64_t *max_probe, int64_t *wrapped);

/* A host mesh becomes the mesh result, as acmmp_fusion_set_scene does for clouds: vertices nv x 9 floats (position,
 * normal, colour), faces nf x 3 int32 vertex indices.  ACMMP_ERR_INVALID_ARGUMENT: a count below 0 or beyond 2^31 - 1,
 * an index outside [0, nv), a NULL array of a count above 0; any error leaves the object as it was.  Such a mesh has no
 * source and no samples (acmmp_fusion_mesh_samples sees none): it lives until the next successful
 * acmmp_fusion_voxel_mesh or acmmp_fusion_set_mesh, whatever happens to the scene, voxel, clean and visible results. */
acmmp_status acmmp_fusion_set_mesh(acmmp_fusion *f, int64_t nv, const float *vertices, int64_t nf, const int32_t *faces);

/* ---- the mesh result rendered into a view: z-buffer depth, face, normal and colour maps (no reference counterpart) ----
 * acmmp_fusion_mesh_render renders the mesh result into one camera, pinhole or SPHERE.  All arithmetic is IEEE float64
 * with no contraction, on inputs widened from float32, unless float32 is said.
 *  1. Camera.  View i's own camera, or with view == -1 the camera `cam`, of the set's model.  W x H, the map's size,
 *     are the camera's.
 *  2. Vertices in the camera frame.  For a vertex X and k = 0, 1, 2: T_k = ((R[3k]*X.x + R[3k+1]*X.y) + R[3k+2]*X.z) +
 *     t[k].  A face with a non-finite camera-frame coordinate is skipped, and so is, for the pinhole model, a face with
 *     any T_z <= 0 (there is no near-plane clipping); *n_skipped counts them.
 *  3. Ray of pixel (c, r).  Pinhole: d = (((double)c - K[2]) / K[0], ((double)r - K[5]) / K[4], 1).  SPHERE: the float32
 *     PixelToDir of the engine (lon = ((c - cx) / W * 2) * pi_f, lat = (-(r - cy) / H) * pi_f in float32, pi_f =
 *     3.141592654f, the deterministic sine and cosine, d = (cos lat * sin lon, -sin lat, cos lat * cos lon)), widened.
 *  4. Hit test.  For a face (A, B, C) in the camera frame u = d.(B x C), v = d.(C x A), w = d.(A x B), the cross product
 *     (b_y c_z - b_z c_y, b_z c_x - b_x c_z, b_x c_y - b_y c_x), the dot product (d_x n_x + d_y n_y) + d_z n_z, and
 *     s = (u + v) + w.  The ray hits when (s > 0 and u, v, w >= 0) or (s < 0 and u, v, w <= 0), and P.d > 0 for
 *     P = ((u*A + v*B) + w*C) / s per component.  A shared edge gives exactly negated products to its two faces: a ray
 *     on the edge hits both, a ray beside it one of them, and the rendering has no cracks.
 *  5. Depth.  Pinhole P_z, SPHERE sqrt((P_x^2 + P_y^2) + P_z^2); md is that value rounded to float32, and the hit counts
 *     only when md is finite and > 0.
 *  6. Winner.  Per pixel the smallest key (bits(md) << 32) | face index over all faces of the mesh that hit: equal
 *     depths go to the lower face index.  The definition is exhaustive over faces and pixels; the device tests a face
 *     against a conservative bound of its pixels only.
 *  7. Outputs per pixel.  depth: md, 0 where nothing hits.  face: int32, -1 where nothing hits.  normal: N =
 *     ((u*nA + v*nB) + w*nC) / s per component, then N / sqrt((N_x^2 + N_y^2) + N_z^2) rounded to float32, zero unless
 *     that length is > 0; it is in world space, as the .dmb normals are.  colour: ((u*cA + v*cB) + w*cC) / s per
 *     component, rounded to float32.  Both are zero where nothing hits.  A winner is back-facing when s > 0: faces are
 *     counter-clockwise seen from free space, and a camera in free space has s < 0.
 *  8. Agreement, for view >= 0 (with view == -1 all seven counts are 0).  sd = the view's raw depth at the pixel as
 *     uploaded; one that is not finite and > 0 is absent.  In float32 t = rel_tol * sd.  counts[0] agree: both present
 *     and fabsf(md - sd) <= t; [1] mesh in front: both, md < sd, not agree; [2] mesh behind: both, neither of those;
 *     [3] mesh only; [4] raw only; [5] neither; they sum to W * H.  counts[6]: the winners that are back-facing.
 * counts and n_skipped may be NULL.  One render result is resident at a time (acmmp_fusion_render_maps reads it); it
 * is built beside the previous one and any error leaves the object as it was; it is discarded when the mesh result is
 * replaced or discarded; acmmp_fusion_set_view does not touch it.  ACMMP_ERR_INVALID_ARGUMENT: no mesh result, a view
 * outside the set (below -1 included) or never given to acmmp_fusion_set_view, view == -1 with a NULL camera, a camera
 * of another model or with a non-positive size, rel_tol not finite or < 0.  ACMMP_ERR_UNSUPPORTED: more than 2^31 - 1
 * pixels or faces.  Every atomic of the device is an integer minimum or add, and nothing a reader can see depends on
 * the order in which faces are taken.  Device memory: 32 bytes per pixel held with the result (depth, face, normal,
 * colour); 8 bytes per pixel (the keys) and 20 per face (the queue of large faces) while the call runs.  The host
 * waits once, at the end, for the counts. */
acmmp_status acmmp_fusion_mesh_render(acmmp_fusion *f, int view, const acmmp_camera *cam, float rel_tol,
                                      int64_t counts[7], int64_t *n_skipped);
/* The render result to host arrays, any of which may be NULL: depth W x H floats, face W x H int32, normal and colour
 * W x H x 3 floats, row-major.  ACMMP_ERR_INVALID_ARGUMENT without a render result. */
acmmp_status acmmp_fusion_render_maps(acmmp_fusion *f, float *depth, int32_t *face, float *normal, float *colour);
/* Test hook.  A face whose bound holds at most small_max candidate pixels is rendered by its own lane, the others by a
 * workgroup each.  small_max = 0 restores the default threshold (256); any other value is the threshold of the renders
 * that follow (below 0: every face is large).  The outputs, each of which may be NULL, describe the last successful
 * render: faces rendered by their own lane, faces queued, candidate pixels over all faces that were not skipped. */
acmmp_status acmmp_fusion_render_plan(acmmp_fusion *f, int small_max, int64_t *n_small, int64_t *n_large,
                                      int64_t *n_candidates);

/* ---- nearest-neighbour distances between a resident cloud and a reference cloud: accuracy and completeness (no
 * reference counterpart) ----
 * acmmp_fusion_set_reference_cloud makes n >= 0 host points, 3 floats each and taken bit for bit, the object's reference
 * cloud: ground truth, or the cloud of another run.  It lives until the next successful call replaces it; no other call
 * touches it.  ACMMP_ERR_INVALID_ARGUMENT: n < 0 or above 2^31 - 1, a NULL array with n > 0.  Any error leaves the object
 * as it was; a success discards the distance result.  Device memory: 12 bytes per point.
 *
 * acmmp_fusion_cloud_distance measures the resident data cloud `source` against the reference cloud.  The data cloud is
 * the first three floats of the scene points (ACMMP_DIST_FROM_SCENE), of the voxel result (_VOXELS), of the clean
 * result's kept voxels (_CLEAN), of the visible result's kept entries (_VISIBLE), of the mesh vertices (_MESH) or of the mesh's
 * samples (_SAMPLES, acmmp_fusion_mesh_sample), in their order.  With ACMMP_DIST_DATA_TO_REF the queries are the data cloud and the targets the reference cloud (accuracy); with
 * ACMMP_DIST_REF_TO_DATA it is the reverse (completeness).  The definition is exhaustive over the pairs, in plain IEEE
 * arithmetic with no contraction:
 *  1. Validity.  A point is valid when its three coordinates are finite.  Invalid queries are neither matched nor counted
 *     as valid; invalid targets do not exist.
 *  2. Pair distance, in float32: dx = qx - tx, dy = qy - ty, dz = qz - tz, d2 = (dx*dx + dy*dy) + dz*dz.
 *  3. Nearest.  A valid query takes the smallest key (bits(d2) << 32) | j over all valid targets j: equal distances go to
 *     the lower target index.  d2 may be +inf; it is never NaN for valid points.
 *  4. Match.  The query is matched when the winner's d2 <= m2, m2 = max_dist * max_dist formed once in float32.  Per query
 *     the result is d2, +inf when the query is unmatched, invalid or has no target, and nearest as int32, -1 in the same
 *     cases.
 *  5. Summary.  Only integers are summed.  summary[ACMMP_DIST_SUMMARY_WORDS] holds int64 words: [0] n_query, [1] n_valid,
 *     [2] n_matched, [3] sum_q = the sum over the matched queries of q = (int64) rint(sqrt((double)d2) * k) with
 *     k = 1048576.0 / (double)max_dist, [4 .. 12) within[i] = the matched queries with d2 <= tau[i] * tau[i], the product
 *     formed in float32 (entries from n_tau on are 0), [12 .. 268) hist[b] = the matched queries with min(q >> 12, 255) == b.
 *     summary may be NULL; tau may be NULL when n_tau is 0.
 * The device searches a uniform grid of the targets ring by ring and skips a pair only where it can prove that the pair
 * loses or is unmatched; every atomic is an integer add, a minimum or a maximum, and no result depends on
 * the grid, on the order of a cell's list or on the order the atomics land in.
 *
 * ACMMP_ERR_INVALID_ARGUMENT: a source or a direction that is none of the constants, no such data result (an empty one is
 * a valid input), no reference cloud (an empty one is valid), max_dist not finite or <= 0, n_tau outside [0, 8], a NULL tau
 * with n_tau > 0, a tau[i] that is not finite, < 0 or > max_dist, a forced cell that is not finite and > 0
 * (acmmp_fusion_distance_grid).  ACMMP_ERR_UNSUPPORTED: more than 2^31 - 1 targets.  No query gives zeros; no target
 * leaves every query unmatched.  One distance result is resident at a time (acmmp_fusion_distance_results reads it); it is
 * built beside the previous one, and any error -- an out-of-memory part-way included -- leaves the object as it was.  It is
 * discarded when its data source is replaced or discarded -- the scene result by acmmp_fusion_run_scene and
 * acmmp_fusion_set_scene, the others by the rules the visible and the mesh result follow, a successful call that replaces
 * the source included -- and when the reference cloud is replaced; acmmp_fusion_set_view does not touch it.  The source
 * results and the reference cloud are never modified.
 * Device memory: 8 bytes per query held with the result (d2, nearest); while the call runs, with S = the smallest power
 * of two >= max(2 T, 1024) for T targets, 16 bytes per slot of the cell table, 8 per slot of the coarse table and 16 per
 * target (the cells' lists: position and index).  The host waits twice: for the targets' bounding box and valid count, from
 * which it chooses the cell, and at the end.  The lists are sized from the target count, so nothing waits for the number
 * of occupied cells. */
#define ACMMP_DIST_FROM_SCENE 0     /* data cloud = the scene result's points */
#define ACMMP_DIST_FROM_VOXELS 1    /* the voxel result */
#define ACMMP_DIST_FROM_CLEAN 2     /* the clean result's kept voxels */
#define ACMMP_DIST_FROM_VISIBLE 3   /* the visible result's kept entries */
#define ACMMP_DIST_FROM_MESH 4      /* the mesh result's vertices */
#define ACMMP_DIST_FROM_SAMPLES 6   /* the sample result's points (acmmp_fusion_mesh_sample); 5 is ACMMP_SURF_FROM_REFERENCE */
#define ACMMP_DIST_DATA_TO_REF 0    /* queries = data cloud, targets = reference cloud: accuracy */
#define ACMMP_DIST_REF_TO_DATA 1    /* queries = reference cloud, targets = data cloud: completeness */
#define ACMMP_DIST_MAX_TAU 8
#define ACMMP_DIST_HIST_BINS 256
#define ACMMP_DIST_SUMMARY_N_QUERY 0
#define ACMMP_DIST_SUMMARY_N_VALID 1
#define ACMMP_DIST_SUMMARY_N_MATCHED 2
#define ACMMP_DIST_SUMMARY_SUM_Q 3
#define ACMMP_DIST_SUMMARY_WITHIN 4
#define ACMMP_DIST_SUMMARY_HIST 12
#define ACMMP_DIST_SUMMARY_WORDS 268
acmmp_status acmmp_fusion_set_reference_cloud(acmmp_fusion *f, int64_t n, const float *xyz);
acmmp_status acmmp_fusion_cloud_distance(acmmp_fusion *f, int source, int direction, float max_dist, int n_tau,
                                         const float *tau, int64_t *summary);
/* Results of queries [first, first + n) of the distance result to host arrays, either of which may be NULL: d2 n floats,
 * nearest n int32.  Ranges as acmmp_fusion_voxel_points (no distance result: every range but an empty one at 0 is
 * refused). */
acmmp_status acmmp_fusion_distance_results(acmmp_fusion *f, int64_t first, int64_t n, float *d2, int32_t *nearest);
/* Test hook, in the spirit of acmmp_fusion_voxel_table.  force_cell = 0: the cell of the search grid is chosen from the
 * targets' bounding box and number; otherwise it is the cell of the distance calls that follow (enlarged where the
 * targets' extent would need more than 2^20 cells on an axis), and one that is not finite and > 0 makes the next distance
 * call return ACMMP_ERR_INVALID_ARGUMENT.  The outputs, each of which may be NULL, describe the last successful distance
 * call: the cell used, the occupied cells, the longest cell list and the largest ring a query searched.  They are
 * informational: no result depends on them. */
acmmp_status acmmp_fusion_distance_grid(acmmp_fusion *f, float force_cell, float *cell, int64_t *cells, int64_t *max_list,
                                        int64_t *rings);

/* ---- registration of the data cloud to the reference cloud: a transform and ICP (no reference counterpart) ----
 * acmmp_fusion_set_cloud_transform gives the object a row-major 3x4 float64 matrix M; NULL clears it.  While it is set,
 * acmmp_fusion_cloud_distance reads every data point (x, y, z) of every ACMMP_DIST_FROM_* source, in both directions, as
 * x', per row k:
 *   x'_k = (float)(((M[4k] * (double)x + M[4k+1] * (double)y) + M[4k+2] * (double)z) + M[4k+3]),
 * IEEE float64 with no contraction, rounded once to float32; step 1 of the distance definition (validity) then applies to
 * x'.  The reference cloud is never transformed and the source results are never modified.  The transform belongs to the
 * object, not to a source: it lives until it is cleared or replaced, and no other call touches it.  A successful set or
 * clear discards the distance result, as replacing the reference cloud does.  ACMMP_ERR_INVALID_ARGUMENT: an entry that
 * is not finite; an error leaves the object as it was.  acmmp_fusion_get_cloud_transform copies M out (is_set 0: the
 * identity); either output may be NULL.
 *
 * acmmp_fusion_cloud_align registers the data cloud `source` to the reference cloud by iterated closest points and returns
 * the transform in M_out; it neither reads nor writes the transform that has been set (the caller installs M_out with
 * acmmp_fusion_set_cloud_transform).  init = M_0, NULL for the identity.  Iteration k = 0, 1, ... under M_k:
 *  1. Queries.  The data points i with i % stride == 0, read as x'_i under M_k as above.  The targets are the valid
 *     reference points.  Nearest and match are steps 1 to 4 of acmmp_fusion_cloud_distance with max_dist: the float32 d2,
 *     the (bits(d2) << 32 | j) key, the cap m2.
 *  2. Quantisation, in float64.  c = the per-axis minimum of the valid targets (0 with none), kq = 65536.0 /
 *     (double)max_dist.  For a matched pair P_a = (int64) rint(((double)x'_a - c_a) * kq) and Q_a the same of the target.
 *     The pair is in range when every |P_a| and |Q_a| is < 2^30; otherwise it counts in n_out_of_range and enters no
 *     moment.
 *  3. Record.  ACMMP_ALIGN_RECORD_WORDS int64 words, only integers are summed: n_query (the queries of step 1), n_valid,
 *     n_matched and sum_q exactly as the distance summary forms them; n_out_of_range; N = the matched pairs in range;
 *     over those pairs the sums of P_a (3 words) and of Q_a (3 words); for each of the nine products w = P_a * Q_b, at
 *     ACMMP_ALIGN_RECORD_PQ + 2 (3 a + b), the sum of w >> 32 (arithmetic shift) and then the sum of w & 0xffffffff; the
 *     same two sums of w = P_x^2 + P_y^2 + P_z^2 at ACMMP_ALIGN_RECORD_PP.  The true sum of a product is hi * 2^32 + lo.
 *     Nothing overflows for up to 2^31 - 1 pairs: |P_a|, |Q_b| < 2^30 give |w| < 2^60 (< 2^62 for the three squares), so
 *     |w >> 32| < 2^30 and its sum is < 2^61; 0 <= w & 0xffffffff < 2^32 and its sum is < 2^63; |sum of P_a| < 2^61.
 *  4. Fit.  The host solves in exact 128-bit integers, then float64.  A_ab = N * sum(P_a Q_b) - sum(P_a) * sum(Q_b),
 *     exact because |A_ab| < 2^123; H_ab = (double)A_ab / ((double)N * (double)N); var = (double)(N * sum|P|^2 -
 *     |sum P|^2) / ((double)N * (double)N).  H = U diag(d) V^T with d0 >= d1 >= d2 >= 0, g = sign det(V U^T),
 *     R = V diag(1, 1, g) U^T, s = (d0 + d1 + g d2) / var for ACMMP_ALIGN_SIMILARITY and 1 for ACMMP_ALIGN_RIGID,
 *     D = (s R | t) with t = (c + Qm / kq) - s R (c + Pm / kq), Pm = sum P / N, Qm = sum Q / N.  The iteration is
 *     degenerate when N < 3, var is 0 or d1 <= d0 * 2^-40 (collinear pairs): the call ends with ACMMP_ALIGN_DEGENERATE
 *     and M_out = M_k.
 *  5. Step.  M_{k+1} = D o M_k, per entry (D_a0 * M_0b + D_a1 * M_1b) + D_a2 * M_2b, plus D_a3 in the last column.
 *     shift = the largest float64 Euclidean |D c' - c'| over the eight corners c' of the valid targets' bounding box.  The
 *     call stops with ACMMP_ALIGN_CONVERGED when shift <= min_shift, else with ACMMP_ALIGN_MAX_ITERATIONS after
 *     max_iterations iterations.  M_out = the last M.
 * n_iterations = the iterations that ran; M_out, n_iterations and stop_reason may each be NULL.
 * acmmp_fusion_align_records reads iterations [first, first + n) of the last successful align call: per iteration the
 * ACMMP_ALIGN_RECORD_WORDS words, the 12 doubles of the M_k it ran under, and its shift (0 for a degenerate iteration);
 * each array may be NULL.  Ranges as acmmp_fusion_distance_results (no records: every range but an empty one at 0 is
 * refused).  The records follow the distance result's lifetime rules with respect to the source and
 * the reference cloud; the cloud transform and acmmp_fusion_set_view do not touch them, and an align call does not touch
 * the distance result.
 *
 * ACMMP_ERR_INVALID_ARGUMENT: a source or a mode that is none of the constants, no such data result (an empty one is
 * valid and degenerate), no reference cloud, max_dist not finite or <= 0, max_iterations outside [1, 1024], stride < 1,
 * min_shift not finite or < 0, an init entry that is not finite, a forced cell that is not finite and > 0.
 * ACMMP_ERR_UNSUPPORTED: more than 2^31 - 1 targets.  Any error -- an out-of-memory part-way included -- leaves the object
 * as it was.  acmmp_fusion_distance_grid's forced cell applies to align calls too, and its outputs describe the last
 * successful distance or align call.
 * The grid over the targets is built once per call and serves every iteration; an iteration is one launch, which reduces
 * its words over the wave and the workgroup and issues one integer atomic add per word per workgroup, so no result
 * depends on the order of execution.  Device memory: a distance call's scratch (no per-query array) and the 32 words.
 * The host waits once for the targets' bounding box and once per iteration for the words. */
#define ACMMP_ALIGN_RIGID 0
#define ACMMP_ALIGN_SIMILARITY 1
#define ACMMP_ALIGN_MAX_ITERATIONS 0   /* stop_reason: max_iterations iterations ran */
#define ACMMP_ALIGN_CONVERGED 1        /* shift <= min_shift */
#define ACMMP_ALIGN_DEGENERATE 2       /* step 4 could not fit */
#define ACMMP_ALIGN_RECORD_N_QUERY 0
#define ACMMP_ALIGN_RECORD_N_VALID 1
#define ACMMP_ALIGN_RECORD_N_MATCHED 2
#define ACMMP_ALIGN_RECORD_SUM_Q 3
#define ACMMP_ALIGN_RECORD_N_OUT_OF_RANGE 4
#define ACMMP_ALIGN_RECORD_N 5
#define ACMMP_ALIGN_RECORD_SUM_P 6     /* 3 words */
#define ACMMP_ALIGN_RECORD_SUM_Q3 9    /* 3 words: the sums of Q_a */
#define ACMMP_ALIGN_RECORD_PQ 12       /* 18 words: (hi, lo) of P_a Q_b at + 2 (3 a + b) */
#define ACMMP_ALIGN_RECORD_PP 30       /* 2 words: (hi, lo) of |P|^2 */
#define ACMMP_ALIGN_RECORD_WORDS 32
acmmp_status acmmp_fusion_set_cloud_transform(acmmp_fusion *f, const double M[12]);
acmmp_status acmmp_fusion_get_cloud_transform(const acmmp_fusion *f, double M[12], int *is_set);
acmmp_status acmmp_fusion_cloud_align(acmmp_fusion *f, int source, int mode, float max_dist, int max_iterations,
                                      int stride, double min_shift, const double init[12], double M_out[12],
                                      int *n_iterations, int *stop_reason);
acmmp_status acmmp_fusion_align_records(acmmp_fusion *f, int64_t first, int64_t n, int64_t *words, double *M,
                                        double *shift);

/* ---- point-to-plane registration: the data cloud's own normals (no reference counterpart) ----
 * acmmp_fusion_cloud_align_plane refines a transform by iterated closest points with a point-to-plane residual.  Two
 * independent samplings of one surface never hold the same points, and the point-to-point fit above then slides along
 * the surface; a residual measured along the normal does not.  The fit is rigid only: scale is poorly determined by
 * plane residuals and does not fit the integer budget of step 3, so a similarity frame is found by
 * acmmp_fusion_cloud_align first and its M_out is this call's init (NULL: the identity).  The normal of data point i is
 * floats 3..5 of that point, which every ACMMP_DIST_FROM_* source holds; the reference cloud stays xyz only.  The call
 * neither reads nor writes the transform that has been set.
 * Before iteration 0 the call launches one pass of acmmp_fusion_cloud_align's iteration under M_0, which is not an
 * iteration: it is not recorded and takes no step; the pivot g_0 is taken from its words SUM_Q3 and N as in step 6 (0
 * when N is 0).  Iteration k = 0, 1, ... under M_k with the pivot g_k (three int64):
 *  1. Queries and matching.  Exactly step 1 of acmmp_fusion_cloud_align: every stride-th data point read as x' under M_k,
 *     the float32 d2, the (bits(d2) << 32 | j) key, the cap m2.
 *  2. Normal, in float64 with no contraction.  With (nx, ny, nz) the data point's normal as doubles,
 *     u_a = (M[4a] * nx + M[4a+1] * ny) + M[4a+2] * nz, l2 = (u0*u0 + u1*u1) + u2*u2.  The normal is usable when nx, ny, nz
 *     are finite and l2 is finite and > 0; then Nn_a = (int64) rint(u_a / sqrt(l2) * 4096.0), so |Nn_a| <= 4096.  For a
 *     rigid or similarity M_k this is the rotated unit normal; for any other init it is still the definition.
 *  3. Quantisation.  c, kq, P_a and Q_a as in step 2 of acmmp_fusion_cloud_align.  The pair is in range when every |P_a|,
 *     every |Q_a| and every |Q_a - g_a| is < 2^30; otherwise it counts in n_out_of_range.  An in-range pair whose normal
 *     is unusable counts in n_no_normal; N counts the rest, and only those enter the moments.  The lever is
 *     L_a = (Q_a - g_a) >> 12 (arithmetic shift), so |L_a| <= 2^18 and one lever step is max_dist / 16.  D_a = P_a - Q_a.
 *     |D_a| < 2^17 for a matched pair: d2 <= m2 in float32 gives, per axis, |x'_a - t_a| <= max_dist (1 + 2^-22) -- m2 and
 *     d2 are each within a few float32 roundings of the exact products, the float32 difference x'_a - t_a is within
 *     2^-24 relative of the exact one -- so |(x'_a - t_a) kq| <= 65536 (1 + 2^-22) < 65537, and the two rint add at most
 *     one lattice step: |D_a| <= 65538 < 2^17.  (This needs m2 to be a normal float32, max_dist >= 2^-60; below that a
 *     product can underflow to 0 <= m2 for a pair further apart than max_dist, and the words are then sums modulo 2^64.)
 *     Row c = (L x Nn, Nn), six int64: c_0 = L_1 Nn_2 - L_2 Nn_1, c_1 = L_2 Nn_0 - L_0 Nn_2, c_2 = L_0 Nn_1 - L_1 Nn_0,
 *     c_{3+a} = Nn_a.  Residual r = (D_0 Nn_0 + D_1 Nn_1) + D_2 Nn_2.  |c_a| < 2^31: a quantised unit normal cannot have
 *     two components of 4096 -- |Nn| <= 4096 + sqrt(3)/2, so |Nn_1| + |Nn_2| <= sqrt(2) |Nn| < 5795 -- and
 *     |c_0| <= 2^18 (|Nn_1| + |Nn_2|) < 2^18 * 8192.  |r| <= |D| |Nn| < sqrt(3) * 65538 * 4097 < 2^29.  So every product
 *     of two of c_0..c_5, r is < 2^62 in magnitude: it fits int64, its >> 32 is < 2^30 in magnitude and sums below 2^61
 *     over up to 2^31 - 1 pairs, and its & 0xffffffff sums below 2^63.
 *  4. Record.  ACMMP_ALIGN_PLANE_RECORD_WORDS int64 words, only integers are summed: [0..4) n_query, n_valid, n_matched,
 *     sum_q as acmmp_fusion_cloud_align's record forms them; [4] n_out_of_range; [5] n_no_normal; [6] N; [7..10) the sums
 *     of Q_a over the N pairs; [10..13) g_k, written by the host as n_query is; [13] 0; [14..56) for the 21 pairs a <= b of
 *     c_a c_b in row-major order (00, 01, .., 05, 11, .., 55), the sum of w >> 32 and then the sum of w & 0xffffffff;
 *     [56..68) the same two sums of c_a r for a = 0..5; [68..70) of r r.  The true sum of a product is hi * 2^32 + lo.
 *  5. Fit.  The host joins the split sums in 128-bit integers, then float64.  S_ab = (double) sum(c_a c_b),
 *     b_a = -(double) sum(c_a r).  Jacobi scaling: s_a = sqrt(S_aa), S'_ab = S_ab / (s_a s_b), b'_a = b_a / s_a (the
 *     rotation and the translation columns differ by 2^19 in unit).  S' = sum_i lambda_i v_i v_i^T by cyclic Jacobi
 *     rotations.  The iteration is degenerate when N < 6, any S_aa is 0, or lambda_min <= lambda_max * 2^-40 -- the rule of
 *     acmmp_fusion_cloud_align for collinear pairs; a single plane and a cylinder along an axis are degenerate by it.
 *     Noise floor: the lever's shift rounds (Q_a - g_a) / 4096 down by e_a in [0, 1); the mean of e x Nn is a combination
 *     of the normal columns, which tau absorbs, and the rest has variance |Nn|^2 / 18 per rotation column, so over the
 *     pairs the rounding alone puts F = ((S_33 + S_44) + S_55) / 18 on the rotation block's diagonal.  With P the rotation
 *     block of S^-1, P_ab = (sum_i v_i[a] v_i[b] / lambda_i) / (s_a s_b) for a, b < 3 -- the inverse of what the
 *     translation columns leave unexplained of the rotation columns -- and mu its largest eigenvalue (cyclic Jacobi), the
 *     iteration is also degenerate unless 1 > 4 F mu: a rotation that rests on less than four times the levers' rounding
 *     is not determined.  This is what makes a sphere at its correspondences degenerate: its rotation columns
 *     (q - G) x n vanish up to that rounding, which the scaling would otherwise normalise to unit diagonal.
 *     x' = sum_i v_i (v_i . b') / lambda_i, x_a = x'_a / s_a, omega = x_{0..2} / 4096, tau = x_{3..5} / kq: in lattice units
 *     the linearised residual of a pair is r + c . x.  R = I + A K + B K^2 with K = [omega]x, theta2 =
 *     |omega|^2, theta = sqrt(theta2); A = sin(theta) / theta, B = (1 - cos(theta)) / theta2 when theta2 >= 2^-40, else
 *     A = 1 - theta2 / 6, B = 0.5 - theta2 / 24.  G_a = c_a + g_a / kq (c the lattice's corner of step 3), and
 *     D = (R | G + tau - R G).
 *  6. Pivot.  g_{k+1,a} = floor((2 * sumQ_a + N) / (2 * N)), a floor division in integers, from iteration k's words [7..10)
 *     and [6].  The pivot keeps the float64 solve well conditioned when a few far targets stretch the box; it changes
 *     only what tau means, never the exactness of the integer definition.
 *  7. Step and stop.  Exactly step 5 of acmmp_fusion_cloud_align: M_{k+1} = D o M_k, shift over the eight corners of the
 *     valid targets' box, ACMMP_ALIGN_CONVERGED when shift <= min_shift, ACMMP_ALIGN_MAX_ITERATIONS after max_iterations,
 *     ACMMP_ALIGN_DEGENERATE (M_out = M_k, shift 0) for a degenerate iteration or a step that is not finite.
 * acmmp_fusion_align_plane_records reads the iterations of the last successful plane call as acmmp_fusion_align_records
 * does for a point call, ACMMP_ALIGN_PLANE_RECORD_WORDS words per iteration.  The object holds the records of the last
 * successful align call of either kind: a plane call discards the point records (acmmp_fusion_align_records then refuses
 * as with none) and a point call discards the plane records; otherwise the plane records follow the point records' rules
 * with respect to the source, the reference cloud, the transform and acmmp_fusion_set_view.  Neither call touches the
 * distance result or the installed transform.
 * The argument checks (there is no mode), the stop reasons, "any error leaves the object as it was", the forced cell and
 * acmmp_fusion_distance_grid's outputs are acmmp_fusion_cloud_align's.  An iteration is one launch that reduces its words
 * over the wave and the workgroup and issues one integer atomic add per word per workgroup.  Device memory: a distance
 * call's scratch (no per-query array) and the 70 words.  The host waits for the targets' bounding box, for the pivot pass
 * and once per iteration. */
#define ACMMP_ALIGN_PLANE_RECORD_N_QUERY 0
#define ACMMP_ALIGN_PLANE_RECORD_N_VALID 1
#define ACMMP_ALIGN_PLANE_RECORD_N_MATCHED 2
#define ACMMP_ALIGN_PLANE_RECORD_SUM_Q 3
#define ACMMP_ALIGN_PLANE_RECORD_N_OUT_OF_RANGE 4
#define ACMMP_ALIGN_PLANE_RECORD_N_NO_NORMAL 5
#define ACMMP_ALIGN_PLANE_RECORD_N 6
#define ACMMP_ALIGN_PLANE_RECORD_SUM_Q3 7    /* 3 words: the sums of Q_a */
#define ACMMP_ALIGN_PLANE_RECORD_PIVOT 10    /* 3 words: g_k, host-written */
#define ACMMP_ALIGN_PLANE_RECORD_ZERO 13     /* 1 word: 0 */
#define ACMMP_ALIGN_PLANE_RECORD_CC 14       /* 42 words: (hi, lo) of c_a c_b, a <= b, row-major */
#define ACMMP_ALIGN_PLANE_RECORD_CR 56       /* 12 words: (hi, lo) of c_a r */
#define ACMMP_ALIGN_PLANE_RECORD_RR 68       /* 2 words: (hi, lo) of r r */
#define ACMMP_ALIGN_PLANE_RECORD_WORDS 70
acmmp_status acmmp_fusion_cloud_align_plane(acmmp_fusion *f, int source, float max_dist, int max_iterations,
                                            int stride, double min_shift, const double init[12], double M_out[12],
                                            int *n_iterations, int *stop_reason);
acmmp_status acmmp_fusion_align_plane_records(acmmp_fusion *f, int64_t first, int64_t n, int64_t *words, double *M,
                                              double *shift);

/* ---- point-to-triangle distances from a cloud to the mesh result's surface (no reference counterpart) ----
 * acmmp_fusion_surface_distance measures the points of the cloud `query` against the faces of the mesh result
 * (acmmp_fusion_voxel_mesh, acmmp_fusion_set_mesh).  ACMMP_SURF_FROM_REFERENCE: the queries are the reference cloud -- how
 * much of it lies within tau of the surface, which acmmp_fusion_cloud_distance with ACMMP_DIST_FROM_MESH can only say of the
 * vertices.  ACMMP_SURF_FROM_SCENE, _VOXELS, _CLEAN, _VISIBLE: the queries are the first three floats of each point of that
 * resident data cloud -- how far the mesh strays from the cloud it was extracted from.  The definition is exhaustive over
 * the (query, face) pairs, in plain IEEE arithmetic with no contraction:
 *  1. Frames.  With a reference query and a cloud transform set (acmmp_fusion_set_cloud_transform), every mesh vertex is
 *     read under M exactly as a data point of acmmp_fusion_cloud_distance is: float64, rounded once to float32.  With a
 *     data-cloud query neither side is transformed: both live in the data frame.  The reference cloud is never
 *     transformed.  The call never modifies the transform, the mesh or any source.
 *  2. Validity.  A query is valid when its three floats are finite; a face when its three vertices, after step 1, are
 *     finite.  Invalid queries are neither matched nor counted as valid; invalid faces do not exist, and
 *     acmmp_fusion_surface_plan's *n_skipped counts them.
 *  3. Pair distance of query p and face (A, B, C), in float64 on the float32 inputs widened, with
 *     dot(u, v) = (u_x v_x + u_y v_y) + u_z v_z: ap = p - A, bp = p - B, cp = p - C, ab = B - A, ac = C - A, bc = C - B;
 *     d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp);
 *     vc = d1*d4 - d3*d2, vb = d5*d2 - d1*d6, va = d3*d6 - d5*d4.  The offset e from the query to the closest point is,
 *     per component k, that of the first case that applies, in this order:
 *       d1 <= 0 && d2 <= 0:                               e = -ap
 *       d3 >= 0 && d4 <= d3:                              e = -bp
 *       vc <= 0 && d1 >= 0 && d3 <= 0:                    v = d1 / (d1 - d3), e_k = v*ab_k - ap_k
 *       d6 >= 0 && d5 <= d6:                              e = -cp
 *       vb <= 0 && d2 >= 0 && d6 <= 0:                    w = d2 / (d2 - d6), e_k = w*ac_k - ap_k
 *       va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0:      w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), e_k = w*bc_k - bp_k
 *       otherwise:                                        s = (va + vb) + vc, v = vb / s, w = vc / s,
 *                                                         e_k = (v*ab_k + w*ac_k) - ap_k
 *     Then the clamp: lo_k = min(-ap_k, -bp_k, -cp_k), hi_k the maximum of the same three,
 *     e_k = e_k < lo_k ? lo_k : (e_k > hi_k ? hi_k : e_k); a NaN passes through.  The clamp is the identity in exact
 *     arithmetic; it keeps the closest point inside the face's bounding box, which the device's skips rest on.  Finally
 *     D2 = (float)((e_x*e_x + e_y*e_y) + e_z*e_z).  A pair whose D2 is NaN is not a candidate (only a degenerate face
 *     produces one); D2 may be +inf.
 *  4. Nearest.  A valid query takes the smallest key (bits(D2) << 32) | j over the valid faces j that are candidates:
 *     equal distances go to the lower face index.
 *  5. Match, per-query results and summary: steps 4 and 5 of acmmp_fusion_cloud_distance with D2 for d2 -- m2, k, q,
 *     within, the histogram, the ACMMP_DIST_SUMMARY_* offsets and ACMMP_DIST_MAX_TAU.  nearest_face is -1 and d2 is +inf when
 *     the query is unmatched, invalid or has no candidate.
 * The device lists every valid face in every cell of a uniform grid that its vertex bounding box overlaps, except faces
 * that overlap more than small_max cells (64; acmmp_fusion_surface_plan), which go to one overflow list that every query
 * past the box reject tests in full.  A query walks the grid ring by ring and skips a face only where the bounds of
 * DESIGN.md §8 prove that it loses or is unmatched; a face met in several cells is evaluated again, which a key minimum
 * does not notice.  No result depends on the grid, on small_max or on the order the atomics land in.
 *
 * ACMMP_ERR_INVALID_ARGUMENT: a query that is none of the constants, no such query result (an empty one is valid; for
 * ACMMP_SURF_FROM_REFERENCE: no reference cloud), no mesh result (an empty one is valid), max_dist not finite or <= 0, n_tau
 * outside [0, 8], a NULL tau with n_tau > 0, a tau[i] that is not finite, < 0 or > max_dist, a forced cell that is not finite
 * and > 0 (acmmp_fusion_surface_grid).  ACMMP_ERR_UNSUPPORTED: more than
 * 2^31 - 1 faces or queries, more than 2^32 - 1 registrations.  No query gives zeros; no valid face leaves every query
 * unmatched.  One surface result is resident, separate from the distance result (acmmp_fusion_surface_results reads it); it
 * is built beside the previous one, and any error -- an out-of-memory part-way included -- leaves the object as it was.
 * It is discarded when the mesh result is replaced or discarded, when its query source is replaced or discarded, and, for
 * a reference query only, when the reference cloud is replaced or the transform is set or cleared.
 * acmmp_fusion_set_view, the align calls and acmmp_fusion_cloud_distance do not touch it, and this call touches neither
 * the distance result nor the align records.
 * Device memory: 8 bytes per query held with the result (d2, nearest_face); while the call runs, 48 bytes per
 * registration and per large face (the three vertices after step 1 and the face index, so that a query never gathers
 * vertices), and 16 bytes per slot of the cell table, S = the smallest power of two >= max(2 min(R, cells of the grid),
 * 1024) slots for R registrations.  The host waits three times: for the faces' bounding box and valid count, from which it
 * chooses the cell; for the plan (small faces, large faces, registrations), from which it sizes the table and the lists
 * exactly; and at the end. */
#define ACMMP_SURF_FROM_SCENE 0       /* queries = the scene result's points (the values of ACMMP_DIST_FROM_*) */
#define ACMMP_SURF_FROM_VOXELS 1      /* the voxel result */
#define ACMMP_SURF_FROM_CLEAN 2       /* the clean result's kept voxels */
#define ACMMP_SURF_FROM_VISIBLE 3     /* the visible result's kept entries */
#define ACMMP_SURF_FROM_REFERENCE 5   /* the reference cloud */
acmmp_status acmmp_fusion_surface_distance(acmmp_fusion *f, int query, float max_dist, int n_tau, const float *tau,
                                           int64_t *summary);
/* Results of queries [first, first + n) of the surface result to host arrays, either of which may be NULL: d2 n floats,
 * nearest_face n int32.  Ranges as acmmp_fusion_distance_results. */
acmmp_status acmmp_fusion_surface_results(acmmp_fusion *f, int64_t first, int64_t n, float *d2, int32_t *nearest_face);
/* Test hook, in the spirit of acmmp_fusion_render_plan.  small_max = 0: a face that overlaps more than 64 cells is a large
 * face; small_max > 0: more than small_max cells; small_max < 0: every face is large.  It holds for the surface calls
 * that follow.  The outputs, each of which may be NULL, describe the last successful surface call: the faces registered
 * in the grid, the large faces, the (face, cell) registrations, the invalid faces. */
acmmp_status acmmp_fusion_surface_plan(acmmp_fusion *f, int small_max, int64_t *n_small, int64_t *n_large,
                                       int64_t *n_registrations, int64_t *n_skipped);
/* Test hook: acmmp_fusion_distance_grid for the face grid of the surface calls, apart from it -- neither hook's forced
 * cell reaches the other's calls, and neither call changes what the other's hook reports.  force_cell = 0: the cell is
 * chosen from the valid faces' bounding box and number; otherwise it is the cell of the surface calls that follow
 * (enlarged where the extent would need more than 2^20 cells on an axis), and one that is not finite and > 0 makes the
 * next surface call return ACMMP_ERR_INVALID_ARGUMENT.  The outputs, each of which may be NULL, describe the last
 * successful surface call: the cell used, the occupied cells, the longest cell list and the largest ring a query
 * searched.  They are informational: no result depends on them. */
acmmp_status acmmp_fusion_surface_grid(acmmp_fusion *f, float force_cell, float *cell, int64_t *cells, int64_t *max_list,
                                       int64_t *rings);

/* ---- the mesh result's surface as an area-uniform cloud of samples (no reference counterpart) ----
 * acmmp_fusion_mesh_sample turns the faces of the mesh result (acmmp_fusion_voxel_mesh, acmmp_fusion_set_mesh) into
 * points spread over their area, about one per spacing^2: the cloud that "accuracy of the mesh" is measured on, where the
 * vertices (ACMMP_DIST_FROM_MESH) weigh a face by its corners and not by its size.  The samples are a resident cloud,
 * ACMMP_DIST_FROM_SAMPLES, of acmmp_fusion_cloud_distance (both directions), acmmp_fusion_cloud_align and
 * acmmp_fusion_cloud_align_plane (they carry normals); acmmp_fusion_surface_distance does not take them.  The definition
 * is over the faces f = 0 .. nf in their order.  All float arithmetic is IEEE float64 on inputs widened from float32, with
 * no contraction; every choice is made in integers, all 64-bit integer arithmetic is mod 2^64, and x >> s is the logical
 * shift.
 *  0. Constants.  mix(z): z += 0x9e3779b97f4a7c15; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9; z = (z ^ (z >> 27)) *
 *     0x94d049bb133111eb; the result is z ^ (z >> 31) (splitmix64's finaliser, which the voxel table hashes with).
 *     G1 = 0xC13FA9A902A6328F and G2 = 0x91E10DA5C79E7B1D: 2^64 / p and 2^64 / p^2 for the plastic number p (the R2
 *     lattice), the second rounded up to odd.
 *  1. Validity.  A face is valid when the nine position coordinates of its three vertices (A, B, C) are finite.  An
 *     invalid face has no samples; *n_skipped counts the invalid faces.
 *  2. Area.  E1 = B - A, E2 = C - A per component; N = (E1y*E2z - E1z*E2y, E1z*E2x - E1x*E2z, E1x*E2y - E1y*E2x);
 *     area = 0.5 * sqrt((Nx*Nx + Ny*Ny) + Nz*Nz).  It cannot overflow for float32 inputs; a degenerate face has area 0
 *     and is valid.
 *  3. Count.  e = area / ((double)spacing * (double)spacing).  With e >= 2^31 the face counts n_f = 2^31.  Otherwise
 *     k = floor(e), r = e - k, T = (uint64)(r * 9007199254740992.0), h_f = mix(seed ^ mix((uint64) f)) and
 *     n_f = k + ((h_f >> 11) < T ? 1 : 0): the expected count is e, so faces smaller than spacing^2 are sampled in
 *     proportion to their area and not dropped.
 *  4. Total.  N = the 64-bit sum of n_f.  N > 2^31 - 1 is ACMMP_ERR_UNSUPPORTED (the distance calls take at most that
 *     many targets); it is known before any output is allocated.
 *  5. Sample j of face f, 0 <= j < n_f.  o1 = mix(h_f), o2 = mix(o1); i1 = (o1 + j*G1) >> 11, i2 = (o2 + j*G2) >> 11.
 *     If i1 + i2 > 2^53 then i1 = 2^53 - i1 and i2 = 2^53 - i2 (the fold into the triangle, so that no weight is
 *     negative); i0 = 2^53 - i1 - i2.  w_k = (double)i_k * 2^-53, which is exact, and w0 + w1 + w2 = 1 exactly.
 *     Position, per component: (float)((w0*A + w1*B) + w2*C).  Normal: M = (w0*nA + w1*nB) + w2*nC per component, then
 *     M / sqrt((Mx*Mx + My*My) + Mz*Mz) rounded to float32, zero unless that length is > 0 (step 7 of
 *     acmmp_fusion_mesh_render).  Colour: (float)((w0*cA + w1*cB) + w2*cC) per component.
 *  6. Order.  The samples are listed in ascending (f, j): sample offset[f] + j, offset the exclusive 64-bit prefix sum
 *     of n_f, holds the 9 floats of a cloud point (position, normal, colour) and face = f.
 * n_samples and n_skipped may be NULL.  ACMMP_ERR_INVALID_ARGUMENT: no mesh result (an empty one is valid and gives no
 * samples), a spacing that is not finite and > 0.  ACMMP_ERR_UNSUPPORTED: step 4.  One sample result is resident at a
 * time (acmmp_fusion_sample_points reads it); it is built beside the previous one, and any error -- an out-of-memory
 * part-way included -- leaves the object as it was.  It is discarded when the mesh result is replaced or discarded (a
 * successful acmmp_fusion_voxel_mesh or acmmp_fusion_set_mesh, and whatever discards the mesh's source), and a distance
 * result or align records of the samples go when the samples are replaced or discarded; acmmp_fusion_set_view,
 * acmmp_fusion_set_reference_cloud, acmmp_fusion_mesh_render and the distance, align and surface calls leave it alone.
 * The only atomic of the device is an integer add (the skipped faces, one per wave); a sample is written by the one lane
 * that computes it, which finds its face in the offsets by binary search.
 * Device memory: 40 bytes per sample held with the result (36 for the point, 4 for the face); 8 bytes per face (its
 * offset within its chunk of 256 faces, from which n_f follows) and 16 per chunk (the chunk's count and offset) while
 * the call runs.  The host waits twice: for the total, and at the end. */
acmmp_status acmmp_fusion_mesh_sample(acmmp_fusion *f, float spacing, uint64_t seed, int64_t *n_samples,
                                      int64_t *n_skipped);
/* Samples [first, first + n) of the sample result to host arrays, either of which may be NULL: points n x 9 floats,
 * face n int32.  Ranges as acmmp_fusion_voxel_points (no sample result: every range but an empty one at 0 is refused). */
acmmp_status acmmp_fusion_sample_points(acmmp_fusion *f, int64_t first, int64_t n, float *points, int32_t *face);

/* ---- evaluation regions: crop volumes and observation masks for the measuring calls (no reference counterpart) ----
 * A region says which points of one side of the comparison take part in it: the data side (every ACMMP_DIST_FROM_*
 * cloud) or the reference side (the reference cloud).  It is the intersection of up to three optional parts:
 *   planes  n_planes in [0, 8] half-spaces (a, b, c, d) at planes[4 i .. + 4); 0 = no planes.
 *   prism   n_vertices = 0 (no prism) or in [3, 256]; an orthogonal axis w in {0, 1, 2}, axis_min <= axis_max, and a
 *           polygon of (u, v) pairs at polygon[2 i .. + 2) in the other two coordinates in increasing index order:
 *           w = 0 gives (y, z), w = 1 gives (x, z), w = 2 gives (x, y) -- Open3D's SelectionPolygonVolume.
 *   grid    dims all 0 (no grid) or each in [1, 4096]; origin o, cell c > 0 and ceil(nx ny nz / 8) bytes of bits: cell
 *           (ix, iy, iz) is bit k & 7, least significant first, of byte k >> 3, k = ix + nx (iy + ny iz).  x runs
 *           fastest, so a column-major MATLAB logical ObsMask(ix, iy, iz) packed in that order is a plain dump.
 * acmmp_fusion_set_region copies the struct, the polygon and the bits (the caller's arrays may go away) and makes them
 * the region of `side`, ACMMP_REGION_DATA or ACMMP_REGION_REFERENCE; r = NULL clears it.  flags is 0 or
 * ACMMP_REGION_QUERIES_ONLY.  A region belongs to the object, as the cloud transform does: it lives until it is cleared
 * or replaced and survives every replacement of a source or of the reference cloud.  A successful set or clear discards
 * the distance result, the surface result and the align records of both kinds; it keeps the sources, the reference
 * cloud and the transform.  ACMMP_ERR_INVALID_ARGUMENT: a side or a flag that is none of the constants, a count outside
 * the ranges above, an axis outside {0, 1, 2}, any number of a part that is present that is not finite,
 * axis_min > axis_max, c <= 0, a NULL array with a positive count.  Any error leaves the object as it was.
 * acmmp_fusion_get_region reports the region of a side: *is_set, *flags, *n_planes, *n_vertices and dims[3] (zeros with
 * none set); each output may be NULL.  Device memory: 16 bytes per vertex and the bits.
 *
 * The definition.  Arithmetic is IEEE float64 with no contraction on the point's float32 coordinates widened.  A data-side
 * point is x' under the cloud transform when one is set, exactly as rule 1 of acmmp_fusion_cloud_distance reads it
 * (float64, rounded once to float32, then widened); inside an align call it is x' under that iteration's M_k.  A
 * reference-side point is never transformed.  Every part is evaluated for every valid point, with no short-circuit, and
 * the result is one class byte per point:
 *   bit 0 (ACMMP_REGION_CLASS_INVALID)  a coordinate is not finite; the other bits are then 0.
 *   bit 1 (ACMMP_REGION_CLASS_PLANES)   a plane fails: s = ((a x + b y) + c z) + d, and the point passes when s >= 0
 *                                       (s = -0.0 passes).
 *   bit 2 (ACMMP_REGION_CLASS_PRISM)    the prism fails: the point passes when axis_min <= p_w <= axis_max and the crossing
 *                                       parity is odd.  The parity starts even; for each edge i with j = (i + 1) mod n it
 *                                       toggles when (v_i > p_v) != (v_j > p_v) and
 *                                       p_u < (((u_j - u_i) * (p_v - v_i)) / (v_j - v_i)) + u_i.
 *                                       This is Open3D's rule, so points on an edge or a vertex fall where its tool puts them.
 *   bit 3 (ACMMP_REGION_CLASS_GRID)     the grid fails: i_a = rint((p_a - o_a) / c), ties to even; the point passes when
 *                                       0 <= i_a < n_a on all three axes, compared in float64 before any conversion,
 *                                       and the cell's bit is set.
 * Class 0 is inside.  A part that is absent never fails, and without a region every valid point is inside.
 *
 * What honours it.  In acmmp_fusion_cloud_distance (both directions), acmmp_fusion_surface_distance (the query cloud's
 * side; the mesh's faces are never cropped), acmmp_fusion_cloud_align and acmmp_fusion_cloud_align_plane a point of a
 * side whose region is set and whose class is not 0 is treated exactly as if its coordinates were not finite (rule 1 of
 * the distance definition): it is no valid query and does not exist as a target.  Indices, n_query, the result lengths
 * and the nearest indices of the other points are unchanged.  With ACMMP_REGION_QUERIES_ONLY the side's points are
 * removed as queries only and remain targets (DTU's completeness is measured to the whole reconstruction).  The data
 * queries of a surface call are classified under the transform that is set, although the call itself reads them in the
 * data frame; the data queries of an align call are classified again under each iteration's M_k (Tanks and Temples'
 * cropped refinement).  The device classifies every cloud of a call once (the data side of an align call once per
 * iteration) in a pass of its own before the search, never per pair; with no region set no pass runs and the calls are
 * what they were.
 *
 * acmmp_fusion_region_classify classifies the cloud `source` -- an ACMMP_DIST_FROM_* constant, or
 * ACMMP_SURF_FROM_REFERENCE for the reference cloud -- under the region of its side (the data side under the transform
 * that is set), keeps the class bytes resident and returns counts[ACMMP_REGION_COUNT_WORDS]: [0] points, [1] invalid,
 * [2] inside, and the points that fail [3] a plane, [4] the prism, [5] the grid (a point can count in several of the
 * last three).  counts may be NULL.  ACMMP_ERR_INVALID_ARGUMENT: a source that is none of the constants, no such result.
 * acmmp_fusion_region_classes reads classes [first, first + n); ranges as acmmp_fusion_distance_results.  One class
 * result is resident; it is built beside the previous one and any error leaves the object as it was.  It goes when its
 * source is replaced or discarded, when a region of either side is set or cleared, and, for a data cloud, when the
 * transform is set or cleared; the measuring calls neither read nor write it.  Only integers are summed: the counts are
 * reduced over the wave and the workgroup and added with one atomic per word per workgroup, so no result depends on the
 * order of execution.  Device memory: 1 byte per point; a measuring call with a region adds 1 byte per point of each
 * cropped cloud while it runs.  The host waits once. */
#define ACMMP_REGION_DATA 0
#define ACMMP_REGION_REFERENCE 1
#define ACMMP_REGION_QUERIES_ONLY 1
#define ACMMP_REGION_MAX_PLANES 8
#define ACMMP_REGION_MAX_VERTICES 256
#define ACMMP_REGION_MAX_DIM 4096
#define ACMMP_REGION_CLASS_INVALID 1
#define ACMMP_REGION_CLASS_PLANES 2
#define ACMMP_REGION_CLASS_PRISM 4
#define ACMMP_REGION_CLASS_GRID 8
#define ACMMP_REGION_COUNT_WORDS 6
typedef struct acmmp_region {
    int32_t n_planes;                 /* 0 .. 8 */
    int32_t n_vertices;               /* 0 (no prism) or 3 .. 256 */
    int32_t axis;                     /* the prism's orthogonal axis w */
    int32_t dims[3];                  /* nx, ny, nz: all 0 (no grid) or each 1 .. 4096 */
    double planes[4 * ACMMP_REGION_MAX_PLANES];
    double axis_min, axis_max;
    double origin[3];
    double cell;
    const double *polygon;            /* n_vertices x (u, v) */
    const uint8_t *bits;              /* ceil(nx ny nz / 8) bytes */
} acmmp_region;
acmmp_status acmmp_fusion_set_region(acmmp_fusion *f, int side, const acmmp_region *r, int flags);
acmmp_status acmmp_fusion_get_region(const acmmp_fusion *f, int side, int *is_set, int *flags, int *n_planes,
                                     int *n_vertices, int *dims);
acmmp_status acmmp_fusion_region_classify(acmmp_fusion *f, int source, int64_t *counts);
acmmp_status acmmp_fusion_region_classes(acmmp_fusion *f, int64_t first, int64_t n, uint8_t *cls);

/* ---- planar-prior host side (no GPU; ACMMP.cpp:904-1011, main.cpp:113-181) ---------------
 * Host restatements of the reference's planar-prior helpers, so a caller can run ProcessProblem's
 * planar pass without OpenCV.  Delaunay ties / triangle order differ from cv::Subdiv2D
 * (parity unpinned).  Output arrays are caller-allocated; when `cap` is too small
 * the call returns ACMMP_ERR_INVALID_ARGUMENT with the required count in *n_out / *n_tri. */

/* ACMMP::GetSupportPoints (ACMMP.cpp:904-930): per 5x5 tile the min-cost pixel if cost < 0.1;
 * xy = (x, y) pairs in the reference's order (tile columns outer, tile rows inner). */
acmmp_status acmmp_support_points(const float *costs, int W, int H, int *xy, int cap, int *n_out);

/* ACMMP::DelaunayTriangulation (ACMMP.cpp:932-955): triangles as 6 ints (x1 y1 x2 y2 x3 y3). */
acmmp_status acmmp_delaunay(const int *xy, int n, int W, int H, int *tri_xy, int cap, int *n_tri);

/* ACMMP::GetPriorPlaneParams (ACMMP.cpp:957-989): plane (n, w), |n| = 1, w >= 0, through the
 * triangle's three reference-camera points at `depths` (W x H). */
acmmp_status acmmp_prior_plane_params(const acmmp_camera *cam0, const float *depths, int W, int H,
                                      const int tri_xy[6], float plane[4]);

/* ACMMP::GetDepthFromPlaneParam (ACMMP.cpp:991-1011). */
float acmmp_depth_from_plane_param(const acmmp_camera *cam0, const float plane[4], int x, int y);

/* The planar block of ProcessProblem (main.cpp:113-181) + CudaPlanarPriorInitialization's
 * expansion (ACMMP.cpp:851-861): support points, Delaunay, rasterised triangle labels, per-triangle
 * planes, prior-depth range mask -> per-pixel prior planes (float4[P]) and labels (u32[P]) ready for
 * acmmp_set_planar_prior.  depths/costs: the first RunPatchMatch's output. */
acmmp_status acmmp_planar_prior_host(const acmmp_camera *cam0, const float *depths, const float *costs, int W,
                                     int H, float depth_min, float depth_max, float *prior_planes,
                                     uint32_t *masks, int *n_triangles);

/* The same planar block with its per-pixel work on this context's GPU, straight into the context's
 * planar-prior state: support points, Delaunay and the per-triangle planes on the host (depths/costs:
 * the first RunPatchMatch's output, W x H of the uploaded reference view), the triangle
 * rasterisation (main.cpp:153-159), the prior-depth range mask (main.cpp:168-180) and the per-pixel
 * expansion (ACMMP.cpp:855-862) on the device.  Equivalent to acmmp_planar_prior_host followed by
 * acmmp_set_planar_prior, bit for bit (tests/test_gpu_parity.py), without the host raster and the
 * 20 B/pixel upload.  No reference counterpart. */
acmmp_status acmmp_set_planar_prior_from_maps(acmmp_ctx *ctx, const float *depths, const float *costs,
                                              float depth_min, float depth_max, int *n_triangles);
/* The same planar block from the context's own last RunPatchMatch output in HBM (main.cpp:113-181 runs
 * it on the first run's depths and costs): GetSupportPoints (ACMMP.cpp:904-929) on the device, only the
 * support points (and their depths) to the host for the Delaunay triangulation and the per-triangle planes,
 * then the raster / mask / expansion of acmmp_set_planar_prior_from_maps.  Equal to
 * acmmp_set_planar_prior_from_maps on the downloaded maps, bit for bit (tests/test_gpu_planar_state.py);
 * no full-map download.  Both calls return once the raster and mask kernels are enqueued on the context's
 * stream (its next RunPatchMatch runs after them; acmmp_download_planar_prior waits for them). */
acmmp_status acmmp_set_planar_prior_from_state(acmmp_ctx *ctx, float depth_min, float depth_max, int *n_triangles);
/* Test hook: the planar-prior state of the context (P float4 planes, P labels; either may be NULL). */
acmmp_status acmmp_download_planar_prior(acmmp_ctx *ctx, float *prior_planes, uint32_t *masks);

/* RunJBU / JBU::CudaRun (ACMMP.cpp:1071-1122, ACMMP.cu:1558-1649): joint bilateral
 * upsampling of `coarse` (sw x sh) guided by `ref` (W x H).  imagescale as the
 * reference computes it: max(H / sh, W / sw) (integer division). */
acmmp_status acmmp_jbu(acmmp_ctx *ctx, const float *ref, int W, int H, const float *coarse, int sw, int sh,
                       int imagescale, float *out);

/* ---- test hooks: evaluate the device cost functions on arbitrary inputs ---- */
/* costs[k*(num_images-1) + v] = ComputeBilateralNCC (ACMMP.cu:405-516) of plane k at
 * pixel (px[k], py[k]) against source v+1. */
acmmp_status acmmp_debug_ncc(acmmp_ctx *ctx, int n, const int *px, const int *py, const float *planes,
                             float *costs);
/* costs[(k*8 + h)*(num_images-1) + v] = ComputeBilateralNCC (ACMMP.cu:405-516) of plane
 * planes[k*8 + h] at pixel (px[k], py[k]) against source v+1, evaluated by k_eval_nb's own NCC
 * code (the propagation kernel of CheckerboardPropagation, ACMMP.cu:1146-1233): in the fast math
 * mode on SPHERE views whose 6x6 patch spans at most 5 pixels of 2 pi / 2000 rad (patch_size 11,
 * radius_increment 2: from 2000x1000 up; patch_size 21 / increment 4: from 4000x2000 up), with its
 * interpolated sample coordinates and their deferred per-sample fallbacks. */
acmmp_status acmmp_debug_ncc_nb(acmmp_ctx *ctx, int n, const int *px, const int *py, const float *planes,
                                float *costs);
/* costs[(k*5 + h)*(num_images-1) + v]: the same NCC of plane planes[k*5 + h] at pixel (px[k], py[k]) as
 * PlaneHypothesisRefinement (ACMMP.cu:797-936) evaluates its 5 candidates -- k_eval_ref's staging and NCC
 * instance, which in the fast math mode interpolates SPHERE sample coordinates above 4 source views (the
 * size gate of acmmp_debug_ncc_nb); the views whose interpolation falls back are queued as k_eval_ref queues
 * them and recomputed with every sample projected by the per-entry code of k_nb_fix<1, true>, the
 * production path of those fallbacks. */
acmmp_status acmmp_debug_ncc_ref(acmmp_ctx *ctx, int n, const int *px, const int *py, const float *planes,
                                 float *costs);
/* out[k*(num_images-1) + v] = ComputeGeomConsistencyCost (ACMMP.cu:646-671). */
acmmp_status acmmp_debug_geom(acmmp_ctx *ctx, int n, const int *px, const int *py, const float *planes,
                              float *out);

#ifdef __cplusplus
}
#endif
#endif
