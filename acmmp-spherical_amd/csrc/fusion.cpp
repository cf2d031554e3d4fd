// fusion.cpp -- host object of the GPU depth-map fusion.
//
// Replaces RunFusionCuda's device half (ACMMP.cu:1817-2105): one upload per view of what the
// reference puts into textures (depth, normals, the colour image as float RGBA / 255), then per
// reference view SimpleFusionKernel (`k_fuse`) and an in-order compaction of the valid pixels -- the
// order RunFusionCuda's host loop collects them in (ACMMP.cu:2064-2071).  Everything stays in HBM; only
// the fused points come back.
//
// acmmp_fusion_run_scene is the same for a whole list of reference views in one call: the chunk prefix sum
// runs on the device, the points and their provenance (view, pixel, consistent-source mask) stay in HBM until
// acmmp_fusion_scene_points copies a range out, the count is 64-bit, and ACMMP_FUSE_UNIQUE keeps per-view
// `used` masks so that a depth sample contributes to the points of one reference view only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "acmmp.h"
#include "devbuf.h"
#include "fusion.h"
#include "fusion_results.h"

using namespace acmmp;

namespace {

// The buffers of one view of the fusion set; FuseView holds their addresses for the device.
struct ViewBuf {
    DevBuf<float> depth, normal, rgba;
    DevBuf<uint8_t> used;
};

// The four arrays of a scene result.
struct SceneBuf {
    DevBuf<float> pts;                           // 9 floats per point
    DevBuf<int> ref;                             // position in the run's reference list
    DevBuf<int> pix;                             // r * W + c
    DevBuf<uint32_t> mask;                       // consistent sources
    size_t cap = 0;                              // points allocated
};

int log2_ceil(unsigned long long x) {
    int l = 0;
    while ((1ull << l) < x) ++l;
    return l;
}

// The arrays of the voxel hash table; view() holds their addresses for the device.
struct VoxTableBuf {
    DevBuf<unsigned long long> keys, first, oid;
    DevBuf<uint32_t> cnt;
    unsigned long long slots = 0;
    VoxTable view() const { return {keys, first, oid, cnt, slots, log2_ceil(slots)}; }
    // every slot empty
    hipError_t reset_async(hipStream_t s) const {
        hipError_t e = hipMemsetAsync(keys, 0xff, sizeof(unsigned long long) * slots, s);
        if (e == hipSuccess) e = hipMemsetAsync(first, 0xff, sizeof(unsigned long long) * slots, s);
        if (e == hipSuccess) e = hipMemsetAsync(oid, 0xff, sizeof(unsigned long long) * slots, s);
        if (e == hipSuccess) e = hipMemsetAsync(cnt, 0, sizeof(uint32_t) * slots, s);
        return e;
    }
};

// The scratch of the ordered compactions (Compaction, fusion.h), one segment's worth: every stage's passes borrow it.
struct SegScratch {
    DevBuf<int> flags;                           // per item of a segment
    DevBuf<int> counts, offsets;                 // per 256-item chunk of a segment
    DevBuf<int> seg_count;
    DevBuf<unsigned long long> words;            // running, seg_base
    size_t cap = 0;                              // items of a segment allocated
    // room for segments of n items (exact size: contents are not kept)
    hipError_t reserve(size_t n) {
        hipError_t e = hipSuccess;
        if (!seg_count) e = seg_count.alloc(1);
        if (e == hipSuccess && !words) e = words.alloc(2);
        if (e != hipSuccess || cap >= n) return e;
        cap = 0;
        e = flags.alloc(n);
        if (e == hipSuccess) e = counts.alloc((n + 255) / 256);
        if (e == hipSuccess) e = offsets.alloc((n + 255) / 256);
        if (e == hipSuccess) cap = n;
        return e;
    }
    Compaction view(unsigned long long out_cap) const { return {flags, counts, offsets, seg_count, words, words + 1, out_cap}; }
};

// The resident results.  A record owns its buffers and holds its counts, `source`, the cloud it was computed from (what
// goes_with reads), and `have`; a default-constructed record is the absent result, so releasing one is rec = {}.  A
// stage's *Out type is its record plus the call's scratch and statistics, built beside the result held: a successful
// call installs it with f->rec = std::move(out), which takes the record and leaves the rest to end with the call.
struct VoxelRec {
    DevBuf<float> pts;                           // 9 floats per voxel
    DevBuf<int32_t> cnt;                         // points per voxel
    DevBuf<unsigned long long> slot;             // table slot per voxel (for acmmp_fusion_voxel_clean)
    unsigned long long total = 0;                // voxels held
    VoxGrid grid = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // origin and size
    Res source = R_SCENE;
    bool have = false;
};
struct CleanRec {
    DevBuf<float> pts;                           // 9 floats per kept voxel
    DevBuf<int32_t> cnt;                         // points per kept voxel
    DevBuf<long long> comp;                      // component id per kept voxel
    DevBuf<unsigned long long> vox;              // voxel index per kept voxel
    DevBuf<unsigned long long> lab;              // per voxel of the voxel result: label, ~0 = unsupported
    DevBuf<uint32_t> mask;                       // per voxel: its neighbours, one bit each
    DevBuf<long long> table;                     // roots, then voxels, then points, comps of each
    unsigned long long kept = 0, comps = 0;      // kept voxels, components
    Res source = R_VOXELS;
    bool have = false;
};
struct VisRec {
    DevBuf<float> pts;                           // 9 floats per kept entry
    DevBuf<int32_t> cnt;                         // points per kept entry
    DevBuf<int32_t> kept_tal;                    // 3 per kept entry
    DevBuf<int32_t> tal;                         // 3 per entry of the source
    DevBuf<unsigned long long> vox;              // voxel index per kept entry
    unsigned long long kept = 0, entries = 0;    // kept entries, entries of the source
    Res source = R_NONE;
    bool have = false;
};
struct MeshRec {
    DevBuf<float> verts;                         // 9 floats per vertex
    DevBuf<int32_t> faces;                       // 3 per triangle
    DevBuf<unsigned long long> skey;             // packed cell per sample
    DevBuf<int32_t> tsdf;                        // (S, n) per sample
    DevBuf<long long> sent;                      // remembered entry per sample, -1 = none
    unsigned long long nv = 0, nf = 0, ns = 0;   // vertices, triangles, samples
    Res source = R_NONE;                         // stays R_NONE for a mesh that acmmp_fusion_set_mesh installed
    bool have = false;
};
struct SampleRec {
    DevBuf<float> pts;                           // 9 floats per sample
    DevBuf<int32_t> face;                        // the sample's face
    unsigned long long n = 0, skipped = 0;       // samples held, invalid faces
    Res source = R_MESH;
    bool have = false;
};
struct RenderRec {
    DevBuf<float> depth, normal, colour;        // 1, 3 and 3 floats per pixel
    DevBuf<int32_t> face;                        // the winner per pixel, -1 = none
    int W = 0, H = 0;
    Res source = R_MESH;
    bool have = false;
};
struct RefRec {
    DevBuf<float> pts;                           // 3 floats per point
    unsigned long long n = 0;
    bool have = false;
};
// A distance result, and a surface result: `source` is the data cloud, and the query cloud.
struct DistRec {
    DevBuf<float> d2;                            // per query
    DevBuf<int32_t> nn;                          // per query: the nearest target or face, -1 = none
    unsigned long long n = 0;                    // queries
    Res source = R_NONE;
    bool have = false;
};
// The records of the last successful align call of either kind, on the host: per iteration ACMMP_ALIGN_RECORD_WORDS or
// ACMMP_ALIGN_PLANE_RECORD_WORDS words, the 12 doubles of M_k, the shift.
struct AlignRec {
    std::vector<int64_t> words;
    std::vector<double> M, shift;
    bool plane = false;                          // it was the point-to-plane call
    Res source = R_NONE;
    bool have = false;
};
// The region of one side (acmmp_fusion_set_region): the caller's struct with its two arrays copied to the device.  It
// is no result: it is replaced by a set and by nothing else.
struct RegionSet {
    bool set = false;
    int flags = 0;
    acmmp_region r = {};                         // polygon and bits NULL: the copies are below
    DevBuf<double> poly;                         // (u, v) per vertex
    DevBuf<uint8_t> bits;
    RegionDev dev() const {
        RegionDev d = {};
        if (!set) return d;                      // no part: every valid point is inside
        d.n_planes = r.n_planes;
        std::memcpy(d.planes, r.planes, sizeof(d.planes));
        d.n_vertices = r.n_vertices;
        d.axis = r.axis;
        d.axis_min = r.axis_min;
        d.axis_max = r.axis_max;
        d.poly = poly;
        for (int a = 0; a < 3; ++a) { d.dims[a] = r.dims[a]; d.o[a] = r.origin[a]; }
        d.cell = r.cell;
        d.bits = bits;
        return d;
    }
};
// The class result of acmmp_fusion_region_classify: `source` is the cloud classified.
struct RegionRec {
    DevBuf<uint8_t> cls;                         // per point
    unsigned long long n = 0;                    // points
    Res source = R_NONE;
    bool have = false;
};

}  // namespace

struct acmmp_fusion {
    int device = 0, model = 0, n = 0;
    hipStream_t stream = nullptr;
    std::vector<DevCam> cams;
    std::vector<ViewBuf> view_bufs;
    std::vector<FuseView> views;                 // view_bufs' addresses, as d_views holds them
    DevBuf<DevCam> d_cams;
    DevBuf<FuseView> d_views;
    DevBuf<int> d_srcs;
    DevBuf<float> d_dense;
    DevBuf<int> d_flags, d_counts, d_offsets;
    DevBuf<float> d_out;
    size_t cap_P = 0, cap_out = 0;
    // whole-scene pass: the resident result of the last acmmp_fusion_run_scene ...
    SceneBuf scene;
    unsigned long long s_total = 0;              // points held
    // ... and its scratch
    DevBuf<uint32_t> d_smask;                    // per pixel, cap_smask pixels
    size_t cap_smask = 0;
    DevBuf<int> d_scene_srcs;                    // 32 per reference view
    DevBuf<int> d_view_counts;                   // per reference view
    DevBuf<unsigned long long> d_view_base;      // per reference view: scene offset of its first point
    size_t cap_refs = 0;
    DevBuf<unsigned long long> d_running;        // running scene offset of a scene pass
    PinnedBuf<int> h_count;                      // the one word the host reads per view
    bool s_have = false;                         // a run_scene has succeeded
    // the resident results, one record each (absent when default-constructed); invalidate() knows which goes with which
    VoxelRec voxels;                             // acmmp_fusion_voxelize
    CleanRec clean;                              // acmmp_fusion_voxel_clean
    VisRec visible;                              // acmmp_fusion_voxel_visibility
    MeshRec mesh;                                // acmmp_fusion_voxel_mesh, acmmp_fusion_set_mesh
    SampleRec samples;                           // acmmp_fusion_mesh_sample
    RenderRec render;                            // acmmp_fusion_mesh_render
    RefRec ref;                                  // acmmp_fusion_set_reference_cloud
    DistRec dist, surf;                          // acmmp_fusion_cloud_distance, acmmp_fusion_surface_distance
    AlignRec align;                              // acmmp_fusion_cloud_align, acmmp_fusion_cloud_align_plane
    RegionRec classes;                           // acmmp_fusion_region_classify
    // the evaluation regions of the data and the reference side (acmmp_fusion_set_region)
    RegionSet region[2];
    // the transform of the data cloud (acmmp_fusion_set_cloud_transform)
    bool xf_set = false;
    double xf[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    // what outlives the results: the test hooks' knobs (0 = automatic) ...
    long long v_force_slots = 0, m_force_slots = 0;   // table size of the next voxelize / mesh call
    long long r_small_max = 0, surf_small_max = 0;    // the small / large threshold of a render / surface call
    float dist_force_cell = 0.0f, surf_force_cell = 0.0f;   // the cell of the next distance and align / surface calls
    // ... and what they report of the last successful call
    long long v_stats[4] = {0, 0, 0, 0}, m_stats[4] = {0, 0, 0, 0};   // slots, occupied, max_probe, wrapped
    long long r_plan[3] = {0, 0, 0};             // small faces, large faces, candidates
    long long surf_plan[4] = {0, 0, 0, 0};       // small faces, large faces, registrations, skipped
    float dist_cell = 0.0f, surf_cell = 0.0f;    // the cell ...
    long long dist_stats[3] = {0, 0, 0}, surf_stats[3] = {0, 0, 0};   // ... its occupied cells, longest list, largest ring
    // the scratch, kept between calls; the tables and seg are dropped with the scene result they were sized for
    VoxTableBuf v_tab, v_tab_spare;              // v_tab_spare: filled by a voxelize while v_tab belongs to a result
    bool v_tab_live = false;                     // v_tab is the table of the voxel result held (else scratch)
    SegScratch seg;                              // of voxelize's compaction and of every later stage's
    DevBuf<int> vis_list;                        // the view list, kVisMaxList positions
    DevBuf<unsigned long long> v_words;          // kVoxWords run words, then the 3 minima (32-bit each, in 2 words)
    DevBuf<unsigned long long> c_words, vis_words, m_words, r_words, dist_words, surf_words, smp_words, reg_words;   // k*Words device words each
    std::string err;
};

namespace {

acmmp_status ffail(acmmp_fusion* f, acmmp_status s, const std::string& m) {
    if (f) f->err = m;
    return s;
}

#define F_HIP(f, expr)                                                                          \
    do {                                                                                        \
        const hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                                   \
            return ffail((f), e_ == hipErrorOutOfMemory ? ACMMP_ERR_OUT_OF_MEMORY : ACMMP_ERR_HIP, \
                         std::string(#expr) + ": " + hipGetErrorString(e_));                     \
    } while (0)

template <typename T, bool PINNED>
hipError_t alloc(DevBuf<T, PINNED>& b, size_t count) { return b.alloc(count); }

}  // namespace

extern "C" {

acmmp_status acmmp_fusion_create(int device, int n_views, const acmmp_camera* cams, acmmp_fusion** out) {
    if (!out || !cams || n_views < 1) return ACMMP_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) return ACMMP_ERR_NO_DEVICE;
    if (device < 0 || device >= nd) return ACMMP_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n_views; ++i) {
        if (cams[i].model != ACMMP_PINHOLE && cams[i].model != ACMMP_SPHERE) return ACMMP_ERR_INVALID_ARGUMENT;
        if (cams[i].model != cams[0].model) return ACMMP_ERR_UNSUPPORTED;
        if (cams[i].width <= 0 || cams[i].height <= 0) return ACMMP_ERR_INVALID_ARGUMENT;
    }
    if (hipSetDevice(device) != hipSuccess) return ACMMP_ERR_HIP;
    acmmp_fusion* f = new acmmp_fusion();
    f->device = device;
    f->model = cams[0].model;
    f->n = n_views;
    f->cams.resize(n_views);
    for (int i = 0; i < n_views; ++i) f->cams[i] = make_devcam(cams[i]);
    f->view_bufs.resize(n_views);
    f->views.assign(n_views, FuseView{nullptr, nullptr, nullptr, 0, 0, nullptr});
    acmmp_status s = ACMMP_OK;
    if (hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking) != hipSuccess ||
        alloc(f->d_cams, n_views) != hipSuccess || alloc(f->d_views, n_views) != hipSuccess ||
        alloc(f->d_srcs, 32) != hipSuccess || alloc(f->d_running, 1) != hipSuccess ||
        alloc(f->h_count, 1) != hipSuccess ||
        hipMemcpy(f->d_cams, f->cams.data(), sizeof(DevCam) * n_views, hipMemcpyHostToDevice) != hipSuccess)
        s = ACMMP_ERR_HIP;
    if (s != ACMMP_OK) { acmmp_fusion_destroy(f); return s; }
    *out = f;
    return ACMMP_OK;
}

void acmmp_fusion_destroy(acmmp_fusion* f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->stream) {
        (void)hipStreamSynchronize(f->stream);
        (void)hipStreamDestroy(f->stream);
    }
    delete f;                                      // the buffers free themselves, on this device
}

const char* acmmp_fusion_last_error(const acmmp_fusion* f) { return f ? f->err.c_str() : ""; }

acmmp_status acmmp_fusion_set_view(acmmp_fusion* f, int view, const float* depth, const float* normals,
                                   const uint8_t* bgr) {
    if (!f || !depth || !normals || !bgr) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "null argument");
    if (view < 0 || view >= f->n) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "view index out of range");
    F_HIP(f, hipSetDevice(f->device));
    const int W = f->cams[view].W, H = f->cams[view].H;
    const size_t P = static_cast<size_t>(W) * H;
    // the reference's colour texture: cvtColor(BGR2RGBA) + convertTo(CV_32FC4, 1/255) (ACMMP.cu:1950-1953)
    std::vector<float> rgba(4 * P);
    const float s = static_cast<float>(1.0 / 255.0);
    for (size_t i = 0; i < P; ++i) {
        rgba[4 * i + 0] = static_cast<float>(bgr[3 * i + 2]) * s;
        rgba[4 * i + 1] = static_cast<float>(bgr[3 * i + 1]) * s;
        rgba[4 * i + 2] = static_cast<float>(bgr[3 * i + 0]) * s;
        rgba[4 * i + 3] = 255.0f * s;
    }
    // the new buffers are built beside the view's present ones and installed only when every step succeeded;
    // on a failure they free themselves and the view, host and device copy, is as it was
    DevBuf<float> d, nrm, col;
    DevBuf<uint8_t> usd;
    F_HIP(f, alloc(d, P));
    F_HIP(f, alloc(nrm, 3 * P));
    F_HIP(f, alloc(col, 4 * P));
    F_HIP(f, alloc(usd, P));
    const FuseView v{d, nrm, col, W, H, usd};
    F_HIP(f, hipMemset(usd, 0, P));                 // a newly set view has no used sample
    F_HIP(f, hipMemcpy(d, depth, sizeof(float) * P, hipMemcpyHostToDevice));
    F_HIP(f, hipMemcpy(nrm, normals, sizeof(float) * 3 * P, hipMemcpyHostToDevice));
    F_HIP(f, hipMemcpy(col, rgba.data(), sizeof(float) * 4 * P, hipMemcpyHostToDevice));
    F_HIP(f, hipMemcpy(f->d_views + view, &v, sizeof(FuseView), hipMemcpyHostToDevice));
    f->views[view] = v;
    ViewBuf& b = f->view_bufs[view];
    b.depth = std::move(d); b.normal = std::move(nrm); b.rgba = std::move(col); b.used = std::move(usd);
    return ACMMP_OK;
}

acmmp_status acmmp_fusion_run(acmmp_fusion* f, int ref, int n_src, const int* src_views, float* points, int cap,
                              int* n_points) {
    if (!f || !n_points || n_src < 0 || n_src > 32 || (n_src > 0 && !src_views) || cap < 0 || (cap > 0 && !points))
        return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "bad argument");
    if (ref < 0 || ref >= f->n) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "reference index out of range");
    for (int j = 0; j < n_src; ++j)
        if (src_views[j] >= f->n) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "source index out of range");
    std::vector<int> used(1, ref);
    for (int j = 0; j < n_src; ++j) if (src_views[j] >= 0) used.push_back(src_views[j]);
    for (int v : used)
        if (!f->views[v].depth) return ffail(f, ACMMP_ERR_STATE, "set_view first for every view used");
    F_HIP(f, hipSetDevice(f->device));
    const int W = f->cams[ref].W, H = f->cams[ref].H;
    const size_t P = static_cast<size_t>(W) * H;
    const size_t nblk = (P + 255) / 256;
    if (f->cap_P < P) {
        F_HIP(f, alloc(f->d_dense, 9 * P));
        F_HIP(f, alloc(f->d_flags, P));
        F_HIP(f, alloc(f->d_counts, nblk));
        F_HIP(f, alloc(f->d_offsets, nblk));
        f->cap_P = P;
    }
    hipStream_t s = f->stream;
    if (n_src > 0) F_HIP(f, hipMemcpyAsync(f->d_srcs, src_views, sizeof(int) * n_src, hipMemcpyHostToDevice, s));
    F_HIP(f, launch_fuse(f->model, f->d_cams, f->d_views, ref, W, H, f->d_srcs, n_src, f->d_dense, f->d_flags,
                         f->d_counts, s));
    std::vector<int> counts(nblk);
    F_HIP(f, hipMemcpyAsync(counts.data(), f->d_counts, sizeof(int) * nblk, hipMemcpyDeviceToHost, s));
    F_HIP(f, hipStreamSynchronize(s));
    long long total = 0;
    for (size_t b = 0; b < nblk; ++b) { const int c = counts[b]; counts[b] = static_cast<int>(total); total += c; }
    *n_points = static_cast<int>(total);
    if (total > cap) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "points capacity too small");
    if (total == 0) return ACMMP_OK;
    if (f->cap_out < static_cast<size_t>(total)) {
        F_HIP(f, alloc(f->d_out, 9 * static_cast<size_t>(total)));
        f->cap_out = static_cast<size_t>(total);
    }
    F_HIP(f, hipMemcpyAsync(f->d_offsets, counts.data(), sizeof(int) * nblk, hipMemcpyHostToDevice, s));
    F_HIP(f, launch_fuse_compact(W, H, f->d_dense, f->d_flags, f->d_offsets, f->d_out, s));
    F_HIP(f, hipMemcpyAsync(points, f->d_out, sizeof(float) * 9 * total, hipMemcpyDeviceToHost, s));
    F_HIP(f, hipStreamSynchronize(s));
    return ACMMP_OK;
}

}  // extern "C"

namespace {

// `what` has been replaced or discarded: every held result that goes with it (goes_with, fusion_results.h) is released,
// and in turn what goes with that one.  The one place where results are released: an entry point installs its record
// and calls this.  The scratch sized for a scene goes with the scene.
void invalidate(acmmp_fusion* f, Res what) {
    const auto drop = [&](auto& rec, Res r) {
        if (!rec.have || !goes_with(r, rec.source, what)) return;
        rec = {};
        invalidate(f, r);
    };
    drop(f->voxels, R_VOXELS);
    drop(f->clean, R_CLEAN);
    drop(f->visible, R_VISIBLE);
    drop(f->mesh, R_MESH);
    drop(f->samples, R_SAMPLES);
    drop(f->render, R_RENDER);
    drop(f->dist, R_DIST);
    drop(f->surf, R_SURF);
    drop(f->align, R_ALIGN);
    drop(f->classes, R_CLASSES);
    if (what == R_SCENE) {
        f->v_tab = VoxTableBuf();
        f->v_tab_spare = VoxTableBuf();
        f->v_tab_live = false;
        f->seg = SegScratch();
    }
}

// A resident cloud as a stage reads it: 9 floats per point (3 for the reference cloud), and where the cloud has them
// the points per entry and the entries' voxel indices.
struct Cloud {
    bool have = false;
    const float* pts = nullptr;
    int stride = 9;
    unsigned long long n = 0;
    const int32_t* cnt = nullptr;
    const unsigned long long* vox = nullptr;
    DistCloud dist() const { return DistCloud{pts, stride, n}; }
};

Cloud cloud(const acmmp_fusion* f, Res id) {
    switch (id) {
        case R_SCENE: return {f->s_have, f->scene.pts, 9, f->s_total};
        case R_VOXELS: return {f->voxels.have, f->voxels.pts, 9, f->voxels.total, f->voxels.cnt};
        case R_CLEAN: return {f->clean.have, f->clean.pts, 9, f->clean.kept, f->clean.cnt, f->clean.vox};
        case R_VISIBLE: return {f->visible.have, f->visible.pts, 9, f->visible.kept, f->visible.cnt, f->visible.vox};
        case R_MESH: return {f->mesh.have, f->mesh.verts, 9, f->mesh.nv};
        case R_REFERENCE: return {f->ref.have, f->ref.pts, 3, f->ref.n};
        case R_SAMPLES: return {f->samples.have, f->samples.pts, 9, f->samples.n};
        default: return {};
    }
}

// After a failed *_run: the device's error cleared and the stream drained, the run's message kept.
acmmp_status run_failed(acmmp_fusion* f, acmmp_status st) {
    const std::string why = f->err;
    (void)hipGetLastError();
    (void)hipStreamSynchronize(f->stream);
    f->err = why;
    return st;
}

// The pre-pass of a measuring call for one cloud: where its side's region rs applies -- it is set, and the cloud is a
// query or the region is not ACMMP_REGION_QUERIES_ONLY -- the classes of `read_as` (the cloud as the region reads it) go
// to buf, the call's scratch, on the stream, and c reads through them.  Otherwise c is as it was: the path without a region.
acmmp_status region_crop(acmmp_fusion* f, const RegionSet& rs, bool as_target, const DistCloud& read_as, DevBuf<uint8_t>& buf,
                         DistCloud& c) {
    if (!rs.set || (as_target && (rs.flags & ACMMP_REGION_QUERIES_ONLY))) return ACMMP_OK;
    F_HIP(f, alloc(buf, static_cast<size_t>(c.n)));
    F_HIP(f, launch_region_classify(read_as, rs.dev(), buf, nullptr, f->stream));
    c.cls = buf;
    return ACMMP_OK;
}

bool finite32(float x) {
    uint32_t b;
    std::memcpy(&b, &x, 4);
    return (b & 0x7f800000u) != 0x7f800000u;
}

constexpr int kVisMaxList = 4096;

acmmp_status check_view_list(acmmp_fusion* f, int n_list, const int* views) {
    if (n_list < 1 || n_list > kVisMaxList || !views)
        return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "the view list must hold 1 to 4096 views");
    for (int j = 0; j < n_list; ++j) {
        if (views[j] < 0 || views[j] >= f->n) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "view index out of range");
        if (!f->views[views[j]].depth) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "set_view first for every view listed");
    }
    return ACMMP_OK;
}

acmmp_status check_tau_list(acmmp_fusion* f, float max_dist, int n_tau, const float* tau) {
    if (!finite32(max_dist) || !(max_dist > 0.0f)) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "max_dist must be finite and > 0");
    if (n_tau < 0 || n_tau > ACMMP_DIST_MAX_TAU || (n_tau > 0 && !tau))
        return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "n_tau must be 0 to 8");
    for (int i = 0; i < n_tau; ++i)
        if (!finite32(tau[i]) || !(tau[i] >= 0.0f) || tau[i] > max_dist)
            return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "every tau must be finite and in [0, max_dist]");
    return ACMMP_OK;
}

// Copies [first, first + n) of `count`-element device arrays to the host ones that are not NULL.
template <typename T>
hipError_t read_range(T* dst, const T* src, size_t first, size_t n, size_t per = 1) {
    return dst ? hipMemcpy(dst, src + per * first, sizeof(T) * per * n, hipMemcpyDeviceToHost) : hipSuccess;
}

bool bad_range(int64_t first, int64_t n, unsigned long long total) {
    return static_cast<unsigned long long>(first) > total || static_cast<unsigned long long>(n) > total - first;
}

// A range reader: [first, first + n) checked against the `total` elements the record holds (`beyond` is the refusal's
// message), then, unless the range is empty, reads(first, n) on the object's device.  f is not NULL.
template <class Reads>
acmmp_status read_result(acmmp_fusion* f, int64_t first, int64_t n, unsigned long long total, const char* beyond, Reads reads) {
    if (first < 0 || n < 0) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "bad argument");
    if (bad_range(first, n, total)) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, beyond);
    if (n == 0) return ACMMP_OK;
    F_HIP(f, hipSetDevice(f->device));
    return reads(static_cast<size_t>(first), static_cast<size_t>(n));
}

// b := arrays of at least `need` points (geometric growth) holding b's first `live` points.  b is unchanged
// when an allocation fails.
acmmp_status scene_grow(acmmp_fusion* f, SceneBuf& b, size_t need, size_t live, hipStream_t s) {
    SceneBuf nb;
    nb.cap = std::max(need, 2 * b.cap);
    if (alloc(nb.pts, 9 * nb.cap) != hipSuccess || alloc(nb.ref, nb.cap) != hipSuccess ||
        alloc(nb.pix, nb.cap) != hipSuccess || alloc(nb.mask, nb.cap) != hipSuccess) {
        (void)hipGetLastError();
        return ffail(f, ACMMP_ERR_OUT_OF_MEMORY, "scene buffer of " + std::to_string(need) + " points");
    }
    hipError_t e = hipSuccess;
    if (live > 0) {
        e = hipMemcpyAsync(nb.pts, b.pts, sizeof(float) * 9 * live, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(nb.ref, b.ref, sizeof(int) * live, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(nb.pix, b.pix, sizeof(int) * live, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(nb.mask, b.mask, sizeof(uint32_t) * live, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    if (e != hipSuccess) return ffail(f, ACMMP_ERR_HIP, std::string("scene buffer copy: ") + hipGetErrorString(e));
    b = std::move(nb);
    return ACMMP_OK;
}

// The views of a scene run, fused in order into `out` (see acmmp_fusion_run_scene); counts[k] per view.
acmmp_status scene_views(acmmp_fusion* f, int n_refs, const int* refs, const int* n_src, bool unique, SceneBuf& out,
                         std::vector<int>& counts, unsigned long long& total) {
    hipStream_t s = f->stream;
    F_HIP(f, hipMemsetAsync(f->d_running, 0, sizeof(unsigned long long), s));
    total = 0;
    for (int k = 0; k < n_refs; ++k) {
        const int ref = refs[k];
        const int W = f->cams[ref].W, H = f->cams[ref].H;
        F_HIP(f, launch_fuse_scene(f->model, unique, f->d_cams, f->d_views, ref, W, H, f->d_scene_srcs + 32 * k, n_src[k],
                                   f->d_dense, f->d_flags, f->d_smask, f->d_counts, f->d_offsets, f->d_view_counts + k,
                                   f->d_running, f->d_view_base + k, s));
        // the one host wait of the view: its 4-byte count, to size the output before anything is written there
        F_HIP(f, hipMemcpyAsync(f->h_count, f->d_view_counts + k, sizeof(int), hipMemcpyDeviceToHost, s));
        F_HIP(f, hipStreamSynchronize(s));
        const int c = *f->h_count;
        counts[k] = c;
        if (c > 0) {
            if (total + static_cast<unsigned long long>(c) > out.cap) {
                const acmmp_status st = scene_grow(f, out, static_cast<size_t>(total) + c, static_cast<size_t>(total), s);
                if (st != ACMMP_OK) return st;
            }
            F_HIP(f, launch_fuse_scatter_scene(W, H, f->d_dense, f->d_flags, f->d_smask, f->d_offsets, f->d_view_base + k, k,
                                               out.cap, out.pts, out.ref, out.pix, out.mask, s));
        }
        total += static_cast<unsigned long long>(c);
    }
    F_HIP(f, hipStreamSynchronize(s));
    return ACMMP_OK;
}

}  // namespace

extern "C" {

acmmp_status acmmp_fusion_run_scene(acmmp_fusion* f, int n_refs, const int* refs, const int* n_src, const int* src_views,
                                    int flags, int* counts, int64_t* n_points) {
    if (!f || !n_points || n_refs < 0 || (n_refs > 0 && (!refs || !n_src || !src_views)) ||
        (flags & ~ACMMP_FUSE_UNIQUE) != 0)
        return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "bad argument");
    const bool unique = (flags & ACMMP_FUSE_UNIQUE) != 0;
    size_t maxP = 0;
    for (int k = 0; k < n_refs; ++k) {
        if (refs[k] < 0 || refs[k] >= f->n) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "reference index out of range");
        if (n_src[k] < 0 || n_src[k] > 32) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "more than 32 source views");
        if (!f->views[refs[k]].depth) return ffail(f, ACMMP_ERR_STATE, "set_view first for every view used");
        for (int j = 0; j < n_src[k]; ++j) {
            const int v = src_views[32 * k + j];
            if (v >= f->n) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "source index out of range");
            if (v >= 0 && !f->views[v].depth) return ffail(f, ACMMP_ERR_STATE, "set_view first for every view used");
        }
        maxP = std::max(maxP, static_cast<size_t>(f->cams[refs[k]].W) * f->cams[refs[k]].H);
    }
    F_HIP(f, hipSetDevice(f->device));
    // scratch (no part of the object's visible state)
    const size_t nblk = (maxP + 255) / 256;
    if (f->cap_P < maxP) {
        f->cap_P = 0;
        F_HIP(f, alloc(f->d_dense, 9 * maxP));
        F_HIP(f, alloc(f->d_flags, maxP));
        F_HIP(f, alloc(f->d_counts, nblk));
        F_HIP(f, alloc(f->d_offsets, nblk));
        f->cap_P = maxP;
    }
    if (f->cap_smask < maxP) {
        f->cap_smask = 0;
        F_HIP(f, alloc(f->d_smask, maxP));
        f->cap_smask = maxP;
    }
    if (f->cap_refs < static_cast<size_t>(n_refs)) {
        f->cap_refs = 0;
        F_HIP(f, alloc(f->d_scene_srcs, 32 * static_cast<size_t>(n_refs)));
        F_HIP(f, alloc(f->d_view_counts, static_cast<size_t>(n_refs)));
        F_HIP(f, alloc(f->d_view_base, static_cast<size_t>(n_refs)));
        f->cap_refs = static_cast<size_t>(n_refs);
    }
    std::vector<int> srcs(32 * static_cast<size_t>(n_refs), -1);
    for (int k = 0; k < n_refs; ++k)
        for (int j = 0; j < n_src[k]; ++j) srcs[32 * static_cast<size_t>(k) + j] = src_views[32 * k + j];
    hipStream_t s = f->stream;
    if (n_refs > 0)
        F_HIP(f, hipMemcpyAsync(f->d_scene_srcs, srcs.data(), sizeof(int) * srcs.size(), hipMemcpyHostToDevice, s));
    // unique: the used masks as they are now, to put back if the run fails part-way
    std::vector<DevBuf<uint8_t>> saved(unique ? f->n : 0);
    for (size_t v = 0; v < saved.size(); ++v) {
        if (!f->views[v].used) continue;
        const size_t P = static_cast<size_t>(f->views[v].W) * f->views[v].H;
        hipError_t e = alloc(saved[v], P);
        if (e == hipSuccess) e = hipMemcpyAsync(saved[v], f->views[v].used, P, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            (void)hipStreamSynchronize(s);
            return ffail(f, e == hipErrorOutOfMemory ? ACMMP_ERR_OUT_OF_MEMORY : ACMMP_ERR_HIP,
                         std::string("used-mask snapshot: ") + hipGetErrorString(e));
        }
    }
    // the new result is built beside the previous one and replaces it only when the whole run succeeded
    SceneBuf out;
    std::vector<int> view_counts(n_refs, 0);
    unsigned long long total = 0;
    const acmmp_status st = scene_views(f, n_refs, refs, n_src, unique, out, view_counts, total);
    if (st != ACMMP_OK) {                               // (not run_failed: the masks go back between the two waits)
        const std::string why = f->err;
        (void)hipStreamSynchronize(s);
        for (size_t v = 0; v < saved.size(); ++v)
            if (saved[v])
                (void)hipMemcpyAsync(f->views[v].used, saved[v], static_cast<size_t>(f->views[v].W) * f->views[v].H,
                                     hipMemcpyDeviceToDevice, s);
        (void)hipStreamSynchronize(s);
        f->err = why;
        return st;
    }
    f->scene = std::move(out);
    f->s_total = total;
    f->s_have = true;
    invalidate(f, R_SCENE);                           // it described the previous scene, or was sized for it
    if (counts) std::copy(view_counts.begin(), view_counts.end(), counts);
    *n_points = static_cast<int64_t>(total);
    return ACMMP_OK;
}

acmmp_status acmmp_fusion_scene_points(acmmp_fusion* f, int64_t first, int64_t n, float* points, int32_t* ref_index,
                                       int32_t* pixel, uint32_t* src_mask) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    return read_result(f, first, n, f->s_total, "range beyond the scene result", [&](size_t a, size_t m) -> acmmp_status {
        F_HIP(f, read_range<float>(points, f->scene.pts, a, m, 9));
        F_HIP(f, read_range<int>(ref_index, f->scene.ref, a, m));
        F_HIP(f, read_range<int>(pixel, f->scene.pix, a, m));
        F_HIP(f, read_range<uint32_t>(src_mask, f->scene.mask, a, m));
        return ACMMP_OK;
    });
}

acmmp_status acmmp_fusion_set_scene(acmmp_fusion* f, int64_t n, const float* points, const int32_t* ref_index,
                                    const int32_t* pixel, const uint32_t* src_mask) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    if (n < 0 || (n > 0 && !points)) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "bad argument");
    F_HIP(f, hipSetDevice(f->device));
    const size_t m = static_cast<size_t>(n);
    // built beside the present scene result, installed when every copy has succeeded
    SceneBuf out;
    out.cap = m;
    F_HIP(f, alloc(out.pts, 9 * m));
    F_HIP(f, alloc(out.ref, m));
    F_HIP(f, alloc(out.pix, m));
    F_HIP(f, alloc(out.mask, m));
    hipStream_t s = f->stream;
    const hipError_t e = [&]() -> hipError_t {
        if (m == 0) return hipSuccess;
        hipError_t r = hipMemcpyAsync(out.pts, points, sizeof(float) * 9 * m, hipMemcpyHostToDevice, s);
        if (r == hipSuccess)
            r = ref_index ? hipMemcpyAsync(out.ref, ref_index, sizeof(int) * m, hipMemcpyHostToDevice, s)
                          : hipMemsetAsync(out.ref, 0xff, sizeof(int) * m, s);
        if (r == hipSuccess)
            r = pixel ? hipMemcpyAsync(out.pix, pixel, sizeof(int) * m, hipMemcpyHostToDevice, s)
                      : hipMemsetAsync(out.pix, 0xff, sizeof(int) * m, s);
        if (r == hipSuccess)
            r = src_mask ? hipMemcpyAsync(out.mask, src_mask, sizeof(uint32_t) * m, hipMemcpyHostToDevice, s)
                         : hipMemsetAsync(out.mask, 0, sizeof(uint32_t) * m, s);
        return r;
    }();
    const hipError_t w = hipStreamSynchronize(s);      // the host arrays are the caller's again, also after a failure
    F_HIP(f, e);
    F_HIP(f, w);
    f->scene = std::move(out);
    f->s_total = static_cast<unsigned long long>(n);
    f->s_have = true;
    invalidate(f, R_SCENE);                           // it described the previous scene, or was sized for it
    return ACMMP_OK;
}

acmmp_status acmmp_fusion_reset_used(acmmp_fusion* f) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    F_HIP(f, hipSetDevice(f->device));
    for (const FuseView& v : f->views)
        if (v.used) F_HIP(f, hipMemsetAsync(v.used, 0, static_cast<size_t>(v.W) * v.H, f->stream));
    F_HIP(f, hipStreamSynchronize(f->stream));
    return ACMMP_OK;
}

acmmp_status acmmp_fusion_download_used(acmmp_fusion* f, int view, uint8_t* mask) {
    if (!f || !mask) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "null argument");
    if (view < 0 || view >= f->n) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "view index out of range");
    const size_t P = static_cast<size_t>(f->cams[view].W) * f->cams[view].H;
    if (!f->views[view].used) { std::memset(mask, 0, P); return ACMMP_OK; }   // never set: nothing used
    F_HIP(f, hipSetDevice(f->device));
    F_HIP(f, hipMemcpy(mask, f->views[view].used, P, hipMemcpyDeviceToHost));
    return ACMMP_OK;
}

}  // extern "C"

// ---- voxel-grid reduction of the resident scene result (include/acmmp.h; kernels: k_voxel_*) --------------

namespace {

// Points per compaction segment: the scan's chunk offsets are 32-bit.  ACMMP_VOXEL_SEGMENT_POINTS (a multiple of
// 256, tests) makes a small scene take the multi-segment path.
unsigned long long voxel_segment_points() {
    const unsigned long long dflt = 1ull << 30;
    const char* e = std::getenv("ACMMP_VOXEL_SEGMENT_POINTS");
    if (!e || !*e) return dflt;
    const long long v = std::atoll(e);
    return (v >= 256 && v % 256 == 0 && static_cast<unsigned long long>(v) <= dflt) ? static_cast<unsigned long long>(v) : dflt;
}

// The new result of a voxel run.
struct VoxelOut : VoxelRec {
    DevBuf<unsigned long long> sums;         // scratch: 9 int64 per kept voxel
};

// fn(i0, n) over the items [0, N) in segments of voxel_segment_points(), in ascending order; the first error ends it.
template <class Fn>
hipError_t for_segments(unsigned long long N, Fn fn) {
    const unsigned long long seg = voxel_segment_points();
    for (unsigned long long i0 = 0; i0 < N; i0 += seg) {
        const hipError_t e = fn(i0, static_cast<int>(std::min(seg, N - i0)));
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The scratch for compaction passes over up to N items.
hipError_t segment_reserve(acmmp_fusion* f, unsigned long long N) {
    return f->seg.reserve(static_cast<size_t>(std::min(N, voxel_segment_points())));
}

// One ordered compaction of the items [0, N) into at most `cap` outputs, all in stream order: launch(i0, n, c) per
// segment (a stage's launcher, see Compaction), then the copy of the number compacted to *done, which holds it after
// the caller's next wait for the stream.
template <class Launch>
hipError_t compact_pass(acmmp_fusion* f, unsigned long long N, unsigned long long cap, unsigned long long* done,
                        Launch launch) {
    const Compaction c = f->seg.view(cap);
    hipError_t e = hipMemsetAsync(c.running, 0, sizeof(unsigned long long), f->stream);
    if (e == hipSuccess) e = for_segments(N, [&](unsigned long long i0, int n) { return launch(i0, n, c); });
    if (e == hipSuccess) e = hipMemcpyAsync(done, c.running, sizeof(unsigned long long), hipMemcpyDeviceToHost, f->stream);
    return e;
}

// `tab`: the table the run fills -- the object's scratch table, or a new one while the object's belongs to the
// voxel result held, which a failed run must leave usable.
acmmp_status voxel_run(acmmp_fusion* f, VoxGrid& g, bool find_origin, int min_points, unsigned long long slots,
                       VoxTableBuf& tab, VoxelOut& out, unsigned long long words[kVoxWords]) {
    hipStream_t s = f->stream;
    const unsigned long long N = f->s_total;
    // scratch
    if (!f->v_words) F_HIP(f, alloc(f->v_words, kVoxWords + 2));
    if (tab.slots != slots) {
        tab.slots = 0;
        F_HIP(f, alloc(tab.keys, slots));
        F_HIP(f, alloc(tab.first, slots));
        F_HIP(f, alloc(tab.oid, slots));
        F_HIP(f, alloc(tab.cnt, slots));
        tab.slots = slots;
    }
    F_HIP(f, segment_reserve(f, N));
    const VoxTable t = tab.view();
    unsigned long long* st = f->v_words;
    uint32_t* mn = reinterpret_cast<uint32_t*>(f->v_words + kVoxWords);
    F_HIP(f, hipMemsetAsync(st, 0, sizeof(unsigned long long) * kVoxWords, s));
    if (find_origin) {
        uint32_t h_mn[3];
        F_HIP(f, hipMemsetAsync(mn, 0xff, sizeof(uint32_t) * 4, s));
        F_HIP(f, for_segments(N, [&](unsigned long long i0, int n) { return launch_voxel_min(f->scene.pts, i0, n, mn, s); }));
        F_HIP(f, hipMemcpyAsync(h_mn, mn, sizeof(h_mn), hipMemcpyDeviceToHost, s));
        F_HIP(f, hipStreamSynchronize(s));
        // no point passed the finiteness test: the origin is (0, 0, 0), and every point is rejected below
        const bool any = h_mn[0] != 0xffffffffu;
        g.ox = any ? vox_decode_ordered(h_mn[0]) : 0.0f;
        g.oy = any ? vox_decode_ordered(h_mn[1]) : 0.0f;
        g.oz = any ? vox_decode_ordered(h_mn[2]) : 0.0f;
    }
    // insert pass, then the table's counts
    F_HIP(f, tab.reset_async(s));
    F_HIP(f, for_segments(N, [&](unsigned long long i0, int n) { return launch_voxel_insert(f->scene.pts, i0, n, g, t, st, s); }));
    F_HIP(f, launch_voxel_stats(t, min_points, st, s));
    F_HIP(f, hipMemcpyAsync(words, st, sizeof(unsigned long long) * kVoxWords, hipMemcpyDeviceToHost, s));
    F_HIP(f, hipStreamSynchronize(s));
    if (words[kVoxErr]) return ffail(f, ACMMP_ERR_HIP, "voxel table: a probe sequence covered every slot");
    const unsigned long long kept = words[kVoxKept];
    F_HIP(f, alloc(out.pts, 9 * static_cast<size_t>(kept)));
    F_HIP(f, alloc(out.cnt, static_cast<size_t>(kept)));
    F_HIP(f, alloc(out.sums, 9 * static_cast<size_t>(kept)));
    F_HIP(f, alloc(out.slot, static_cast<size_t>(kept)));
    if (kept == 0) return ACMMP_OK;
    // compaction in order of first appearance, the sums, the means
    unsigned long long end[2] = {0, 0};                                  // error word, voxels compacted
    F_HIP(f, hipMemsetAsync(out.sums, 0, sizeof(unsigned long long) * 9 * kept, s));
    F_HIP(f, hipMemsetAsync(out.slot, 0xff, sizeof(unsigned long long) * kept, s));
    F_HIP(f, compact_pass(f, N, kept, &end[1], [&](unsigned long long i0, int n, Compaction c) {
        return launch_voxel_compact(f->scene.pts, i0, n, g, t, min_points, c, out.slot, st, s);
    }));
    F_HIP(f, for_segments(N, [&](unsigned long long i0, int n) { return launch_voxel_accumulate(f->scene.pts, i0, n, g, t, out.sums, st, s); }));
    F_HIP(f, launch_voxel_finalise(kept, out.slot, t, out.sums, g, out.pts, out.cnt, s));
    F_HIP(f, hipMemcpyAsync(&end[0], st + kVoxErr, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    F_HIP(f, hipStreamSynchronize(s));
    if (end[0] || end[1] != kept)
        return ffail(f, ACMMP_ERR_HIP, "voxel table: lookup failed (flags " + std::to_string(end[0]) + ", compacted " +
                                           std::to_string(end[1]) + " of " + std::to_string(kept) + ")");
    return ACMMP_OK;
}

}  // namespace

extern "C" {

acmmp_status acmmp_fusion_voxelize(acmmp_fusion* f, float voxel_size, const float* origin, int min_points,
                                   int64_t* n_voxels, int64_t* n_occupied, int64_t* n_rejected, float* origin_used) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    if (!finite32(voxel_size) || !(voxel_size > 0.0f)) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "voxel size must be finite and > 0");
    if (min_points < 1) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "min_points must be at least 1");
    if (origin && !(finite32(origin[0]) && finite32(origin[1]) && finite32(origin[2])))
        return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "origin must be finite");
    if (!f->s_have) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "no scene result: acmmp_fusion_run_scene first");
    const unsigned long long N = f->s_total;
    unsigned long long slots = 1024;
    if (f->v_force_slots != 0) {
        const long long v = f->v_force_slots;
        if (v < 64 || (v & (v - 1)) != 0 || static_cast<unsigned long long>(v) <= N)
            return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "forced table size must be a power of two >= 64 and > the scene's points");
        slots = static_cast<unsigned long long>(v);
    } else {
        if (N > (1ull << 61)) return ffail(f, ACMMP_ERR_UNSUPPORTED, "scene too large for the voxel table");
        while (slots < 2 * N) slots <<= 1;
    }
    F_HIP(f, hipSetDevice(f->device));
    VoxGrid g;
    g.ox = origin ? origin[0] : 0.0f;
    g.oy = origin ? origin[1] : 0.0f;
    g.oz = origin ? origin[2] : 0.0f;
    g.size = voxel_size;
    g.inv = 1.0f / voxel_size;
    VoxelOut out;
    unsigned long long words[kVoxWords] = {0};
    // the table of the voxel result held stays as it is until the run has succeeded: the run fills the spare one,
    // and the two change places
    VoxTableBuf& from = f->v_tab_live ? f->v_tab_spare : f->v_tab;
    VoxTableBuf tab = std::move(from);
    from = VoxTableBuf();
    if (N > 0) {
        const acmmp_status st = voxel_run(f, g, origin == nullptr, min_points, slots, tab, out, words);
        if (st != ACMMP_OK) {
            (void)run_failed(f, st);
            from = std::move(tab);                    // after the stream has drained
            return st;
        }
    }
    out.sums.reset();
    if (f->v_tab_live) f->v_tab_spare = std::move(f->v_tab);
    f->v_tab = std::move(tab);
    f->v_tab_live = N > 0;
    out.total = words[kVoxKept];
    out.grid = g;
    out.have = true;
    f->voxels = std::move(out);
    invalidate(f, R_VOXELS);                          // whatever described the previous voxel result
    f->v_stats[0] = static_cast<long long>(slots);
    f->v_stats[1] = static_cast<long long>(words[kVoxOccupied]);
    f->v_stats[2] = static_cast<long long>(words[kVoxMaxProbe]);
    f->v_stats[3] = static_cast<long long>(words[kVoxWrapped]);
    if (n_voxels) *n_voxels = static_cast<int64_t>(words[kVoxKept]);
    if (n_occupied) *n_occupied = static_cast<int64_t>(words[kVoxOccupied]);
    if (n_rejected) *n_rejected = static_cast<int64_t>(words[kVoxRejected]);
    if (origin_used) { origin_used[0] = g.ox; origin_used[1] = g.oy; origin_used[2] = g.oz; }
    return ACMMP_OK;
}

acmmp_status acmmp_fusion_voxel_points(acmmp_fusion* f, int64_t first, int64_t n, float* points, int32_t* counts) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    return read_result(f, first, n, f->voxels.total, "range beyond the voxel result", [&](size_t a, size_t m) -> acmmp_status {
        F_HIP(f, read_range<float>(points, f->voxels.pts, a, m, 9));
        F_HIP(f, read_range<int32_t>(counts, f->voxels.cnt, a, m));
        return ACMMP_OK;
    });
}

acmmp_status acmmp_fusion_voxel_table(acmmp_fusion* f, int64_t force_slots, int64_t* slots, int64_t* occupied,
                                      int64_t* max_probe, int64_t* wrapped) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    f->v_force_slots = force_slots;                   // checked against the scene by the next voxelize
    if (slots) *slots = f->v_stats[0];
    if (occupied) *occupied = f->v_stats[1];
    if (max_probe) *max_probe = f->v_stats[2];
    if (wrapped) *wrapped = f->v_stats[3];
    return ACMMP_OK;
}

}  // extern "C"

// ---- cleaning the voxel result (include/acmmp.h; kernels: k_clean_*) ---------------------------------------

namespace {

// The new result of a clean run.
struct CleanOut : CleanRec {
    DevBuf<unsigned long long> scratch;      // per voxel: component voxels, points, dense id
    unsigned long long comps_kept = 0, unsupported = 0, rounds = 0;
};

acmmp_status clean_run(acmmp_fusion* f, int connectivity, int min_neighbours, unsigned long long min_voxels,
                       unsigned long long min_points, CleanOut& out) {
    hipStream_t s = f->stream;
    const unsigned long long nv = f->voxels.total;
    const size_t n = static_cast<size_t>(nv);
    if (!f->c_words) F_HIP(f, alloc(f->c_words, kCleanWords));
    F_HIP(f, segment_reserve(f, nv));
    F_HIP(f, alloc(out.lab, n));
    F_HIP(f, alloc(out.mask, n));
    F_HIP(f, alloc(out.scratch, 3 * n));
    const VoxTable t = f->v_tab.view();
    unsigned long long* w = f->c_words;
    const CleanComp c = {out.scratch, out.scratch + n, out.scratch + 2 * n, min_voxels, min_points};
    unsigned long long h[kCleanWords] = {0};
    F_HIP(f, hipMemsetAsync(w, 0, sizeof(unsigned long long) * kCleanWords, s));
    F_HIP(f, hipMemsetAsync(out.scratch, 0, sizeof(unsigned long long) * 2 * n, s));
    F_HIP(f, launch_clean_support(nv, f->voxels.slot, t, connectivity, min_neighbours, out.mask, out.lab, w, s));
    // Rounds until one lowers no label.  After k rounds a label is at most the smallest index within k edges, so
    // nv rounds settle every label and one more sees no change: a run past that bound has gone wrong.
    for (;;) {
        if (out.rounds > nv + 1) return ffail(f, ACMMP_ERR_HIP, "voxel clean: the labelling did not settle in nv + 2 rounds");
        ++out.rounds;
        F_HIP(f, hipMemsetAsync(w + kCleanChanged, 0, sizeof(unsigned long long), s));
        F_HIP(f, launch_clean_round(nv, f->voxels.slot, t, out.mask, out.lab, w, s));
        F_HIP(f, hipMemcpyAsync(h, w, sizeof(unsigned long long) * 2, hipMemcpyDeviceToHost, s));
        F_HIP(f, hipStreamSynchronize(s));
        if (h[kCleanErr]) return ffail(f, ACMMP_ERR_HIP, "voxel clean: lookup failed (flags " + std::to_string(h[kCleanErr]) + ")");
        if (!h[kCleanChanged]) break;
    }
    F_HIP(f, launch_clean_sizes(nv, out.lab, f->voxels.cnt, c, w, s));
    F_HIP(f, hipMemcpyAsync(h, w, sizeof(unsigned long long) * kCleanWords, hipMemcpyDeviceToHost, s));
    F_HIP(f, hipStreamSynchronize(s));
    out.unsupported = h[kCleanUnsupported];
    out.comps = h[kCleanComps];
    out.comps_kept = h[kCleanCompsKept];
    out.kept = h[kCleanKept];
    if (out.comps > nv || out.kept > nv) return ffail(f, ACMMP_ERR_HIP, "voxel clean: counts beyond the voxel result");
    const size_t nc = static_cast<size_t>(out.comps), nk = static_cast<size_t>(out.kept);
    F_HIP(f, alloc(out.table, 3 * nc));
    F_HIP(f, alloc(out.pts, 9 * nk));
    F_HIP(f, alloc(out.cnt, nk));
    F_HIP(f, alloc(out.comp, nk));
    F_HIP(f, alloc(out.vox, nk));
    // the roots, then the kept voxels, each compacted in voxel order, segment after segment
    unsigned long long done[2] = {0, 0};
    F_HIP(f, compact_pass(f, nv, out.comps, &done[0], [&](unsigned long long i0, int m, Compaction k) {
        return launch_clean_compact_roots(nv, i0, m, out.lab, c, k, out.table, out.table + nc, out.table + 2 * nc, s);
    }));
    F_HIP(f, compact_pass(f, nv, out.kept, &done[1], [&](unsigned long long i0, int m, Compaction k) {
        return launch_clean_compact_kept(nv, i0, m, out.lab, c, k, f->voxels.pts, f->voxels.cnt, out.pts, out.cnt, out.comp, out.vox, s);
    }));
    F_HIP(f, hipStreamSynchronize(s));
    if (done[0] != out.comps || done[1] != out.kept)
        return ffail(f, ACMMP_ERR_HIP, "voxel clean: compacted " + std::to_string(done[0]) + " of " + std::to_string(out.comps) +
                                           " components, " + std::to_string(done[1]) + " of " + std::to_string(out.kept) + " voxels");
    return ACMMP_OK;
}

}  // namespace

extern "C" {

acmmp_status acmmp_fusion_voxel_clean(acmmp_fusion* f, int connectivity, int min_neighbours, int64_t min_component_voxels,
                                      int64_t min_component_points, int64_t* n_kept, int64_t* n_components,
                                      int64_t* n_components_kept, int64_t* n_unsupported, int64_t* rounds) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    if (connectivity != 6 && connectivity != 18 && connectivity != 26)
        return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "connectivity must be 6, 18 or 26");
    if (min_neighbours < 0) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "min_neighbours must not be negative");
    if (min_component_voxels < 1 || min_component_points < 1)
        return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "component thresholds must be at least 1");
    if (!f->voxels.have) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "no voxel result: acmmp_fusion_voxelize first");
    F_HIP(f, hipSetDevice(f->device));
    CleanOut out;
    if (f->voxels.total > 0) {
        const acmmp_status st = clean_run(f, connectivity, min_neighbours, static_cast<unsigned long long>(min_component_voxels),
                                          static_cast<unsigned long long>(min_component_points), out);
        if (st != ACMMP_OK) return run_failed(f, st);
    }
    out.have = true;
    f->clean = std::move(out);
    invalidate(f, R_CLEAN);                           // whatever was computed from the previous clean result
    if (n_kept) *n_kept = static_cast<int64_t>(out.kept);
    if (n_components) *n_components = static_cast<int64_t>(out.comps);
    if (n_components_kept) *n_components_kept = static_cast<int64_t>(out.comps_kept);
    if (n_unsupported) *n_unsupported = static_cast<int64_t>(out.unsupported);
    if (rounds) *rounds = static_cast<int64_t>(out.rounds);
    return ACMMP_OK;
}

acmmp_status acmmp_fusion_clean_points(acmmp_fusion* f, int64_t first, int64_t n, float* points, int32_t* counts,
                                       int64_t* component) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    return read_result(f, first, n, f->clean.kept, "range beyond the clean result", [&](size_t a, size_t m) -> acmmp_status {
        F_HIP(f, read_range<float>(points, f->clean.pts, a, m, 9));
        F_HIP(f, read_range<int32_t>(counts, f->clean.cnt, a, m));
        F_HIP(f, read_range<long long>(reinterpret_cast<long long*>(component), f->clean.comp, a, m));
        return ACMMP_OK;
    });
}

acmmp_status acmmp_fusion_voxel_labels(acmmp_fusion* f, int64_t first, int64_t n, int64_t* label, int32_t* support) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    return read_result(f, first, n, f->clean.have ? f->voxels.total : 0ull, "range beyond the labelled voxel result",
                       [&](size_t a, size_t m) -> acmmp_status {
        // the device holds ~0 for an unsupported voxel, which reads as -1, and the neighbours as one bit each
        F_HIP(f, read_range<unsigned long long>(reinterpret_cast<unsigned long long*>(label), f->clean.lab, a, m));
        F_HIP(f, read_range<uint32_t>(reinterpret_cast<uint32_t*>(support), f->clean.mask, a, m));
        if (support)
            for (size_t i = 0; i < m; ++i) support[i] = __builtin_popcount(static_cast<uint32_t>(support[i]));
        return ACMMP_OK;
    });
}

acmmp_status acmmp_fusion_component_table(acmmp_fusion* f, int64_t first, int64_t n, int64_t* root, int64_t* voxels,
                                          int64_t* points) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    return read_result(f, first, n, f->clean.comps, "range beyond the component table", [&](size_t a, size_t m) -> acmmp_status {
        const size_t nc = static_cast<size_t>(f->clean.comps);
        F_HIP(f, read_range<long long>(reinterpret_cast<long long*>(root), f->clean.table, a, m));
        F_HIP(f, read_range<long long>(reinterpret_cast<long long*>(voxels), f->clean.table + nc, a, m));
        F_HIP(f, read_range<long long>(reinterpret_cast<long long*>(points), f->clean.table + 2 * nc, a, m));
        return ACMMP_OK;
    });
}

}  // extern "C"

// ---- visibility check of the voxel or clean result (include/acmmp.h; kernels: k_vis_*) ----------------------

namespace {

// The new result of a visibility run.
struct VisOut : VisRec {
    unsigned long long no_support = 0, conflicting = 0, classes[4] = {0, 0, 0, 0};
};

acmmp_status visibility_run(acmmp_fusion* f, const Cloud& src, int n_list, const int* views, float rel_tol, int radius,
                            int min_support, int max_conflicts, VisOut& out) {
    hipStream_t s = f->stream;
    const unsigned long long N = src.n;
    if (!f->vis_words) F_HIP(f, alloc(f->vis_words, kVisWords));
    if (!f->vis_list) F_HIP(f, alloc(f->vis_list, kVisMaxList));
    F_HIP(f, segment_reserve(f, N));
    F_HIP(f, alloc(out.tal, 3 * static_cast<size_t>(N)));
    unsigned long long* w = f->vis_words;
    unsigned long long h[kVisWords] = {0};
    F_HIP(f, hipMemsetAsync(w, 0, sizeof(unsigned long long) * kVisWords, s));
    F_HIP(f, hipMemcpyAsync(f->vis_list, views, sizeof(int) * n_list, hipMemcpyHostToDevice, s));
    F_HIP(f, launch_vis_tally(f->model, f->d_cams, f->d_views, f->vis_list, n_list, src.pts, N, rel_tol, radius, out.tal, s));
    F_HIP(f, launch_vis_count(N, out.tal, n_list, min_support, max_conflicts, w, s));
    // the first host wait: the kept count, to size the result before anything is written there
    F_HIP(f, hipMemcpyAsync(h, w, sizeof(unsigned long long) * kVisWords, hipMemcpyDeviceToHost, s));
    F_HIP(f, hipStreamSynchronize(s));
    out.kept = h[kVisKept];
    out.no_support = h[kVisNoSupport];
    out.conflicting = h[kVisConflicting];
    for (int k = 0; k < 4; ++k) out.classes[k] = h[kVisSupport + k];
    if (out.kept > N) return ffail(f, ACMMP_ERR_HIP, "voxel visibility: kept count beyond the source");
    const size_t nk = static_cast<size_t>(out.kept);
    F_HIP(f, alloc(out.pts, 9 * nk));
    F_HIP(f, alloc(out.cnt, nk));
    F_HIP(f, alloc(out.kept_tal, 3 * nk));
    F_HIP(f, alloc(out.vox, nk));
    // the kept entries, compacted in entry order, segment after segment
    unsigned long long done = 0;
    F_HIP(f, compact_pass(f, N, out.kept, &done, [&](unsigned long long i0, int n, Compaction c) {
        return launch_vis_compact(i0, n, out.tal, min_support, max_conflicts, c, src.pts, src.cnt, out.pts, out.cnt,
                                  out.kept_tal, src.vox, out.vox, s);
    }));
    F_HIP(f, hipStreamSynchronize(s));
    if (done != out.kept)
        return ffail(f, ACMMP_ERR_HIP, "voxel visibility: compacted " + std::to_string(done) + " of " +
                                           std::to_string(out.kept) + " entries");
    return ACMMP_OK;
}

}  // namespace

extern "C" {

acmmp_status acmmp_fusion_voxel_visibility(acmmp_fusion* f, int source, int n_list, const int* views, float rel_tol,
                                           int radius, int min_support, int max_conflicts, int64_t* n_kept,
                                           int64_t* n_unsupported, int64_t* n_conflicting, int64_t class_totals[4]) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    const Res id = vis_source(source);
    if (id == R_NONE) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "source must be ACMMP_VIS_FROM_VOXELS or ACMMP_VIS_FROM_CLEAN");
    const Cloud src = cloud(f, id);
    if (!src.have)
        return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, id == R_VOXELS ? "no voxel result: acmmp_fusion_voxelize first"
                                                                   : "no clean result: acmmp_fusion_voxel_clean first");
    const acmmp_status listed = check_view_list(f, n_list, views);
    if (listed != ACMMP_OK) return listed;
    if (!finite32(rel_tol) || !(rel_tol >= 0.0f)) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "rel_tol must be finite and >= 0");
    if (radius != 0 && radius != 1) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "radius must be 0 or 1");
    if (min_support < 0 || max_conflicts < 0)
        return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "min_support and max_conflicts must not be negative");
    F_HIP(f, hipSetDevice(f->device));
    VisOut out;
    if (src.n > 0) {
        const acmmp_status st = visibility_run(f, src, n_list, views, rel_tol, radius, min_support, max_conflicts, out);
        if (st != ACMMP_OK) return run_failed(f, st);
    }
    out.entries = src.n;
    out.source = id;
    out.have = true;
    f->visible = std::move(out);
    invalidate(f, R_VISIBLE);                         // whatever was computed from the previous visible result
    if (n_kept) *n_kept = static_cast<int64_t>(out.kept);
    if (n_unsupported) *n_unsupported = static_cast<int64_t>(out.no_support);
    if (n_conflicting) *n_conflicting = static_cast<int64_t>(out.conflicting);
    if (class_totals)
        for (int k = 0; k < 4; ++k) class_totals[k] = static_cast<int64_t>(out.classes[k]);
    return ACMMP_OK;
}

acmmp_status acmmp_fusion_visible_points(acmmp_fusion* f, int64_t first, int64_t n, float* points, int32_t* counts,
                                         int32_t* tallies) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    return read_result(f, first, n, f->visible.kept, "range beyond the visible result", [&](size_t a, size_t m) -> acmmp_status {
        F_HIP(f, read_range<float>(points, f->visible.pts, a, m, 9));
        F_HIP(f, read_range<int32_t>(counts, f->visible.cnt, a, m));
        F_HIP(f, read_range<int32_t>(tallies, f->visible.kept_tal, a, m, 3));
        return ACMMP_OK;
    });
}

acmmp_status acmmp_fusion_visibility_tallies(acmmp_fusion* f, int64_t first, int64_t n, int32_t* tallies) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    return read_result(f, first, n, f->visible.entries, "range beyond the tallied source", [&](size_t a, size_t m) -> acmmp_status {
        F_HIP(f, read_range<int32_t>(tallies, f->visible.tal, a, m, 3));
        return ACMMP_OK;
    });
}

}  // extern "C"

// ---- surface mesh of the voxel, clean or visible result (include/acmmp.h; kernels: k_mesh_*) -----------------

namespace {

// The new result of a mesh call and the call's sample table (scratch).
struct MeshOut : MeshRec {
    DevBuf<unsigned long long> keys, rank, ent, sid;       // the table, `slots` of each
    unsigned long long slots = 0;
    DevBuf<unsigned long long> ekey;                       // per entry
    DevBuf<uint8_t> cflag, fbits;                          // per sample
    DevBuf<int32_t> vid;                                   // per sample
    unsigned long long valid = 0, cubes = 0, uncoloured = 0;
    long long stats[4] = {0, 0, 0, 0};
    MeshTable table() const { return {keys, rank, ent, sid, slots, log2_ceil(slots)}; }
    // every slot empty
    hipError_t table_reset_async(hipStream_t s) const {
        hipError_t e = hipSuccess;
        for (unsigned long long* a : {keys.get(), rank.get(), ent.get(), sid.get()})
            if (e == hipSuccess) e = hipMemsetAsync(a, 0xff, sizeof(unsigned long long) * slots, s);
        return e;
    }
};

acmmp_status mesh_run(acmmp_fusion* f, const Cloud& src, int n_list, const int* views, float trunc, int min_weight,
                      unsigned long long slots, MeshOut& out) {
    hipStream_t s = f->stream;
    const unsigned long long ne = src.n, pairs = 27ull * ne;
    if (!f->m_words) F_HIP(f, alloc(f->m_words, kMeshWords));
    if (!f->vis_list) F_HIP(f, alloc(f->vis_list, kVisMaxList));
    F_HIP(f, segment_reserve(f, pairs));
    F_HIP(f, alloc(out.keys, slots));
    F_HIP(f, alloc(out.rank, slots));
    F_HIP(f, alloc(out.ent, slots));
    F_HIP(f, alloc(out.sid, slots));
    out.slots = slots;
    F_HIP(f, alloc(out.ekey, static_cast<size_t>(ne)));
    const VoxTable vt = f->v_tab.view();
    const MeshTable m = out.table();
    unsigned long long* w = f->m_words;
    unsigned long long h[kMeshWords] = {0};
    F_HIP(f, hipMemsetAsync(w, 0, sizeof(unsigned long long) * kMeshWords, s));
    F_HIP(f, out.table_reset_async(s));
    F_HIP(f, hipMemcpyAsync(f->vis_list, views, sizeof(int) * n_list, hipMemcpyHostToDevice, s));
    // the samples: insert, then the table's counts
    F_HIP(f, launch_mesh_keys(ne, src.vox, f->voxels.total, f->voxels.slot, vt, out.ekey, w, s));
    F_HIP(f, for_segments(pairs, [&](unsigned long long p0, int n) { return launch_mesh_insert(p0, n, out.ekey, m, w, s); }));
    F_HIP(f, launch_mesh_stats(m, w, s));
    // the first host wait: the sample count, to size the per-sample arrays
    F_HIP(f, hipMemcpyAsync(h, w, sizeof(unsigned long long) * kMeshWords, hipMemcpyDeviceToHost, s));
    F_HIP(f, hipStreamSynchronize(s));
    if (h[kMeshErr] & 1ull) return ffail(f, ACMMP_ERR_HIP, "voxel mesh: an entry's voxel is not in the voxel table");
    if (h[kMeshErr]) return ffail(f, ACMMP_ERR_HIP, "voxel mesh: the sample table is full (" + std::to_string(slots) + " slots)");
    out.ns = h[kMeshOccupied];
    out.stats[0] = static_cast<long long>(slots);
    out.stats[1] = static_cast<long long>(h[kMeshOccupied]);
    out.stats[2] = static_cast<long long>(h[kMeshMaxProbe]);
    out.stats[3] = static_cast<long long>(h[kMeshWrapped]);
    if (out.ns > pairs) return ffail(f, ACMMP_ERR_HIP, "voxel mesh: more samples than (entry, offset) pairs");
    const size_t ns = static_cast<size_t>(out.ns);
    // the compactions run over the 27 ne pairs, the ns samples and the 3 ns (sample, axis) pairs
    F_HIP(f, segment_reserve(f, std::max(pairs, 3ull * out.ns)));
    F_HIP(f, alloc(out.skey, ns));
    F_HIP(f, alloc(out.tsdf, 2 * ns));
    F_HIP(f, alloc(out.sent, ns));
    F_HIP(f, alloc(out.cflag, ns));
    F_HIP(f, alloc(out.fbits, ns));
    F_HIP(f, alloc(out.vid, ns));
    const MeshSamples smp = {out.skey, out.tsdf, out.sent, out.ns};
    unsigned long long done[3] = {0, 0, 0};
    F_HIP(f, compact_pass(f, pairs, out.ns, &done[0], [&](unsigned long long p0, int n, Compaction c) {
        return launch_mesh_number(p0, n, out.ekey, m, c, smp, w, s);
    }));
    // the distances, the cubes, the pairs that emit faces
    F_HIP(f, launch_mesh_tsdf(f->model, f->d_cams, f->d_views, f->vis_list, n_list, smp, f->voxels.grid, trunc, s));
    F_HIP(f, launch_mesh_cubes(smp, m, min_weight, out.cflag, out.fbits, w, s));
    // the second host wait: the vertex and face counts, to size the result
    F_HIP(f, hipMemcpyAsync(h, w, sizeof(unsigned long long) * kMeshWords, hipMemcpyDeviceToHost, s));
    F_HIP(f, hipStreamSynchronize(s));
    if (h[kMeshErr] || done[0] != out.ns)
        return ffail(f, ACMMP_ERR_HIP, "voxel mesh: sample lookup failed (flags " + std::to_string(h[kMeshErr]) + ", numbered " +
                                           std::to_string(done[0]) + " of " + std::to_string(out.ns) + ")");
    out.valid = h[kMeshValid];
    out.cubes = h[kMeshCubes];
    out.nv = h[kMeshActive];
    const unsigned long long n_pairs = h[kMeshPairs];
    out.nf = 2ull * n_pairs;
    if (out.nv > out.ns || n_pairs > 3ull * out.ns) return ffail(f, ACMMP_ERR_HIP, "voxel mesh: counts beyond the samples");
    if (out.nv > 0x7fffffffull) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "voxel mesh: more than 2^31 - 1 vertices");
    F_HIP(f, alloc(out.verts, 9 * static_cast<size_t>(out.nv)));
    F_HIP(f, alloc(out.faces, 6 * static_cast<size_t>(n_pairs)));
    F_HIP(f, hipMemsetAsync(out.vid, 0xff, sizeof(int32_t) * ns, s));
    F_HIP(f, compact_pass(f, out.ns, out.nv, &done[1], [&](unsigned long long i0, int n, Compaction c) {
        return launch_mesh_vertices(i0, n, smp, m, f->voxels.grid, out.cflag, src.pts, c, out.verts, out.vid, w, s);
    }));
    F_HIP(f, compact_pass(f, 3ull * out.ns, n_pairs, &done[2], [&](unsigned long long p0, int n, Compaction c) {
        return launch_mesh_faces(p0, n, smp, m, out.cflag, out.fbits, out.vid, c, out.faces, w, s);
    }));
    // the third host wait: the end
    F_HIP(f, hipMemcpyAsync(h, w, sizeof(unsigned long long) * kMeshWords, hipMemcpyDeviceToHost, s));
    F_HIP(f, hipStreamSynchronize(s));
    if (h[kMeshErr] || done[1] != out.nv || done[2] != n_pairs)
        return ffail(f, ACMMP_ERR_HIP, "voxel mesh: extraction failed (flags " + std::to_string(h[kMeshErr]) + ", " +
                                           std::to_string(done[1]) + " of " + std::to_string(out.nv) + " vertices, " +
                                           std::to_string(done[2]) + " of " + std::to_string(n_pairs) + " quads)");
    out.uncoloured = h[kMeshUncoloured];
    return ACMMP_OK;
}

}  // namespace

extern "C" {

acmmp_status acmmp_fusion_voxel_mesh(acmmp_fusion* f, int source, int n_list, const int* views, float trunc, int min_weight,
                                     int64_t* n_vertices, int64_t* n_faces, int64_t* n_samples, int64_t* n_valid,
                                     int64_t* n_cubes, int64_t* n_uncoloured) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    const Res id = mesh_source(source);
    if (id == R_NONE) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "source must be one of ACMMP_MESH_FROM_*");
    const Cloud src = cloud(f, id);
    if (!src.have) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "no such source result");
    const acmmp_status listed = check_view_list(f, n_list, views);
    if (listed != ACMMP_OK) return listed;
    if (!finite32(trunc) || !(trunc > 0.0f)) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "trunc must be finite and > 0");
    if (min_weight < 1) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "min_weight must be at least 1");
    const unsigned long long ne = src.n;
    unsigned long long slots = 1024;
    if (f->m_force_slots != 0) {
        const long long v = f->m_force_slots;
        if (v < 64 || (v & (v - 1)) != 0) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "forced table size must be a power of two >= 64");
        slots = static_cast<unsigned long long>(v);
    } else {
        if (ne > (1ull << 54)) return ffail(f, ACMMP_ERR_UNSUPPORTED, "source too large for the sample table");
        while (slots < 54ull * ne) slots <<= 1;
    }
    F_HIP(f, hipSetDevice(f->device));
    MeshOut out;
    if (ne > 0) {
        const acmmp_status st = mesh_run(f, src, n_list, views, trunc, min_weight, slots, out);
        if (st != ACMMP_OK) return run_failed(f, st);
    } else {
        out.stats[0] = static_cast<long long>(slots);
    }
    out.source = id;
    out.have = true;
    invalidate(f, R_MESH);                            // what showed the previous mesh result or was measured on it
    f->mesh = std::move(out);
    std::copy(out.stats, out.stats + 4, f->m_stats);
    if (n_vertices) *n_vertices = static_cast<int64_t>(out.nv);
    if (n_faces) *n_faces = static_cast<int64_t>(out.nf);
    if (n_samples) *n_samples = static_cast<int64_t>(out.ns);
    if (n_valid) *n_valid = static_cast<int64_t>(out.valid);
    if (n_cubes) *n_cubes = static_cast<int64_t>(out.cubes);
    if (n_uncoloured) *n_uncoloured = static_cast<int64_t>(out.uncoloured);
    return ACMMP_OK;
}

acmmp_status acmmp_fusion_mesh_vertices(acmmp_fusion* f, int64_t first, int64_t n, float* vertices) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    return read_result(f, first, n, f->mesh.nv, "range beyond the mesh result's vertices", [&](size_t a, size_t m) -> acmmp_status {
        F_HIP(f, read_range<float>(vertices, f->mesh.verts, a, m, 9));
        return ACMMP_OK;
    });
}

acmmp_status acmmp_fusion_mesh_faces(acmmp_fusion* f, int64_t first, int64_t n, int32_t* faces) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    return read_result(f, first, n, f->mesh.nf, "range beyond the mesh result's faces", [&](size_t a, size_t m) -> acmmp_status {
        F_HIP(f, read_range<int32_t>(faces, f->mesh.faces, a, m, 3));
        return ACMMP_OK;
    });
}

acmmp_status acmmp_fusion_mesh_samples(acmmp_fusion* f, int64_t first, int64_t n, int32_t* cells, int32_t* tsdf, int64_t* entry) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    return read_result(f, first, n, f->mesh.ns, "range beyond the mesh result's samples", [&](size_t a, size_t m) -> acmmp_status {
        if (cells) {
            std::vector<unsigned long long> keys(m);
            F_HIP(f, read_range<unsigned long long>(keys.data(), f->mesh.skey, a, m));
            for (size_t i = 0; i < m; ++i)
                for (int k = 0; k < 3; ++k) cells[3 * i + k] = static_cast<int32_t>((keys[i] >> (21 * k)) & 0x1fffffull);
        }
        F_HIP(f, read_range<int32_t>(tsdf, f->mesh.tsdf, a, m, 2));
        F_HIP(f, read_range<long long>(reinterpret_cast<long long*>(entry), f->mesh.sent, a, m));
        return ACMMP_OK;
    });
}

acmmp_status acmmp_fusion_mesh_table(acmmp_fusion* f, int64_t force_slots, int64_t* slots, int64_t* occupied,
                                     int64_t* max_probe, int64_t* wrapped) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    f->m_force_slots = force_slots;                   // checked by the next mesh call
    if (slots) *slots = f->m_stats[0];
    if (occupied) *occupied = f->m_stats[1];
    if (max_probe) *max_probe = f->m_stats[2];
    if (wrapped) *wrapped = f->m_stats[3];
    return ACMMP_OK;
}

acmmp_status acmmp_fusion_set_mesh(acmmp_fusion* f, int64_t nv, const float* vertices, int64_t nf, const int32_t* faces) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    if (nv < 0 || nf < 0 || nv > 0x7fffffffll || nf > 0x7fffffffll || (nv > 0 && !vertices) || (nf > 0 && !faces))
        return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "bad argument");
    for (int64_t i = 0; i < 3 * nf; ++i)
        if (faces[i] < 0 || faces[i] >= nv) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "vertex index out of range");
    F_HIP(f, hipSetDevice(f->device));
    // built beside the present mesh result, installed when both copies have succeeded; no result is its source
    MeshRec out;
    const size_t n = static_cast<size_t>(nv), m = static_cast<size_t>(nf);
    F_HIP(f, alloc(out.verts, 9 * n));
    F_HIP(f, alloc(out.faces, 3 * m));
    if (n > 0) F_HIP(f, hipMemcpy(out.verts, vertices, sizeof(float) * 9 * n, hipMemcpyHostToDevice));
    if (m > 0) F_HIP(f, hipMemcpy(out.faces, faces, sizeof(int32_t) * 3 * m, hipMemcpyHostToDevice));
    out.nv = static_cast<unsigned long long>(nv);
    out.nf = static_cast<unsigned long long>(nf);
    out.have = true;
    invalidate(f, R_MESH);
    f->mesh = std::move(out);
    return ACMMP_OK;
}

}  // extern "C"

// ---- the mesh result sampled into an area-uniform cloud (include/acmmp.h; kernels: k_sample_*) ----------------

namespace {

// The new result of a sample call and the call's offsets (scratch).
struct SampleOut : SampleRec {
    DevBuf<unsigned long long> loc;                        // per face: the samples before it in its chunk of 256 faces
    DevBuf<unsigned long long> chunk_tot, base;            // per chunk: its samples, the samples before it
};

acmmp_status sample_run(acmmp_fusion* f, double s2, unsigned long long seed, SampleOut& out) {
    hipStream_t s = f->stream;
    const MeshRec& m = f->mesh;
    const unsigned nf = static_cast<unsigned>(m.nf);
    const size_t n_chunks = (static_cast<size_t>(nf) + 255) / 256;
    if (!f->smp_words) F_HIP(f, alloc(f->smp_words, kSampleWords));
    F_HIP(f, alloc(out.loc, nf));
    F_HIP(f, alloc(out.chunk_tot, n_chunks));
    F_HIP(f, alloc(out.base, n_chunks));
    unsigned long long h[kSampleWords] = {0};
    F_HIP(f, hipMemsetAsync(f->smp_words, 0, sizeof(h), s));
    F_HIP(f, launch_sample_count(m.verts, m.nv, m.faces, nf, s2, seed, out.loc, out.chunk_tot, out.base, f->smp_words, s));
    // the first host wait: the total, to size the result
    F_HIP(f, hipMemcpyAsync(h, f->smp_words, sizeof(h), hipMemcpyDeviceToHost, s));
    F_HIP(f, hipStreamSynchronize(s));
    out.n = h[kSampleTotal];
    out.skipped = h[kSampleSkipped];
    if (out.n > 0x7fffffffull)
        return ffail(f, ACMMP_ERR_UNSUPPORTED, "mesh sample: " + std::to_string(out.n) + " samples, more than 2^31 - 1");
    const size_t N = static_cast<size_t>(out.n);
    F_HIP(f, alloc(out.pts, 9 * N));
    F_HIP(f, alloc(out.face, N));
    F_HIP(f, launch_sample_emit(m.verts, m.nv, m.faces, nf, seed, out.loc, out.base, out.n, out.pts, out.face, s));
    // the second host wait: the end
    F_HIP(f, hipStreamSynchronize(s));
    return ACMMP_OK;
}

}  // namespace

extern "C" {

acmmp_status acmmp_fusion_mesh_sample(acmmp_fusion* f, float spacing, uint64_t seed, int64_t* n_samples, int64_t* n_skipped) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    if (!f->mesh.have) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "no mesh result: acmmp_fusion_voxel_mesh or acmmp_fusion_set_mesh first");
    if (!finite32(spacing) || !(spacing > 0.0f)) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "spacing must be finite and > 0");
    if (f->mesh.nf > 0x7fffffffull) return ffail(f, ACMMP_ERR_UNSUPPORTED, "more than 2^31 - 1 faces");
    F_HIP(f, hipSetDevice(f->device));
    SampleOut out;
    const double s2 = static_cast<double>(spacing) * static_cast<double>(spacing);
    const acmmp_status st = sample_run(f, s2, static_cast<unsigned long long>(seed), out);
    if (st != ACMMP_OK) return run_failed(f, st);
    out.have = true;
    invalidate(f, R_SAMPLES);                         // what was measured on the previous samples or aligned from them
    f->samples = std::move(out);
    if (n_samples) *n_samples = static_cast<int64_t>(f->samples.n);
    if (n_skipped) *n_skipped = static_cast<int64_t>(f->samples.skipped);
    return ACMMP_OK;
}

acmmp_status acmmp_fusion_sample_points(acmmp_fusion* f, int64_t first, int64_t n, float* points, int32_t* face) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    return read_result(f, first, n, f->samples.n, "range beyond the sample result", [&](size_t a, size_t m) -> acmmp_status {
        F_HIP(f, read_range<float>(points, f->samples.pts, a, m, 9));
        F_HIP(f, read_range<int32_t>(face, f->samples.face, a, m));
        return ACMMP_OK;
    });
}

}  // extern "C"

// ---- the mesh result rendered into one camera (include/acmmp.h; kernels: k_render_*) ------------------------

namespace {

// The new result of a render.
struct RenderOut : RenderRec {
    DevBuf<unsigned long long> keys;                       // scratch: the z-buffer
    DevBuf<uint8_t> queue;                                 // scratch: the large faces
    unsigned long long words[kRenderWords] = {0};
};

acmmp_status render_run(acmmp_fusion* f, const DevCam& cam, const float* raw, float rel_tol, RenderOut& out) {
    hipStream_t s = f->stream;
    const size_t P = static_cast<size_t>(cam.W) * cam.H;
    const unsigned nf = static_cast<unsigned>(f->mesh.nf);
    if (!f->r_words) F_HIP(f, alloc(f->r_words, kRenderWords));
    F_HIP(f, alloc(out.depth, P));
    F_HIP(f, alloc(out.face, P));
    F_HIP(f, alloc(out.normal, 3 * P));
    F_HIP(f, alloc(out.colour, 3 * P));
    F_HIP(f, alloc(out.keys, P));
    F_HIP(f, alloc(out.queue, kRenderItemBytes * static_cast<size_t>(nf)));
    F_HIP(f, hipMemsetAsync(f->r_words, 0, sizeof(unsigned long long) * kRenderWords, s));
    F_HIP(f, hipMemsetAsync(out.keys, 0xff, sizeof(unsigned long long) * P, s));
    const long long small_max = f->r_small_max != 0 ? f->r_small_max : kRenderSmallMax;
    F_HIP(f, launch_render(f->model, cam, f->mesh.verts, f->mesh.nv, f->mesh.faces, nf, small_max, out.keys, out.queue.get(), raw, rel_tol,
                           out.depth, out.face, out.normal, out.colour, f->r_words, s));
    // the one host wait: the counts
    F_HIP(f, hipMemcpyAsync(out.words, f->r_words, sizeof(out.words), hipMemcpyDeviceToHost, s));
    F_HIP(f, hipStreamSynchronize(s));
    return ACMMP_OK;
}

}  // namespace

extern "C" {

acmmp_status acmmp_fusion_mesh_render(acmmp_fusion* f, int view, const acmmp_camera* cam, float rel_tol, int64_t counts[7],
                                      int64_t* n_skipped) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    if (!f->mesh.have) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "no mesh result: acmmp_fusion_voxel_mesh or acmmp_fusion_set_mesh first");
    if (!finite32(rel_tol) || !(rel_tol >= 0.0f)) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "rel_tol must be finite and >= 0");
    if (view < -1 || view >= f->n) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "view index out of range");
    DevCam dc;
    const float* raw = nullptr;
    if (view >= 0) {
        if (!f->views[view].depth) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "set_view first for the view rendered");
        dc = f->cams[view];
        raw = f->views[view].depth;
    } else {
        if (!cam) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "view -1 needs a camera");
        if (cam->model != f->model) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "the camera's model is not the set's");
        if (cam->width <= 0 || cam->height <= 0) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "the camera's size must be positive");
        dc = make_devcam(*cam);
    }
    if (static_cast<long long>(dc.W) * dc.H > 0x7fffffffll) return ffail(f, ACMMP_ERR_UNSUPPORTED, "more than 2^31 - 1 pixels");
    if (f->mesh.nf > 0x7fffffffull) return ffail(f, ACMMP_ERR_UNSUPPORTED, "more than 2^31 - 1 faces");
    F_HIP(f, hipSetDevice(f->device));
    RenderOut out;
    const acmmp_status st = render_run(f, dc, raw, rel_tol, out);
    if (st != ACMMP_OK) return run_failed(f, st);
    out.W = dc.W;
    out.H = dc.H;
    out.have = true;
    f->render = std::move(out);
    f->r_plan[0] = static_cast<long long>(out.words[kRenderSmall]);
    f->r_plan[1] = static_cast<long long>(out.words[kRenderLarge]);
    f->r_plan[2] = static_cast<long long>(out.words[kRenderCandidates]);
    if (counts)
        for (int k = 0; k < 7; ++k) counts[k] = static_cast<int64_t>(out.words[kRenderCounts + k]);
    if (n_skipped) *n_skipped = static_cast<int64_t>(out.words[kRenderSkipped]);
    return ACMMP_OK;
}

acmmp_status acmmp_fusion_render_maps(acmmp_fusion* f, float* depth, int32_t* face, float* normal, float* colour) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    if (!f->render.have) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "no render result: acmmp_fusion_mesh_render first");
    F_HIP(f, hipSetDevice(f->device));
    const RenderRec& r = f->render;
    const size_t P = static_cast<size_t>(r.W) * r.H;
    F_HIP(f, read_range<float>(depth, r.depth, 0, P));
    F_HIP(f, read_range<int32_t>(face, r.face, 0, P));
    F_HIP(f, read_range<float>(normal, r.normal, 0, P, 3));
    F_HIP(f, read_range<float>(colour, r.colour, 0, P, 3));
    return ACMMP_OK;
}

acmmp_status acmmp_fusion_render_plan(acmmp_fusion* f, int small_max, int64_t* n_small, int64_t* n_large, int64_t* n_candidates) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    f->r_small_max = small_max;
    if (n_small) *n_small = f->r_plan[0];
    if (n_large) *n_large = f->r_plan[1];
    if (n_candidates) *n_candidates = f->r_plan[2];
    return ACMMP_OK;
}

}  // extern "C"

// ---- nearest-neighbour distances between two clouds (include/acmmp.h; kernels: k_dist_*) ---------------------

namespace {

// The new result of a distance call and the call's scratch.
struct DistOut : DistRec {
    DevBuf<unsigned long long> keys, ckeys;                // scratch: the cell table and the coarse table
    DevBuf<uint32_t> start, cnt;
    DevBuf<float4> list;                                   // scratch: the cells' lists
    DevBuf<uint8_t> qcls, tcls;                            // scratch: the classes of a cropped query and target cloud
    double cell = 0.0;
    unsigned long long words[kDistWords] = {0};
};

// A grid of `cell` over the box [lo, hi]: the arithmetic of dist_axis (fusion_kernels.hip), on the host.
DistGrid dist_grid(const double lo[3], const double hi[3], double cell) {
    DistGrid g;
    g.cell = cell;
    g.inv = 1.0 / cell;
    for (int a = 0; a < 3; ++a) {
        g.o[a] = lo[a];
        g.cmax[a] = static_cast<int>(std::floor((hi[a] - lo[a]) * g.inv));
    }
    return g;
}

// The search grid over the targets of a distance or align call, and what the query passes need of it.
struct DistIndex {
    DistGrid g = {{0.0, 0.0, 0.0}, 1.0, 1.0, {0, 0, 0}}, cg = g;
    DistTable fine = {nullptr, nullptr, nullptr, 0, 0}, coarse = fine;
    DistQuery p;
    unsigned long long valid_targets = 0;
};

// Build: the device words cleared, the valid targets' bounding box and number (the first host wait), the cell, the
// tables and the cells' lists into out's scratch.  n_tau thresholds go into ix.p.
acmmp_status distance_build(acmmp_fusion* f, DistCloud t, float max_dist, int n_tau, const float* tau, DistOut& out,
                            DistIndex& ix) {
    hipStream_t s = f->stream;
    if (!f->dist_words) F_HIP(f, alloc(f->dist_words, kDistWords));
    unsigned long long* w = f->dist_words;
    F_HIP(f, hipMemsetAsync(w, 0, sizeof(unsigned long long) * kDistWords, s));
    F_HIP(f, hipMemsetAsync(w + kDistMin, 0xff, sizeof(unsigned long long) * 3, s));
    DistQuery& p = ix.p;
    p.m2 = max_dist * max_dist;
    p.k = 1048576.0 / static_cast<double>(max_dist);
    p.n_tau = n_tau;
    for (int i = 0; i < 8; ++i) p.tau2[i] = i < n_tau ? tau[i] * tau[i] : 0.0f;
    for (int a = 0; a < 3; ++a) p.lo[a] = p.hi[a] = 0.0;
    p.have_targets = 0;
    DistGrid& g = ix.g;
    DistGrid& cg = ix.cg;
    DistTable& fine = ix.fine;
    DistTable& coarse = ix.coarse;
    unsigned long long& valid_targets = ix.valid_targets;
    if (t.n > 0) {
        // the first host wait: the valid targets' bounding box and number, from which the cell is chosen
        unsigned long long h[kDistSummary] = {0};
        F_HIP(f, launch_dist_bounds(t, w, s));
        F_HIP(f, hipMemcpyAsync(h, w, sizeof(h), hipMemcpyDeviceToHost, s));
        F_HIP(f, hipStreamSynchronize(s));
        valid_targets = h[kDistValidTargets];
        if (valid_targets > t.n) return ffail(f, ACMMP_ERR_HIP, "cloud distance: more valid targets than targets");
        if (valid_targets > 0) {
            uint32_t mn[6];
            std::memcpy(mn, h + kDistMin, sizeof(mn));
            double ext = 0.0;
            for (int a = 0; a < 3; ++a) {
                p.lo[a] = static_cast<double>(vox_decode_ordered(mn[a]));
                p.hi[a] = -static_cast<double>(vox_decode_ordered(mn[3 + a]));
                ext = std::max(ext, p.hi[a] - p.lo[a]);
            }
            // a handful of targets per occupied cell for a cloud that fills its box, some tens for a surface, and no
            // wider than max_dist, so that a few outliers that stretch the box do not put the cloud into one cell;
            // never more than 2^20 cells on an axis, so that every target has a cell
            double cell = f->dist_force_cell != 0.0f
                              ? static_cast<double>(f->dist_force_cell)
                              : std::min(ext / std::cbrt(static_cast<double>(valid_targets)), static_cast<double>(max_dist));
            cell = std::max(cell, ext / 1048576.0);
            if (!(cell > 0.0)) cell = 1.0;
            g = dist_grid(p.lo, p.hi, cell);
            out.cell = cell;
            unsigned long long slots = 1024;
            while (slots < 2 * t.n) slots <<= 1;
            const int log2_slots = log2_ceil(slots);
            F_HIP(f, alloc(out.keys, slots));
            F_HIP(f, alloc(out.start, slots));
            F_HIP(f, alloc(out.cnt, slots));
            F_HIP(f, alloc(out.list, static_cast<size_t>(t.n)));
            fine = DistTable{out.keys, out.start, out.cnt, slots, log2_slots};
            F_HIP(f, hipMemsetAsync(out.keys, 0xff, sizeof(unsigned long long) * slots, s));
            F_HIP(f, hipMemsetAsync(out.cnt, 0, sizeof(uint32_t) * slots, s));
            // the coarse level, cells a little wider than max_dist; not where max_dist^2 is near the underflow range
            const double md = static_cast<double>(max_dist);
            if (md * md >= 0x1p-120) {
                cg = dist_grid(p.lo, p.hi, std::max(md * (1.0 + 0x1p-10), ext / 1048576.0));
                F_HIP(f, alloc(out.ckeys, slots));
                F_HIP(f, hipMemsetAsync(out.ckeys, 0xff, sizeof(unsigned long long) * slots, s));
                coarse = DistTable{out.ckeys, nullptr, nullptr, slots, log2_slots};
            }
            F_HIP(f, launch_dist_insert(t, g, fine, cg, coarse, w, s));
            F_HIP(f, launch_dist_lists(t, g, fine, out.list, w, s));
            p.have_targets = 1;
        }
    }
    return ACMMP_OK;
}

// The flags and the cursor of the device words after a query pass.
acmmp_status distance_check(acmmp_fusion* f, const unsigned long long* words, unsigned long long valid_targets) {
    if (words[kDistErr] || words[kDistCursor] != valid_targets)
        return ffail(f, ACMMP_ERR_HIP, "cloud distance: the cell table failed (flags " + std::to_string(words[kDistErr]) +
                                           ", listed " + std::to_string(words[kDistCursor]) + " of " +
                                           std::to_string(valid_targets) + " targets)");
    return ACMMP_OK;
}

acmmp_status distance_run(acmmp_fusion* f, DistCloud q, DistCloud t, float max_dist, int n_tau, const float* tau,
                          DistOut& out) {
    hipStream_t s = f->stream;
    F_HIP(f, alloc(out.d2, static_cast<size_t>(q.n)));
    F_HIP(f, alloc(out.nn, static_cast<size_t>(q.n)));
    DistIndex ix;
    const acmmp_status st = distance_build(f, t, max_dist, n_tau, tau, out, ix);
    if (st != ACMMP_OK) return st;
    unsigned long long* w = f->dist_words;
    F_HIP(f, launch_dist_query(q, ix.g, ix.fine, ix.cg, ix.coarse, out.list, ix.p, out.d2, out.nn, w, s));
    // the second host wait: the end
    F_HIP(f, hipMemcpyAsync(out.words, w, sizeof(out.words), hipMemcpyDeviceToHost, s));
    F_HIP(f, hipStreamSynchronize(s));
    const acmmp_status ck = distance_check(f, out.words, ix.valid_targets);
    if (ck != ACMMP_OK) return ck;
    out.words[kDistSummary + ACMMP_DIST_SUMMARY_N_QUERY] = q.n;
    return ACMMP_OK;
}

}  // namespace

extern "C" {

acmmp_status acmmp_fusion_set_reference_cloud(acmmp_fusion* f, int64_t n, const float* xyz) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    if (n < 0 || n > 0x7fffffffll || (n > 0 && !xyz)) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "bad argument");
    F_HIP(f, hipSetDevice(f->device));
    // built beside the present reference cloud, installed when the copy has succeeded
    RefRec out;
    const size_t m = static_cast<size_t>(n);
    F_HIP(f, alloc(out.pts, 3 * m));
    if (m > 0) F_HIP(f, hipMemcpy(out.pts, xyz, sizeof(float) * 3 * m, hipMemcpyHostToDevice));
    out.n = static_cast<unsigned long long>(n);
    out.have = true;
    f->ref = std::move(out);
    invalidate(f, R_REFERENCE);                       // what was measured against the previous one or aligned to it
    return ACMMP_OK;
}

acmmp_status acmmp_fusion_cloud_distance(acmmp_fusion* f, int source, int direction, float max_dist, int n_tau,
                                         const float* tau, int64_t* summary) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    const Res id = dist_source(source);
    if (id == R_NONE) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "source must be one of ACMMP_DIST_FROM_*");
    const Cloud src = cloud(f, id);
    DistCloud data = src.dist();
    if (f->xf_set) {
        data.xf = 1;
        std::memcpy(data.M, f->xf, sizeof(data.M));
    }
    if (direction != ACMMP_DIST_DATA_TO_REF && direction != ACMMP_DIST_REF_TO_DATA)
        return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "direction must be ACMMP_DIST_DATA_TO_REF or ACMMP_DIST_REF_TO_DATA");
    if (!src.have) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "no such data result");
    if (!f->ref.have) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "no reference cloud: acmmp_fusion_set_reference_cloud first");
    const acmmp_status taus = check_tau_list(f, max_dist, n_tau, tau);
    if (taus != ACMMP_OK) return taus;
    if (f->dist_force_cell != 0.0f && (!finite32(f->dist_force_cell) || !(f->dist_force_cell > 0.0f)))
        return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "the forced cell must be finite and > 0");
    const DistCloud ref = cloud(f, R_REFERENCE).dist();
    const bool d2r = direction == ACMMP_DIST_DATA_TO_REF;
    DistCloud q = d2r ? data : ref;
    DistCloud t = d2r ? ref : data;
    if (t.n > 0x7fffffffull) return ffail(f, ACMMP_ERR_UNSUPPORTED, "more than 2^31 - 1 targets");
    F_HIP(f, hipSetDevice(f->device));
    DistOut out;
    const RegionSet& qr = f->region[d2r ? ACMMP_REGION_DATA : ACMMP_REGION_REFERENCE];
    const RegionSet& tr = f->region[d2r ? ACMMP_REGION_REFERENCE : ACMMP_REGION_DATA];
    acmmp_status st = region_crop(f, qr, false, q, out.qcls, q);
    if (st == ACMMP_OK) st = region_crop(f, tr, true, t, out.tcls, t);
    if (st == ACMMP_OK) st = distance_run(f, q, t, max_dist, n_tau, tau, out);
    if (st != ACMMP_OK) return run_failed(f, st);
    out.n = q.n;
    out.source = id;
    out.have = true;
    f->dist = std::move(out);
    f->dist_cell = static_cast<float>(out.cell);
    f->dist_stats[0] = static_cast<long long>(out.words[kDistOccupied]);
    f->dist_stats[1] = static_cast<long long>(out.words[kDistMaxList]);
    f->dist_stats[2] = static_cast<long long>(out.words[kDistRings]);
    if (summary)
        for (int k = 0; k < ACMMP_DIST_SUMMARY_WORDS; ++k) summary[k] = static_cast<int64_t>(out.words[kDistSummary + k]);
    return ACMMP_OK;
}

acmmp_status acmmp_fusion_distance_results(acmmp_fusion* f, int64_t first, int64_t n, float* d2, int32_t* nearest) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    return read_result(f, first, n, f->dist.n, "range beyond the distance result", [&](size_t a, size_t m) -> acmmp_status {
        F_HIP(f, read_range<float>(d2, f->dist.d2, a, m));
        F_HIP(f, read_range<int32_t>(nearest, f->dist.nn, a, m));
        return ACMMP_OK;
    });
}

acmmp_status acmmp_fusion_distance_grid(acmmp_fusion* f, float force_cell, float* cell, int64_t* cells, int64_t* max_list,
                                        int64_t* rings) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    f->dist_force_cell = force_cell;                  // checked by the next distance call
    if (cell) *cell = f->dist_cell;
    if (cells) *cells = f->dist_stats[0];
    if (max_list) *max_list = f->dist_stats[1];
    if (rings) *rings = f->dist_stats[2];
    return ACMMP_OK;
}

}  // extern "C"

// ---- point-to-triangle distances from a cloud to the mesh result (include/acmmp.h; kernels: k_surf_*) ---------

namespace {

// The new result of a surface call and the call's scratch.
struct SurfOut : DistRec {
    DevBuf<unsigned long long> keys;                       // scratch: the cell table
    DevBuf<uint32_t> start, cnt;
    DevBuf<float4> list, large;                            // scratch: the cells' lists and the overflow list
    DevBuf<uint8_t> qcls;                                  // scratch: the classes of a cropped query cloud
    double cell = 0.0;
    unsigned long long valid_faces = 0;
    unsigned long long words[kSurfWords] = {0};
};

// The cell of the face grid: the edge of the mean face of a closed surface that fills its box.  Half the box's area
// is A = ex ey + ey ez + ez ex; F triangles of edge s cover about F s^2 / 2, so s = 2 sqrt(A / F).  A face then overlaps
// a handful of cells and a cell lists a handful of faces.  Unlike the cloud grid the cell is not capped by max_dist: a
// cell narrower than the faces would turn every face into a large one, and a wider one costs the capped search only the
// lists of the 27 cells around the query.  A box without area falls back to the cloud rule; never more than 2^20 cells
// on an axis.
double surface_cell(const double lo[3], const double hi[3], unsigned long long faces, float forced) {
    const double e[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
    const double ext = std::max(e[0], std::max(e[1], e[2])), n = static_cast<double>(faces);
    double cell = 2.0 * std::sqrt(((e[0] * e[1] + e[1] * e[2]) + e[2] * e[0]) / n);
    if (!(cell > 0.0) || !std::isfinite(cell)) cell = ext / std::cbrt(n);
    if (forced != 0.0f) cell = static_cast<double>(forced);
    cell = std::max(cell, ext / 1048576.0);
    if (!(cell > 0.0) || !std::isfinite(cell)) cell = 1.0;
    return cell;
}

acmmp_status surface_run(acmmp_fusion* f, DistCloud q, SurfMesh m, float max_dist, int n_tau, const float* tau, SurfOut& out) {
    hipStream_t s = f->stream;
    F_HIP(f, alloc(out.d2, static_cast<size_t>(q.n)));
    F_HIP(f, alloc(out.nn, static_cast<size_t>(q.n)));
    if (!f->surf_words) F_HIP(f, alloc(f->surf_words, kSurfWords));
    unsigned long long* w = f->surf_words;
    F_HIP(f, hipMemsetAsync(w, 0, sizeof(unsigned long long) * kSurfWords, s));
    F_HIP(f, hipMemsetAsync(w + kDistMin, 0xff, sizeof(unsigned long long) * 3, s));
    DistQuery p;
    p.m2 = max_dist * max_dist;
    p.k = 1048576.0 / static_cast<double>(max_dist);
    p.n_tau = n_tau;
    for (int i = 0; i < 8; ++i) p.tau2[i] = i < n_tau ? tau[i] * tau[i] : 0.0f;
    for (int a = 0; a < 3; ++a) p.lo[a] = p.hi[a] = 0.0;
    p.have_targets = 0;
    DistGrid g = {{0.0, 0.0, 0.0}, 1.0, 1.0, {0, 0, 0}};
    DistTable fine = {nullptr, nullptr, nullptr, 0, 0};
    unsigned long long regs = 0, n_large = 0;
    unsigned long long h[kDistSummary] = {0};
    if (m.nf > 0) {
        // the first host wait: the valid faces' bounding box and number, from which the cell is chosen
        F_HIP(f, launch_surf_bounds(m, w, s));
        F_HIP(f, hipMemcpyAsync(h, w, sizeof(h), hipMemcpyDeviceToHost, s));
        F_HIP(f, hipStreamSynchronize(s));
        out.valid_faces = h[kDistValidTargets];
        if (out.valid_faces > m.nf) return ffail(f, ACMMP_ERR_HIP, "surface distance: more valid faces than faces");
    }
    if (out.valid_faces > 0) {
        uint32_t mn[6];
        std::memcpy(mn, h + kDistMin, sizeof(mn));
        for (int a = 0; a < 3; ++a) {
            p.lo[a] = static_cast<double>(vox_decode_ordered(mn[a]));
            p.hi[a] = -static_cast<double>(vox_decode_ordered(mn[3 + a]));
        }
        out.cell = surface_cell(p.lo, p.hi, out.valid_faces, f->surf_force_cell);
        g = dist_grid(p.lo, p.hi, out.cell);
        const long long small_max = f->surf_small_max != 0 ? f->surf_small_max : kSurfSmallMax;
        // the second host wait: the plan, from which the table and the two lists are sized
        unsigned long long plan[kSurfWords] = {0};
        F_HIP(f, launch_surf_plan(m, g, small_max, w, s));
        F_HIP(f, hipMemcpyAsync(plan, w, sizeof(plan), hipMemcpyDeviceToHost, s));
        F_HIP(f, hipStreamSynchronize(s));
        regs = plan[kSurfRegs];
        n_large = plan[kSurfLarge];
        if (plan[kSurfSmall] + n_large != out.valid_faces)
            return ffail(f, ACMMP_ERR_HIP, "surface distance: the plan does not add up to the valid faces");
        if (regs > 0xffffffffull) return ffail(f, ACMMP_ERR_UNSUPPORTED, "more than 2^32 - 1 registrations: a larger cell or a smaller small_max");
        // no more cells can be occupied than the grid has or than there are registrations
        const double grid_cells = (g.cmax[0] + 1.0) * (g.cmax[1] + 1.0) * (g.cmax[2] + 1.0);
        const unsigned long long most = grid_cells < static_cast<double>(regs) ? static_cast<unsigned long long>(grid_cells) : regs;
        unsigned long long slots = 1024;
        while (slots < 2 * most) slots <<= 1;
        F_HIP(f, alloc(out.keys, slots));
        F_HIP(f, alloc(out.start, slots));
        F_HIP(f, alloc(out.cnt, slots));
        F_HIP(f, alloc(out.list, kSurfEntryWords * static_cast<size_t>(regs)));
        F_HIP(f, alloc(out.large, kSurfEntryWords * static_cast<size_t>(n_large)));
        fine = DistTable{out.keys, out.start, out.cnt, slots, log2_ceil(slots)};
        F_HIP(f, hipMemsetAsync(out.keys, 0xff, sizeof(unsigned long long) * slots, s));
        F_HIP(f, hipMemsetAsync(out.cnt, 0, sizeof(uint32_t) * slots, s));
        F_HIP(f, launch_surf_lists(m, g, fine, small_max, out.list, regs, out.large, n_large, w, s));
        p.have_targets = 1;
    }
    F_HIP(f, launch_surf_query(q, g, fine, out.list, out.large, static_cast<unsigned>(n_large), p, out.d2, out.nn, w, s));
    // the last host wait: the end
    F_HIP(f, hipMemcpyAsync(out.words, w, sizeof(out.words), hipMemcpyDeviceToHost, s));
    F_HIP(f, hipStreamSynchronize(s));
    if (out.words[kDistErr] || out.words[kDistCursor] != regs || out.words[kSurfLargeCursor] != n_large)
        return ffail(f, ACMMP_ERR_HIP, "surface distance: the cell table failed (flags " + std::to_string(out.words[kDistErr]) +
                                           ", listed " + std::to_string(out.words[kDistCursor]) + " of " + std::to_string(regs) +
                                           " registrations, " + std::to_string(out.words[kSurfLargeCursor]) + " of " +
                                           std::to_string(n_large) + " large faces)");
    out.words[kDistSummary + ACMMP_DIST_SUMMARY_N_QUERY] = q.n;
    return ACMMP_OK;
}

}  // namespace

extern "C" {

acmmp_status acmmp_fusion_surface_distance(acmmp_fusion* f, int query, float max_dist, int n_tau, const float* tau,
                                           int64_t* summary) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    const Res id = surf_source(query);
    if (id == R_NONE) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "query must be one of ACMMP_SURF_FROM_*");
    const Cloud src = cloud(f, id);
    DistCloud q = src.dist();
    if (!src.have) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "no such query result");
    if (!f->mesh.have) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "no mesh result: acmmp_fusion_voxel_mesh or acmmp_fusion_set_mesh first");
    const acmmp_status taus = check_tau_list(f, max_dist, n_tau, tau);
    if (taus != ACMMP_OK) return taus;
    if (f->surf_force_cell != 0.0f && (!finite32(f->surf_force_cell) || !(f->surf_force_cell > 0.0f)))
        return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "the forced cell must be finite and > 0");
    if (f->mesh.nf > 0x7fffffffull) return ffail(f, ACMMP_ERR_UNSUPPORTED, "more than 2^31 - 1 faces");
    if (q.n > 0x7fffffffull) return ffail(f, ACMMP_ERR_UNSUPPORTED, "more than 2^31 - 1 queries");
    // the frames: reference queries see the mesh under the transform, data queries share its frame
    SurfMesh m = {DistCloud{f->mesh.verts, 9, f->mesh.nv}, f->mesh.faces, static_cast<unsigned>(f->mesh.nf)};
    if (id == R_REFERENCE && f->xf_set) {
        m.v.xf = 1;
        std::memcpy(m.v.M, f->xf, sizeof(m.v.M));
    }
    F_HIP(f, hipSetDevice(f->device));
    SurfOut out;
    // the query side's region: a data query is classified where the region lives, under the transform that is set
    DistCloud read_as = q;
    if (id != R_REFERENCE && f->xf_set) {
        read_as.xf = 1;
        std::memcpy(read_as.M, f->xf, sizeof(read_as.M));
    }
    acmmp_status st = region_crop(f, f->region[id == R_REFERENCE ? ACMMP_REGION_REFERENCE : ACMMP_REGION_DATA], false, read_as,
                                  out.qcls, q);
    if (st == ACMMP_OK) st = surface_run(f, q, m, max_dist, n_tau, tau, out);
    if (st != ACMMP_OK) return run_failed(f, st);
    out.n = q.n;
    out.source = id;
    out.have = true;
    f->surf = std::move(out);
    f->surf_plan[0] = static_cast<long long>(out.words[kSurfSmall]);
    f->surf_plan[1] = static_cast<long long>(out.words[kSurfLarge]);
    f->surf_plan[2] = static_cast<long long>(out.words[kSurfRegs]);
    f->surf_plan[3] = static_cast<long long>(f->mesh.nf - out.valid_faces);
    f->surf_cell = static_cast<float>(out.cell);
    f->surf_stats[0] = static_cast<long long>(out.words[kDistOccupied]);
    f->surf_stats[1] = static_cast<long long>(out.words[kDistMaxList]);
    f->surf_stats[2] = static_cast<long long>(out.words[kDistRings]);
    if (summary)
        for (int k = 0; k < ACMMP_DIST_SUMMARY_WORDS; ++k) summary[k] = static_cast<int64_t>(out.words[kDistSummary + k]);
    return ACMMP_OK;
}

acmmp_status acmmp_fusion_surface_results(acmmp_fusion* f, int64_t first, int64_t n, float* d2, int32_t* nearest_face) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    return read_result(f, first, n, f->surf.n, "range beyond the surface result", [&](size_t a, size_t m) -> acmmp_status {
        F_HIP(f, read_range<float>(d2, f->surf.d2, a, m));
        F_HIP(f, read_range<int32_t>(nearest_face, f->surf.nn, a, m));
        return ACMMP_OK;
    });
}

acmmp_status acmmp_fusion_surface_plan(acmmp_fusion* f, int small_max, int64_t* n_small, int64_t* n_large,
                                       int64_t* n_registrations, int64_t* n_skipped) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    f->surf_small_max = small_max;
    if (n_small) *n_small = f->surf_plan[0];
    if (n_large) *n_large = f->surf_plan[1];
    if (n_registrations) *n_registrations = f->surf_plan[2];
    if (n_skipped) *n_skipped = f->surf_plan[3];
    return ACMMP_OK;
}

acmmp_status acmmp_fusion_surface_grid(acmmp_fusion* f, float force_cell, float* cell, int64_t* cells, int64_t* max_list,
                                       int64_t* rings) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    f->surf_force_cell = force_cell;                  // checked by the next surface call
    if (cell) *cell = f->surf_cell;
    if (cells) *cells = f->surf_stats[0];
    if (max_list) *max_list = f->surf_stats[1];
    if (rings) *rings = f->surf_stats[2];
    return ACMMP_OK;
}

}  // extern "C"

// ---- registration of the data cloud to the reference cloud (include/acmmp.h; kernel: k_align_iter) -----------

namespace {

typedef __int128 i128;

// hi * 2^32 + lo of a split product sum.
i128 align_join(const int64_t* w) { return static_cast<i128>(w[0]) * (static_cast<i128>(1) << 32) + static_cast<i128>(w[1]); }

void align_cross(const double a[3], const double b[3], double c[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// H = U diag(d) V^T by one-sided Jacobi rotations of H's columns, d sorted descending, columns of U and V in u[i], v[i].
// u[2] and v[2] are the cross products of the first two, so that both bases are right-handed and the third singular
// value carries a sign: sd2 = u2^T H v2, |sd2| = d2, and its sign is sign det(V U^T) of the unsigned decomposition.
void align_svd(const double H[9], double d[3], double u[3][3], double v[3][3], double& sd2) {
    double a[3][3], w[3][3];                               // a[j] = column j of H V, w[j] = column j of V
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) { a[j][i] = H[3 * i + j]; w[j][i] = i == j ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int i = 0; i < 3; ++i) { al += a[p][i] * a[p][i]; be += a[q][i] * a[q][i]; ga += a[p][i] * a[q][i]; }
                if (ga == 0.0 || std::fabs(ga) <= 0x1p-53 * std::sqrt(al * be)) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), sn = c * t;
                for (int i = 0; i < 3; ++i) {
                    const double x = a[p][i], y = a[q][i];
                    a[p][i] = c * x - sn * y; a[q][i] = sn * x + c * y;
                    const double vx = w[p][i], vy = w[q][i];
                    w[p][i] = c * vx - sn * vy; w[q][i] = sn * vx + c * vy;
                }
            }
        if (!rotated) break;
    }
    double n[3];
    int o[3] = {0, 1, 2};
    for (int j = 0; j < 3; ++j) n[j] = std::sqrt(a[j][0] * a[j][0] + a[j][1] * a[j][1] + a[j][2] * a[j][2]);
    std::sort(o, o + 3, [&](int x, int y) { return n[x] > n[y] || (n[x] == n[y] && x < y); });
    for (int k = 0; k < 3; ++k) {
        d[k] = n[o[k]];
        for (int i = 0; i < 3; ++i) {
            u[k][i] = d[k] > 0.0 ? a[o[k]][i] / d[k] : 0.0;
            v[k][i] = w[o[k]][i];
        }
    }
    align_cross(u[0], u[1], u[2]);
    align_cross(v[0], v[1], v[2]);
    double hv[3];
    for (int i = 0; i < 3; ++i) hv[i] = H[3 * i] * v[2][0] + H[3 * i + 1] * v[2][1] + H[3 * i + 2] * v[2][2];
    sd2 = u[2][0] * hv[0] + u[2][1] * hv[1] + u[2][2] * hv[2];
}

// Step 4 of acmmp_fusion_cloud_align: D from the record; false = degenerate.
bool align_fit(const int64_t* r, const double c[3], double kq, int mode, double D[12]) {
    const i128 N = r[ACMMP_ALIGN_RECORD_N];
    if (N < 3) return false;
    const double NN = static_cast<double>(r[ACMMP_ALIGN_RECORD_N]) * static_cast<double>(r[ACMMP_ALIGN_RECORD_N]);
    const int64_t* sp = r + ACMMP_ALIGN_RECORD_SUM_P;
    const int64_t* sq = r + ACMMP_ALIGN_RECORD_SUM_Q3;
    double H[9];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const i128 A = N * align_join(r + ACMMP_ALIGN_RECORD_PQ + 2 * (3 * a + b)) - static_cast<i128>(sp[a]) * static_cast<i128>(sq[b]);
            H[3 * a + b] = static_cast<double>(A) / NN;
        }
    i128 V = N * align_join(r + ACMMP_ALIGN_RECORD_PP);
    for (int a = 0; a < 3; ++a) V -= static_cast<i128>(sp[a]) * static_cast<i128>(sp[a]);
    if (V == 0) return false;
    const double var = static_cast<double>(V) / NN;
    double d[3], u[3][3], v[3][3], sd2;
    align_svd(H, d, u, v, sd2);
    if (!(d[1] > d[0] * 0x1p-40)) return false;
    const double s = mode == ACMMP_ALIGN_SIMILARITY ? (d[0] + d[1] + sd2) / var : 1.0;
    const double n = static_cast<double>(r[ACMMP_ALIGN_RECORD_N]);
    double pm[3], qm[3];
    for (int a = 0; a < 3; ++a) {
        pm[a] = c[a] + (static_cast<double>(sp[a]) / n) / kq;
        qm[a] = c[a] + (static_cast<double>(sq[a]) / n) / kq;
    }
    for (int a = 0; a < 3; ++a) {
        double t = qm[a];
        for (int b = 0; b < 3; ++b) {
            // R = V diag(1, 1, g) U^T with the unsigned third pair = v0 u0^T + v1 u1^T + v2 u2^T with the signed one
            const double R = (v[0][a] * u[0][b] + v[1][a] * u[1][b]) + v[2][a] * u[2][b];
            D[4 * a + b] = s * R;
            t -= D[4 * a + b] * pm[b];
        }
        D[4 * a + 3] = t;
    }
    return true;
}

// Step 5: M := D o M, and the largest displacement of a corner of the box [lo, hi] under D.
double align_step(const double D[12], const double lo[3], const double hi[3], double M[12]) {
    double out[12];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 4; ++b) {
            out[4 * a + b] = (D[4 * a] * M[b] + D[4 * a + 1] * M[4 + b]) + D[4 * a + 2] * M[8 + b];
            if (b == 3) out[4 * a + b] += D[4 * a + 3];
        }
    std::memcpy(M, out, sizeof(out));
    double shift = 0.0;
    for (int k = 0; k < 8; ++k) {
        const double x[3] = {k & 1 ? hi[0] : lo[0], k & 2 ? hi[1] : lo[1], k & 4 ? hi[2] : lo[2]};
        double e2 = 0.0;
        for (int a = 0; a < 3; ++a) {
            const double y = ((D[4 * a] * x[0] + D[4 * a + 1] * x[1]) + D[4 * a + 2] * x[2]) + D[4 * a + 3];
            e2 += (y - x[a]) * (y - x[a]);
        }
        shift = std::max(shift, std::sqrt(e2));
    }
    return shift;
}

// What a successful align call installs, and what it reports.
struct AlignOut : AlignRec {
    double last[12];
    int stop = ACMMP_ALIGN_MAX_ITERATIONS;
    double cell = 0.0;
    unsigned long long stats[3] = {0, 0, 0};
};

acmmp_status align_run(acmmp_fusion* f, DistCloud data, DistCloud ref, int mode, float max_dist, int max_iterations,
                       unsigned long long stride, double min_shift, AlignOut& out) {
    hipStream_t s = f->stream;
    DistOut scratch;
    DistIndex ix;
    const acmmp_status rc = region_crop(f, f->region[ACMMP_REGION_REFERENCE], true, ref, scratch.tcls, ref);
    if (rc != ACMMP_OK) return rc;
    const acmmp_status st = distance_build(f, ref, max_dist, 0, nullptr, scratch, ix);   // the one build of the call
    if (st != ACMMP_OK) return st;
    // the data side's region follows the transform: its classes are formed again under every M_k
    const RegionSet& dr = f->region[ACMMP_REGION_DATA];
    if (dr.set) {
        F_HIP(f, alloc(scratch.qcls, static_cast<size_t>(data.n)));
        data.cls = scratch.qcls;
    }
    out.cell = scratch.cell;
    unsigned long long* w = f->dist_words;
    unsigned long long* rec = w + kDistSummary;            // the summary's words are free in an align call
    static_assert(kAlignWords <= ACMMP_DIST_SUMMARY_WORDS, "the record lives in the summary's words");
    const double kq = 65536.0 / static_cast<double>(max_dist);
    const unsigned long long nq = (data.n + stride - 1ull) / stride;
    data.xf = 1;
    std::memcpy(data.M, out.last, sizeof(data.M));
    for (int k = 0; k < max_iterations; ++k) {
        unsigned long long h[kDistSummary + kAlignWords];
        F_HIP(f, hipMemsetAsync(rec, 0, sizeof(unsigned long long) * kAlignWords, s));
        if (dr.set) F_HIP(f, launch_region_classify(data, dr.dev(), scratch.qcls, nullptr, s));
        F_HIP(f, launch_align_iter(data, stride, ref, ix.g, ix.fine, ix.cg, ix.coarse, scratch.list, ix.p, kq, w, rec, s));
        // the iteration's host wait: the record, from which the host fits and decides whether to stop
        F_HIP(f, hipMemcpyAsync(h, w, sizeof(h), hipMemcpyDeviceToHost, s));
        F_HIP(f, hipStreamSynchronize(s));
        const acmmp_status ck = distance_check(f, h, ix.valid_targets);
        if (ck != ACMMP_OK) return ck;
        out.stats[0] = h[kDistOccupied]; out.stats[1] = h[kDistMaxList]; out.stats[2] = h[kDistRings];
        int64_t r[kAlignWords];
        for (int i = 0; i < kAlignWords; ++i) r[i] = static_cast<int64_t>(h[kDistSummary + i]);
        r[ACMMP_ALIGN_RECORD_N_QUERY] = static_cast<int64_t>(nq);
        out.words.insert(out.words.end(), r, r + kAlignWords);
        out.M.insert(out.M.end(), data.M, data.M + 12);
        double D[12];
        if (!align_fit(r, ix.p.lo, kq, mode, D)) {
            out.shift.push_back(0.0);
            out.stop = ACMMP_ALIGN_DEGENERATE;
            break;
        }
        const double shift = align_step(D, ix.p.lo, ix.p.hi, data.M);
        bool finite = std::isfinite(shift);
        for (int i = 0; i < 12; ++i) finite = finite && std::isfinite(data.M[i]);
        if (!finite) {                                     // a fit that left float64: keep M_k
            std::memcpy(data.M, &out.M[out.M.size() - 12], sizeof(data.M));
            out.shift.push_back(0.0);
            out.stop = ACMMP_ALIGN_DEGENERATE;
            break;
        }
        out.shift.push_back(shift);
        if (shift <= min_shift) { out.stop = ACMMP_ALIGN_CONVERGED; break; }
    }
    std::memcpy(out.last, data.M, sizeof(out.last));
    return ACMMP_OK;
}

// ---- point-to-plane (acmmp_fusion_cloud_align_plane; kernel: k_align_plane_iter)

// Step 6: floor((2 sumQ_a + N) / (2 N)) in integers, 0 when N is 0.
void align_pivot(const int64_t* sum_q3, int64_t n, long long g[3]) {
    for (int a = 0; a < 3; ++a) {
        g[a] = 0;
        if (n <= 0) continue;
        const i128 num = 2 * static_cast<i128>(sum_q3[a]) + n, den = 2 * static_cast<i128>(n);
        i128 q = num / den;
        if (num % den != 0 && num < 0) --q;
        g[a] = static_cast<long long>(q);
    }
}

// A = sum_i lam[i] v[i] v[i]^T for a symmetric n x n A by cyclic Jacobi rotations, in the manner of align_svd.
template <int n>
void align_eig(double A[n][n], double lam[n], double v[n][n]) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) v[i][j] = i == j ? 1.0 : 0.0;      // v[j] = column j of V
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double ga = A[p][q];
                if (ga == 0.0 || std::fabs(ga) <= 0x1p-53 * std::sqrt(std::fabs(A[p][p] * A[q][q]))) continue;
                rotated = true;
                const double zeta = (A[q][q] - A[p][p]) / (2.0 * ga);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), sn = c * t;
                for (int i = 0; i < n; ++i) {                             // A := A J
                    const double x = A[i][p], y = A[i][q];
                    A[i][p] = c * x - sn * y; A[i][q] = sn * x + c * y;
                }
                for (int i = 0; i < n; ++i) {                             // A := J^T A
                    const double x = A[p][i], y = A[q][i];
                    A[p][i] = c * x - sn * y; A[q][i] = sn * x + c * y;
                }
                A[p][q] = A[q][p] = 0.0;
                for (int i = 0; i < n; ++i) {
                    const double x = v[p][i], y = v[q][i];
                    v[p][i] = c * x - sn * y; v[q][i] = sn * x + c * y;
                }
            }
        if (!rotated) break;
    }
    for (int i = 0; i < n; ++i) lam[i] = A[i][i];
}

// Step 5 of acmmp_fusion_cloud_align_plane: D from the record; false = degenerate.
bool align_plane_fit(const int64_t* r, const double c[3], double kq, double D[12]) {
    if (r[ACMMP_ALIGN_PLANE_RECORD_N] < 6) return false;
    double S[6][6], b[6], s[6];
    int k = ACMMP_ALIGN_PLANE_RECORD_CC;
    for (int a = 0; a < 6; ++a)
        for (int e = a; e < 6; ++e, k += 2) S[a][e] = S[e][a] = static_cast<double>(align_join(r + k));
    for (int a = 0; a < 6; ++a) {
        b[a] = -static_cast<double>(align_join(r + ACMMP_ALIGN_PLANE_RECORD_CR + 2 * a));
        if (S[a][a] == 0.0) return false;
        s[a] = std::sqrt(S[a][a]);
    }
    double A[6][6], bs[6], lam[6], v[6][6];
    for (int a = 0; a < 6; ++a) {
        bs[a] = b[a] / s[a];
        for (int e = 0; e < 6; ++e) A[a][e] = S[a][e] / (s[a] * s[e]);
    }
    align_eig<6>(A, lam, v);
    double lmin = lam[0], lmax = lam[0];
    for (int i = 1; i < 6; ++i) { lmin = std::min(lmin, lam[i]); lmax = std::max(lmax, lam[i]); }
    if (!(lmin > lmax * 0x1p-40)) return false;
    // the noise floor: what the translation columns do not explain of the rotation columns (the Schur complement, whose
    // inverse is the rotation block of S^-1) must exceed four times what the levers' rounding alone puts there
    double P[3][3], mu[3], pv[3][3];
    for (int a = 0; a < 3; ++a)
        for (int e = 0; e < 3; ++e) {
            double t = 0.0;
            for (int i = 0; i < 6; ++i) t += v[i][a] * v[i][e] / lam[i];
            P[a][e] = t / (s[a] * s[e]);
        }
    for (int a = 0; a < 3; ++a)
        for (int e = a + 1; e < 3; ++e) P[e][a] = P[a][e];
    align_eig<3>(P, mu, pv);
    const double noise = ((S[3][3] + S[4][4]) + S[5][5]) / 18.0;
    if (!(1.0 > 4.0 * noise * std::max(mu[0], std::max(mu[1], mu[2])))) return false;
    double x[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 6; ++i) {
        double dot = 0.0;
        for (int a = 0; a < 6; ++a) dot += v[i][a] * bs[a];
        for (int a = 0; a < 6; ++a) x[a] += v[i][a] * (dot / lam[i]);
    }
    double om[3], tau[3], G[3];
    for (int a = 0; a < 3; ++a) {
        om[a] = x[a] / s[a] / 4096.0;
        tau[a] = x[3 + a] / s[3 + a] / kq;
        G[a] = c[a] + static_cast<double>(r[ACMMP_ALIGN_PLANE_RECORD_PIVOT + a]) / kq;
    }
    const double theta2 = (om[0] * om[0] + om[1] * om[1]) + om[2] * om[2];
    double ca, cb;
    if (theta2 >= 0x1p-40) {
        const double theta = std::sqrt(theta2);
        ca = std::sin(theta) / theta;
        cb = (1.0 - std::cos(theta)) / theta2;
    } else {
        ca = 1.0 - theta2 / 6.0;
        cb = 0.5 - theta2 / 24.0;
    }
    const double K[3][3] = {{0.0, -om[2], om[1]}, {om[2], 0.0, -om[0]}, {-om[1], om[0], 0.0}};
    for (int a = 0; a < 3; ++a) {
        double t = G[a] + tau[a];
        for (int e = 0; e < 3; ++e) {
            const double k2 = (K[a][0] * K[0][e] + K[a][1] * K[1][e]) + K[a][2] * K[2][e];
            D[4 * a + e] = ((a == e ? 1.0 : 0.0) + ca * K[a][e]) + cb * k2;
        }
        for (int e = 0; e < 3; ++e) t -= D[4 * a + e] * G[e];
        D[4 * a + 3] = t;
    }
    return true;
}

// One launch of an align kernel and its host wait: the words to h (kDistSummary + n_rec of them), checked.
template <class Launch>
acmmp_status align_pass(acmmp_fusion* f, const DistIndex& ix, int n_rec, unsigned long long* h, Launch launch) {
    hipStream_t s = f->stream;
    unsigned long long* w = f->dist_words;
    F_HIP(f, hipMemsetAsync(w + kDistSummary, 0, sizeof(unsigned long long) * n_rec, s));
    F_HIP(f, launch());
    F_HIP(f, hipMemcpyAsync(h, w, sizeof(unsigned long long) * (kDistSummary + n_rec), hipMemcpyDeviceToHost, s));
    F_HIP(f, hipStreamSynchronize(s));
    return distance_check(f, h, ix.valid_targets);
}

acmmp_status align_plane_run(acmmp_fusion* f, DistCloud data, DistCloud ref, float max_dist, int max_iterations,
                             unsigned long long stride, double min_shift, AlignOut& out) {
    hipStream_t s = f->stream;
    DistOut scratch;
    DistIndex ix;
    const acmmp_status rc = region_crop(f, f->region[ACMMP_REGION_REFERENCE], true, ref, scratch.tcls, ref);
    if (rc != ACMMP_OK) return rc;
    const acmmp_status st = distance_build(f, ref, max_dist, 0, nullptr, scratch, ix);   // the one build of the call
    if (st != ACMMP_OK) return st;
    // the data side's region follows the transform: its classes are formed again under every M_k
    const RegionSet& dr = f->region[ACMMP_REGION_DATA];
    if (dr.set) {
        F_HIP(f, alloc(scratch.qcls, static_cast<size_t>(data.n)));
        data.cls = scratch.qcls;
    }
    out.cell = scratch.cell;
    unsigned long long* w = f->dist_words;
    unsigned long long* rec = w + kDistSummary;            // the summary's words are free in an align call
    static_assert(kAlignPlaneWords <= ACMMP_DIST_SUMMARY_WORDS, "the record lives in the summary's words");
    const double kq = 65536.0 / static_cast<double>(max_dist);
    const unsigned long long nq = (data.n + stride - 1ull) / stride;
    data.xf = 1;
    std::memcpy(data.M, out.last, sizeof(data.M));
    unsigned long long h[kDistSummary + kAlignPlaneWords];
    AlignPivot pivot;
    {
        // the pivot pass: the point kernel under M_0, for the mean target only; not an iteration
        const acmmp_status ck = align_pass(f, ix, kAlignWords, h, [&] {
            if (dr.set) {
                const hipError_t e = launch_region_classify(data, dr.dev(), scratch.qcls, nullptr, s);
                if (e != hipSuccess) return e;
            }
            return launch_align_iter(data, stride, ref, ix.g, ix.fine, ix.cg, ix.coarse, scratch.list, ix.p, kq, w, rec, s);
        });
        if (ck != ACMMP_OK) return ck;
        int64_t r[kAlignWords];
        for (int i = 0; i < kAlignWords; ++i) r[i] = static_cast<int64_t>(h[kDistSummary + i]);
        align_pivot(r + ACMMP_ALIGN_RECORD_SUM_Q3, r[ACMMP_ALIGN_RECORD_N], pivot.g);
    }
    for (int k = 0; k < max_iterations; ++k) {
        // the iteration's host wait: the record, from which the host fits and decides whether to stop
        const acmmp_status ck = align_pass(f, ix, kAlignPlaneWords, h, [&] {
            if (dr.set) {
                const hipError_t e = launch_region_classify(data, dr.dev(), scratch.qcls, nullptr, s);
                if (e != hipSuccess) return e;
            }
            return launch_align_plane_iter(data, stride, ref, ix.g, ix.fine, ix.cg, ix.coarse, scratch.list, ix.p, kq, pivot,
                                           w, rec, s);
        });
        if (ck != ACMMP_OK) return ck;
        out.stats[0] = h[kDistOccupied]; out.stats[1] = h[kDistMaxList]; out.stats[2] = h[kDistRings];
        int64_t r[kAlignPlaneWords];
        for (int i = 0; i < kAlignPlaneWords; ++i) r[i] = static_cast<int64_t>(h[kDistSummary + i]);
        r[ACMMP_ALIGN_PLANE_RECORD_N_QUERY] = static_cast<int64_t>(nq);
        for (int a = 0; a < 3; ++a) r[ACMMP_ALIGN_PLANE_RECORD_PIVOT + a] = pivot.g[a];
        out.words.insert(out.words.end(), r, r + kAlignPlaneWords);
        out.M.insert(out.M.end(), data.M, data.M + 12);
        double D[12];
        if (!align_plane_fit(r, ix.p.lo, kq, D)) {
            out.shift.push_back(0.0);
            out.stop = ACMMP_ALIGN_DEGENERATE;
            break;
        }
        const double shift = align_step(D, ix.p.lo, ix.p.hi, data.M);
        bool finite = std::isfinite(shift);
        for (int i = 0; i < 12; ++i) finite = finite && std::isfinite(data.M[i]);
        if (!finite) {                                     // a fit that left float64: keep M_k
            std::memcpy(data.M, &out.M[out.M.size() - 12], sizeof(data.M));
            out.shift.push_back(0.0);
            out.stop = ACMMP_ALIGN_DEGENERATE;
            break;
        }
        out.shift.push_back(shift);
        if (shift <= min_shift) { out.stop = ACMMP_ALIGN_CONVERGED; break; }
        align_pivot(r + ACMMP_ALIGN_PLANE_RECORD_SUM_Q3, r[ACMMP_ALIGN_PLANE_RECORD_N], pivot.g);
    }
    std::memcpy(out.last, data.M, sizeof(out.last));
    return ACMMP_OK;
}

bool finite12(const double* M) {
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(M[i])) return false;
    return true;
}

}  // namespace

extern "C" {

acmmp_status acmmp_fusion_set_cloud_transform(acmmp_fusion* f, const double M[12]) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    if (M && !finite12(M)) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "every entry of the transform must be finite");
    const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    std::memcpy(f->xf, M ? M : I, sizeof(f->xf));
    f->xf_set = M != nullptr;
    invalidate(f, R_XFORM);                           // what was measured under the previous transform
    return ACMMP_OK;
}

acmmp_status acmmp_fusion_get_cloud_transform(const acmmp_fusion* f, double M[12], int* is_set) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    if (M) std::memcpy(M, f->xf, sizeof(f->xf));
    if (is_set) *is_set = f->xf_set ? 1 : 0;
    return ACMMP_OK;
}

}  // extern "C"

namespace {

// Both align calls: the argument checks in the order the header lists them (a plane call has no mode), the run, the
// records installed.
acmmp_status align_call(acmmp_fusion* f, bool plane, int source, int mode, float max_dist, int max_iterations, int stride,
                        double min_shift, const double init[12], double M_out[12], int* n_iterations, int* stop_reason) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    const Res id = dist_source(source);
    if (id == R_NONE) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "source must be one of ACMMP_DIST_FROM_*");
    if (!plane && mode != ACMMP_ALIGN_RIGID && mode != ACMMP_ALIGN_SIMILARITY)
        return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "mode must be ACMMP_ALIGN_RIGID or ACMMP_ALIGN_SIMILARITY");
    const Cloud src = cloud(f, id);
    if (!src.have) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "no such data result");
    if (!f->ref.have) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "no reference cloud: acmmp_fusion_set_reference_cloud first");
    if (!finite32(max_dist) || !(max_dist > 0.0f)) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "max_dist must be finite and > 0");
    if (max_iterations < 1 || max_iterations > 1024) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "max_iterations must be 1 to 1024");
    if (stride < 1) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "stride must be at least 1");
    if (!std::isfinite(min_shift) || min_shift < 0.0) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "min_shift must be finite and >= 0");
    if (init && !finite12(init)) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "every entry of init must be finite");
    if (f->dist_force_cell != 0.0f && (!finite32(f->dist_force_cell) || !(f->dist_force_cell > 0.0f)))
        return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "the forced cell must be finite and > 0");
    const DistCloud data = src.dist(), ref = cloud(f, R_REFERENCE).dist();
    if (ref.n > 0x7fffffffull) return ffail(f, ACMMP_ERR_UNSUPPORTED, "more than 2^31 - 1 targets");
    F_HIP(f, hipSetDevice(f->device));
    AlignOut out;
    const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    std::memcpy(out.last, init ? init : I, sizeof(out.last));
    const unsigned long long step = static_cast<unsigned long long>(stride);
    const acmmp_status st = plane ? align_plane_run(f, data, ref, max_dist, max_iterations, step, min_shift, out)
                                  : align_run(f, data, ref, mode, max_dist, max_iterations, step, min_shift, out);
    if (st != ACMMP_OK) return run_failed(f, st);
    out.plane = plane;                                // the other kind's records, if any, go with the record replaced
    out.source = id;
    out.have = true;
    f->align = std::move(out);
    f->dist_cell = static_cast<float>(out.cell);
    for (int k = 0; k < 3; ++k) f->dist_stats[k] = static_cast<long long>(out.stats[k]);
    if (M_out) std::memcpy(M_out, out.last, sizeof(out.last));
    if (n_iterations) *n_iterations = static_cast<int>(f->align.shift.size());
    if (stop_reason) *stop_reason = out.stop;
    return ACMMP_OK;
}

// Iterations [first, first + n) of the records of the given kind (none of the other kind's are visible).
acmmp_status align_read(acmmp_fusion* f, bool plane, int64_t first, int64_t n, int64_t* words, double* M, double* shift) {
    if (!f || first < 0 || n < 0) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "bad argument");
    const AlignRec& r = f->align;
    if (bad_range(first, n, r.plane == plane ? r.shift.size() : 0)) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "range beyond the align records");
    const size_t a = static_cast<size_t>(first), m = static_cast<size_t>(n), nw = plane ? kAlignPlaneWords : kAlignWords;
    if (words && m) std::memcpy(words, r.words.data() + nw * a, sizeof(int64_t) * nw * m);
    if (M && m) std::memcpy(M, r.M.data() + 12 * a, sizeof(double) * 12 * m);
    if (shift && m) std::memcpy(shift, r.shift.data() + a, sizeof(double) * m);
    return ACMMP_OK;
}

}  // namespace

extern "C" {

acmmp_status acmmp_fusion_cloud_align(acmmp_fusion* f, int source, int mode, float max_dist, int max_iterations, int stride,
                                      double min_shift, const double init[12], double M_out[12], int* n_iterations,
                                      int* stop_reason) {
    return align_call(f, false, source, mode, max_dist, max_iterations, stride, min_shift, init, M_out, n_iterations, stop_reason);
}

acmmp_status acmmp_fusion_align_records(acmmp_fusion* f, int64_t first, int64_t n, int64_t* words, double* M, double* shift) {
    return align_read(f, false, first, n, words, M, shift);
}

acmmp_status acmmp_fusion_cloud_align_plane(acmmp_fusion* f, int source, float max_dist, int max_iterations, int stride,
                                            double min_shift, const double init[12], double M_out[12], int* n_iterations,
                                            int* stop_reason) {
    return align_call(f, true, source, ACMMP_ALIGN_RIGID, max_dist, max_iterations, stride, min_shift, init, M_out, n_iterations,
                      stop_reason);
}

acmmp_status acmmp_fusion_align_plane_records(acmmp_fusion* f, int64_t first, int64_t n, int64_t* words, double* M,
                                              double* shift) {
    return align_read(f, true, first, n, words, M, shift);
}

}  // extern "C"

// ---- evaluation regions (include/acmmp.h; kernel: k_region_classify) ------------------------------------------

namespace {

bool finite_all(const double* x, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(x[i])) return false;
    return true;
}

// The checks of acmmp_fusion_set_region on the struct, in the order the header lists them; NULL = it passes.
const char* region_refusal(const acmmp_region& r) {
    if (r.n_planes < 0 || r.n_planes > ACMMP_REGION_MAX_PLANES) return "n_planes must be 0 to 8";
    if (r.n_vertices != 0 && (r.n_vertices < 3 || r.n_vertices > ACMMP_REGION_MAX_VERTICES))
        return "n_vertices must be 0 or 3 to 256";
    const bool grid = r.dims[0] != 0 || r.dims[1] != 0 || r.dims[2] != 0;
    for (int a = 0; a < 3; ++a)
        if (grid && (r.dims[a] < 1 || r.dims[a] > ACMMP_REGION_MAX_DIM)) return "every grid dimension must be 1 to 4096";
    if (!finite_all(r.planes, 4 * r.n_planes)) return "every plane coefficient must be finite";
    if (r.n_vertices > 0) {
        if (r.axis < 0 || r.axis > 2) return "the prism's axis must be 0, 1 or 2";
        if (!std::isfinite(r.axis_min) || !std::isfinite(r.axis_max)) return "axis_min and axis_max must be finite";
        if (r.axis_min > r.axis_max) return "axis_min must not exceed axis_max";
        if (!r.polygon) return "a NULL polygon with n_vertices > 0";
        if (!finite_all(r.polygon, 2 * r.n_vertices)) return "every polygon coordinate must be finite";
    }
    if (grid) {
        if (!finite_all(r.origin, 3) || !std::isfinite(r.cell)) return "the grid's origin and cell must be finite";
        if (!(r.cell > 0.0)) return "the grid's cell must be > 0";
        if (!r.bits) return "NULL bits with a grid";
    }
    return nullptr;
}

size_t region_grid_bytes(const acmmp_region& r) {
    const unsigned long long cells = static_cast<unsigned long long>(r.dims[0]) * static_cast<unsigned long long>(r.dims[1]) *
                                     static_cast<unsigned long long>(r.dims[2]);
    return static_cast<size_t>((cells + 7ull) / 8ull);
}

}  // namespace

extern "C" {

acmmp_status acmmp_fusion_set_region(acmmp_fusion* f, int side, const acmmp_region* r, int flags) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    if (side != ACMMP_REGION_DATA && side != ACMMP_REGION_REFERENCE)
        return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "side must be ACMMP_REGION_DATA or ACMMP_REGION_REFERENCE");
    if (flags != 0 && flags != ACMMP_REGION_QUERIES_ONLY)
        return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "flags must be 0 or ACMMP_REGION_QUERIES_ONLY");
    // built beside the present region, installed when every copy has succeeded
    RegionSet out;
    if (r) {
        if (const char* why = region_refusal(*r)) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, why);
        F_HIP(f, hipSetDevice(f->device));
        out.set = true;
        out.flags = flags;
        out.r = *r;
        out.r.polygon = nullptr;
        out.r.bits = nullptr;
        if (r->n_vertices > 0) {
            const size_t n = 2 * static_cast<size_t>(r->n_vertices);
            F_HIP(f, alloc(out.poly, n));
            F_HIP(f, hipMemcpy(out.poly, r->polygon, sizeof(double) * n, hipMemcpyHostToDevice));
        }
        if (r->dims[0] > 0) {
            const size_t n = region_grid_bytes(*r);
            F_HIP(f, alloc(out.bits, n));
            F_HIP(f, hipMemcpy(out.bits, r->bits, n, hipMemcpyHostToDevice));
        }
    } else {
        F_HIP(f, hipSetDevice(f->device));
    }
    F_HIP(f, hipStreamSynchronize(f->stream));        // nothing in flight reads the arrays that go
    f->region[side] = std::move(out);
    invalidate(f, R_REGION);                          // what was measured inside the previous region
    return ACMMP_OK;
}

acmmp_status acmmp_fusion_get_region(const acmmp_fusion* f, int side, int* is_set, int* flags, int* n_planes, int* n_vertices,
                                     int* dims) {
    if (!f || (side != ACMMP_REGION_DATA && side != ACMMP_REGION_REFERENCE)) return ACMMP_ERR_INVALID_ARGUMENT;
    const RegionSet& rs = f->region[side];
    if (is_set) *is_set = rs.set ? 1 : 0;
    if (flags) *flags = rs.flags;
    if (n_planes) *n_planes = rs.r.n_planes;
    if (n_vertices) *n_vertices = rs.r.n_vertices;
    if (dims)
        for (int a = 0; a < 3; ++a) dims[a] = rs.r.dims[a];
    return ACMMP_OK;
}

acmmp_status acmmp_fusion_region_classify(acmmp_fusion* f, int source, int64_t* counts) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    const Res id = region_source(source);
    if (id == R_NONE)
        return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "source must be one of ACMMP_DIST_FROM_* or ACMMP_SURF_FROM_REFERENCE");
    const Cloud src = cloud(f, id);
    if (!src.have) return ffail(f, ACMMP_ERR_INVALID_ARGUMENT, "no such result");
    DistCloud c = src.dist();
    if (id != R_REFERENCE && f->xf_set) {
        c.xf = 1;
        std::memcpy(c.M, f->xf, sizeof(c.M));
    }
    F_HIP(f, hipSetDevice(f->device));
    hipStream_t s = f->stream;
    RegionRec out;
    unsigned long long h[kRegionWords] = {0};
    const auto run = [&]() -> acmmp_status {
        F_HIP(f, alloc(out.cls, static_cast<size_t>(c.n)));
        if (!f->reg_words) F_HIP(f, alloc(f->reg_words, kRegionWords));
        F_HIP(f, hipMemsetAsync(f->reg_words, 0, sizeof(unsigned long long) * kRegionWords, s));
        F_HIP(f, launch_region_classify(c, f->region[id == R_REFERENCE ? ACMMP_REGION_REFERENCE : ACMMP_REGION_DATA].dev(),
                                        out.cls, f->reg_words, s));
        // the one host wait: the counts
        F_HIP(f, hipMemcpyAsync(h, f->reg_words, sizeof(h), hipMemcpyDeviceToHost, s));
        F_HIP(f, hipStreamSynchronize(s));
        return ACMMP_OK;
    };
    const acmmp_status st = run();
    if (st != ACMMP_OK) return run_failed(f, st);
    if (h[0] != c.n) return ffail(f, ACMMP_ERR_HIP, "region classify: the counts do not add up to the points");
    out.n = c.n;
    out.source = id;
    out.have = true;
    f->classes = std::move(out);
    if (counts)
        for (int k = 0; k < kRegionWords; ++k) counts[k] = static_cast<int64_t>(h[k]);
    return ACMMP_OK;
}

acmmp_status acmmp_fusion_region_classes(acmmp_fusion* f, int64_t first, int64_t n, uint8_t* cls) {
    if (!f) return ACMMP_ERR_INVALID_ARGUMENT;
    return read_result(f, first, n, f->classes.n, "range beyond the class result", [&](size_t a, size_t m) -> acmmp_status {
        F_HIP(f, read_range<uint8_t>(cls, f->classes.cls, a, m));
        return ACMMP_OK;
    });
}

}  // extern "C"
