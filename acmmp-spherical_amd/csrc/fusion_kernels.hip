// fusion_kernels.hip -- gfx950 kernels of the depth-map fusion (SimpleFusionKernel, ACMMP.cu:1662-1814, its
// whole-scene pass and their in-order compaction), of the voxel-grid reduction of the fused scene cloud and of the
// cleaning, the visibility check and the surface mesh of that voxel cloud, and of the rendering of that mesh into a
// view, with their host launchers (fusion.h).  One translation unit, compiled once.
#include <algorithm>

#include "camera_dev.h"
#include "detmath.h"
#include "fusion.h"

namespace acmmp {

// ------------------------------------------------------------------ kernel: fusion

// tex2D<float4>(linear filter, unnormalised (c, r)) at an integer texel index WITHOUT the +0.5
// (ACMMP.cu:1690, 1768): the footprint is texels (c-1, c) x (r-1, r), both weights 0.5, clamped
// (wrap is undefined for unnormalised coordinates and acts as clamp).  fp32 fused lerps.
__device__ __forceinline__ float4 fuse_colour(const float* rgba, int W, int H, int c, int r) {
    const int x0 = c - 1 < 0 ? 0 : c - 1, x1 = c > W - 1 ? W - 1 : c;
    const int y0 = r - 1 < 0 ? 0 : r - 1, y1 = r > H - 1 ? H - 1 : r;
    const float4 t00 = reinterpret_cast<const float4*>(rgba)[static_cast<long long>(y0) * W + x0];
    const float4 t10 = reinterpret_cast<const float4*>(rgba)[static_cast<long long>(y0) * W + x1];
    const float4 t01 = reinterpret_cast<const float4*>(rgba)[static_cast<long long>(y1) * W + x0];
    const float4 t11 = reinterpret_cast<const float4*>(rgba)[static_cast<long long>(y1) * W + x1];
    auto lerp = [](float a, float b) { return fmaf(0.5f, b - a, a); };
    const float4 top = make_float4(lerp(t00.x, t10.x), lerp(t00.y, t10.y), lerp(t00.z, t10.z), lerp(t00.w, t10.w));
    const float4 bot = make_float4(lerp(t01.x, t11.x), lerp(t01.y, t11.y), lerp(t01.z, t11.z), lerp(t01.w, t11.w));
    return make_float4(lerp(top.x, bot.x), lerp(top.y, bot.y), lerp(top.z, bot.z), lerp(top.w, bot.w));
}

// SimpleFusionKernel, ACMMP.cu:1662-1814: per reference pixel, the source views whose depth
// reprojects within 1 px, 1% depth and 0.149 rad of normal; >= 3 consistent (the reference
// included) -> averaged point, normal and colour.  out: 9 floats per pixel (x y z nx ny nz c0 c1 c2,
// c0 = 255 * texture .z as the reference stores it).
//
// Two compile-time variants serve the whole-scene pass (acmmp_fusion_run_scene): PROV also writes, per
// pixel, the mask of consistent sources (bit j = srcs[j]); UNIQUE reads every depth through the views'
// `used` byte masks -- a used pixel reads as depth 0, so a used reference pixel is skipped and a used
// source sample is skipped, with the arithmetic, the thresholds and the order of the sums untouched.
// k_fuse<MODEL> is the reference-equal kernel of acmmp_fusion_run (neither variant), k_fuse_scene the
// kernel of the scene pass.
template <int MODEL, bool PROV, bool UNIQUE>
__device__ __forceinline__ void fuse_pixel(const DevCam* __restrict__ cams, const FuseView* __restrict__ views, int ref,
                                           int W, int H, const int* __restrict__ srcs, int n_src, float* __restrict__ out,
                                           int* __restrict__ flags, uint32_t* __restrict__ src_mask) {
    const int c = blockIdx.x * 16 + (threadIdx.x & 15);
    const int r = blockIdx.y * 16 + (threadIdx.x >> 4);
    const bool inside = c < W && r < H;
    int valid = 0;
    const long long idx = static_cast<long long>(r) * W + c;
    if (inside) {
        const DevCam& rc = cams[ref];
        const FuseView rv = views[ref];
        float ref_depth = rv.depth[idx];
        if constexpr (UNIQUE) { if (rv.used[idx]) ref_depth = 0.0f; }
        uint32_t consistent = 0;
        if (!(ref_depth <= 0.0f)) {
            const float3 X = world_point<MODEL>(rc, static_cast<float>(c), static_cast<float>(r), ref_depth);
            const float rn0 = rv.normal[3 * idx], rn1 = rv.normal[3 * idx + 1], rn2 = rv.normal[3 * idx + 2];
            const float4 rcol = fuse_colour(rv.rgba, W, H, c, r);
            float ps0 = X.x, ps1 = X.y, ps2 = X.z;
            float ns0 = rn0, ns1 = rn1, ns2 = rn2;
            float cs0 = rcol.z * 255.0f, cs1 = rcol.y * 255.0f, cs2 = rcol.x * 255.0f;
            int n = 1;
            for (int j = 0; j < n_src; ++j) {
                const int si = srcs[j];
                if (si < 0) continue;
                const DevCam& sc = cams[si];
                const FuseView sv = views[si];
                float px, py, pd;
                project<MODEL, const DevCam, true>(sc, X, px, py, pd);
                const int src_c = f2i_sat(px + 0.5f), src_r = f2i_sat(py + 0.5f);
                if (src_c < 0 || src_c >= sc.W || src_r < 0 || src_r >= sc.H) continue;
                const long long sidx = static_cast<long long>(src_r) * sv.W + src_c;
                float sd = sv.depth[sidx];
                if constexpr (UNIQUE) { if (sv.used[sidx]) sd = 0.0f; }
                if (sd <= 0.0f) continue;
                const float3 Xs = world_point<MODEL>(sc, static_cast<float>(src_c), static_cast<float>(src_r), sd);
                float qx, qy, qd;
                project<MODEL, const DevCam, true>(rc, Xs, qx, qy, qd);
                const float err = det_hypot(static_cast<float>(c) - qx, static_cast<float>(r) - qy);
                const float rel = fabsf(pd - sd) / sd;
                const float sn0 = sv.normal[3 * sidx], sn1 = sv.normal[3 * sidx + 1], sn2 = sv.normal[3 * sidx + 2];
                float dp = dot3(rn0, rn1, rn2, sn0, sn1, sn2);
                dp = fmaxf(-1.0f, fminf(1.0f, dp));
                const float ang = det_acos(dp);
                if (err < 1.0f && rel < 0.01f && ang < 0.149f) {
                    ps0 += Xs.x; ps1 += Xs.y; ps2 += Xs.z;
                    ns0 += sn0; ns1 += sn1; ns2 += sn2;
                    const float4 scol = fuse_colour(sv.rgba, sv.W, sv.H, src_c, src_r);
                    cs0 = fmaf(scol.z, 255.0f, cs0);
                    cs1 = fmaf(scol.y, 255.0f, cs1);
                    cs2 = fmaf(scol.x, 255.0f, cs2);
                    ++n;
                    if constexpr (PROV) consistent |= 1u << j;
                }
            }
            if (n >= 3) {
                const float fn = static_cast<float>(n);
                float* o = out + 9 * idx;
                o[0] = ps0 / fn; o[1] = ps1 / fn; o[2] = ps2 / fn;
                float a0 = ns0 / fn, a1 = ns1 / fn, a2 = ns2 / fn;
                const float len = det_hypot(det_hypot(a0, a1), a2);
                if (len > 0.0f) { a0 /= len; a1 /= len; a2 /= len; }
                o[3] = a0; o[4] = a1; o[5] = a2;
                o[6] = cs0 / fn; o[7] = cs1 / fn; o[8] = cs2 / fn;
                valid = 1;
            }
        }
        flags[idx] = valid;
        if constexpr (PROV) src_mask[idx] = valid ? consistent : 0u;
    }
}

template <int MODEL>
__global__ void k_fuse(const DevCam* __restrict__ cams, const FuseView* __restrict__ views, int ref, int W, int H,
                       const int* __restrict__ srcs, int n_src, float* __restrict__ out, int* __restrict__ flags) {
    fuse_pixel<MODEL, false, false>(cams, views, ref, W, H, srcs, n_src, out, flags, nullptr);
}

template <int MODEL, bool UNIQUE>
__global__ void k_fuse_scene(const DevCam* __restrict__ cams, const FuseView* __restrict__ views, int ref, int W, int H,
                             const int* __restrict__ srcs, int n_src, float* __restrict__ out, int* __restrict__ flags,
                             uint32_t* __restrict__ src_mask) {
    fuse_pixel<MODEL, true, UNIQUE>(cams, views, ref, W, H, srcs, n_src, out, flags, src_mask);
}

// After a unique-mode k_fuse_scene of view `ref`, before the next view's: every sample that contributed
// to an emitted point is marked used -- the reference pixel, and for each consistent source j the pixel
// (src_c, src_r) k_fuse sampled, recomputed by the same device functions from the same depth (an emitted
// pixel was not used when k_fuse read it, so the raw depth is what it saw).  Plain byte stores of 1: lanes
// that hit the same byte store the same value.
template <int MODEL>
__global__ void k_fuse_mark(const DevCam* __restrict__ cams, const FuseView* __restrict__ views, int ref, int W, int H,
                            const int* __restrict__ srcs, int n_src, const int* __restrict__ flags,
                            const uint32_t* __restrict__ src_mask) {
    const int c = blockIdx.x * 16 + (threadIdx.x & 15);
    const int r = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (c >= W || r >= H) return;
    const long long idx = static_cast<long long>(r) * W + c;
    if (!flags[idx]) return;
    const DevCam& rc = cams[ref];
    const FuseView rv = views[ref];
    const uint32_t m = src_mask[idx];
    const float3 X = world_point<MODEL>(rc, static_cast<float>(c), static_cast<float>(r), rv.depth[idx]);
    rv.used[idx] = 1;
    for (int j = 0; j < n_src; ++j) {
        if (!((m >> j) & 1u)) continue;
        const int si = srcs[j];
        const DevCam& sc = cams[si];
        const FuseView sv = views[si];
        float px, py, pd;
        project<MODEL, const DevCam, true>(sc, X, px, py, pd);
        const int src_c = f2i_sat(px + 0.5f), src_r = f2i_sat(py + 0.5f);
        if (src_c < 0 || src_c >= sc.W || src_r < 0 || src_r >= sc.H) continue;   // (never: the bit says it was inside)
        sv.used[static_cast<long long>(src_r) * sv.W + src_c] = 1;
    }
}

// counts of valid pixels per 256-pixel chunk of the row-major image
__global__ void k_fuse_count(const int* __restrict__ flags, long long P, int* __restrict__ counts) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    const int f = i < P ? flags[i] : 0;
    const int n = __syncthreads_count(f);
    if (threadIdx.x == 0) counts[blockIdx.x] = n;
}

// Output position of a lane within its 256-lane chunk (one workgroup): offsets[chunk] + the flagged lanes
// before it.  Within a wave the rank is the popcount of the ballot below the lane; the four wave totals meet
// in LDS.  Every lane of the workgroup calls it.
__device__ __forceinline__ int chunk_rank(int f, const int* __restrict__ offsets) {
    __shared__ int wave_tot[4];
    const unsigned long long b = __ballot(f);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int below = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[wave] = __popcll(b);
    __syncthreads();
    int base = offsets[blockIdx.x];
    for (int w = 0; w < wave; ++w) base += wave_tot[w];
    return base + below;
}

// scatter the valid pixels of each chunk to offsets[chunk] + rank within the chunk (pixel order)
__global__ void k_fuse_scatter(const float* __restrict__ dense, const int* __restrict__ flags, long long P,
                               const int* __restrict__ offsets, float* __restrict__ out) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    const int f = i < P ? flags[i] : 0;
    const int pos = chunk_rank(f, offsets);
    if (f) {
        float* o = out + 9ll * pos;
        const float* d = dense + 9 * i;
#pragma unroll
        for (int k = 0; k < 9; ++k) o[k] = d[k];
    }
}

// Exclusive scan of the chunk counts of one view (each 0..256) and the scene bookkeeping, one workgroup
// of 1024 lanes walking the chunks in tiles of 1024 with a running carry.  Within a wave the prefix is
// built bit plane by bit plane from ballots: popcount(ballot(bit b of count) below my lane) << b, summed
// over the 9 planes; the 16 wave totals meet in LDS.  Lane 0 then publishes the view's point count, takes
// the 64-bit running scene offset as this view's base and advances it.
__global__ __launch_bounds__(1024) void k_fuse_scan(const int* __restrict__ counts, int n_chunks, int* __restrict__ offsets,
                                                    int* __restrict__ view_count, unsigned long long* __restrict__ running,
                                                    unsigned long long* __restrict__ view_base) {
    __shared__ int wave_tot[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    int carry = 0;
    for (int t0 = 0; t0 < n_chunks; t0 += 1024) {
        const int i = t0 + static_cast<int>(threadIdx.x);
        const int v = i < n_chunks ? counts[i] : 0;
        int excl = 0, tot = 0;
#pragma unroll
        for (int b = 0; b < 9; ++b) {
            const unsigned long long m = __ballot((v >> b) & 1);
            excl += __popcll(m & below) << b;
            tot += __popcll(m) << b;
        }
        if (lane == 0) wave_tot[wave] = tot;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const int x = wave_tot[w];
            all += x;
            if (w < wave) before += x;
        }
        if (i < n_chunks) offsets[i] = carry + before + excl;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *view_count = carry;
        const unsigned long long t = *running;
        *view_base = t;
        *running = t + static_cast<unsigned long long>(carry);
    }
}

// k_fuse_scatter into the scene buffers at *view_base + offsets[chunk] + rank: the point and its provenance
// (position of the view in the run's reference list, pixel r*W + c, consistent-source mask).  Nothing is
// written at or beyond `cap` points.
__global__ void k_fuse_scatter_scene(const float* __restrict__ dense, const int* __restrict__ flags,
                                     const uint32_t* __restrict__ src_mask, long long P, const int* __restrict__ offsets,
                                     const unsigned long long* __restrict__ view_base, int ref_pos, unsigned long long cap,
                                     float* __restrict__ out, int* __restrict__ out_ref, int* __restrict__ out_pix,
                                     uint32_t* __restrict__ out_mask) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    const int f = i < P ? flags[i] : 0;
    const int rank = chunk_rank(f, offsets);
    const unsigned long long pos = *view_base + static_cast<unsigned long long>(rank);
    if (f && pos < cap) {
        float* o = out + 9ull * pos;
        const float* d = dense + 9 * i;
#pragma unroll
        for (int k = 0; k < 9; ++k) o[k] = d[k];
        out_ref[pos] = ref_pos;
        out_pix[pos] = static_cast<int>(i);
        out_mask[pos] = src_mask[i];
    }
}

hipError_t launch_fuse(int model, const DevCam* cams, const FuseView* views, int ref, int W, int H, const int* srcs,
                       int n_src, float* out_dense, int* flags, int* block_counts, hipStream_t s) {
    dim3 grd(cdiv(W, 16), cdiv(H, 16));
    if (model == kSphere) k_fuse<kSphere><<<grd, 256, 0, s>>>(cams, views, ref, W, H, srcs, n_src, out_dense, flags);
    else k_fuse<kPinhole><<<grd, 256, 0, s>>>(cams, views, ref, W, H, srcs, n_src, out_dense, flags);
    const long long P = static_cast<long long>(W) * H;
    k_fuse_count<<<static_cast<unsigned>((P + 255) / 256), 256, 0, s>>>(flags, P, block_counts);
    return hipGetLastError();
}

hipError_t launch_fuse_compact(int W, int H, const float* out_dense, const int* flags, const int* block_offsets,
                               float* out, hipStream_t s) {
    const long long P = static_cast<long long>(W) * H;
    k_fuse_scatter<<<static_cast<unsigned>((P + 255) / 256), 256, 0, s>>>(out_dense, flags, P, block_offsets, out);
    return hipGetLastError();
}

hipError_t launch_fuse_scene(int model, bool unique, const DevCam* cams, const FuseView* views, int ref, int W, int H,
                             const int* srcs, int n_src, float* out_dense, int* flags, uint32_t* src_mask,
                             int* block_counts, int* block_offsets, int* view_count, unsigned long long* running,
                             unsigned long long* view_base, hipStream_t s) {
    dim3 grd(cdiv(W, 16), cdiv(H, 16));
    if (model == kSphere) {
        if (unique) k_fuse_scene<kSphere, true><<<grd, 256, 0, s>>>(cams, views, ref, W, H, srcs, n_src, out_dense, flags, src_mask);
        else k_fuse_scene<kSphere, false><<<grd, 256, 0, s>>>(cams, views, ref, W, H, srcs, n_src, out_dense, flags, src_mask);
    } else {
        if (unique) k_fuse_scene<kPinhole, true><<<grd, 256, 0, s>>>(cams, views, ref, W, H, srcs, n_src, out_dense, flags, src_mask);
        else k_fuse_scene<kPinhole, false><<<grd, 256, 0, s>>>(cams, views, ref, W, H, srcs, n_src, out_dense, flags, src_mask);
    }
    const long long P = static_cast<long long>(W) * H;
    const int n_chunks = static_cast<int>((P + 255) / 256);
    k_fuse_count<<<static_cast<unsigned>(n_chunks), 256, 0, s>>>(flags, P, block_counts);
    k_fuse_scan<<<1, 1024, 0, s>>>(block_counts, n_chunks, block_offsets, view_count, running, view_base);
    if (unique) {
        if (model == kSphere) k_fuse_mark<kSphere><<<grd, 256, 0, s>>>(cams, views, ref, W, H, srcs, n_src, flags, src_mask);
        else k_fuse_mark<kPinhole><<<grd, 256, 0, s>>>(cams, views, ref, W, H, srcs, n_src, flags, src_mask);
    }
    return hipGetLastError();
}

hipError_t launch_fuse_scatter_scene(int W, int H, const float* out_dense, const int* flags, const uint32_t* src_mask,
                                     const int* block_offsets, const unsigned long long* view_base, int ref_pos,
                                     unsigned long long cap, float* out, int* out_ref, int* out_pix, uint32_t* out_mask,
                                     hipStream_t s) {
    const long long P = static_cast<long long>(W) * H;
    k_fuse_scatter_scene<<<static_cast<unsigned>((P + 255) / 256), 256, 0, s>>>(out_dense, flags, src_mask, P, block_offsets,
                                                                               view_base, ref_pos, cap, out, out_ref,
                                                                               out_pix, out_mask);
    return hipGetLastError();
}

// ------------------------------------------------------------------ ordered compaction of a segment
//
// Compaction (fusion.h) for the stages below.  A stage is an Op, a small struct passed by value: keep(idx, lane) says
// whether item idx is kept, emit(idx, pos, lane) writes kept item idx as output pos.  `lane` is the Op's per-lane state
// (Op::Lane); once the items are through, every lane of the workgroup hands it to mark_end / scatter_end, where an Op
// folds it into its run words (block_or, wave_add).  CompactOp holds the defaults: no state, nothing to fold.
struct CompactOp {
    struct Lane {};
    template <class L> __device__ void mark_end(const L&) const {}
    template <class L> __device__ void scatter_end(const L&) const {}
};

// flags[i] = item i0 + i is kept; counts[chunk] as k_fuse_count
template <class Op>
__global__ __launch_bounds__(256) void k_compact_mark(const Op op, unsigned long long i0, int n, int* __restrict__ flags,
                                                      int* __restrict__ counts) {
    const int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    typename Op::Lane lane{};
    int f = 0;
    if (i < n) {
        f = op.keep(i0 + static_cast<unsigned long long>(i), lane) ? 1 : 0;
        flags[i] = f;
    }
    const int c = __syncthreads_count(f);
    if (threadIdx.x == 0) counts[blockIdx.x] = c;
    op.mark_end(lane);
}

// the flagged items of each chunk in order: output position = *seg_base + offsets[chunk] + rank
template <class Op>
__global__ __launch_bounds__(256) void k_compact_scatter(const Op op, unsigned long long i0, int n,
                                                         const int* __restrict__ flags, const int* __restrict__ offsets,
                                                         const unsigned long long* __restrict__ seg_base,
                                                         unsigned long long cap) {
    const int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    const int f = i < n ? flags[i] : 0;
    const int rank = chunk_rank(f, offsets);
    const unsigned long long pos = *seg_base + static_cast<unsigned long long>(rank);
    typename Op::Lane lane{};
    if (f && pos < cap) op.emit(i0 + static_cast<unsigned long long>(i), pos, lane);
    op.scatter_end(lane);
}

template <class Op>
static hipError_t compact_segment(const Op& op, unsigned long long i0, int n, const Compaction& c, hipStream_t s) {
    const int n_chunks = cdiv(n, 256);
    k_compact_mark<Op><<<static_cast<unsigned>(n_chunks), 256, 0, s>>>(op, i0, n, c.flags, c.counts);
    k_fuse_scan<<<1, 1024, 0, s>>>(c.counts, n_chunks, c.offsets, c.seg_count, c.running, c.seg_base);
    k_compact_scatter<Op><<<static_cast<unsigned>(n_chunks), 256, 0, s>>>(op, i0, n, c.flags, c.offsets, c.seg_base, c.cap);
    return hipGetLastError();
}

// ------------------------------------------------------------------ voxel-grid reduction of the scene cloud
//
// acmmp_fusion_voxelize (include/acmmp.h).  Everything a result depends on is an integer: the
// cell index, the 16.16 fixed-point channels and their 64-bit sums, the count and the smallest scene index of
// a cell.  Integer adds and minima commute, so the order in which the atomics land is invisible; the only
// racy thing is which slot of the hash table a cell gets, and no output depends on it.

constexpr unsigned long long kVoxEmpty = ~0ull;

__device__ __forceinline__ bool vox_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// step 1: all nine finite, normal and colour within 2^20
__device__ __forceinline__ bool vox_load(const float* __restrict__ p, float v[9]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        v[k] = p[k];
        ok = ok && !vox_nonfinite(v[k]);
    }
#pragma unroll
    for (int k = 3; k < 9; ++k) ok = ok && fabsf(v[k]) <= 1048576.0f;
    return ok;
}

// step 2: the cell of (x, y, z) and the position inside it, frac[a] = t - floorf(t) (exact); false = outside
// the 2^21 cells per axis (a NaN index, from 0 * inf with a denormal size, is outside too)
__device__ __forceinline__ bool vox_cell(const float v[9], const VoxGrid& g, unsigned long long& key, float frac[3]) {
    const float o[3] = {g.ox, g.oy, g.oz};
    key = 0;
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float t = (v[a] - o[a]) * g.inv;
        const float c = floorf(t);
        const bool in = c >= 0.0f && c < 2097152.0f;
        ok = ok && in;
        key |= (in ? static_cast<unsigned long long>(c) : 0ull) << (21 * a);
        frac[a] = t - c;
    }
    return ok;
}

__device__ __forceinline__ unsigned long long vox_home(unsigned long long key, int log2_slots) {
    unsigned long long z = key + 0x9e3779b97f4a7c15ull;       // splitmix64's finaliser
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return z >> (64 - log2_slots);
}

// The probe of every table here (VoxTable, MeshTable, DistTable): linear from the key's home slot, at most `slots`
// steps.  The lookup of a key after the insert pass: 0 = found (its slot), 1 = absent, 2 = the probe sequence covered
// every slot.
__device__ __forceinline__ int table_find(const unsigned long long* keys, unsigned long long slots, int log2_slots,
                                          unsigned long long key, unsigned long long& slot) {
    const unsigned long long mask = slots - 1ull;
    unsigned long long s = vox_home(key, log2_slots);
    for (unsigned long long probe = 0; probe < slots; ++probe) {
        const unsigned long long k = keys[s];
        if (k == key) { slot = s; return 0; }
        if (k == kVoxEmpty) return 1;
        s = (s + 1ull) & mask;
    }
    return 2;
}

// The slot of `key` in the insert pass, claimed when the key is new; false = the probe sequence covered every slot.
__device__ __forceinline__ bool table_claim(unsigned long long* keys, unsigned long long slots, int log2_slots,
                                            unsigned long long key, unsigned long long& slot) {
    const unsigned long long mask = slots - 1ull;
    unsigned long long s = vox_home(key, log2_slots);
    for (unsigned long long probe = 0; probe < slots; ++probe) {
        // a slot's key changes once, from empty: a plain read that shows a key is final, one that shows
        // empty (stale or not) is settled by the CAS
        unsigned long long k = keys[s];
        if (k == kVoxEmpty) k = atomicCAS(&keys[s], kVoxEmpty, key);
        if (k == kVoxEmpty || k == key) { slot = s; return true; }
        s = (s + 1ull) & mask;
    }
    return false;
}

template <class Table>
__device__ __forceinline__ int table_find(const Table& t, unsigned long long key, unsigned long long& slot) {
    return table_find(t.keys, t.slots, t.log2_slots, key, slot);
}
template <class Table>
__device__ __forceinline__ bool table_claim(const Table& t, unsigned long long key, unsigned long long& slot) {
    return table_claim(t.keys, t.slots, t.log2_slots, key, slot);
}

__device__ __forceinline__ uint32_t vox_ordered(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(256) void k_voxel_min(const float* __restrict__ pts, unsigned long long i0, int n,
                                                   uint32_t* __restrict__ mn) {
    __shared__ uint32_t blk[3];
    if (threadIdx.x < 3) blk[threadIdx.x] = 0xffffffffu;
    __syncthreads();
    const int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    uint32_t m[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};
    if (i < n) {
        float v[9];
        if (vox_load(pts + 9ull * (i0 + static_cast<unsigned long long>(i)), v)) {
#pragma unroll
            for (int a = 0; a < 3; ++a) m[a] = vox_ordered(v[a]);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m[a] = min(m[a], static_cast<uint32_t>(__shfl_xor(static_cast<int>(m[a]), d)));
        if ((threadIdx.x & 63) == 0 && m[a] != 0xffffffffu) atomicMin(&blk[a], m[a]);
    }
    __syncthreads();
    if (threadIdx.x < 3 && blk[threadIdx.x] != 0xffffffffu) atomicMin(&mn[threadIdx.x], blk[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_voxel_insert(const float* __restrict__ pts, unsigned long long i0, int n,
                                                      const VoxGrid g, const VoxTable t, unsigned long long* __restrict__ st) {
    const int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    const unsigned long long idx = i0 + static_cast<unsigned long long>(i);
    bool ok = false;
    unsigned long long key = 0;
    if (i < n) {
        float v[9], frac[3];
        ok = vox_load(pts + 9ull * idx, v) && vox_cell(v, g, key, frac);
    }
    const int rejected = __syncthreads_count(i < n && !ok);
    if (threadIdx.x == 0 && rejected) atomicAdd(&st[kVoxRejected], static_cast<unsigned long long>(rejected));
    if (!ok) return;
    unsigned long long s;
    if (!table_claim(t, key, s)) { atomicOr(&st[kVoxErr], 1ull); return; }
    atomicAdd(&t.cnt[s], 1u);
    atomicMin(&t.first[s], idx);
}

__global__ __launch_bounds__(256) void k_voxel_stats(const VoxTable t, int min_points, unsigned long long* __restrict__ st) {
    unsigned long long occ = 0, kept = 0, wrapped = 0, far = 0;
    const unsigned long long mask = t.slots - 1ull;
    for (unsigned long long s = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x; s < t.slots;
         s += static_cast<unsigned long long>(gridDim.x) * 256) {
        const unsigned long long k = t.keys[s];
        if (k == kVoxEmpty) continue;
        const unsigned long long h = vox_home(k, t.log2_slots);
        ++occ;
        kept += t.cnt[s] >= static_cast<uint32_t>(min_points) ? 1ull : 0ull;
        wrapped += s < h ? 1ull : 0ull;
        far = max(far, ((s - h) & mask) + 1ull);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        occ += __shfl_xor(occ, d);
        kept += __shfl_xor(kept, d);
        wrapped += __shfl_xor(wrapped, d);
        far = max(far, static_cast<unsigned long long>(__shfl_xor(far, d)));
    }
    if ((threadIdx.x & 63) == 0) {
        if (occ) atomicAdd(&st[kVoxOccupied], occ);
        if (kept) atomicAdd(&st[kVoxKept], kept);
        if (wrapped) atomicAdd(&st[kVoxWrapped], wrapped);
        if (far) atomicMax(&st[kVoxMaxProbe], far);
    }
}

// kept: the first point of a voxel that is kept; its position is the voxel's output id
struct VoxelCompact : CompactOp {
    const float* pts;
    VoxGrid g;
    VoxTable t;
    int min_points;
    unsigned long long* vslot;
    unsigned long long* st;
    __device__ bool keep(unsigned long long idx, Lane&) const {
        float v[9], frac[3];
        unsigned long long key, s;
        if (!(vox_load(pts + 9ull * idx, v) && vox_cell(v, g, key, frac))) return false;
        if (table_find(t, key, s) != 0) { atomicOr(&st[kVoxErr], 2ull); return false; }
        return t.first[s] == idx && t.cnt[s] >= static_cast<uint32_t>(min_points);
    }
    __device__ void emit(unsigned long long idx, unsigned long long pos, Lane&) const {
        float v[9], frac[3];
        unsigned long long key, s;
        if (vox_load(pts + 9ull * idx, v) && vox_cell(v, g, key, frac) && table_find(t, key, s) == 0) {
            t.oid[s] = pos;
            vslot[pos] = s;
        } else {
            atomicOr(&st[kVoxErr], 4ull);
        }
    }
};

__global__ __launch_bounds__(256) void k_voxel_accumulate(const float* __restrict__ pts, unsigned long long i0, int n,
                                                          const VoxGrid g, const VoxTable t,
                                                          unsigned long long* __restrict__ sums,
                                                          unsigned long long* __restrict__ st) {
    const int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (i >= n) return;
    float v[9], frac[3];
    unsigned long long key, s;
    if (!(vox_load(pts + 9ull * (i0 + static_cast<unsigned long long>(i)), v) && vox_cell(v, g, key, frac))) return;
    if (table_find(t, key, s) != 0) { atomicOr(&st[kVoxErr], 8ull); return; }
    const unsigned long long o = t.oid[s];
    if (o == kVoxEmpty) return;                      // fewer than min_points
    unsigned long long* acc = sums + 9ull * o;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        // step 3: 16.16 fixed point, round half to even; the product by a power of two is exact
        const float q = rintf((k < 3 ? frac[k] : v[k]) * 65536.0f);
        atomicAdd(&acc[k], static_cast<unsigned long long>(static_cast<long long>(q)));
    }
}

__global__ __launch_bounds__(256) void k_voxel_finalise(unsigned long long nv, const unsigned long long* __restrict__ vslot,
                                                        const VoxTable t, const unsigned long long* __restrict__ sums,
                                                        const VoxGrid g, float* __restrict__ out,
                                                        int32_t* __restrict__ out_cnt) {
    const unsigned long long v = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    if (v >= nv) return;
    const unsigned long long s = vslot[v];
    if (s >= t.slots) return;                        // an id the compaction did not fill (the host reports it)
    const unsigned long long key = t.keys[s];
    const uint32_t n = t.cnt[s];
    const double div = static_cast<double>(n) * 65536.0;
    const double o[3] = {static_cast<double>(g.ox), static_cast<double>(g.oy), static_cast<double>(g.oz)};
    const unsigned long long* acc = sums + 9ull * v;
    float* dst = out + 9ull * v;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const double mean = static_cast<double>(static_cast<long long>(acc[k])) / div;
        if (k < 3) {
            const double cell = static_cast<double>((key >> (21 * k)) & 0x1fffffull);
            dst[k] = static_cast<float>(o[k] + (cell + mean) * static_cast<double>(g.size));
        } else {
            dst[k] = static_cast<float>(mean);
        }
    }
    out_cnt[v] = static_cast<int32_t>(n);
}

hipError_t launch_voxel_min(const float* pts, unsigned long long i0, int n, uint32_t* mn, hipStream_t s) {
    k_voxel_min<<<static_cast<unsigned>(cdiv(n, 256)), 256, 0, s>>>(pts, i0, n, mn);
    return hipGetLastError();
}

hipError_t launch_voxel_insert(const float* pts, unsigned long long i0, int n, VoxGrid g, VoxTable t,
                               unsigned long long* st, hipStream_t s) {
    k_voxel_insert<<<static_cast<unsigned>(cdiv(n, 256)), 256, 0, s>>>(pts, i0, n, g, t, st);
    return hipGetLastError();
}

hipError_t launch_voxel_stats(VoxTable t, int min_points, unsigned long long* st, hipStream_t s) {
    const unsigned long long blocks = std::min<unsigned long long>((t.slots + 255ull) / 256ull, 4096ull);
    k_voxel_stats<<<static_cast<unsigned>(blocks), 256, 0, s>>>(t, min_points, st);
    return hipGetLastError();
}

hipError_t launch_voxel_compact(const float* pts, unsigned long long i0, int n, VoxGrid g, VoxTable t, int min_points,
                                Compaction c, unsigned long long* vslot, unsigned long long* st, hipStream_t s) {
    return compact_segment(VoxelCompact{{}, pts, g, t, min_points, vslot, st}, i0, n, c, s);
}

hipError_t launch_voxel_accumulate(const float* pts, unsigned long long i0, int n, VoxGrid g, VoxTable t,
                                   unsigned long long* sums, unsigned long long* st, hipStream_t s) {
    k_voxel_accumulate<<<static_cast<unsigned>(cdiv(n, 256)), 256, 0, s>>>(pts, i0, n, g, t, sums, st);
    return hipGetLastError();
}

hipError_t launch_voxel_finalise(unsigned long long nv, const unsigned long long* vslot, VoxTable t,
                                 const unsigned long long* sums, VoxGrid g, float* out, int32_t* out_cnt, hipStream_t s) {
    if (nv == 0) return hipSuccess;
    k_voxel_finalise<<<static_cast<unsigned>((nv + 255ull) / 256ull), 256, 0, s>>>(nv, vslot, t, sums, g, out, out_cnt);
    return hipGetLastError();
}

// ------------------------------------------------------------------ cleaning the voxel cloud
//
// acmmp_fusion_voxel_clean (include/acmmp.h): support count, connected components and the kept
// voxels of the resident voxel result, through the table that voxelize left (cell -> slot -> oid).  Everything
// is an integer, and every atomic is a minimum, an or or an integer add: no result depends on the order they land in.

// Neighbour `b` (0 .. 27, b = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)) of the cell `key`, offsets applied per axis
// on the unpacked 21-bit indices; false = that cell does not exist.
__device__ __forceinline__ bool clean_neighbour(unsigned long long key, int b, unsigned long long& nkey) {
    const int d[3] = {b % 3 - 1, (b / 3) % 3 - 1, b / 9 - 1};
    nkey = 0;
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int g = static_cast<int>((key >> (21 * a)) & 0x1fffffull) + d[a];
        ok = ok && g >= 0 && g < (1 << 21);
        nkey |= static_cast<unsigned long long>(ok ? g : 0) << (21 * a);
    }
    return ok;
}

// dst[0 .. 9) = src[0 .. 9) of another array: the nine loads go out ahead of the stores.
__device__ __forceinline__ void copy9(float* __restrict__ dst, const float* __restrict__ src) {
#pragma unroll
    for (int k = 0; k < 9; ++k) dst[k] = src[k];
}

// *word |= the or of `bits` over the workgroup, one atomic per workgroup.  Every lane calls it.
__device__ __forceinline__ void block_or(unsigned bits, unsigned long long* word) {
    __shared__ unsigned acc;
    if (threadIdx.x == 0) acc = 0u;
    __syncthreads();
    if (bits) atomicOr(&acc, bits);
    __syncthreads();
    if (threadIdx.x == 0 && acc) atomicOr(word, static_cast<unsigned long long>(acc));
}

// *word += the sum of x over the wave, one atomic per wave.  Every lane of the wave calls it.
__device__ __forceinline__ void wave_add(unsigned long long x, unsigned long long* word) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    if ((threadIdx.x & 63) == 0 && x) atomicAdd(word, x);
}

// Step 1 and 2: nbmask[v] = bit b set when neighbour b of voxel v is a voxel (its popcount is support(v)),
// lab[v] = v for a supported voxel and ~0 for the others.
__global__ __launch_bounds__(256) void k_clean_support(unsigned long long nv, const unsigned long long* __restrict__ vslot,
                                                       const VoxTable t, int max_l1, int min_neighbours,
                                                       uint32_t* __restrict__ nbmask, unsigned long long* __restrict__ lab,
                                                       unsigned long long* __restrict__ words) {
    const unsigned long long v = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    unsigned err = 0u;
    unsigned long long unsupported = 0;
    if (v < nv) {
        const unsigned long long s = vslot[v];
        uint32_t m = 0u;
        if (s >= t.slots) {
            err |= 1u;
        } else {
            const unsigned long long key = t.keys[s];
            for (int b = 0; b < 27; ++b) {
                const int l1 = abs(b % 3 - 1) + abs((b / 3) % 3 - 1) + abs(b / 9 - 1);
                unsigned long long nkey, ns;
                if (l1 == 0 || l1 > max_l1 || !clean_neighbour(key, b, nkey)) continue;
                const int r = table_find(t, nkey, ns);
                if (r == 2) err |= 2u;
                if (r == 0 && t.oid[ns] < nv) m |= 1u << b;          // a cell below min_points has no oid
            }
        }
        const bool in = __popc(m) >= min_neighbours;
        nbmask[v] = m;
        lab[v] = in ? v : kVoxEmpty;
        unsupported = in ? 0ull : 1ull;
    }
    wave_add(unsupported, &words[kCleanUnsupported]);
    block_or(err, &words[kCleanErr]);
}

// One labelling round.  lab[x] only ever holds the index of a supported voxel of x's component that is <= x, and
// only ever decreases, so whatever a load returns here -- the value at the start of the launch or one that another
// workgroup has written since -- is such an index: a stale load can cost a round, never correctness.  A voxel takes
// the smallest label among its own and its supported neighbours', follows the labels from there to a voxel that
// labels itself (at most nv steps: each is strictly smaller), and lowers its label and its previous label's to it.
// A launch in which no lane lowers anything has read only the values of its start, which then satisfy
// lab[v] <= lab[u] over every edge and lab[lab[v]] = lab[v]: the smallest index of each component.
__global__ __launch_bounds__(256) void k_clean_round(unsigned long long nv, const unsigned long long* __restrict__ vslot,
                                                     const VoxTable t, const uint32_t* __restrict__ nbmask,
                                                     unsigned long long* lab, unsigned long long* __restrict__ words) {
    const unsigned long long v = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    unsigned err = 0u, changed = 0u;
    const unsigned long long cur = v < nv ? lab[v] : kVoxEmpty;
    const unsigned long long slot = v < nv ? vslot[v] : kVoxEmpty;
    if (cur != kVoxEmpty && slot >= t.slots) {
        err |= 1u;
    } else if (cur != kVoxEmpty) {
        unsigned long long m = cur;
        const unsigned long long key = t.keys[slot];
        for (uint32_t left = nbmask[v]; left; left &= left - 1u) {
            unsigned long long nkey, ns;
            if (!clean_neighbour(key, __ffs(static_cast<int>(left)) - 1, nkey) || table_find(t, nkey, ns) != 0) { err |= 4u; continue; }
            const unsigned long long o = t.oid[ns];
            if (o >= nv) { err |= 4u; continue; }
            m = min(m, lab[o]);                                      // ~0 (unsupported) never wins
        }
        unsigned long long steps = 0;
        for (; steps <= nv && m < nv; ++steps) {
            const unsigned long long p = lab[m];
            if (p >= m) break;
            m = p;
        }
        if (steps > nv || m >= nv) {
            err |= 8u;
        } else if (m < cur) {
            atomicMin(&lab[v], m);
            atomicMin(&lab[cur], m);
            changed = 1u;
        }
    }
    block_or(changed, &words[kCleanChanged]);
    block_or(err, &words[kCleanErr]);
}

// Step 4's sizes: cvox[label] += 1, cpts[label] += count, 64-bit integer adds.  A wave whose supported lanes share
// one label -- the usual case, a surface is few components -- adds once.
__global__ __launch_bounds__(256) void k_clean_sizes(unsigned long long nv, const unsigned long long* __restrict__ lab,
                                                     const int32_t* __restrict__ cnt, unsigned long long* __restrict__ cvox,
                                                     unsigned long long* __restrict__ cpts) {
    const unsigned long long v = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    const unsigned long long L = v < nv ? lab[v] : kVoxEmpty;
    const bool in = L < nv;
    unsigned long long c = in ? static_cast<unsigned long long>(cnt[v]) : 0ull;
    const unsigned long long active = __ballot(in);
    if (!active) return;
    const int leader = __ffsll(active) - 1;
    const unsigned long long Lf = __shfl(L, leader);
    if (__all(!in || L == Lf)) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
        if ((threadIdx.x & 63) == leader) {
            atomicAdd(&cvox[Lf], static_cast<unsigned long long>(__popcll(active)));
            atomicAdd(&cpts[Lf], c);
        }
    } else if (in) {
        atomicAdd(&cvox[L], 1ull);
        atomicAdd(&cpts[L], c);
    }
}

__device__ __forceinline__ bool clean_component_kept(unsigned long long L, const unsigned long long* __restrict__ cvox,
                                                     const unsigned long long* __restrict__ cpts, unsigned long long min_voxels,
                                                     unsigned long long min_points) {
    return cvox[L] >= min_voxels && cpts[L] >= min_points;
}

// components, kept components and kept voxels
__global__ __launch_bounds__(256) void k_clean_count(unsigned long long nv, const unsigned long long* __restrict__ lab,
                                                     const unsigned long long* __restrict__ cvox,
                                                     const unsigned long long* __restrict__ cpts, unsigned long long min_voxels,
                                                     unsigned long long min_points, unsigned long long* __restrict__ words) {
    const unsigned long long v = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    const unsigned long long L = v < nv ? lab[v] : kVoxEmpty;
    const bool in = L < nv;
    const bool kept = in && clean_component_kept(L, cvox, cpts, min_voxels, min_points);
    wave_add(in && L == v ? 1ull : 0ull, &words[kCleanComps]);
    wave_add(kept && L == v ? 1ull : 0ull, &words[kCleanCompsKept]);
    wave_add(kept ? 1ull : 0ull, &words[kCleanKept]);
}

// kept: the voxels that label themselves (the roots of the components), in ascending order; a root's position is its
// component's id: its table entry, c.id[root] = id
struct CleanRoots : CompactOp {
    unsigned long long nv;
    const unsigned long long* lab;
    CleanComp c;
    long long* out_root;
    long long* out_voxels;
    long long* out_points;
    __device__ bool keep(unsigned long long v, Lane&) const {
        const unsigned long long L = lab[v];
        return L < nv && L == v;
    }
    __device__ void emit(unsigned long long v, unsigned long long pos, Lane&) const {
        c.id[v] = pos;
        out_root[pos] = static_cast<long long>(v);
        out_voxels[pos] = static_cast<long long>(c.voxels[v]);
        out_points[pos] = static_cast<long long>(c.points[v]);
    }
};

// kept: the voxels of kept components, in ascending order: the voxel's 9 floats and count as they are, and its
// component's id
struct CleanKept : CompactOp {
    unsigned long long nv;
    const unsigned long long* lab;
    CleanComp c;
    const float* v_pts;
    const int32_t* v_cnt;
    float* out;
    int32_t* out_cnt;
    long long* out_comp;
    unsigned long long* out_vox;
    __device__ bool keep(unsigned long long v, Lane&) const {
        const unsigned long long L = lab[v];
        return L < nv && clean_component_kept(L, c.voxels, c.points, c.min_voxels, c.min_points);
    }
    __device__ void emit(unsigned long long v, unsigned long long pos, Lane&) const {
        copy9(out + 9ull * pos, v_pts + 9ull * v);
        out_cnt[pos] = v_cnt[v];
        out_comp[pos] = static_cast<long long>(c.id[lab[v]]);
        out_vox[pos] = v;
    }
};

static unsigned clean_blocks(unsigned long long nv) { return static_cast<unsigned>((nv + 255ull) / 256ull); }

hipError_t launch_clean_support(unsigned long long nv, const unsigned long long* vslot, VoxTable t, int connectivity,
                                int min_neighbours, uint32_t* nbmask, unsigned long long* lab, unsigned long long* words,
                                hipStream_t s) {
    const int max_l1 = connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3;
    k_clean_support<<<clean_blocks(nv), 256, 0, s>>>(nv, vslot, t, max_l1, min_neighbours, nbmask, lab, words);
    return hipGetLastError();
}

hipError_t launch_clean_round(unsigned long long nv, const unsigned long long* vslot, VoxTable t, const uint32_t* nbmask,
                              unsigned long long* lab, unsigned long long* words, hipStream_t s) {
    k_clean_round<<<clean_blocks(nv), 256, 0, s>>>(nv, vslot, t, nbmask, lab, words);
    return hipGetLastError();
}

hipError_t launch_clean_sizes(unsigned long long nv, const unsigned long long* lab, const int32_t* cnt, CleanComp c,
                              unsigned long long* words, hipStream_t s) {
    k_clean_sizes<<<clean_blocks(nv), 256, 0, s>>>(nv, lab, cnt, c.voxels, c.points);
    k_clean_count<<<clean_blocks(nv), 256, 0, s>>>(nv, lab, c.voxels, c.points, c.min_voxels, c.min_points, words);
    return hipGetLastError();
}

hipError_t launch_clean_compact_roots(unsigned long long nv, unsigned long long i0, int n, const unsigned long long* lab,
                                      CleanComp c, Compaction k, long long* out_root, long long* out_voxels,
                                      long long* out_points, hipStream_t s) {
    return compact_segment(CleanRoots{{}, nv, lab, c, out_root, out_voxels, out_points}, i0, n, k, s);
}

hipError_t launch_clean_compact_kept(unsigned long long nv, unsigned long long i0, int n, const unsigned long long* lab,
                                     CleanComp c, Compaction k, const float* v_pts, const int32_t* v_cnt, float* out,
                                     int32_t* out_cnt, long long* out_comp, unsigned long long* out_vox, hipStream_t s) {
    return compact_segment(CleanKept{{}, nv, lab, c, v_pts, v_cnt, out, out_cnt, out_comp, out_vox}, i0, n, k, s);
}

// ------------------------------------------------------------------ visibility check of the voxel cloud
//
// acmmp_fusion_voxel_visibility (include/acmmp.h): every entry of the voxel or clean result is
// projected into every listed view and classed against that view's raw depth map.  The classes are decided by
// float32 comparisons of one entry against one pixel; what is summed is the integer count of each class, so no
// result depends on the order the adds land in.

// Steps 1 and 2: the projection of X into one view, its depth pd and its pixel (c, r); false = unobserved.
template <int MODEL>
__device__ __forceinline__ bool vis_pixel(const DevCam& cam, const FuseView& view, float3 X, int& c, int& r, float& pd) {
    float px, py;
    project<MODEL, const DevCam, true>(cam, X, px, py, pd);
    if (vox_nonfinite(px) || vox_nonfinite(py) || vox_nonfinite(pd) || !(pd > 0.0f)) return false;
    c = f2i_sat(px + 0.5f);
    r = f2i_sat(py + 0.5f);
    return c >= 0 && c < view.W && r >= 0 && r < view.H;
}

// The class of entry X in one view: 0 support, 1 conflict, 2 occluded, 3 unobserved.
template <int MODEL>
__device__ __forceinline__ int vis_class(const DevCam& cam, const FuseView& view, float3 X, float rel_tol, int radius) {
    int c, r;
    float pd;
    if (!vis_pixel<MODEL>(cam, view, X, c, r, pd)) return 3;
    bool any = false, agree = false, behind = false;
    for (int dy = -radius; dy <= radius; ++dy) {
        const int rr = r + dy;
        if (rr < 0 || rr >= view.H) continue;
        for (int dx = -radius; dx <= radius; ++dx) {
            const int cc = c + dx;
            if (cc < 0 || cc >= view.W) continue;
            const float sd = view.depth[static_cast<long long>(rr) * view.W + cc];
            if (vox_nonfinite(sd) || !(sd > 0.0f)) continue;
            const float t = rel_tol * sd, d = pd - sd;
            any = true;
            agree = agree || fabsf(d) <= t;
            behind = behind || d > t;
        }
    }
    return !any ? 3 : agree ? 0 : behind ? 2 : 1;
}

// One lane per entry, blockIdx.y = a chunk of kVisChunk list positions.  The view index of a position is the same
// for every lane, so the camera and the view's addresses load as scalars; neighbouring entries are neighbours in
// space (first-appearance order), so a wave's depth gathers fall close together.  ATOMIC: more than one chunk, the
// lane adds its chunk's counts to tallies that were zeroed; otherwise it stores them.
template <int MODEL, bool ATOMIC>
__global__ __launch_bounds__(256) void k_vis_tally(const DevCam* __restrict__ cams, const FuseView* __restrict__ views,
                                                   const int* __restrict__ list, int n_list, const float* __restrict__ pts,
                                                   unsigned long long n, float rel_tol, int radius, int32_t* tallies) {
    const unsigned long long e = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= n) return;
    const float* p = pts + 9ull * e;
    const float3 X = make_float3(p[0], p[1], p[2]);
    const int j0 = static_cast<int>(blockIdx.y) * kVisChunk;
    const int j1 = min(j0 + kVisChunk, n_list);
    int cls[3] = {0, 0, 0};
    for (int j = j0; j < j1; ++j) {
        const int vi = list[j];
        const FuseView view = views[vi];
        const int k = vis_class<MODEL>(cams[vi], view, X, rel_tol, radius);
        cls[0] += k == 0 ? 1 : 0;
        cls[1] += k == 1 ? 1 : 0;
        cls[2] += k == 2 ? 1 : 0;
    }
    int32_t* t = tallies + 3ull * e;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if constexpr (ATOMIC) { if (cls[k]) atomicAdd(&t[k], cls[k]); }
        else t[k] = cls[k];
    }
}

__device__ __forceinline__ bool vis_kept(const int32_t* __restrict__ t, int min_support, int max_conflicts) {
    return t[0] >= min_support && t[1] <= max_conflicts;
}

// the sums of the four classes, and the entries that are kept, that lack support, that conflict
__global__ __launch_bounds__(256) void k_vis_count(unsigned long long n, const int32_t* __restrict__ tallies, int n_list,
                                                   int min_support, int max_conflicts, unsigned long long* __restrict__ words) {
    const unsigned long long e = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    const bool in = e < n;
    const int32_t* t = tallies + 3ull * (in ? e : 0ull);
    const unsigned long long s = in ? t[0] : 0, c = in ? t[1] : 0, o = in ? t[2] : 0;
    wave_add(s, &words[kVisSupport]);
    wave_add(c, &words[kVisConflict]);
    wave_add(o, &words[kVisOccluded]);
    wave_add(in ? static_cast<unsigned long long>(n_list) - s - c - o : 0ull, &words[kVisUnobserved]);
    wave_add(in && vis_kept(t, min_support, max_conflicts) ? 1ull : 0ull, &words[kVisKept]);
    wave_add(in && t[0] < min_support ? 1ull : 0ull, &words[kVisNoSupport]);
    wave_add(in && t[1] > max_conflicts ? 1ull : 0ull, &words[kVisConflicting]);
}

// kept: the kept entries, in ascending order: the entry's 9 floats and count as they are, and its tallies
struct VisCompact : CompactOp {
    const int32_t* tallies;
    int min_support, max_conflicts;
    const float* src_pts;
    const int32_t* src_cnt;
    float* out;
    int32_t* out_cnt;
    int32_t* out_tal;
    const unsigned long long* src_vox;
    unsigned long long* out_vox;
    __device__ bool keep(unsigned long long e, Lane&) const { return vis_kept(tallies + 3ull * e, min_support, max_conflicts); }
    __device__ void emit(unsigned long long e, unsigned long long pos, Lane&) const {
        copy9(out + 9ull * pos, src_pts + 9ull * e);
        out_cnt[pos] = src_cnt[e];
#pragma unroll
        for (int k = 0; k < 3; ++k) out_tal[3ull * pos + k] = tallies[3ull * e + k];
        out_vox[pos] = src_vox ? src_vox[e] : e;
    }
};

hipError_t launch_vis_tally(int model, const DevCam* cams, const FuseView* views, const int* list, int n_list,
                            const float* pts, unsigned long long n, float rel_tol, int radius, int32_t* tallies,
                            hipStream_t s) {
    const int chunks = cdiv(n_list, kVisChunk);
    const dim3 grd(clean_blocks(n), static_cast<unsigned>(chunks));
    if (chunks > 1) {
        const hipError_t e = hipMemsetAsync(tallies, 0, sizeof(int32_t) * 3ull * n, s);
        if (e != hipSuccess) return e;
        if (model == kSphere) k_vis_tally<kSphere, true><<<grd, 256, 0, s>>>(cams, views, list, n_list, pts, n, rel_tol, radius, tallies);
        else k_vis_tally<kPinhole, true><<<grd, 256, 0, s>>>(cams, views, list, n_list, pts, n, rel_tol, radius, tallies);
    } else {
        if (model == kSphere) k_vis_tally<kSphere, false><<<grd, 256, 0, s>>>(cams, views, list, n_list, pts, n, rel_tol, radius, tallies);
        else k_vis_tally<kPinhole, false><<<grd, 256, 0, s>>>(cams, views, list, n_list, pts, n, rel_tol, radius, tallies);
    }
    return hipGetLastError();
}

hipError_t launch_vis_count(unsigned long long n, const int32_t* tallies, int n_list, int min_support, int max_conflicts,
                            unsigned long long* words, hipStream_t s) {
    k_vis_count<<<clean_blocks(n), 256, 0, s>>>(n, tallies, n_list, min_support, max_conflicts, words);
    return hipGetLastError();
}

hipError_t launch_vis_compact(unsigned long long i0, int n, const int32_t* tallies, int min_support, int max_conflicts,
                              Compaction c, const float* src_pts, const int32_t* src_cnt, float* out, int32_t* out_cnt,
                              int32_t* out_tal, const unsigned long long* src_vox, unsigned long long* out_vox,
                              hipStream_t s) {
    return compact_segment(VisCompact{{}, tallies, min_support, max_conflicts, src_pts, src_cnt, out, out_cnt, out_tal,
                                      src_vox, out_vox}, i0, n, c, s);
}

// ------------------------------------------------------------------ surface mesh of the voxel cloud
//
// acmmp_fusion_voxel_mesh (include/acmmp.h): the cells within one cell of an entry are the samples of
// a truncated signed distance to the views' raw depth maps, summed as integers; the cubes of eight valid samples
// whose signs differ give one vertex each (surface nets) and the sign changes along the axes give the quads between
// them.  The sample table is VoxTable's scheme; which slot a cell gets is the only racy thing, and nothing that is
// read back depends on it: samples are numbered by rank, vertices by sample, faces by (sample, axis).

// The number of the sample at offset `b` (clean_neighbour's index) of the cell `key`: 0 = found, 1 = no such sample,
// 2 = the probe sequence covered every slot or the slot holds no number.
__device__ __forceinline__ int mesh_sample(const MeshTable& m, unsigned long long ns, unsigned long long key, int b,
                                           unsigned long long& sid) {
    unsigned long long nkey, s;
    if (!clean_neighbour(key, b, nkey)) return 1;
    const int r = table_find(m, nkey, s);
    if (r != 0) return r;
    sid = m.sid[s];
    return sid < ns ? 0 : 2;
}

// clean_neighbour's index of the offset (dx, dy, dz)
__device__ __forceinline__ int mesh_offset(int dx, int dy, int dz) { return (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1); }

__global__ __launch_bounds__(256) void k_mesh_keys(unsigned long long ne, const unsigned long long* __restrict__ vox,
                                                   unsigned long long nv, const unsigned long long* __restrict__ vslot,
                                                   const VoxTable t, unsigned long long* __restrict__ ekey,
                                                   unsigned long long* __restrict__ words) {
    const unsigned long long e = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    unsigned err = 0u;
    if (e < ne) {
        const unsigned long long v = vox ? vox[e] : e;
        const unsigned long long s = v < nv ? vslot[v] : kVoxEmpty;
        if (s < t.slots) ekey[e] = t.keys[s];
        else { ekey[e] = kVoxEmpty; err = 1u; }
    }
    block_or(err, &words[kMeshErr]);
}

__global__ __launch_bounds__(256) void k_mesh_insert(unsigned long long p0, int n, const unsigned long long* __restrict__ ekey,
                                                     const MeshTable m, unsigned long long* __restrict__ words) {
    const int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (i >= n) return;
    const unsigned long long p = p0 + static_cast<unsigned long long>(i);
    const unsigned long long e = p / 27ull;
    const int b = static_cast<int>(p % 27ull);
    const unsigned long long key = ekey[e];
    unsigned long long nkey;
    if (key == kVoxEmpty || !clean_neighbour(key, b, nkey)) return;
    unsigned long long s;
    if (!table_claim(m, nkey, s)) { atomicOr(&words[kMeshErr], 2ull); return; }
    atomicMin(&m.rank[s], p);
    if (b == 13) m.ent[s] = e;                            // one entry at most has this cell
}

__global__ __launch_bounds__(256) void k_mesh_stats(const MeshTable m, unsigned long long* __restrict__ words) {
    unsigned long long occ = 0, wrapped = 0, far = 0;
    const unsigned long long mask = m.slots - 1ull;
    for (unsigned long long s = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x; s < m.slots;
         s += static_cast<unsigned long long>(gridDim.x) * 256) {
        const unsigned long long k = m.keys[s];
        if (k == kVoxEmpty) continue;
        const unsigned long long h = vox_home(k, m.log2_slots);
        ++occ;
        wrapped += s < h ? 1ull : 0ull;
        far = max(far, ((s - h) & mask) + 1ull);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        occ += __shfl_xor(occ, d);
        wrapped += __shfl_xor(wrapped, d);
        far = max(far, static_cast<unsigned long long>(__shfl_xor(far, d)));
    }
    if ((threadIdx.x & 63) == 0) {
        if (occ) atomicAdd(&words[kMeshOccupied], occ);
        if (wrapped) atomicAdd(&words[kMeshWrapped], wrapped);
        if (far) atomicMax(&words[kMeshMaxProbe], far);
    }
}

// The slot of pair p's cell when the pair owns the cell's rank: the pair that numbers the sample.
__device__ __forceinline__ bool mesh_owner(const MeshTable& m, const unsigned long long* __restrict__ ekey,
                                           unsigned long long p, unsigned long long& nkey, unsigned long long& slot,
                                           unsigned& err) {
    const unsigned long long key = ekey[p / 27ull];
    if (key == kVoxEmpty || !clean_neighbour(key, static_cast<int>(p % 27ull), nkey)) return false;
    if (table_find(m, nkey, slot) == 0) return m.rank[slot] == p;
    err |= 4u;                                            // the insert pass put every pair's cell there
    return false;
}

// The per-lane error bits of a mesh compaction, one block_or per workgroup into words[kMeshErr].
struct MeshLane {
    unsigned err = 0u;
};

// kept: the pairs that own their cell's rank, in ascending order; a pair's position is the sample's number
struct MeshNumber : CompactOp {
    using Lane = MeshLane;
    const unsigned long long* ekey;
    MeshTable m;
    MeshSamples out;
    unsigned long long* words;
    __device__ bool keep(unsigned long long p, Lane& lane) const {
        unsigned long long nkey, slot;
        return mesh_owner(m, ekey, p, nkey, slot, lane.err);
    }
    __device__ void mark_end(const Lane& lane) const { block_or(lane.err, &words[kMeshErr]); }
    __device__ void emit(unsigned long long p, unsigned long long pos, Lane& lane) const {
        unsigned long long nkey, slot;
        if (mesh_owner(m, ekey, p, nkey, slot, lane.err)) {              // (the mark pass has reported a failure)
            m.sid[slot] = pos;
            out.key[pos] = nkey;
            out.ent[pos] = static_cast<long long>(m.ent[slot]);          // ~0 reads as -1
        }
    }
};

// One lane per sample, blockIdx.y = a chunk of kVisChunk list positions, as k_vis_tally.
template <int MODEL, bool ATOMIC>
__global__ __launch_bounds__(256) void k_mesh_tsdf(const DevCam* __restrict__ cams, const FuseView* __restrict__ views,
                                                   const int* __restrict__ list, int n_list, const MeshSamples smp,
                                                   const VoxGrid g, float trunc, float k) {
    const unsigned long long s = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    if (s >= smp.n) return;
    const unsigned long long key = smp.key[s];
    const double o[3] = {static_cast<double>(g.ox), static_cast<double>(g.oy), static_cast<double>(g.oz)};
    float x[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        x[a] = static_cast<float>(o[a] + (static_cast<double>((key >> (21 * a)) & 0x1fffffull) + 0.5) * static_cast<double>(g.size));
    const float3 X = make_float3(x[0], x[1], x[2]);
    const int j0 = static_cast<int>(blockIdx.y) * kVisChunk;
    const int j1 = min(j0 + kVisChunk, n_list);
    int S = 0, cnt = 0;
    for (int j = j0; j < j1; ++j) {
        const int vi = list[j];
        const FuseView view = views[vi];
        int c, r;
        float pd;
        if (!vis_pixel<MODEL>(cams[vi], view, X, c, r, pd)) continue;
        const float sd = view.depth[static_cast<long long>(r) * view.W + c];
        if (vox_nonfinite(sd) || !(sd > 0.0f)) continue;
        const float u = sd - pd;
        if (u < -trunc) continue;
        S += static_cast<int>(rintf(fminf(u, trunc) * k));
        ++cnt;
    }
    int32_t* t = smp.tsdf + 2ull * s;
    if constexpr (ATOMIC) {
        if (S) atomicAdd(&t[0], S);
        if (cnt) atomicAdd(&t[1], cnt);
    } else {
        t[0] = S;
        t[1] = cnt;
    }
}

__global__ __launch_bounds__(256) void k_mesh_cubes(const MeshSamples smp, const MeshTable m, int min_weight,
                                                    uint8_t* __restrict__ cflag, unsigned long long* __restrict__ words) {
    const unsigned long long s = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    unsigned err = 0u;
    unsigned bits = 0u;
    if (s < smp.n) {
        const unsigned long long key = smp.key[s];
        const bool valid = smp.tsdf[2ull * s + 1] >= min_weight, inside = smp.tsdf[2ull * s] < 0;
        bool exists = valid, differ = false;
        for (int c = 1; c < 8 && exists; ++c) {
            unsigned long long q;
            const int r = mesh_sample(m, smp.n, key, mesh_offset(c & 1, (c >> 1) & 1, c >> 2), q);
            if (r == 2) err |= 4u;
            exists = r == 0 && smp.tsdf[2ull * q + 1] >= min_weight;
            if (exists) differ = differ || (smp.tsdf[2ull * q] < 0) != inside;
        }
        bits = (exists ? kMeshCubeExists : 0u) | (exists && differ ? kMeshCubeActive : 0u) | (valid ? kMeshSampleValid : 0u) |
               (inside ? kMeshSampleInside : 0u);
        cflag[s] = static_cast<uint8_t>(bits);
    }
    wave_add((bits & kMeshSampleValid) ? 1ull : 0ull, &words[kMeshValid]);
    wave_add((bits & kMeshCubeExists) ? 1ull : 0ull, &words[kMeshCubes]);
    wave_add((bits & kMeshCubeActive) ? 1ull : 0ull, &words[kMeshActive]);
    block_or(err, &words[kMeshErr]);
}

// The four cubes around the edge from sample s along axis a, in the order Q0 .. Q3; false = one of them is no sample.
__device__ __forceinline__ int mesh_quad(const MeshTable& m, unsigned long long ns, unsigned long long key, int a,
                                         unsigned long long s, unsigned long long q[4]) {
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    const int qu[4] = {0, 1, 1, 0}, qv[4] = {0, 0, 1, 1};
    q[0] = s;
    for (int k = 1; k < 4; ++k) {
        int d[3] = {0, 0, 0};
        d[b] = -qu[k];
        d[c] = -qv[k];
        const int r = mesh_sample(m, ns, key, mesh_offset(d[0], d[1], d[2]), q[k]);
        if (r != 0) return r;
    }
    return 0;
}

// fbits[s]: bit a = the pair (s, axis a) emits its two triangles (step 4)
__global__ __launch_bounds__(256) void k_mesh_pairs(const MeshSamples smp, const MeshTable m, const uint8_t* __restrict__ cflag,
                                                    uint8_t* __restrict__ fbits, unsigned long long* __restrict__ words) {
    const unsigned long long s = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    unsigned err = 0u, bits = 0u;
    if (s < smp.n) {
        const unsigned long long key = smp.key[s];
        const unsigned me = cflag[s];
        if (me & kMeshSampleValid) {
            for (int a = 0; a < 3; ++a) {
                unsigned long long o, q[4];
                int r = mesh_sample(m, smp.n, key, mesh_offset(a == 0, a == 1, a == 2), o);
                if (r == 2) err |= 4u;
                if (r != 0) continue;
                const unsigned other = cflag[o];
                if (!(other & kMeshSampleValid) || ((other ^ me) & kMeshSampleInside) == 0u) continue;
                r = mesh_quad(m, smp.n, key, a, s, q);
                if (r == 2) err |= 4u;
                if (r != 0) continue;
                bool all = true;
                for (int k = 0; k < 4; ++k) all = all && (cflag[q[k]] & kMeshCubeExists);
                if (all) bits |= 1u << a;
            }
        }
        fbits[s] = static_cast<uint8_t>(bits);
    }
    wave_add(static_cast<unsigned long long>(__popc(bits)), &words[kMeshPairs]);
    block_or(err, &words[kMeshErr]);
}

// Bit `bit` of bytes[p / per] shifted by p % per: the active cubes (per 1) or the face pairs (per 3).
__device__ __forceinline__ bool mesh_flag(const uint8_t* __restrict__ bytes, int per, int bit, unsigned long long p) {
    return (bytes[p / static_cast<unsigned>(per)] >> (bit + static_cast<int>(p % static_cast<unsigned>(per)))) & 1;
}

// kept: the active cubes, in ascending sample order; step 3 for each: position, normal, colour.
struct MeshVertices : CompactOp {
    struct Lane : MeshLane {
        unsigned long long uncoloured = 0;
    };
    MeshSamples smp;
    MeshTable m;
    VoxGrid g;
    const uint8_t* cflag;
    const float* src_pts;
    float* verts;
    int32_t* vid;
    unsigned long long* words;
    __device__ bool keep(unsigned long long s, Lane&) const { return mesh_flag(cflag, 1, 1, s); }       // kMeshCubeActive
    __device__ void scatter_end(const Lane& lane) const {
        wave_add(lane.uncoloured, &words[kMeshUncoloured]);
        block_or(lane.err, &words[kMeshErr]);
    }
    __device__ void emit(unsigned long long s, unsigned long long pos, Lane& lane) const {
        const unsigned long long key = smp.key[s];
        long long S[8], N[8], ent[8];
        bool ok = true;
        for (int c = 0; c < 8; ++c) {
            unsigned long long q = s;
            if (c > 0 && mesh_sample(m, smp.n, key, mesh_offset(c & 1, (c >> 1) & 1, c >> 2), q) != 0) { ok = false; q = s; }
            S[c] = smp.tsdf[2ull * q];
            N[c] = smp.tsdf[2ull * q + 1];
            ent[c] = smp.ent[q];
        }
        if (!ok) {
            lane.err |= 8u;
        } else {
            double L[3] = {0.0, 0.0, 0.0}, G[3] = {0.0, 0.0, 0.0};
            int crossings = 0;
            for (int e = 0; e < 12; ++e) {
                const int ax = e >> 2, k = e & 3;
                // the four edges of an axis: the corners whose bit `ax` is clear, in ascending order
                const int lowm = (1 << ax) - 1;
                const int p = ((k & ~lowm) << 1) | (k & lowm), q = p | (1 << ax);
                const double fp = static_cast<double>(S[p]) / (1024.0 * static_cast<double>(N[p]));
                const double fq = static_cast<double>(S[q]) / (1024.0 * static_cast<double>(N[q]));
                G[ax] += fq - fp;
                if ((S[p] < 0) == (S[q] < 0)) continue;
                const double A = static_cast<double>(S[p] * N[q]), B = static_cast<double>(S[q] * N[p]);
                const double t = A / (A - B);
#pragma unroll
                for (int a = 0; a < 3; ++a) L[a] += static_cast<double>((p >> a) & 1) + (a == ax ? t : 0.0);
                ++crossings;
            }
            const double o[3] = {static_cast<double>(g.ox), static_cast<double>(g.oy), static_cast<double>(g.oz)};
            float* dst = verts + 9ull * pos;
            const double len = sqrt(G[0] * G[0] + G[1] * G[1] + G[2] * G[2]);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double cell = static_cast<double>((key >> (21 * a)) & 0x1fffffull);
                dst[a] = static_cast<float>(o[a] + ((cell + 0.5) + L[a] / static_cast<double>(crossings)) * static_cast<double>(g.size));
                dst[3 + a] = len > 0.0 ? static_cast<float>(G[a] / len) : 0.0f;
            }
            double col[3] = {0.0, 0.0, 0.0};
            int coloured = 0;
            for (int c = 0; c < 8; ++c) {
                if (ent[c] < 0) continue;
                const float* src = src_pts + 9ull * static_cast<unsigned long long>(ent[c]);
#pragma unroll
                for (int a = 0; a < 3; ++a) col[a] += static_cast<double>(src[6 + a]);
                ++coloured;
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) dst[6 + a] = coloured ? static_cast<float>(col[a] / static_cast<double>(coloured)) : 128.0f;
            lane.uncoloured = coloured ? 0ull : 1ull;
            vid[s] = static_cast<int32_t>(pos);
        }
    }
};

// kept: the (sample, axis) pairs flagged in fbits, in ascending order; step 4 for each: two triangles.
struct MeshFaces : CompactOp {
    using Lane = MeshLane;
    MeshSamples smp;
    MeshTable m;
    const uint8_t* cflag;
    const uint8_t* fbits;
    const int32_t* vid;
    int32_t* faces;
    unsigned long long* words;
    __device__ bool keep(unsigned long long p, Lane&) const { return mesh_flag(fbits, 3, 0, p); }
    __device__ void scatter_end(const Lane& lane) const { block_or(lane.err, &words[kMeshErr]); }
    __device__ void emit(unsigned long long p, unsigned long long pos, Lane& lane) const {
        const unsigned long long s = p / 3ull;
        unsigned long long q[4];
        int32_t v[4] = {-1, -1, -1, -1};
        if (mesh_quad(m, smp.n, smp.key[s], static_cast<int>(p % 3ull), s, q) == 0)
            for (int k = 0; k < 4; ++k) v[k] = vid[q[k]];
        int32_t* dst = faces + 6ull * pos;
        if (v[0] < 0 || v[1] < 0 || v[2] < 0 || v[3] < 0) {
            lane.err |= 16u;
        } else if (cflag[s] & kMeshSampleInside) {
            dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2];
            dst[3] = v[0]; dst[4] = v[2]; dst[5] = v[3];
        } else {
            dst[0] = v[0]; dst[1] = v[3]; dst[2] = v[2];
            dst[3] = v[0]; dst[4] = v[2]; dst[5] = v[1];
        }
    }
};

hipError_t launch_mesh_keys(unsigned long long ne, const unsigned long long* vox, unsigned long long nv,
                            const unsigned long long* vslot, VoxTable t, unsigned long long* ekey,
                            unsigned long long* words, hipStream_t s) {
    k_mesh_keys<<<clean_blocks(ne), 256, 0, s>>>(ne, vox, nv, vslot, t, ekey, words);
    return hipGetLastError();
}

hipError_t launch_mesh_insert(unsigned long long p0, int n, const unsigned long long* ekey, MeshTable m,
                              unsigned long long* words, hipStream_t s) {
    k_mesh_insert<<<static_cast<unsigned>(cdiv(n, 256)), 256, 0, s>>>(p0, n, ekey, m, words);
    return hipGetLastError();
}

hipError_t launch_mesh_stats(MeshTable m, unsigned long long* words, hipStream_t s) {
    const unsigned long long blocks = std::min<unsigned long long>((m.slots + 255ull) / 256ull, 4096ull);
    k_mesh_stats<<<static_cast<unsigned>(blocks), 256, 0, s>>>(m, words);
    return hipGetLastError();
}

hipError_t launch_mesh_number(unsigned long long p0, int n, const unsigned long long* ekey, MeshTable m, Compaction c,
                              MeshSamples out, unsigned long long* words, hipStream_t s) {
    return compact_segment(MeshNumber{{}, ekey, m, out, words}, p0, n, c, s);
}

hipError_t launch_mesh_tsdf(int model, const DevCam* cams, const FuseView* views, const int* list, int n_list,
                            MeshSamples smp, VoxGrid g, float trunc, hipStream_t s) {
    const int chunks = cdiv(n_list, kVisChunk);
    const dim3 grd(clean_blocks(smp.n), static_cast<unsigned>(chunks));
    const float k = 1024.0f / trunc;
    if (chunks > 1) {
        const hipError_t e = hipMemsetAsync(smp.tsdf, 0, sizeof(int32_t) * 2ull * smp.n, s);
        if (e != hipSuccess) return e;
        if (model == kSphere) k_mesh_tsdf<kSphere, true><<<grd, 256, 0, s>>>(cams, views, list, n_list, smp, g, trunc, k);
        else k_mesh_tsdf<kPinhole, true><<<grd, 256, 0, s>>>(cams, views, list, n_list, smp, g, trunc, k);
    } else {
        if (model == kSphere) k_mesh_tsdf<kSphere, false><<<grd, 256, 0, s>>>(cams, views, list, n_list, smp, g, trunc, k);
        else k_mesh_tsdf<kPinhole, false><<<grd, 256, 0, s>>>(cams, views, list, n_list, smp, g, trunc, k);
    }
    return hipGetLastError();
}

hipError_t launch_mesh_cubes(MeshSamples smp, MeshTable m, int min_weight, uint8_t* cflag, uint8_t* fbits,
                             unsigned long long* words, hipStream_t s) {
    k_mesh_cubes<<<clean_blocks(smp.n), 256, 0, s>>>(smp, m, min_weight, cflag, words);
    k_mesh_pairs<<<clean_blocks(smp.n), 256, 0, s>>>(smp, m, cflag, fbits, words);
    return hipGetLastError();
}

hipError_t launch_mesh_vertices(unsigned long long i0, int n, MeshSamples smp, MeshTable m, VoxGrid g, const uint8_t* cflag,
                                const float* src_pts, Compaction c, float* verts, int32_t* vid, unsigned long long* words,
                                hipStream_t s) {
    return compact_segment(MeshVertices{{}, smp, m, g, cflag, src_pts, verts, vid, words}, i0, n, c, s);
}

hipError_t launch_mesh_faces(unsigned long long p0, int n, MeshSamples smp, MeshTable m, const uint8_t* cflag,
                             const uint8_t* fbits, const int32_t* vid, Compaction c, int32_t* faces,
                             unsigned long long* words, hipStream_t s) {
    return compact_segment(MeshFaces{{}, smp, m, cflag, fbits, vid, faces, words}, p0, n, c, s);
}

// ------------------------------------------------------------------ the mesh rendered into a view
//
// acmmp_fusion_mesh_render (include/acmmp.h): every face is tested against the pixels of a conservative
// bound of its image, in float64 on float32 inputs, and a pixel's winner is the minimum of a 64-bit key (depth bits,
// face index) taken with atomicMin -- the same whatever order the faces arrive in.  The queue of large faces is the only
// racy thing, and nothing that is read back depends on its order.

__device__ __forceinline__ double render_dot(double ax, double ay, double az, double bx, double by, double bz) {
    return (ax * bx + ay * by) + az * bz;
}

// Step 2: the face's vertex indices and its camera-frame vertices T (A, B, C).  false = the face is skipped (a
// non-finite coordinate, pinhole: a vertex with T_z <= 0; an index outside the vertices, which no mesh result holds).
template <int MODEL>
__device__ __forceinline__ bool render_face(const DevCam& cam, const float* __restrict__ verts, unsigned long long nv,
                                            const int32_t* __restrict__ faces, unsigned f, int32_t idx[3], double T[9]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        idx[j] = faces[3ull * f + j];
        if (idx[j] < 0 || static_cast<unsigned long long>(idx[j]) >= nv) { ok = false; idx[j] = 0; }
    }
    if (!ok) return false;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float* X = verts + 9ull * static_cast<unsigned long long>(idx[j]);
        const double x = static_cast<double>(X[0]), y = static_cast<double>(X[1]), z = static_cast<double>(X[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double t = ((static_cast<double>(cam.R[3 * k]) * x + static_cast<double>(cam.R[3 * k + 1]) * y) +
                              static_cast<double>(cam.R[3 * k + 2]) * z) + static_cast<double>(cam.t[k]);
            T[3 * j + k] = t;
            ok = ok && fabs(t) < __builtin_inf();                     // false for an infinity and for a NaN
        }
        if (MODEL == kPinhole) ok = ok && T[3 * j + 2] > 0.0;
    }
    return ok;
}

// Step 3: the ray of pixel (c, r).
template <int MODEL>
__device__ __forceinline__ void render_ray(const DevCam& cam, int c, int r, double d[3]) {
    if (MODEL == kSphere) {
        const float3 p = pixel_to_dir(cam, c, r);
        d[0] = static_cast<double>(p.x); d[1] = static_cast<double>(p.y); d[2] = static_cast<double>(p.z);
    } else {
        d[0] = (static_cast<double>(c) - static_cast<double>(cam.K[2])) / static_cast<double>(cam.K[0]);
        d[1] = (static_cast<double>(r) - static_cast<double>(cam.K[5])) / static_cast<double>(cam.K[4]);
        d[2] = 1.0;
    }
}

// Steps 4 and 5: whether the ray d hits the face T, with the weights (u, v, w), their sum s and the depth md.
template <int MODEL>
__device__ __forceinline__ bool render_hit(const double T[9], const double d[3], double& u, double& v, double& w, double& s,
                                           float& md) {
    const double* A = T;
    const double* B = T + 3;
    const double* C = T + 6;
    u = render_dot(d[0], d[1], d[2], B[1] * C[2] - B[2] * C[1], B[2] * C[0] - B[0] * C[2], B[0] * C[1] - B[1] * C[0]);
    v = render_dot(d[0], d[1], d[2], C[1] * A[2] - C[2] * A[1], C[2] * A[0] - C[0] * A[2], C[0] * A[1] - C[1] * A[0]);
    w = render_dot(d[0], d[1], d[2], A[1] * B[2] - A[2] * B[1], A[2] * B[0] - A[0] * B[2], A[0] * B[1] - A[1] * B[0]);
    s = (u + v) + w;
    const bool inside = (s > 0.0 && u >= 0.0 && v >= 0.0 && w >= 0.0) || (s < 0.0 && u <= 0.0 && v <= 0.0 && w <= 0.0);
    if (!inside) return false;
    const double px = ((u * A[0] + v * B[0]) + w * C[0]) / s;
    const double py = ((u * A[1] + v * B[1]) + w * C[1]) / s;
    const double pz = ((u * A[2] + v * B[2]) + w * C[2]) / s;
    if (!(render_dot(px, py, pz, d[0], d[1], d[2]) > 0.0)) return false;
    md = static_cast<float>(MODEL == kSphere ? sqrt((px * px + py * py) + pz * pz) : pz);
    return md > 0.0f && md < __builtin_inff();
}

// Rows [r0, r0 + nr) and columns (c0 + j) mod W, j in [0, nc), of a face's candidate pixels.
struct RenderBound {
    int r0, nr, c0, nc;
};
struct RenderItem {
    unsigned face;
    RenderBound b;
};

// A conservative bound of the pixels whose ray can hit the face (DESIGN.md §8 argues each case).  The whole image for
// a face whose |det(A, B, C)| is not above 2^-30 |A||B||C| -- edge-on to the camera centre, or of no angular size: its
// weights may be rounding noise, and any pixel may hit.
template <int MODEL>
__device__ __forceinline__ RenderBound render_bound(const DevCam& cam, const double T[9]) {
    constexpr double kPi = 3.14159265358979323846, kPad = 0x1p-16, kGrow = 1.0 + 0x1p-20;
    const int W = cam.W, H = cam.H;
    const RenderBound all = {0, H, 0, W}, none = {0, 0, 0, 0};
    const double* A = T;
    const double* B = T + 3;
    const double* C = T + 6;
    double len[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) len[j] = sqrt(render_dot(T[3 * j], T[3 * j + 1], T[3 * j + 2], T[3 * j], T[3 * j + 1], T[3 * j + 2]));
    const double det = render_dot(A[0], A[1], A[2], B[1] * C[2] - B[2] * C[1], B[2] * C[0] - B[0] * C[2], B[0] * C[1] - B[1] * C[0]);
    if (!(fabs(det) > 0x1p-30 * ((len[0] * len[1]) * len[2]))) return all;
    if (MODEL == kPinhole) {
        // the box of the three projections, a pixel wider on every side; a vertex more than 2^10 focal lengths off
        // the axis, or a focal length that is not positive: the whole image
        const double fx = static_cast<double>(cam.K[0]), fy = static_cast<double>(cam.K[4]);
        if (!(fx > 0.0 && fy > 0.0)) return all;
        double x0 = __builtin_inf(), x1 = -__builtin_inf(), y0 = __builtin_inf(), y1 = -__builtin_inf();
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double* V = T + 3 * j;
            if (!(V[2] * 1024.0 > len[j])) return all;
            const double x = fx * (V[0] / V[2]) + static_cast<double>(cam.K[2]);
            const double y = fy * (V[1] / V[2]) + static_cast<double>(cam.K[5]);
            x0 = fmin(x0, x); x1 = fmax(x1, x); y0 = fmin(y0, y); y1 = fmax(y1, y);
        }
        const double cl = fmax(floor(x0) - 1.0, 0.0), ch = fmin(ceil(x1) + 1.0, static_cast<double>(W - 1));
        const double rl = fmax(floor(y0) - 1.0, 0.0), rh = fmin(ceil(y1) + 1.0, static_cast<double>(H - 1));
        if (!(cl <= ch && rl <= rh)) return none;
        return {static_cast<int>(rl), static_cast<int>(rh - rl) + 1, static_cast<int>(cl), static_cast<int>(ch - cl) + 1};
    } else {
        // rows must map to [-pi/2, pi/2] for the latitude band below to mean rows
        const double cx = static_cast<double>(cam.cx), cy = static_cast<double>(cam.cy);
        if (!(cy >= 0.5 * H - 1.0 && cy <= 0.5 * H)) return all;
        // the cap around the normalised mean of the vertex directions that contains the three of them
        double m[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) m[k] = (A[k] / len[0] + B[k] / len[1]) + C[k] / len[2];
        const double lm = sqrt(render_dot(m[0], m[1], m[2], m[0], m[1], m[2]));
        if (!(lm > 0x1p-10)) return all;
#pragma unroll
        for (int k = 0; k < 3; ++k) m[k] /= lm;
        double cosr = 1.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) cosr = fmin(cosr, render_dot(m[0], m[1], m[2], T[3 * j], T[3 * j + 1], T[3 * j + 2]) / len[j]);
        const double rho = acos(fmax(cosr, -1.0)) * kGrow + kPad;
        if (!(rho < 0.5 * kPi - kPad)) return all;                    // not convex: no bound
        const double phi = asin(fmin(fmax(m[1], -1.0), 1.0));         // the angle below the equator: row = cy + phi H / pi
        const double rpr = static_cast<double>(H) / kPi, cpr = static_cast<double>(W) / (2.0 * kPi);
        const double rl = fmax(floor(cy + (phi - rho) * rpr) - 1.0, 0.0);
        const double rh = fmin(ceil(cy + (phi + rho) * rpr) + 1.0, static_cast<double>(H - 1));
        if (!(rl <= rh)) return none;
        const int r0 = static_cast<int>(rl), nr = static_cast<int>(rh - rl) + 1;
        if (!(fabs(phi) + rho < 0.5 * kPi - kPad)) return {r0, nr, 0, W};          // the cap touches a pole
        const double dl = asin(fmin(sin(rho) / cos(phi), 1.0)) * kGrow + kPad;
        const double lam = atan2(m[0], m[2]);
        const double lo = floor(cx + (lam - dl) * cpr) - 1.0, hi = ceil(cx + (lam + dl) * cpr) + 1.0;
        const double n = (hi - lo) + 1.0;
        if (!(n < static_cast<double>(W))) return {r0, nr, 0, W};
        const long long c0 = ((static_cast<long long>(lo) % W) + W) % W;          // |lo| < W + |cx| + 2
        return {r0, nr, static_cast<int>(c0), static_cast<int>(n)};
    }
}

// Step 6 for one candidate pixel.
template <int MODEL>
__device__ __forceinline__ void render_candidate(const DevCam& cam, const double T[9], unsigned f, const RenderBound& b,
                                                 long long k, unsigned long long* __restrict__ keys) {
    const int r = b.r0 + static_cast<int>(k / b.nc);
    int c = b.c0 + static_cast<int>(k % b.nc);
    if (c >= cam.W) c -= cam.W;
    double d[3], u, v, w, s;
    float md;
    render_ray<MODEL>(cam, c, r, d);
    if (!render_hit<MODEL>(T, d, u, v, w, s, md)) return;
    const unsigned long long key = (static_cast<unsigned long long>(__float_as_uint(md)) << 32) | f;
    unsigned long long* dst = keys + static_cast<size_t>(r) * cam.W + c;
    // the key only decreases: a stale value costs an atomic and never skips one that would have won
    if (*reinterpret_cast<volatile unsigned long long*>(dst) > key) atomicMin(dst, key);
}

template <int MODEL>
__global__ __launch_bounds__(256) void k_render_setup(const DevCam cam, const float* __restrict__ verts, unsigned long long nv,
                                                      const int32_t* __restrict__ faces, unsigned nf, long long small_max,
                                                      unsigned long long* __restrict__ keys, RenderItem* __restrict__ queue,
                                                      unsigned long long* __restrict__ words) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    unsigned long long skipped = 0, small = 0, cand = 0;
    if (f < nf) {
        int32_t idx[3];
        double T[9];
        if (!render_face<MODEL>(cam, verts, nv, faces, f, idx, T)) {
            skipped = 1;
        } else {
            const RenderBound b = render_bound<MODEL>(cam, T);
            const long long n = static_cast<long long>(b.nr) * b.nc;
            cand = static_cast<unsigned long long>(n);
            if (n <= small_max) {
                small = 1;
                for (long long k = 0; k < n; ++k) render_candidate<MODEL>(cam, T, f, b, k, keys);
            } else {
                const unsigned long long q = atomicAdd(&words[kRenderLarge], 1ull);   // q < nf: one per face at most
                queue[q] = RenderItem{f, b};
            }
        }
    }
    wave_add(skipped, &words[kRenderSkipped]);
    wave_add(small, &words[kRenderSmall]);
    wave_add(cand, &words[kRenderCandidates]);
}

// One workgroup per queued face, its lanes striding over the face's candidates.
template <int MODEL>
__global__ __launch_bounds__(256) void k_render_large(const DevCam cam, const float* __restrict__ verts, unsigned long long nv,
                                                      const int32_t* __restrict__ faces, unsigned nf,
                                                      unsigned long long* __restrict__ keys, const RenderItem* __restrict__ queue,
                                                      const unsigned long long* __restrict__ words) {
    const unsigned long long n_large = words[kRenderLarge] < nf ? words[kRenderLarge] : nf;
    for (unsigned long long q = blockIdx.x; q < n_large; q += gridDim.x) {
        const RenderItem it = queue[q];
        int32_t idx[3];
        double T[9];
        if (it.face >= nf || !render_face<MODEL>(cam, verts, nv, faces, it.face, idx, T)) continue;
        const long long n = static_cast<long long>(it.b.nr) * it.b.nc;
        for (long long k = threadIdx.x; k < n; k += 256) render_candidate<MODEL>(cam, T, it.face, it.b, k, keys);
    }
}

// *word += the number of lanes of the wave with `on`, one atomic per wave.  Every lane of the wave calls it.
__device__ __forceinline__ void wave_count(bool on, unsigned long long* word) {
    const unsigned long long m = __ballot(on);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(word, static_cast<unsigned long long>(__popcll(m)));
}

// Steps 7 and 8, one lane per pixel: the winner's hit again, the four maps, the counts.
template <int MODEL>
__global__ __launch_bounds__(256) void k_render_resolve(const DevCam cam, const float* __restrict__ verts, unsigned long long nv,
                                                        const int32_t* __restrict__ faces, unsigned nf,
                                                        const unsigned long long* __restrict__ keys, const float* __restrict__ raw,
                                                        float rel_tol, float* __restrict__ depth, int32_t* __restrict__ face,
                                                        float* __restrict__ normal, float* __restrict__ colour,
                                                        unsigned long long* __restrict__ words) {
    const long long P = static_cast<long long>(cam.W) * cam.H;
    const long long p = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    int cls = -1;
    bool back = false;
    if (p < P) {
        const unsigned long long key = keys[p];
        float md = 0.0f, out[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        int32_t win = -1;
        if (key != ~0ull) {
            const unsigned f = static_cast<unsigned>(key & 0xffffffffull);
            int32_t idx[3];
            double T[9], d[3], u, v, w, s;
            float again;
            render_ray<MODEL>(cam, static_cast<int>(p % cam.W), static_cast<int>(p / cam.W), d);
            if (f < nf && render_face<MODEL>(cam, verts, nv, faces, f, idx, T) && render_hit<MODEL>(T, d, u, v, w, s, again)) {
                win = static_cast<int32_t>(f);
                md = __uint_as_float(static_cast<unsigned>(key >> 32));
                back = s > 0.0;
                const float* a = verts + 9ull * static_cast<unsigned long long>(idx[0]);
                const float* b = verts + 9ull * static_cast<unsigned long long>(idx[1]);
                const float* c = verts + 9ull * static_cast<unsigned long long>(idx[2]);
                double n[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    n[k] = ((u * static_cast<double>(a[3 + k]) + v * static_cast<double>(b[3 + k])) + w * static_cast<double>(c[3 + k])) / s;
                    out[3 + k] = static_cast<float>(((u * static_cast<double>(a[6 + k]) + v * static_cast<double>(b[6 + k])) +
                                                     w * static_cast<double>(c[6 + k])) / s);
                }
                const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
#pragma unroll
                for (int k = 0; k < 3; ++k) out[k] = len > 0.0 ? static_cast<float>(n[k] / len) : 0.0f;
            }
        }
        depth[p] = md;
        face[p] = win;
#pragma unroll
        for (int k = 0; k < 3; ++k) { normal[3 * p + k] = out[k]; colour[3 * p + k] = out[3 + k]; }
        if (raw) {
            const float sd = raw[p];
            const bool have_raw = sd > 0.0f && sd < __builtin_inff(), have_mesh = win >= 0;
            if (have_raw && have_mesh) {
                const float t = rel_tol * sd;
                cls = fabsf(md - sd) <= t ? 0 : md < sd ? 1 : 2;
            } else {
                cls = have_mesh ? 3 : have_raw ? 4 : 5;
            }
        } else {
            back = false;
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) wave_count(cls == k, &words[kRenderCounts + k]);
    wave_count(back, &words[kRenderCounts + 6]);
}

hipError_t launch_render(int model, const DevCam& cam, const float* verts, unsigned long long nv, const int32_t* faces,
                         unsigned nf, long long small_max, unsigned long long* keys, void* queue, const float* raw,
                         float rel_tol, float* depth, int32_t* face, float* normal, float* colour, unsigned long long* words,
                         hipStream_t s) {
    const long long P = static_cast<long long>(cam.W) * cam.H;
    const unsigned fb = static_cast<unsigned>((static_cast<unsigned long long>(nf) + 255ull) / 256ull);
    const unsigned lb = std::min(nf, 4096u), pb = static_cast<unsigned>((P + 255) / 256);
    RenderItem* q = static_cast<RenderItem*>(queue);
    static_assert(sizeof(RenderItem) == kRenderItemBytes, "fusion.cpp sizes the queue");
    if (nf > 0) {
        if (model == kSphere) {
            k_render_setup<kSphere><<<fb, 256, 0, s>>>(cam, verts, nv, faces, nf, small_max, keys, q, words);
            k_render_large<kSphere><<<lb, 256, 0, s>>>(cam, verts, nv, faces, nf, keys, q, words);
        } else {
            k_render_setup<kPinhole><<<fb, 256, 0, s>>>(cam, verts, nv, faces, nf, small_max, keys, q, words);
            k_render_large<kPinhole><<<lb, 256, 0, s>>>(cam, verts, nv, faces, nf, keys, q, words);
        }
    }
    if (model == kSphere)
        k_render_resolve<kSphere><<<pb, 256, 0, s>>>(cam, verts, nv, faces, nf, keys, raw, rel_tol, depth, face, normal, colour, words);
    else
        k_render_resolve<kPinhole><<<pb, 256, 0, s>>>(cam, verts, nv, faces, nf, keys, raw, rel_tol, depth, face, normal, colour, words);
    return hipGetLastError();
}

// ------------------------------------------------------------------ nearest-neighbour cloud distances
//
// acmmp_fusion_cloud_distance (include/acmmp.h).  The result is defined over all pairs; the grid only
// decides which pairs are looked at, and a pair is left out only where the bounds of DESIGN.md §8 prove that it loses
// or is unmatched.  The winner is the minimum of a 64-bit (distance bits, index) key, so neither the order of a cell's
// list nor the order of the cells matters.  Cells are computed in float64, where the rounding of the index is below
// 2^-30 of a cell; the pair distance is the float32 expression of the definition.

__device__ __forceinline__ bool dist_load(const DistCloud& c, unsigned long long i, float v[3]) {
    const float* p = c.p + static_cast<unsigned long long>(c.stride) * i;
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
    if (c.xf) {                                      // the cloud transform of acmmp.h: float64, rounded once
        const double x = static_cast<double>(v[0]), y = static_cast<double>(v[1]), z = static_cast<double>(v[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            v[k] = static_cast<float>(((c.M[4 * k] * x + c.M[4 * k + 1] * y) + c.M[4 * k + 2] * z) + c.M[4 * k + 3]);
    }
    if (c.cls && c.cls[i]) return false;             // outside its side's region (k_region_classify): as if not finite
    return !vox_nonfinite(v[0]) && !vox_nonfinite(v[1]) && !vox_nonfinite(v[2]);
}

// The cell of coordinate x on axis a, clamped to the grid; frac = the position inside the cell, 0 with `clamped` set
// for a coordinate outside the grid (targets never are: the host sizes the grid from their bounding box).
__device__ __forceinline__ int dist_axis(const DistGrid& g, int a, float x, double& frac, bool& clamped) {
    const double u = (static_cast<double>(x) - g.o[a]) * g.inv;
    const double c = floor(u);
    frac = 0.0;
    if (!(c >= 0.0)) { clamped = true; return 0; }
    if (c > static_cast<double>(g.cmax[a])) { clamped = true; return g.cmax[a]; }
    frac = u - c;
    return static_cast<int>(c);
}

__device__ __forceinline__ unsigned long long dist_key(int cx, int cy, int cz) {
    return static_cast<unsigned long long>(cx) | static_cast<unsigned long long>(cy) << 21 |
           static_cast<unsigned long long>(cz) << 42;
}

__device__ __forceinline__ unsigned long long dist_cell_key(const DistGrid& g, const float v[3]) {
    double fr;
    bool cl = false;
    const int cx = dist_axis(g, 0, v[0], fr, cl), cy = dist_axis(g, 1, v[1], fr, cl), cz = dist_axis(g, 2, v[2], fr, cl);
    return dist_key(cx, cy, cz);
}

__global__ __launch_bounds__(256) void k_dist_bounds(const DistCloud t, unsigned long long* __restrict__ words) {
    const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    uint32_t m[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    bool ok = false;
    if (i < t.n) {
        float v[3];
        ok = dist_load(t, i, v);
        if (ok) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { m[a] = vox_ordered(v[a]); m[3 + a] = vox_ordered(-v[a]); }
        }
    }
    uint32_t* mn = reinterpret_cast<uint32_t*>(words + kDistMin);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m[a] = min(m[a], static_cast<uint32_t>(__shfl_xor(static_cast<int>(m[a]), d)));
        if ((threadIdx.x & 63) == 0 && m[a] != 0xffffffffu) atomicMin(&mn[a], m[a]);
    }
    wave_count(ok, &words[kDistValidTargets]);
}

__global__ __launch_bounds__(256) void k_dist_insert(const DistCloud t, const DistGrid g, const DistTable fine, const DistGrid cg,
                                                     const DistTable coarse, unsigned long long* __restrict__ words) {
    const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    unsigned err = 0u;
    if (i < t.n) {
        float v[3];
        if (dist_load(t, i, v)) {
            unsigned long long s;
            if (table_claim(fine, dist_cell_key(g, v), s)) atomicAdd(&fine.cnt[s], 1u);
            else err = 1u;
            if (coarse.keys && !table_claim(coarse, dist_cell_key(cg, v), s)) err = 1u;
        }
    }
    block_or(err, &words[kDistErr]);
}

// Every occupied slot takes a run of the list as long as its count: an inclusive scan of the counts within the wave,
// one atomic add of the wave's total to the cursor word.  Which run a cell gets depends on the order the waves arrive
// in, and nothing a reader can see depends on it.  cnt becomes the cell's write cursor.
__global__ __launch_bounds__(256) void k_dist_starts(const DistTable t, unsigned long long* __restrict__ words) {
    const int lane = threadIdx.x & 63;
    unsigned long long occ = 0, longest = 0;
    for (unsigned long long base = static_cast<unsigned long long>(blockIdx.x) * 256; base < t.slots;
         base += static_cast<unsigned long long>(gridDim.x) * 256) {
        const unsigned long long s = base + threadIdx.x;
        const uint32_t c = (s < t.slots && t.keys[s] != kVoxEmpty) ? t.cnt[s] : 0u;
        uint32_t inc = c;
#pragma unroll
        for (int d = 1; d <= 32; d <<= 1) {
            const uint32_t y = static_cast<uint32_t>(__shfl_up(static_cast<int>(inc), d));
            if (lane >= d) inc += y;
        }
        const uint32_t tot = static_cast<uint32_t>(__shfl(static_cast<int>(inc), 63));
        unsigned long long b = 0;
        if (lane == 0 && tot) b = atomicAdd(&words[kDistCursor], static_cast<unsigned long long>(tot));
        b = __shfl(b, 0);
        if (c) {
            const uint32_t st = static_cast<uint32_t>(b) + inc - c;
            t.start[s] = st;
            t.cnt[s] = st;
            ++occ;
            longest = max(longest, static_cast<unsigned long long>(c));
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        occ += __shfl_xor(occ, d);
        longest = max(longest, static_cast<unsigned long long>(__shfl_xor(longest, d)));
    }
    if (lane == 0) {
        if (occ) atomicAdd(&words[kDistOccupied], occ);
        if (longest) atomicMax(&words[kDistMaxList], longest);
    }
}

__global__ __launch_bounds__(256) void k_dist_scatter(const DistCloud t, const DistGrid g, const DistTable fine,
                                                      float4* __restrict__ list, unsigned long long* __restrict__ words) {
    const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    unsigned err = 0u;
    if (i < t.n) {
        float v[3];
        if (dist_load(t, i, v)) {
            unsigned long long s;
            if (table_find(fine, dist_cell_key(g, v), s) == 0) {
                const uint32_t pos = atomicAdd(&fine.cnt[s], 1u);
                if (pos < t.n) list[pos] = make_float4(v[0], v[1], v[2], __uint_as_float(static_cast<uint32_t>(i)));
                else err = 2u;
            } else {
                err = 2u;
            }
        }
    }
    block_or(err, &words[kDistErr]);
}

// A lower bound of the float32 d2 of any pair whose points lie at least L apart on one axis; 0 where
// nothing can be said.
__device__ __forceinline__ double dist_floor2(double L) {
    const double s = L * L;
    return (L > 0.0 && s >= 0x1p-120) ? s * (1.0 - 0x1p-20) : 0.0;
}

// One cell of the fine grid against the query: best = min(best, key) over its list.
__device__ __forceinline__ void dist_visit(const DistTable& fine, const float4* __restrict__ list, const float v[3], int cx,
                                           int cy, int cz, unsigned long long& best, unsigned& err) {
    unsigned long long s;
    const int r = table_find(fine, dist_key(cx, cy, cz), s);
    if (r == 2) err |= 4u;
    if (r != 0) return;
    const uint32_t a = fine.start[s], b = fine.cnt[s];
    for (uint32_t pos = a; pos < b; ++pos) {
        const float4 t = list[pos];
        const float dx = v[0] - t.x, dy = v[1] - t.y, dz = v[2] - t.z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const unsigned long long key =
            static_cast<unsigned long long>(__float_as_uint(d2)) << 32 | static_cast<unsigned long long>(__float_as_uint(t.w));
        best = min(best, key);
    }
}

// The ring walk around a query v whose box reject has let it through: visit(x, y, z, best) for every cell of the rings
// 0, 1, ... of Chebyshev radius r, clipped to the grid, until the stop rule of DESIGN.md §8 fires.  The rule needs of
// `visit` only that what it has not been shown after rings 0 .. r lies at least (r + m - 2^-20) h from v on one axis.
template <class Visit>
__device__ __forceinline__ void dist_walk(const float v[3], const DistGrid& g, double m2d, unsigned long long& best,
                                          unsigned long long& rings, Visit visit) {
    int c[3], rmax = 0;
    double mfrac = 0.5;
    bool clamped = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double fr;
        c[a] = dist_axis(g, a, v[a], fr, clamped);
        mfrac = fmin(mfrac, fmin(fr, 1.0 - fr));
        rmax = max(rmax, max(c[a], g.cmax[a] - c[a]));
    }
    if (clamped) mfrac = 0.0;
    for (int r = 0;; ++r) {
        rings = static_cast<unsigned long long>(r);
        // the shell of Chebyshev radius r, clipped to the grid
        const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, g.cmax[0]);
        const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.cmax[1]);
        const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.cmax[2]);
        for (int z = z0; z <= z1; ++z) {
            const bool zface = z == c[2] - r || z == c[2] + r;
            for (int y = y0; y <= y1; ++y) {
                if (zface || y == c[1] - r || y == c[1] + r) {
                    for (int x = x0; x <= x1; ++x) visit(x, y, z, best);
                } else {
                    if (c[0] - r >= 0) visit(c[0] - r, y, z, best);
                    if (c[0] + r <= g.cmax[0]) visit(c[0] + r, y, z, best);
                }
            }
        }
        if (r >= rmax) break;                       // every cell of the grid has been searched
        // a target not yet searched lies more than L from the query on one axis
        const double lb = dist_floor2((static_cast<double>(r) + mfrac - 0x1p-20) * g.cell);
        if (lb > m2d) break;                        // it is unmatched
        if (best != ~0ull && static_cast<double>(__uint_as_float(static_cast<uint32_t>(best >> 32))) < lb) break;   // it loses
    }
}

// Steps 2 and 3 for one valid query v: the smallest (bits(d2) << 32 | j) key over the valid targets that the bounds of
// DESIGN.md §8 cannot rule out, ~0 with none.  Shared by k_dist_query and k_align_iter.  rings = the largest ring searched.
__device__ __forceinline__ unsigned long long dist_nearest(const float v[3], const DistGrid& g, const DistTable& fine,
                                                           const DistGrid& cg, const DistTable& coarse,
                                                           const float4* __restrict__ list, const DistQuery& p,
                                                           unsigned long long& rings, unsigned& err) {
    const double m2d = static_cast<double>(p.m2);
    unsigned long long best = ~0ull;
    // the bounding box of the targets: a query further from it than max_dist on one axis is unmatched
    double gap = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
        gap = fmax(gap, fmax(p.lo[a] - static_cast<double>(v[a]), static_cast<double>(v[a]) - p.hi[a]));
    bool search = !(dist_floor2(gap) > m2d);
    // the coarse level: cells wider than max_dist; with none of the 27 around the query occupied it is unmatched
    if (search && coarse.keys) {
        double fr;
        bool cl = false;
        int c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = dist_axis(cg, a, v[a], fr, cl);
        bool any = false;
        for (int z = max(c[2] - 1, 0); z <= min(c[2] + 1, cg.cmax[2]) && !any; ++z)
            for (int y = max(c[1] - 1, 0); y <= min(c[1] + 1, cg.cmax[1]) && !any; ++y)
                for (int x = max(c[0] - 1, 0); x <= min(c[0] + 1, cg.cmax[0]) && !any; ++x) {
                    unsigned long long s;
                    const int r = table_find(coarse, dist_key(x, y, z), s);
                    if (r == 2) err |= 4u;
                    any = r != 1;
                }
        search = any;
    }
    if (search)
        dist_walk(v, g, m2d, best, rings, [&](int x, int y, int z, unsigned long long& b) {
            dist_visit(fine, list, v, x, y, z, b, err);
        });
    return best;
}

// The summary of step 5 from one lane per query: integers only, reduced per wave or per workgroup (hist: 256 words of
// LDS, zero, with a barrier behind them) before any global atomic.  Every lane of the workgroup calls it.  It repeats
// k_dist_query's tail, which stays inline there: called from that kernel it costs nine scalar registers.
__device__ __forceinline__ void dist_summarise(bool valid, bool matched, float d2, unsigned long long rings, unsigned err,
                                               const DistQuery& p, unsigned* hist, unsigned long long* __restrict__ words) {
    unsigned long long* sm = words + kDistSummary;
    long long qv = 0;
    if (matched) {
        qv = static_cast<long long>(rint(sqrt(static_cast<double>(d2)) * p.k));
        const long long b = qv >> 12;
        atomicAdd(&hist[b < 255 ? (b < 0 ? 0 : b) : 255], 1u);
    }
    wave_count(valid, &sm[1]);
    wave_count(matched, &sm[2]);
    wave_add(static_cast<unsigned long long>(qv), &sm[3]);
#pragma unroll
    for (int k = 0; k < 8; ++k) wave_count(matched && k < p.n_tau && d2 <= p.tau2[k], &sm[4 + k]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) rings = max(rings, static_cast<unsigned long long>(__shfl_xor(rings, d)));
    if ((threadIdx.x & 63) == 0 && rings) atomicMax(&words[kDistRings], rings);
    block_or(err, &words[kDistErr]);
    if (hist[threadIdx.x]) atomicAdd(&sm[12 + threadIdx.x], static_cast<unsigned long long>(hist[threadIdx.x]));
}

__global__ __launch_bounds__(256) void k_dist_query(const DistCloud q, const DistGrid g, const DistTable fine, const DistGrid cg,
                                                    const DistTable coarse, const float4* __restrict__ list, const DistQuery p,
                                                    float* __restrict__ d2out, int32_t* __restrict__ nnout,
                                                    unsigned long long* __restrict__ words) {
    __shared__ unsigned hist[256];
    hist[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    bool valid = false, matched = false;
    float d2 = __builtin_inff();
    int32_t nn = -1;
    unsigned long long rings = 0;
    unsigned err = 0u;
    if (i < q.n) {
        float v[3];
        valid = dist_load(q, i, v);
        if (valid && p.have_targets) {
            const unsigned long long best = dist_nearest(v, g, fine, cg, coarse, list, p, rings, err);
            if (best != ~0ull) {
                const float w = __uint_as_float(static_cast<uint32_t>(best >> 32));
                if (w <= p.m2) {
                    matched = true;
                    d2 = w;
                    nn = static_cast<int32_t>(static_cast<uint32_t>(best & 0xffffffffull));
                }
            }
        }
        d2out[i] = d2;
        nnout[i] = nn;
    }
    // the summary: integers only, reduced per wave or per workgroup first
    unsigned long long* sm = words + kDistSummary;
    long long qv = 0;
    if (matched) {
        qv = static_cast<long long>(rint(sqrt(static_cast<double>(d2)) * p.k));
        const long long b = qv >> 12;
        atomicAdd(&hist[b < 255 ? (b < 0 ? 0 : b) : 255], 1u);
    }
    wave_count(valid, &sm[1]);
    wave_count(matched, &sm[2]);
    wave_add(static_cast<unsigned long long>(qv), &sm[3]);
#pragma unroll
    for (int k = 0; k < 8; ++k) wave_count(matched && k < p.n_tau && d2 <= p.tau2[k], &sm[4 + k]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) rings = max(rings, static_cast<unsigned long long>(__shfl_xor(rings, d)));
    if ((threadIdx.x & 63) == 0 && rings) atomicMax(&words[kDistRings], rings);
    block_or(err, &words[kDistErr]);
    if (hist[threadIdx.x]) atomicAdd(&sm[12 + threadIdx.x], static_cast<unsigned long long>(hist[threadIdx.x]));
}

// One iteration of acmmp_fusion_cloud_align (include/acmmp.h): lane i takes the data point i * stride under q's
// transform, searches as k_dist_query does, quantises the matched pair and forms the kAlignWords words of the record;
// they are summed over the wave with shuffles, over the workgroup through LDS, and 32 lanes add one word each to
// rec[0 .. 32) (n_query is the host's).  Only integers are summed; nothing is written per query.
__global__ __launch_bounds__(256) void k_align_iter(const DistCloud q, unsigned long long stride, unsigned long long nq,
                                                    const DistCloud t, const DistGrid g, const DistTable fine, const DistGrid cg,
                                                    const DistTable coarse, const float4* __restrict__ list, const DistQuery p,
                                                    double kq, unsigned long long* __restrict__ words,
                                                    unsigned long long* __restrict__ rec) {
    __shared__ unsigned long long part[4][kAlignWords];
    const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    long long m[kAlignWords];
#pragma unroll
    for (int k = 0; k < kAlignWords; ++k) m[k] = 0;
    unsigned long long rings = 0;
    unsigned err = 0u;
    if (i < nq) {
        float v[3];
        if (dist_load(q, i * stride, v)) {
            m[ACMMP_ALIGN_RECORD_N_VALID] = 1;
            unsigned long long best = ~0ull;
            if (p.have_targets) best = dist_nearest(v, g, fine, cg, coarse, list, p, rings, err);
            const float d2 = __uint_as_float(static_cast<uint32_t>(best >> 32));
            const unsigned long long j = best & 0xffffffffull;
            if (best != ~0ull && d2 <= p.m2) {
                float tv[3];
                if (j >= t.n || !dist_load(t, j, tv)) {
                    err |= 8u;
                } else {
                    m[ACMMP_ALIGN_RECORD_N_MATCHED] = 1;
                    m[ACMMP_ALIGN_RECORD_SUM_Q] = static_cast<long long>(rint(sqrt(static_cast<double>(d2)) * p.k));
                    double P[3], Q[3];
                    bool in = true;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        P[a] = rint((static_cast<double>(v[a]) - p.lo[a]) * kq);
                        Q[a] = rint((static_cast<double>(tv[a]) - p.lo[a]) * kq);
                        in = in && fabs(P[a]) < 0x1p30 && fabs(Q[a]) < 0x1p30;
                    }
                    if (!in) {
                        m[ACMMP_ALIGN_RECORD_N_OUT_OF_RANGE] = 1;
                    } else {
                        long long Pi[3], Qi[3];
#pragma unroll
                        for (int a = 0; a < 3; ++a) { Pi[a] = static_cast<long long>(P[a]); Qi[a] = static_cast<long long>(Q[a]); }
                        m[ACMMP_ALIGN_RECORD_N] = 1;
#pragma unroll
                        for (int a = 0; a < 3; ++a) {
                            m[ACMMP_ALIGN_RECORD_SUM_P + a] = Pi[a];
                            m[ACMMP_ALIGN_RECORD_SUM_Q3 + a] = Qi[a];
#pragma unroll
                            for (int b = 0; b < 3; ++b) {
                                const long long w = Pi[a] * Qi[b];
                                m[ACMMP_ALIGN_RECORD_PQ + 2 * (3 * a + b)] = w >> 32;
                                m[ACMMP_ALIGN_RECORD_PQ + 2 * (3 * a + b) + 1] = w & 0xffffffffll;
                            }
                        }
                        const long long w = Pi[0] * Pi[0] + Pi[1] * Pi[1] + Pi[2] * Pi[2];
                        m[ACMMP_ALIGN_RECORD_PP] = w >> 32;
                        m[ACMMP_ALIGN_RECORD_PP + 1] = w & 0xffffffffll;
                    }
                }
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kAlignWords; ++k) {
        unsigned long long x = static_cast<unsigned long long>(m[k]);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
        if (lane == 0) part[wave][k] = x;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) rings = max(rings, static_cast<unsigned long long>(__shfl_xor(rings, d)));
    if (lane == 0 && rings) atomicMax(&words[kDistRings], rings);
    __syncthreads();
    if (threadIdx.x < kAlignWords) {
        const unsigned long long x = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
        if (x) atomicAdd(&rec[threadIdx.x], x);
    }
    block_or(err, &words[kDistErr]);
}

// The sum of x over the wave to part[k] (lane 0 writes).  Every lane of the wave calls it.
__device__ __forceinline__ void align_wave_word(unsigned long long x, unsigned long long* part, int k) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    if ((threadIdx.x & 63) == 0) part[k] = x;
}

// The split sums of the product w over the wave: part[k] = the sum of w >> 32, part[k + 1] = the sum of w & 0xffffffff.
__device__ __forceinline__ void align_wave_split(long long w, unsigned long long* part, int k) {
    align_wave_word(static_cast<unsigned long long>(w >> 32), part, k);
    align_wave_word(static_cast<unsigned long long>(w & 0xffffffffll), part, k + 1);
}

// One iteration of acmmp_fusion_cloud_align_plane (include/acmmp.h): k_align_iter's lane mapping, search and reduction,
// with the point-to-plane row.  After the search a lane holds its flags, sum_q, Q and nine small integers -- the lever
// L, the quantised normal Nn and D = P - Q, all zero for a lane that contributes no pair -- and every word is formed from
// them just before its reduction, so that the 70 words are never live together.  Only integers are summed; nothing is
// written per query.
__global__ __launch_bounds__(256) void k_align_plane_iter(const DistCloud q, unsigned long long stride, unsigned long long nq,
                                                          const DistCloud t, const DistGrid g, const DistTable fine,
                                                          const DistGrid cg, const DistTable coarse,
                                                          const float4* __restrict__ list, const DistQuery p, double kq,
                                                          const AlignPivot pivot, unsigned long long* __restrict__ words,
                                                          unsigned long long* __restrict__ rec) {
    __shared__ unsigned long long part[4][kAlignPlaneWords];
    const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    bool valid = false, matched = false, out_of_range = false, no_normal = false, pair = false;
    long long sum_q = 0, Qi[3] = {0, 0, 0};
    int L[3] = {0, 0, 0}, Nn[3] = {0, 0, 0}, D[3] = {0, 0, 0};
    unsigned long long rings = 0;
    unsigned err = 0u;
    if (i < nq) {
        float v[3];
        if (dist_load(q, i * stride, v)) {
            valid = true;
            unsigned long long best = ~0ull;
            if (p.have_targets) best = dist_nearest(v, g, fine, cg, coarse, list, p, rings, err);
            const float d2 = __uint_as_float(static_cast<uint32_t>(best >> 32));
            const unsigned long long j = best & 0xffffffffull;
            if (best != ~0ull && d2 <= p.m2) {
                float tv[3];
                if (j >= t.n || !dist_load(t, j, tv)) {
                    err |= 8u;
                } else {
                    matched = true;
                    sum_q = static_cast<long long>(rint(sqrt(static_cast<double>(d2)) * p.k));
                    double P[3], Q[3];
                    bool in = true;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        P[a] = rint((static_cast<double>(v[a]) - p.lo[a]) * kq);
                        Q[a] = rint((static_cast<double>(tv[a]) - p.lo[a]) * kq);
                        in = in && fabs(P[a]) < 0x1p30 && fabs(Q[a]) < 0x1p30;
                    }
                    long long lever[3] = {0, 0, 0};
                    if (in) {
#pragma unroll
                        for (int a = 0; a < 3; ++a) {
                            lever[a] = static_cast<long long>(Q[a]) - pivot.g[a];
                            in = in && lever[a] > -(1ll << 30) && lever[a] < (1ll << 30);
                        }
                    }
                    if (!in) {
                        out_of_range = true;
                    } else {
                        // the data point's own normal under the linear part of the transform, float64, no contraction
                        const float* np = q.p + static_cast<unsigned long long>(q.stride) * (i * stride) + 3;
                        const float nf[3] = {np[0], np[1], np[2]};
                        const double nx = static_cast<double>(nf[0]), ny = static_cast<double>(nf[1]), nz = static_cast<double>(nf[2]);
                        double u[3];
#pragma unroll
                        for (int a = 0; a < 3; ++a) u[a] = (q.M[4 * a] * nx + q.M[4 * a + 1] * ny) + q.M[4 * a + 2] * nz;
                        const double l2 = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2];
                        const bool usable = !vox_nonfinite(nf[0]) && !vox_nonfinite(nf[1]) && !vox_nonfinite(nf[2]) &&
                                            l2 > 0.0 && l2 < __builtin_inf();
                        if (!usable) {
                            no_normal = true;
                        } else {
                            pair = true;
                            const double len = sqrt(l2);
#pragma unroll
                            for (int a = 0; a < 3; ++a) {
                                Qi[a] = static_cast<long long>(Q[a]);
                                L[a] = static_cast<int>(lever[a] >> 12);
                                Nn[a] = static_cast<int>(rint(u[a] / len * 4096.0));
                                D[a] = static_cast<int>(static_cast<long long>(P[a]) - Qi[a]);
                            }
                        }
                    }
                }
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long* my = part[wave];
    const unsigned long long counts[5] = {__ballot(valid), __ballot(matched), __ballot(out_of_range), __ballot(no_normal),
                                          __ballot(pair)};
    if (lane == 0) {
        my[ACMMP_ALIGN_PLANE_RECORD_N_QUERY] = 0ull;
        my[ACMMP_ALIGN_PLANE_RECORD_N_VALID] = static_cast<unsigned long long>(__popcll(counts[0]));
        my[ACMMP_ALIGN_PLANE_RECORD_N_MATCHED] = static_cast<unsigned long long>(__popcll(counts[1]));
        my[ACMMP_ALIGN_PLANE_RECORD_N_OUT_OF_RANGE] = static_cast<unsigned long long>(__popcll(counts[2]));
        my[ACMMP_ALIGN_PLANE_RECORD_N_NO_NORMAL] = static_cast<unsigned long long>(__popcll(counts[3]));
        my[ACMMP_ALIGN_PLANE_RECORD_N] = static_cast<unsigned long long>(__popcll(counts[4]));
#pragma unroll
        for (int k = ACMMP_ALIGN_PLANE_RECORD_PIVOT; k < ACMMP_ALIGN_PLANE_RECORD_CC; ++k) my[k] = 0ull;   // the host's, and the 0
    }
    align_wave_word(static_cast<unsigned long long>(sum_q), my, ACMMP_ALIGN_PLANE_RECORD_SUM_Q);
#pragma unroll
    for (int a = 0; a < 3; ++a) align_wave_word(static_cast<unsigned long long>(Qi[a]), my, ACMMP_ALIGN_PLANE_RECORD_SUM_Q3 + a);
    // the row c = (L x Nn, Nn) and the residual r: |c_a| < 2^31, |r| < 2^31 (include/acmmp.h), so every product fits
    long long c[6];
    c[0] = static_cast<long long>(L[1]) * Nn[2] - static_cast<long long>(L[2]) * Nn[1];
    c[1] = static_cast<long long>(L[2]) * Nn[0] - static_cast<long long>(L[0]) * Nn[2];
    c[2] = static_cast<long long>(L[0]) * Nn[1] - static_cast<long long>(L[1]) * Nn[0];
    c[3] = Nn[0]; c[4] = Nn[1]; c[5] = Nn[2];
    const long long r = (static_cast<long long>(D[0]) * Nn[0] + static_cast<long long>(D[1]) * Nn[1]) + static_cast<long long>(D[2]) * Nn[2];
    int k = ACMMP_ALIGN_PLANE_RECORD_CC;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b, k += 2) align_wave_split(c[a] * c[b], my, k);
#pragma unroll
    for (int a = 0; a < 6; ++a) align_wave_split(c[a] * r, my, ACMMP_ALIGN_PLANE_RECORD_CR + 2 * a);
    align_wave_split(r * r, my, ACMMP_ALIGN_PLANE_RECORD_RR);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) rings = max(rings, static_cast<unsigned long long>(__shfl_xor(rings, d)));
    if (lane == 0 && rings) atomicMax(&words[kDistRings], rings);
    __syncthreads();
    if (threadIdx.x < kAlignPlaneWords) {
        const unsigned long long x = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
        if (x) atomicAdd(&rec[threadIdx.x], x);
    }
    block_or(err, &words[kDistErr]);
}

static unsigned dist_blocks(unsigned long long n) { return static_cast<unsigned>((n + 255ull) / 256ull); }

hipError_t launch_dist_bounds(DistCloud t, unsigned long long* words, hipStream_t s) {
    if (t.n == 0) return hipSuccess;
    k_dist_bounds<<<dist_blocks(t.n), 256, 0, s>>>(t, words);
    return hipGetLastError();
}

hipError_t launch_dist_insert(DistCloud t, DistGrid g, DistTable fine, DistGrid cg, DistTable coarse,
                              unsigned long long* words, hipStream_t s) {
    if (t.n == 0) return hipSuccess;
    k_dist_insert<<<dist_blocks(t.n), 256, 0, s>>>(t, g, fine, cg, coarse, words);
    return hipGetLastError();
}

hipError_t launch_dist_lists(DistCloud t, DistGrid g, DistTable fine, float4* list, unsigned long long* words,
                             hipStream_t s) {
    if (t.n == 0) return hipSuccess;
    const unsigned long long blocks = std::min<unsigned long long>((fine.slots + 255ull) / 256ull, 4096ull);
    k_dist_starts<<<static_cast<unsigned>(blocks), 256, 0, s>>>(fine, words);
    k_dist_scatter<<<dist_blocks(t.n), 256, 0, s>>>(t, g, fine, list, words);
    return hipGetLastError();
}

hipError_t launch_dist_query(DistCloud q, DistGrid g, DistTable fine, DistGrid cg, DistTable coarse, const float4* list,
                             DistQuery p, float* d2, int32_t* nearest, unsigned long long* words, hipStream_t s) {
    if (q.n == 0) return hipSuccess;
    k_dist_query<<<dist_blocks(q.n), 256, 0, s>>>(q, g, fine, cg, coarse, list, p, d2, nearest, words);
    return hipGetLastError();
}

hipError_t launch_align_iter(DistCloud q, unsigned long long stride, DistCloud t, DistGrid g, DistTable fine, DistGrid cg,
                             DistTable coarse, const float4* list, DistQuery p, double kq, unsigned long long* words,
                             unsigned long long* rec, hipStream_t s) {
    const unsigned long long nq = (q.n + stride - 1ull) / stride;
    if (nq == 0) return hipSuccess;
    k_align_iter<<<dist_blocks(nq), 256, 0, s>>>(q, stride, nq, t, g, fine, cg, coarse, list, p, kq, words, rec);
    return hipGetLastError();
}

hipError_t launch_align_plane_iter(DistCloud q, unsigned long long stride, DistCloud t, DistGrid g, DistTable fine,
                                   DistGrid cg, DistTable coarse, const float4* list, DistQuery p, double kq,
                                   AlignPivot pivot, unsigned long long* words, unsigned long long* rec, hipStream_t s) {
    const unsigned long long nq = (q.n + stride - 1ull) / stride;
    if (nq == 0) return hipSuccess;
    k_align_plane_iter<<<dist_blocks(nq), 256, 0, s>>>(q, stride, nq, t, g, fine, cg, coarse, list, p, kq, pivot, words, rec);
    return hipGetLastError();
}

// ------------------------------------------------------------------ evaluation regions
//
// acmmp_fusion_set_region (include/acmmp.h): the class byte of every point of a cloud, one lane per point,
// in the float64 arithmetic of the definition.  The polygon is staged once per workgroup into LDS (at most 256 x 2
// doubles, 4 KB); the edge loop's trip count and addresses are the same for every lane, so each LDS read is a
// broadcast.  The divide of the crossing test runs only under the lanes whose edge straddles p_v -- a wave in which no
// lane straddles skips it -- and a horizontal edge (v_j == v_i) never straddles, so no lane divides by zero.  The counts
// are ballots per wave, summed over the workgroup through LDS, one atomic add per word per workgroup.
__global__ __launch_bounds__(256) void k_region_classify(const DistCloud c, const RegionDev r, uint8_t* __restrict__ cls,
                                                         unsigned long long* __restrict__ words) {
    __shared__ double poly[2 * ACMMP_REGION_MAX_VERTICES];
    __shared__ unsigned part[4][kRegionWords];
    for (int k = threadIdx.x; k < 2 * r.n_vertices; k += 256) poly[k] = r.poly[k];
    __syncthreads();
    const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    const bool here = i < c.n;
    unsigned cl = 0u;
    if (here) {
        float v[3];
        if (!dist_load(c, i, v)) {
            cl = ACMMP_REGION_CLASS_INVALID;
        } else {
            const double x = static_cast<double>(v[0]), y = static_cast<double>(v[1]), z = static_cast<double>(v[2]);
            bool fail = false;
            for (int k = 0; k < r.n_planes; ++k) {
                const double s = ((r.planes[4 * k] * x + r.planes[4 * k + 1] * y) + r.planes[4 * k + 2] * z) + r.planes[4 * k + 3];
                fail = fail || !(s >= 0.0);
            }
            if (fail) cl |= ACMMP_REGION_CLASS_PLANES;
            if (r.n_vertices > 0) {
                const double pw = r.axis == 0 ? x : r.axis == 1 ? y : z;
                const double pu = r.axis == 0 ? y : x, pv = r.axis == 2 ? y : z;
                bool odd = false;
                double ui = poly[2 * (r.n_vertices - 1)], vi = poly[2 * (r.n_vertices - 1) + 1];   // edge n - 1 first
                for (int e = 0; e < r.n_vertices; ++e) {
                    // the edge from vertex e - 1 (mod n) to vertex e: the definition's edge i = e - 1, j = e
                    const double uj = poly[2 * e], vj = poly[2 * e + 1];
                    if ((vi > pv) != (vj > pv)) {
                        const double cross = (((uj - ui) * (pv - vi)) / (vj - vi)) + ui;
                        odd = odd != (pu < cross);
                    }
                    ui = uj;
                    vi = vj;
                }
                if (!(pw >= r.axis_min && pw <= r.axis_max && odd)) cl |= ACMMP_REGION_CLASS_PRISM;
            }
            if (r.dims[0] > 0) {
                const double ix = rint((x - r.o[0]) / r.cell), iy = rint((y - r.o[1]) / r.cell), iz = rint((z - r.o[2]) / r.cell);
                bool in = ix >= 0.0 && ix < static_cast<double>(r.dims[0]) && iy >= 0.0 && iy < static_cast<double>(r.dims[1]) &&
                          iz >= 0.0 && iz < static_cast<double>(r.dims[2]);
                if (in) {
                    const unsigned long long nx = static_cast<unsigned long long>(r.dims[0]), ny = static_cast<unsigned long long>(r.dims[1]);
                    const unsigned long long k = static_cast<unsigned long long>(ix) +
                                                 nx * (static_cast<unsigned long long>(iy) + ny * static_cast<unsigned long long>(iz));
                    in = (r.bits[k >> 3] >> (k & 7ull)) & 1u;
                }
                if (!in) cl |= ACMMP_REGION_CLASS_GRID;
            }
        }
        cls[i] = static_cast<uint8_t>(cl);
    }
    if (!words) return;                               // a measuring call's pre-pass: no counts (uniform over the grid)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b[kRegionWords] = {__ballot(here), __ballot(here && cl == ACMMP_REGION_CLASS_INVALID),
                                                __ballot(here && cl == 0u), __ballot((cl & ACMMP_REGION_CLASS_PLANES) != 0u),
                                                __ballot((cl & ACMMP_REGION_CLASS_PRISM) != 0u),
                                                __ballot((cl & ACMMP_REGION_CLASS_GRID) != 0u)};
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kRegionWords; ++k) part[wave][k] = static_cast<unsigned>(__popcll(b[k]));
    }
    __syncthreads();
    if (threadIdx.x < kRegionWords) {
        const unsigned x = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
        if (x) atomicAdd(&words[threadIdx.x], static_cast<unsigned long long>(x));
    }
}

hipError_t launch_region_classify(DistCloud c, RegionDev r, uint8_t* cls, unsigned long long* words, hipStream_t s) {
    if (c.n == 0) return hipSuccess;
    c.cls = nullptr;
    k_region_classify<<<dist_blocks(c.n), 256, 0, s>>>(c, r, cls, words);
    return hipGetLastError();
}

// ------------------------------------------------------------------ point-to-triangle distances to the mesh
//
// acmmp_fusion_surface_distance (include/acmmp.h).  As above the result is defined over all (query, face)
// pairs and the grid only decides which are looked at.  A face is listed in every cell its vertex box overlaps, so a
// face not yet met after rings 0 .. r has a box that misses the cube of those rings; the clamp of step 3 keeps the
// closest point inside that box, which is what turns the cell gap into a bound on D2.

// Step 3: the float32 D2 of query p and face (A, B, C); NaN for a pair that is no candidate.
__device__ __forceinline__ float surf_pair_d2(const float p[3], const float A[3], const float B[3], const float C[3]) {
    double ap[3], bp[3], cp[3], ab[3], ac[3], bc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double pk = static_cast<double>(p[k]), a = static_cast<double>(A[k]), b = static_cast<double>(B[k]),
                     c = static_cast<double>(C[k]);
        ap[k] = pk - a; bp[k] = pk - b; cp[k] = pk - c;
        ab[k] = b - a; ac[k] = c - a; bc[k] = c - b;
    }
    const double d1 = (ab[0] * ap[0] + ab[1] * ap[1]) + ab[2] * ap[2];
    const double d2 = (ac[0] * ap[0] + ac[1] * ap[1]) + ac[2] * ap[2];
    const double d3 = (ab[0] * bp[0] + ab[1] * bp[1]) + ab[2] * bp[2];
    const double d4 = (ac[0] * bp[0] + ac[1] * bp[1]) + ac[2] * bp[2];
    const double d5 = (ab[0] * cp[0] + ab[1] * cp[1]) + ab[2] * cp[2];
    const double d6 = (ac[0] * cp[0] + ac[1] * cp[1]) + ac[2] * cp[2];
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    double e[3];
    if (d1 <= 0.0 && d2 <= 0.0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) e[k] = -ap[k];
    } else if (d3 >= 0.0 && d4 <= d3) {
#pragma unroll
        for (int k = 0; k < 3; ++k) e[k] = -bp[k];
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double v = d1 / (d1 - d3);
#pragma unroll
        for (int k = 0; k < 3; ++k) e[k] = v * ab[k] - ap[k];
    } else if (d6 >= 0.0 && d5 <= d6) {
#pragma unroll
        for (int k = 0; k < 3; ++k) e[k] = -cp[k];
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double w = d2 / (d2 - d6);
#pragma unroll
        for (int k = 0; k < 3; ++k) e[k] = w * ac[k] - ap[k];
    } else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
        const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
#pragma unroll
        for (int k = 0; k < 3; ++k) e[k] = w * bc[k] - bp[k];
    } else {
        const double s = (va + vb) + vc, v = vb / s, w = vc / s;
#pragma unroll
        for (int k = 0; k < 3; ++k) e[k] = (v * ab[k] + w * ac[k]) - ap[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double lo = fmin(-ap[k], fmin(-bp[k], -cp[k])), hi = fmax(-ap[k], fmax(-bp[k], -cp[k]));
        e[k] = e[k] < lo ? lo : (e[k] > hi ? hi : e[k]);
    }
    return static_cast<float>((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
}

// Steps 1 and 2 for face j: its vertices as dist_load reads them; false = not a valid face.
__device__ __forceinline__ bool surf_face(const SurfMesh& m, unsigned j, float A[3], float B[3], float C[3]) {
    const int32_t* t = m.faces + 3ull * j;
    const unsigned long long ia = static_cast<uint32_t>(t[0]), ib = static_cast<uint32_t>(t[1]), ic = static_cast<uint32_t>(t[2]);
    if (ia >= m.v.n || ib >= m.v.n || ic >= m.v.n) return false;
    const bool oa = dist_load(m.v, ia, A), ob = dist_load(m.v, ib, B), oc = dist_load(m.v, ic, C);
    return oa && ob && oc;
}

__global__ __launch_bounds__(256) void k_surf_bounds(const SurfMesh m, unsigned long long* __restrict__ words) {
    const unsigned long long j = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    uint32_t mm[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    bool ok = false;
    if (j < m.nf) {
        float A[3], B[3], C[3];
        ok = surf_face(m, static_cast<unsigned>(j), A, B, C);
        if (ok) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                mm[a] = vox_ordered(fminf(A[a], fminf(B[a], C[a])));
                mm[3 + a] = vox_ordered(-fmaxf(A[a], fmaxf(B[a], C[a])));
            }
        }
    }
    uint32_t* mn = reinterpret_cast<uint32_t*>(words + kDistMin);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) mm[a] = min(mm[a], static_cast<uint32_t>(__shfl_xor(static_cast<int>(mm[a]), d)));
        if ((threadIdx.x & 63) == 0 && mm[a] != 0xffffffffu) atomicMin(&mn[a], mm[a]);
    }
    wave_count(ok, &words[kDistValidTargets]);
}

// The three passes over the faces.  kSurfPlan: the counts of the plan.  kSurfCount: a small face claims its cells and
// adds 1 to each count, a large face goes to the overflow list.  kSurfScatter: a small face goes to its cells' lists.
enum { kSurfPlan = 0, kSurfCount = 1, kSurfScatter = 2 };
template <int PASS>
__global__ __launch_bounds__(256) void k_surf_faces(const SurfMesh m, const DistGrid g, const DistTable fine, long long small_max,
                                                    float4* __restrict__ list, unsigned long long cap_list,
                                                    float4* __restrict__ large, unsigned long long cap_large,
                                                    unsigned long long* __restrict__ words) {
    const unsigned long long j = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    unsigned err = 0u;
    bool is_small = false, is_large = false;
    unsigned long long cells = 0;
    if (j < m.nf) {
        float A[3], B[3], C[3];
        if (surf_face(m, static_cast<unsigned>(j), A, B, C)) {
            int c0[3], c1[3];
            cells = 1;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                double fr;
                bool cl = false;
                c0[a] = dist_axis(g, a, fminf(A[a], fminf(B[a], C[a])), fr, cl);
                c1[a] = dist_axis(g, a, fmaxf(A[a], fmaxf(B[a], C[a])), fr, cl);
                cells *= static_cast<unsigned long long>(c1[a] - c0[a] + 1);
            }
            is_large = small_max < 0 || cells > static_cast<unsigned long long>(small_max);
            is_small = !is_large;
            const float4 ea = make_float4(A[0], A[1], A[2], __uint_as_float(static_cast<uint32_t>(j)));
            const float4 eb = make_float4(B[0], B[1], B[2], 0.0f), ec = make_float4(C[0], C[1], C[2], 0.0f);
            if (PASS == kSurfCount && is_large) {
                const unsigned long long pos = atomicAdd(&words[kSurfLargeCursor], 1ull);
                if (pos < cap_large) { large[3 * pos] = ea; large[3 * pos + 1] = eb; large[3 * pos + 2] = ec; }
                else err = 2u;
            }
            if (PASS != kSurfPlan && is_small) {
                for (int z = c0[2]; z <= c1[2]; ++z)
                    for (int y = c0[1]; y <= c1[1]; ++y)
                        for (int x = c0[0]; x <= c1[0]; ++x) {
                            unsigned long long s;
                            if (PASS == kSurfCount) {
                                if (table_claim(fine, dist_key(x, y, z), s)) atomicAdd(&fine.cnt[s], 1u);
                                else err = 1u;
                            } else if (table_find(fine, dist_key(x, y, z), s) == 0) {
                                const unsigned long long pos = atomicAdd(&fine.cnt[s], 1u);
                                if (pos < cap_list) { list[3 * pos] = ea; list[3 * pos + 1] = eb; list[3 * pos + 2] = ec; }
                                else err = 2u;
                            } else {
                                err = 2u;
                            }
                        }
            }
        }
    }
    if (PASS == kSurfPlan) {
        wave_count(is_small, &words[kSurfSmall]);
        wave_count(is_large, &words[kSurfLarge]);
        wave_add(is_small ? cells : 0ull, &words[kSurfRegs]);
    } else {
        block_or(err, &words[kDistErr]);
    }
}

// One listed face against the query: best = min(best, key) unless D2 is NaN.
__device__ __forceinline__ void surf_entry(const float4* __restrict__ e, const float v[3], unsigned long long& best) {
    const float4 a = e[0], b = e[1], c = e[2];
    const float A[3] = {a.x, a.y, a.z}, B[3] = {b.x, b.y, b.z}, C[3] = {c.x, c.y, c.z};
    const float d2 = surf_pair_d2(v, A, B, C);
    const unsigned long long key =
        static_cast<unsigned long long>(__float_as_uint(d2)) << 32 | static_cast<unsigned long long>(__float_as_uint(a.w));
    if (d2 == d2) best = min(best, key);
}

__global__ __launch_bounds__(256) void k_surf_query(const DistCloud q, const DistGrid g, const DistTable fine,
                                                    const float4* __restrict__ list, const float4* __restrict__ large,
                                                    unsigned n_large, const DistQuery p, float* __restrict__ d2out,
                                                    int32_t* __restrict__ nnout, unsigned long long* __restrict__ words) {
    __shared__ unsigned hist[256];
    hist[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    bool valid = false, matched = false;
    float d2 = __builtin_inff();
    int32_t nn = -1;
    unsigned long long rings = 0;
    unsigned err = 0u;
    if (i < q.n) {
        float v[3];
        valid = dist_load(q, i, v);
        if (valid && p.have_targets) {
            const double m2d = static_cast<double>(p.m2);
            // the bounding box of the faces: the closest point of every face lies in it
            double gap = 0.0;
#pragma unroll
            for (int a = 0; a < 3; ++a)
                gap = fmax(gap, fmax(p.lo[a] - static_cast<double>(v[a]), static_cast<double>(v[a]) - p.hi[a]));
            unsigned long long best = ~0ull;
            if (!(dist_floor2(gap) > m2d)) {
                for (unsigned l = 0; l < n_large; ++l) surf_entry(large + 3ull * l, v, best);
                dist_walk(v, g, m2d, best, rings, [&](int x, int y, int z, unsigned long long& b) {
                    unsigned long long s;
                    const int r = table_find(fine, dist_key(x, y, z), s);
                    if (r == 2) err |= 4u;
                    if (r != 0) return;
                    const uint32_t e0 = fine.start[s], e1 = fine.cnt[s];
                    for (uint32_t pos = e0; pos < e1; ++pos) surf_entry(list + 3ull * pos, v, b);
                });
            }
            if (best != ~0ull) {
                const float w = __uint_as_float(static_cast<uint32_t>(best >> 32));
                if (w <= p.m2) {
                    matched = true;
                    d2 = w;
                    nn = static_cast<int32_t>(static_cast<uint32_t>(best & 0xffffffffull));
                }
            }
        }
        d2out[i] = d2;
        nnout[i] = nn;
    }
    dist_summarise(valid, matched, d2, rings, err, p, hist, words);
}

hipError_t launch_surf_bounds(SurfMesh m, unsigned long long* words, hipStream_t s) {
    if (m.nf == 0) return hipSuccess;
    k_surf_bounds<<<dist_blocks(m.nf), 256, 0, s>>>(m, words);
    return hipGetLastError();
}

hipError_t launch_surf_plan(SurfMesh m, DistGrid g, long long small_max, unsigned long long* words, hipStream_t s) {
    if (m.nf == 0) return hipSuccess;
    const DistTable none = {nullptr, nullptr, nullptr, 0, 0};
    k_surf_faces<kSurfPlan><<<dist_blocks(m.nf), 256, 0, s>>>(m, g, none, small_max, nullptr, 0, nullptr, 0, words);
    return hipGetLastError();
}

hipError_t launch_surf_lists(SurfMesh m, DistGrid g, DistTable fine, long long small_max, float4* list,
                             unsigned long long cap_list, float4* large, unsigned long long cap_large,
                             unsigned long long* words, hipStream_t s) {
    if (m.nf == 0) return hipSuccess;
    const unsigned long long blocks = std::min<unsigned long long>((fine.slots + 255ull) / 256ull, 4096ull);
    k_surf_faces<kSurfCount><<<dist_blocks(m.nf), 256, 0, s>>>(m, g, fine, small_max, list, cap_list, large, cap_large, words);
    k_dist_starts<<<static_cast<unsigned>(blocks), 256, 0, s>>>(fine, words);
    k_surf_faces<kSurfScatter><<<dist_blocks(m.nf), 256, 0, s>>>(m, g, fine, small_max, list, cap_list, large, cap_large, words);
    return hipGetLastError();
}

hipError_t launch_surf_query(DistCloud q, DistGrid g, DistTable fine, const float4* list, const float4* large,
                             unsigned n_large, DistQuery p, float* d2, int32_t* nearest, unsigned long long* words,
                             hipStream_t s) {
    if (q.n == 0) return hipSuccess;
    k_surf_query<<<dist_blocks(q.n), 256, 0, s>>>(q, g, fine, list, large, n_large, p, d2, nearest, words);
    return hipGetLastError();
}

// ------------------------------------------------------------------ area-uniform samples of the mesh
//
// acmmp_fusion_mesh_sample (include/acmmp.h).  Every choice is made in 64-bit integers (the rounding of a
// face's count, the lattice, the fold into the triangle, the weights), so that the float64 blends see exact weights; the
// samples are an expansion of the faces (a face gives 0 .. 2^31 of them), which the ordered compaction does not cover:
// the faces' counts are scanned in chunks of 256 (in the chunk by k_sample_count, the chunks' bases by k_sample_scan),
// and a sample finds its face by two upper-bound searches.

constexpr unsigned long long kSampleG1 = 0xC13FA9A902A6328Full, kSampleG2 = 0x91E10DA5C79E7B1Dull;   // 2^64 / p, 2^64 / p^2
constexpr unsigned long long kSampleOne = 1ull << 53;

// Step 0: splitmix64's finaliser, as vox_home has it.
__device__ __forceinline__ unsigned long long sample_mix(unsigned long long z) {
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// The vertices of face f: v[0 .. 3) point at their 9 floats; false = an index outside the vertices.
__device__ __forceinline__ bool sample_face(const float* __restrict__ verts, unsigned long long nv,
                                            const int32_t* __restrict__ faces, unsigned long long f, const float* v[3]) {
    const int32_t* t = faces + 3ull * f;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const unsigned long long i = static_cast<uint32_t>(t[k]);
        ok = ok && i < nv;
        v[k] = verts + 9ull * (i < nv ? i : 0ull);
    }
    return ok;
}

// Exclusive prefix of x over the 256 lanes of the workgroup in lane order, and their sum.  Every lane calls it.
__device__ __forceinline__ unsigned long long sample_block_scan(unsigned long long x, unsigned long long& total) {
    __shared__ unsigned long long wave_tot[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long incl = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long y = __shfl_up(incl, d);
        if (lane >= d) incl += y;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    unsigned long long before = 0ull;
    total = 0ull;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const unsigned long long t = wave_tot[w];
        total += t;
        if (w < wave) before += t;
    }
    return before + (incl - x);
}

// Steps 1 to 3, one lane per face: loc[f] = the samples of the faces before f in f's chunk of 256 faces, chunk_tot[c] =
// the samples of chunk c, words[kSampleSkipped] += the invalid faces.
__global__ __launch_bounds__(256) void k_sample_count(const float* __restrict__ verts, unsigned long long nv,
                                                      const int32_t* __restrict__ faces, unsigned nf, double s2,
                                                      unsigned long long seed, unsigned long long* __restrict__ loc,
                                                      unsigned long long* __restrict__ chunk_tot,
                                                      unsigned long long* __restrict__ words) {
    const unsigned long long f = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    unsigned long long n = 0ull;
    bool skipped = false;
    if (f < nf) {
        const float* v[3];
        bool ok = sample_face(verts, nv, faces, f, v);
        double P[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float x = v[k][a];
                ok = ok && !vox_nonfinite(x);
                P[k][a] = static_cast<double>(x);
            }
        }
        skipped = !ok;
        if (ok) {
            const double e1x = P[1][0] - P[0][0], e1y = P[1][1] - P[0][1], e1z = P[1][2] - P[0][2];
            const double e2x = P[2][0] - P[0][0], e2y = P[2][1] - P[0][1], e2z = P[2][2] - P[0][2];
            const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
            const double area = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
            const double e = area / s2;
            if (e >= 2147483648.0) {
                n = 1ull << 31;
            } else {
                const double k = floor(e), r = e - k;
                const unsigned long long T = static_cast<unsigned long long>(r * 9007199254740992.0);
                const unsigned long long h = sample_mix(seed ^ sample_mix(f));
                n = static_cast<unsigned long long>(k) + ((h >> 11) < T ? 1ull : 0ull);
            }
        }
    }
    unsigned long long total;
    const unsigned long long before = sample_block_scan(n, total);
    if (f < nf) loc[f] = before;
    if (threadIdx.x == 0) chunk_tot[blockIdx.x] = total;
    wave_count(skipped, &words[kSampleSkipped]);
}

// Step 4: base[c] = the samples of the chunks before c, words[kSampleTotal] = N.  One workgroup of 1024 lanes walks
// the chunks in tiles of 1024 with a running carry, as k_fuse_scan does, over 64-bit counts.
__global__ __launch_bounds__(1024) void k_sample_scan(const unsigned long long* __restrict__ chunk_tot, unsigned n_chunks,
                                                      unsigned long long* __restrict__ base,
                                                      unsigned long long* __restrict__ words) {
    __shared__ unsigned long long wave_tot[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long carry = 0ull;
    for (unsigned t0 = 0; t0 < n_chunks; t0 += 1024u) {
        const unsigned i = t0 + threadIdx.x;
        const unsigned long long x = i < n_chunks ? chunk_tot[i] : 0ull;
        unsigned long long incl = x;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long y = __shfl_up(incl, d);
            if (lane >= d) incl += y;
        }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        unsigned long long before = 0ull, all = 0ull;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const unsigned long long t = wave_tot[w];
            all += t;
            if (w < wave) before += t;
        }
        if (i < n_chunks) base[i] = carry + before + (incl - x);
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) words[kSampleTotal] = carry;
}

// The last of a[0 .. n) that is <= x (the upper bound minus one), for ascending a with a[0] <= x: where several equal
// x, the last of them, which steps over every run of items without samples.
__device__ __forceinline__ unsigned sample_find(const unsigned long long* __restrict__ a, unsigned n, unsigned long long x) {
    unsigned lo = 0u, hi = n;                      // a[lo - 1] <= x < a[hi]
    while (lo < hi) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= x) lo = mid + 1u;
        else hi = mid;
    }
    return lo > 0u ? lo - 1u : 0u;
}

// Steps 5 and 6, one lane per sample i of N: its face from the offsets, its number j in the face, the lattice point, the
// blend of the three vertices.
__global__ __launch_bounds__(256) void k_sample_emit(const float* __restrict__ verts, unsigned long long nv,
                                                     const int32_t* __restrict__ faces, unsigned nf, unsigned long long seed,
                                                     const unsigned long long* __restrict__ loc,
                                                     const unsigned long long* __restrict__ base, unsigned n_chunks,
                                                     unsigned long long N, float* __restrict__ out, int32_t* __restrict__ out_face) {
    const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= N) return;
    const unsigned c = sample_find(base, n_chunks, i);
    const unsigned f0 = c * 256u, m = nf - f0 < 256u ? nf - f0 : 256u;
    const unsigned long long in_chunk = i - base[c];
    const unsigned f = f0 + sample_find(loc + f0, m, in_chunk);
    const unsigned long long j = in_chunk - loc[f];
    const float* v[3];
    (void)sample_face(verts, nv, faces, f, v);
    const unsigned long long h = sample_mix(seed ^ sample_mix(f));
    const unsigned long long o1 = sample_mix(h), o2 = sample_mix(o1);
    unsigned long long i1 = (o1 + j * kSampleG1) >> 11, i2 = (o2 + j * kSampleG2) >> 11;
    if (i1 + i2 > kSampleOne) {
        i1 = kSampleOne - i1;
        i2 = kSampleOne - i2;
    }
    const unsigned long long i0 = kSampleOne - i1 - i2;
    const double scale = 1.0 / 9007199254740992.0;
    const double w0 = static_cast<double>(i0) * scale, w1 = static_cast<double>(i1) * scale, w2 = static_cast<double>(i2) * scale;
    float r[9];
    double M[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const double b = (w0 * static_cast<double>(v[0][k]) + w1 * static_cast<double>(v[1][k])) + w2 * static_cast<double>(v[2][k]);
        if (k >= 3 && k < 6) M[k - 3] = b;
        r[k] = static_cast<float>(b);
    }
    const double len = sqrt((M[0] * M[0] + M[1] * M[1]) + M[2] * M[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) r[3 + k] = len > 0.0 ? static_cast<float>(M[k] / len) : 0.0f;
    float* o = out + 9ull * i;
#pragma unroll
    for (int k = 0; k < 9; ++k) o[k] = r[k];
    out_face[i] = static_cast<int32_t>(f);
}

hipError_t launch_sample_count(const float* verts, unsigned long long nv, const int32_t* faces, unsigned nf, double s2,
                               unsigned long long seed, unsigned long long* loc, unsigned long long* chunk_tot,
                               unsigned long long* base, unsigned long long* words, hipStream_t s) {
    if (nf == 0) return hipSuccess;
    const unsigned n_chunks = dist_blocks(nf);
    k_sample_count<<<n_chunks, 256, 0, s>>>(verts, nv, faces, nf, s2, seed, loc, chunk_tot, words);
    k_sample_scan<<<1, 1024, 0, s>>>(chunk_tot, n_chunks, base, words);
    return hipGetLastError();
}

hipError_t launch_sample_emit(const float* verts, unsigned long long nv, const int32_t* faces, unsigned nf,
                              unsigned long long seed, const unsigned long long* loc, const unsigned long long* base,
                              unsigned long long N, float* out, int32_t* out_face, hipStream_t s) {
    if (N == 0) return hipSuccess;
    k_sample_emit<<<dist_blocks(N), 256, 0, s>>>(verts, nv, faces, nf, seed, loc, base, dist_blocks(nf), N, out, out_face);
    return hipGetLastError();
}

}  // namespace acmmp
