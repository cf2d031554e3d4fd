// aux_kernels.hip -- gfx950 kernels beside the PatchMatch hot path, with their host launchers: the device
// half of the planar prior and the support points (planar.h), the depth export and the plain copies, the
// clock probe and the buffer checksum (engine.h).  One translation unit, compiled once.
#include <algorithm>

#include "engine.h"
#include "planar.h"

namespace acmmp {

// ------------------------------------------------------------------ kernels: planar prior (device half)
//
// ProcessProblem's triangle rasterisation and prior-depth mask (main.cpp:138-181) with the triangles,
// planes and steps the host computed (planar.h).  One thread per (triangle, p step): the p values are
// the reference's running float sums 0, step, 2 step, ... (recomputed by the same additions), the q
// loop runs as in the reference; the reference overwrites labels in triangle order, so a pixel keeps
// the largest label that reaches it -- atomicMax gives that whatever the schedule.  Same float and
// double arithmetic as the reference's C++ (no contraction): the same pixels, bit for bit.
__global__ __launch_bounds__(256) void k_planar_raster(const PlanarDev pd, uint32_t* mask) {
    const long long t = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= pd.n_steps) return;
    int lo = 0, hi = pd.n_tri - 1;                       // triangle k with first[k] <= t < first[k + 1]
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pd.first[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    const int k = lo;
    const long long i = t - pd.first[k];
    const float step = pd.step[k];
    float p = 0.f;
    for (long long a = 0; a < i; ++a) p += step;
    const int* tr = pd.tri + 6 * static_cast<long long>(k);
    const uint32_t label = static_cast<uint32_t>(k) + 1u;
    const double rest = 1.0 - static_cast<double>(p);
    for (float q = 0.f; static_cast<double>(q) < rest; q += step) {
        const double w3 = rest - static_cast<double>(q);
        const int x = static_cast<int>(static_cast<double>(p * static_cast<float>(tr[0]) + q * static_cast<float>(tr[2])) +
                                       w3 * static_cast<double>(tr[4]));
        const int y = static_cast<int>(static_cast<double>(p * static_cast<float>(tr[1]) + q * static_cast<float>(tr[3])) +
                                       w3 * static_cast<double>(tr[5]));
        if (x >= 0 && x < pd.W && y >= 0 && y < pd.H) atomicMax(mask + static_cast<long long>(y) * pd.W + x, label);
    }
}

// GetDepthFromPlaneParam (ACMMP.cpp:991-1011) per labelled pixel; out-of-range prior depths drop the
// label (main.cpp:168-180); CudaPlanarPriorInitialization's expansion (ACMMP.cpp:855-862).
__global__ __launch_bounds__(256) void k_planar_mask(const PlanarDev pd, uint32_t* mask, float4* prior) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (i >= pd.W) return;
    const long long c = static_cast<long long>(j) * pd.W + i;
    uint32_t l = mask[c];
    float4 pl = make_float4(0.f, 0.f, 0.f, 0.f);
    if (l > 0) {
        pl = pd.plane[l - 1];
        float d;
        if (pd.model == kSphere) {
            const float2 lat = pd.row_trig[j], lon = pd.col_trig[i];
            const float dx = lat.y * lon.x, dy = -lat.x, dz = lat.y * lon.y;
            const float denom = pl.x * dx + pl.y * dy + pl.z * dz;
            d = (fabsf(denom) < 1e-6f) ? 1e6f : (-pl.w / denom);
        } else {
            d = -pl.w * pd.K0 / ((static_cast<float>(i) - pd.K2) * pl.x +
                                 (pd.K0 / pd.K4) * (static_cast<float>(j) - pd.K5) * pl.y + pd.K0 * pl.z);
        }
        if (!(d <= pd.depth_max && d >= pd.depth_min)) {
            l = 0;
            pl = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    mask[c] = l;
    prior[c] = pl;
}

hipError_t launch_planar_raster(const PlanarDev& pd, uint32_t* mask, hipStream_t s) {
    if (pd.n_steps > 0) k_planar_raster<<<static_cast<unsigned>(cdiv(pd.n_steps, 256)), 256, 0, s>>>(pd, mask);
    return hipGetLastError();
}

hipError_t launch_planar_mask(const PlanarDev& pd, uint32_t* mask, float4* prior, hipStream_t s) {
    k_planar_mask<<<dim3(cdiv(pd.W, 256), pd.H), 256, 0, s>>>(pd, mask, prior);
    return hipGetLastError();
}

// GetSupportPoints (ACMMP.cpp:904-929) on the context's last RunPatchMatch output: one thread per 5x5
// block, scanned column by column with the reference's strict '>' (the first minimum-cost pixel, costs
// 2.0 and above skipped), kept when the minimum is < 0.1.  out[strip * bh + block row] = (kept, x, y,
// depth bits) -- the reference's point order is strip-major, block rows within a strip.
__global__ __launch_bounds__(256) void k_support_points(const float* __restrict__ costs, const float4* __restrict__ planes,
                                                        int W, int H, int bh, int4* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int bw = (W + 4) / 5;
    if (t >= bw * bh) return;
    const int strip = t / bh, rb = t - strip * bh;
    const int col = strip * 5, row = rb * 5;
    const int cb = min(W, col + 5), rbe = min(H, row + 5);
    float min_cost = 2.0f;
    int tx = 0, ty = 0;
    for (int c = col; c < cb; ++c)
        for (int r = row; r < rbe; ++r) {
            const float v = costs[static_cast<long long>(r) * W + c];
            if (v < 2.0f && min_cost > v) { tx = c; ty = r; min_cost = v; }
        }
    const bool keep = min_cost < 0.1f;
    const float d = keep ? planes[static_cast<long long>(ty) * W + tx].w : 0.0f;
    out[t] = make_int4(keep ? 1 : 0, tx, ty, __float_as_int(d));
}

hipError_t launch_support_points(const float* costs, const float4* planes, int W, int H, int4* out, hipStream_t s) {
    const int bh = (H + 4) / 5, n = ((W + 4) / 5) * bh;
    k_support_points<<<cdiv(n, 256), 256, 0, s>>>(costs, planes, W, H, bh, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------ depth export and plain copies

__global__ void k_export_depth(const float4* __restrict__ planes, long long P, float* __restrict__ dst) {
    const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < P) dst[i] = planes[i].w;
}

// A plain copy of n 16-byte words on the compute queue (the state export / restart of a geom pass: at HBM
// rate, where a device-to-device hipMemcpyAsync of the same 38 MB measured ~9 ms inside the pipeline's
// overlapped passes)
__global__ void k_copy16(const uint4* __restrict__ src, long long n, uint4* __restrict__ dst) {
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * blockDim.x)
        dst[i] = src[i];
}
__global__ void k_copy4(const uint32_t* __restrict__ src, long long n, uint32_t* __restrict__ dst) {
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * blockDim.x)
        dst[i] = src[i];
}

hipError_t launch_copy(const void* src, void* dst, size_t bytes, hipStream_t s) {
    if (bytes == 0) return hipSuccess;
    const bool wide = bytes % 16 == 0 && reinterpret_cast<uintptr_t>(src) % 16 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0;
    const long long n = static_cast<long long>(wide ? bytes / 16 : bytes / 4);
    const unsigned grd = static_cast<unsigned>(std::min<long long>((n + 255) / 256, 8192));
    if (wide) k_copy16<<<grd, 256, 0, s>>>(static_cast<const uint4*>(src), n, static_cast<uint4*>(dst));
    else k_copy4<<<grd, 256, 0, s>>>(static_cast<const uint32_t*>(src), n, static_cast<uint32_t*>(dst));
    return hipGetLastError();
}

hipError_t launch_export_depth(const float4* planes, long long P, float* dst, hipStream_t s) {
    k_export_depth<<<static_cast<unsigned>((P + 255) / 256), 256, 0, s>>>(planes, P, dst);
    return hipGetLastError();
}

// ------------------------------------------------------------------ diagnostic: the shader clock under load
//
// Not on the PatchMatch path (acmmp_clock_probe, bench.py's `clock`).  The chip lowers its clock under load,
// by different amounts on different devices (MI355X_MICROARCH.md "DVFS give-back" (5): 1.51-1.69 GHz across
// devices for issue-dense bodies), and k_eval_nb is issue-dense: its time tracks that clock.  Eight independent
// chains per lane of the logistic map x <- r x (1 - x) at r = 3.99 (a multiply and an fma per step): a
// VALU-dense body whose operands stay chaotic, so their bits keep toggling as k_eval_nb's data does (an fma
// chain converging to a fixed point draws less power and holds a higher clock, ibid. item 1); the first lane
// of each workgroup reads the shader-cycle counter and the constant 100 MHz counter around the loop (ibid.
// item 6), and the host takes the median of the per-workgroup ratios.
__global__ __launch_bounds__(256) void k_clock_probe(const float* __restrict__ rnd, int iters, ClockStamp* stamps,
                                                     float* __restrict__ sink) {
    const unsigned gid = blockIdx.x * 256u + threadIdx.x;
    float x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = 0.25f + 0.5f * fabsf(rnd[(gid * 8u + k) & 65535u]);
    constexpr float r = 3.99f;
    unsigned long long t0 = 0, r0 = 0;
    if (stamps) {
        t0 = __builtin_amdgcn_s_memtime();
        r0 = __builtin_amdgcn_s_memrealtime();
    }
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float t = r * x[k];
            x[k] = fmaf(-t, x[k], t);
        }
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += x[k];
    if (stamps) {
        const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        if (threadIdx.x == 0) {
            ClockStamp c;
            c.cycles = t1 - t0;
            c.ticks = r1 - r0;
            stamps[blockIdx.x] = c;
        }
    }
    sink[gid] = s;
}

hipError_t launch_clock_probe(const float* rnd, int iters, int blocks, ClockStamp* stamps, float* sink, hipStream_t s) {
    k_clock_probe<<<blocks, 256, 0, s>>>(rnd, iters, stamps, sink);
    return hipGetLastError();
}

// ------------------------------------------------------------------ exchange check: checksum of a device buffer
//
// sum over the buffer's 32-bit words w_i of mix64((i << 32) | w_i) mod 2^64 (acmmp_device_checksum): a word's
// value and position both enter, and the sum does not depend on the order it is formed in.  The pipeline
// compares every rank's checksum of each map a pass exchanged (acmmp/pipeline.py RcclExchange), so a wrong
// root, buffer or ordering in the grouped broadcast fails the run instead of feeding a wrong map on.
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void k_checksum(const uint32_t* __restrict__ w, long long n, unsigned long long* out) {
    unsigned long long acc = 0;
    for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * 256)
        acc += mix64((static_cast<unsigned long long>(i) << 32) | w[i]);
    __shared__ unsigned long long part[256];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicAdd(out, part[0]);
}

hipError_t launch_checksum(const void* ptr, size_t bytes, unsigned long long* out, hipStream_t s) {
    const long long n = static_cast<long long>(bytes / 4);
    const unsigned grd = static_cast<unsigned>(std::max<long long>(1, std::min<long long>((n + 255) / 256, 2048)));
    k_checksum<<<grd, 256, 0, s>>>(static_cast<const uint32_t*>(ptr), n, out);
    return hipGetLastError();
}

}  // namespace acmmp
