// camera_dev.h -- the exact camera model on the device: PixelToDir, the world point of a
// pixel at a depth, and the projection into a camera, pinhole and SPHERE.  Shared by the PatchMatch kernels
// (kernels.hip) and the fusion kernels (fusion_kernels.hip); the fast-math sample projection is not here.
#pragma once
#include "detmath.h"
#include "engine.h"

namespace acmmp {

__device__ __forceinline__ void normalize3(float& x, float& y, float& z) {
    const float inv = det_rsqrt(dot3(x, y, z, x, y, z));
    x *= inv; y *= inv; z *= inv;
}

// PixelToDir, ACMMP.cu:119-134
__device__ __forceinline__ float3 pixel_to_dir(const DevCam& c, int px, int py) {
    float3 d;
    if (c.model == kPinhole) {
        d.x = (static_cast<float>(px) - c.K[2]) / c.K[0];
        d.y = (static_cast<float>(py) - c.K[5]) / c.K[4];
        d.z = 1.f;
        normalize3(d.x, d.y, d.z);
    } else {
        const float lon = (static_cast<float>(px) - c.cx) / static_cast<float>(c.W) * 2.0f * kCudartPiF;
        const float lat = -(static_cast<float>(py) - c.cy) / static_cast<float>(c.H) * kCudartPiF;
        float sl, cl, sa, ca;
        det_sincos(lon, &sl, &cl);
        det_sincos(lat, &sa, &ca);
        d.x = ca * sl;
        d.y = -sa;
        d.z = ca * cl;
    }
    return d;
}

template <typename Cam>
__device__ __forceinline__ float3 rotate_to_world(Cam& c, float x, float y, float z) {
    float3 r;
    r.x = dot3(c.R[0], c.R[3], c.R[6], x, y, z) + c.C[0];
    r.y = dot3(c.R[1], c.R[4], c.R[7], x, y, z) + c.C[1];
    r.z = dot3(c.R[2], c.R[5], c.R[8], x, y, z) + c.C[2];
    return r;
}

// Get3DPointonWorld_cu (ACMMP.cu:565-600) at arbitrary float coordinates.
template <int MODEL>
__device__ __forceinline__ float3 world_point(const DevCam& c, float x, float y, float depth) {
    if (MODEL == kSphere) {
        const float lon = (x - c.cx) / static_cast<float>(c.W) * 2.0f * kCudartPiF;
        const float lat = -(y - c.cy) / static_cast<float>(c.H) * kCudartPiF;
        float sl, cl, sa, ca;
        det_sincos(lon, &sl, &cl);
        det_sincos(lat, &sa, &ca);
        return rotate_to_world(c, (ca * sl) * depth, (-sa) * depth, (ca * cl) * depth);
    } else {
        return rotate_to_world(c, (depth * (x - c.K[2])) * c.inv_fx, (depth * (y - c.K[5])) * c.inv_fy, depth);
    }
}

// The same at an integer reference pixel whose ray `d` is already known (SPHERE's
// camera-frame point is ray * depth exactly as Get3DPointonWorld_cu rounds it).
template <int MODEL, typename Cam>
__device__ __forceinline__ float3 world_point_ray(Cam& c, int x, int y, float depth, float4 d) {
    if (MODEL == kSphere) {
        return rotate_to_world(c, d.x * depth, d.y * depth, d.z * depth);
    } else {
        return rotate_to_world(c, (depth * (static_cast<float>(x) - c.K[2])) * c.inv_fx,
                               (depth * (static_cast<float>(y) - c.K[5])) * c.inv_fy, depth);
    }
}

// |a| vs |b| for the atan2 range reductions.  gfx950 wants one wait state between a VALU transcendental
// (v_sqrt, v_rcp, ...) and the first instruction reading its result; the compiler's hazard recognizer inserts
// it for the instructions it can see, not for inline asm.  Round 6 found an inline-asm v_max_f32 scheduled
// directly after the v_sqrt of hypot(x, z): it read a half-written register (wrong costs in lane groups 0-3 of
// every 8 in k_eval_ref's instances, found by a paired-sample loop whose schedule put the two together; the
// round-5 tree had the pair in its V = 1 k_eval_ref instances only).  So:
//   max_abs / min_abs      the builtins (general operands; never signalling NaNs, so no canonicalisation)
//   max_abs_nt / min_abs_nt inline asm, operands never a transcendental's result (the rigid transform's fmas)
//   max_abs_h / min_abs_h  inline asm behind an s_nop 0, for the hypot operand
// The asm maxima are v_max3_f32 with kMaxAbsFloor as third operand (one SGPR, no VALU more than v_max_f32): their only
// use is as the divisor of the fast SPHERE projection's atan ratio min / max, and a point ON the source camera's
// centre or vertical axis (both operands 0) would give 0 * rcp(0) = NaN there.  With the floor the ratio is 0, the
// angle 0, and the pixel the principal point's coordinate -- ProjectonCamera_cu's `d < 1e-6 -> (cx, cy)` and its
// atan2f(0, 0) = 0 (ACMMP.cu:618-631) for the exact zeros.  (tz must be +0 for that: a -0 takes sphere_pixel_fast's
// `pi - r` branch and lands half a width away.  rigid_fast's last fma cancels x + (-x), which is +0 in round to
// nearest.)  Every other operand pair is far above the floor and keeps its bits (tests/test_gpu_rigs.py's degenerate
// queries).
// The asm forms keep the scheduler's round-5 order in the fast SPHERE projections: both pairs on the builtins
// measured k_eval_nb 1.444 ms against 1.428 ms this way (profiles/r06_ab8_hazard_ab.txt).
// scripts/hazard_scan.py checks the device assembly for (transcendental, immediate reader) pairs.
__device__ __forceinline__ float max_abs(float a, float b) { return __builtin_fmaxf(fabsf(a), fabsf(b)); }
__device__ __forceinline__ float min_abs(float a, float b) { return __builtin_fminf(fabsf(a), fabsf(b)); }
constexpr float kMaxAbsFloor = 1e-30f;
__device__ __forceinline__ float max_abs_nt(float a, float b) {
    float r;
    asm("v_max3_f32 %0, |%1|, |%2|, %3" : "=v"(r) : "v"(a), "v"(b), "s"(kMaxAbsFloor));
    return r;
}
__device__ __forceinline__ float min_abs_nt(float a, float b) {
    float r;
    asm("v_min_f32_e64 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float max_abs_h(float a, float b) {
    float r;
    asm("s_nop 0\n\tv_max3_f32 %0, |%1|, |%2|, %3" : "=v"(r) : "v"(a), "v"(b), "s"(kMaxAbsFloor));
    return r;
}
__device__ __forceinline__ float min_abs_h(float a, float b) {
    float r;
    asm("s_nop 0\n\tv_min_f32_e64 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// sqrtf for the SPHERE projection: LLVM's IEEE f32 sqrt lowering (v_sqrt_f32, then the +-1 ulp
// fma fix-up) without its small-argument rescale and its +-0/inf class select.  Bit-identical to
// sqrtf for every x >= 2^-96, +inf and NaN; for smaller x the result is still < 1e-6 and the
// projection replaces it by the principal point (d < 1e-6 select), and the depth it returns is
// unused by every caller, so outputs never differ.
__device__ __forceinline__ float sqrt_proj(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const float sdn = __builtin_bit_cast(float, __builtin_bit_cast(int, s) - 1);
    const float sup = __builtin_bit_cast(float, __builtin_bit_cast(int, s) + 1);
    const float r = fmaf(-sdn, s, x) <= 0.0f ? sdn : s;
    return fmaf(-sup, s, x) > 0.0f ? sup : r;
}

// a / b for the SPHERE projection: LLVM's IEEE f32 division sequence (v_rcp_f32, one Newton step
// on the reciprocal, two residual corrections, the last one fused) without v_div_scale's exponent
// pre-scaling and v_div_fixup's special-case pass.  Bit-identical to a / b whenever |b| lies in
// [2^-125, 2^125] and |a| >= 2^-102 or a == 0 (the sign of a zero quotient may differ); the two
// projection callers (ty / d and the atan2 ratio min / max) only leave that range for a point
// closer than 2^-102 to the camera centre (replaced by the principal point) or a quotient below
// 2^-80, whose contribution to the pixel coordinate is absorbed by cx / cy.
__device__ __forceinline__ float div_proj(float a, float b) {
    float y = __builtin_amdgcn_rcpf(b);
    y = fmaf(fmaf(-b, y, 1.0f), y, y);
    float q = a * y;
    q = fmaf(fmaf(-b, q, a), y, q);
    return fmaf(fmaf(-b, q, a), y, q);
}

__device__ __forceinline__ float atan2_proj(float y, float x) {
    return det_atan2_ratio(y, x, div_proj(min_abs(x, y), max_abs(x, y)));
}

// det_asin with its large-argument square root through sqrt_proj: there z = (1 - |x|) / 2 is 0, NaN,
// negative (|x| > 1 by rounding) or >= 2^-25 (1 - |x| is exact and at least 2^-24), where sqrt_proj
// equals sqrtf bit for bit.
__device__ __forceinline__ float asin_proj(float x) {
    // straight-line: one polynomial on selected arguments (no divergent branch, so the compiler can
    // interleave the views of a chunk; r01_v25 A/B +0.5%)
    const float a = fabsf(x);
    const bool small = a <= 0.5f;
    const float zl = (1.0f - a) * 0.5f;
    const float c = det_asin_core(small ? a : sqrt_proj(zl), small ? a * a : zl);
    return copysignf(small ? c : fmaf(-2.0f, c, kPio2Hi) + kPio2Lo, x);
}

// ProjectonCamera_cu, ACMMP.cu:602-644 (Cam: DevCam in any address space)
template <int MODEL, typename Cam, bool EXACT_DEPTH = false>
__device__ __forceinline__ void project(Cam& c, float3 P, float& ox, float& oy, float& depth) {
    const float tx = dot3(c.R[0], c.R[1], c.R[2], P.x, P.y, P.z) + c.t[0];
    const float ty = dot3(c.R[3], c.R[4], c.R[5], P.x, P.y, P.z) + c.t[1];
    const float tz = dot3(c.R[6], c.R[7], c.R[8], P.x, P.y, P.z) + c.t[2];
    if (MODEL == kSphere) {
        // sqrt_proj differs from sqrtf only below 2^-96, where the point is replaced by the principal
        // point; callers that use the returned depth (fusion) ask for the IEEE square root
        const float d = EXACT_DEPTH ? sqrtf(dot3(tx, ty, tz, tx, ty, tz)) : sqrt_proj(dot3(tx, ty, tz, tx, ty, tz));
        depth = d;
        const float neg_lat = asin_proj(EXACT_DEPTH ? ty / d : div_proj(ty, d));
        const float lon = EXACT_DEPTH ? det_atan2(tx, tz) : atan2_proj(tx, tz);
        ox = fmaf(lon * kInv2Pi, c.Wf, c.cx);
        oy = fmaf(neg_lat * kInvPi, c.Hf, c.cy);
        if (d < 1e-6f) { ox = c.cx; oy = c.cy; }        // (:618-622) selected, not branched around
    } else {
        depth = tz;
        const float inv = 1.0f / tz;
        ox = dot3(c.K[0], c.K[1], c.K[2], tx, ty, tz) * inv;
        oy = dot3(c.K[3], c.K[4], c.K[5], tx, ty, tz) * inv;
    }
}

}  // namespace acmmp
