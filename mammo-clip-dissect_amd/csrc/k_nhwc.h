// k_nhwc.h -- what the channels-last (NHWC) tower kernels share: k_mbconv.hip (K12-K15, K0n), k_resnet.hip (K16-K19) and
// k_clip_rn.hip (K20, K21).  Internal to those three files; mcd_common.h is for all kernels.
#pragma once
#include "mcd_common.h"

namespace {

// Every kernel addresses an image from a 64-bit base with 32-bit offsets inside it, and puts the image on gridDim.y / .z
constexpr int64_t kImageLimit = (int64_t)1 << 31;   // bytes of one image's tensor
constexpr int64_t kBatchLimit = 65535;              // images of one call

__device__ __forceinline__ float relu1(float v) { return v < 0.f ? 0.f : v; }      // keeps a NaN, like ATen's
__device__ __forceinline__ float4 relu4(float4 v) { return make_float4(relu1(v.x), relu1(v.y), relu1(v.z), relu1(v.w)); }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 fma4(float4 a, float4 b, float4 c) {
    return make_float4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w));
}

// blocks of a grid-stride kernel: ceil(n / per_block), at least 1, at most cap
inline unsigned grid_for(int64_t n, int64_t per_block, int64_t cap) {
    const int64_t g = mcd_cdiv(n, per_block);
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// every pointer can be read or written as float4 (NULL, an optional operand left out, passes)
template <class... P>
inline bool aligned16(const P*... p) { return ((((uintptr_t)p) % 16 == 0) && ...); }

// the byte ranges [a, a + abytes) and [b, b + bbytes) share a byte
inline bool overlaps(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

}  // namespace
