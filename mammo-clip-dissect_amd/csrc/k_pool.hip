// k_pool.hip -- K0: forward-hook pooling written straight into the activation matrix (HBM-bound).
//   replaces get_activation() hook bodies, concept_vit/utils.py:27-52 (og_utils.py:31-56,
//   CLIP_og_utils.py:13-36): 4-D -> mean/amax over H,W; 3-D -> token 0; 2-D -> as is,
//   and the list-append + torch.cat that follows (utils.py:143).
// One wave per (image, channel) plane: lanes stride over the H*W plane (coalesced), butterfly
// reduction, one store into dst[(row0+b)*stride_n + (col0+ch)*stride_u].
// ROWS (mcd_hook_pool_rows, include/mcd_cache.h): the same value also goes to rows[b*width + ch], the [B, U_layer] layout of
// the layer's activation-cache file, so that no transposing pass over the activation matrix is needed at the end.
#include "mcd_common.h"
#include "../../include/mcd_cache.h"

namespace {

template <bool VEC4, bool ROWS>
__global__ __launch_bounds__(256) void pool_plane_kernel(const float* __restrict__ x, int64_t planes, int64_t Cout,
                                                          int64_t HW, int mode, float* __restrict__ dst, int64_t row0,
                                                          int64_t col0, int64_t stride_n, int64_t stride_u,
                                                          float* __restrict__ rows, int64_t width) {
    const int lane = threadIdx.x & 63;
    const int64_t plane = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (plane >= planes) return;
    const float* src = x + plane * HW;
    float s = 0.f, m = -INFINITY;
    bool has_nan = false;   // output.amax(dim=[2,3]) propagates NaN (utils.py:44-52); fmaxf alone would drop it
    if constexpr (VEC4) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        const int64_t n4 = HW >> 2;
        for (int64_t i = lane; i < n4; i += 64) {
            const float4 v = s4[i];
            s += (v.x + v.y) + (v.z + v.w);
            m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
            has_nan |= (v.x != v.x) | (v.y != v.y) | (v.z != v.z) | (v.w != v.w);
        }
    } else {
        for (int64_t i = lane; i < HW; i += 64) {
            const float v = src[i];
            s += v;
            m = fmaxf(m, v);
            has_nan |= (v != v);
        }
    }
    s = mcd_wave_sum(s);
    m = mcd_wave_max(m);
    if (__ballot(has_nan)) m = __uint_as_float(0x7fc00000u);
    if (lane == 0) {
        const int64_t b = plane / Cout, ch = plane - b * Cout;
        const float v = (mode == MCD_POOL_AVG) ? s / (float)HW : m;
        dst[(row0 + b) * stride_n + (col0 + ch) * stride_u] = v;
        if constexpr (ROWS) rows[b * width + ch] = v;
    }
}

// CLS / NONE: element (b, f) = x[b*T*F + f].  The load and the rows store are coalesced (f runs with the lane).
template <bool ROWS>
__global__ __launch_bounds__(256) void pool_copy_kernel(const float* __restrict__ x, int64_t B, int64_t F,
                                                         int64_t bstride, float* __restrict__ dst, int64_t row0,
                                                         int64_t col0, int64_t stride_n, int64_t stride_u,
                                                         float* __restrict__ rows, int64_t width) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B * F) return;
    const int64_t b = i / F, f = i - b * F;
    const float v = x[b * bstride + f];
    dst[(row0 + b) * stride_n + (col0 + f) * stride_u] = v;
    if constexpr (ROWS) rows[b * width + f] = v;
}

template <bool ROWS>
int hook_pool(const char* who, const float* x, int64_t B, int64_t Cout, int64_t HW, int mode, float* dst, int64_t row0,
              int64_t col0, int64_t stride_n, int64_t stride_u, float* rows, int64_t width, mcd_stream_t stream) {
    MCD_REQUIRE(x && dst, MCD_E_ARG, "%s: NULL pointer", who);
    MCD_REQUIRE(B >= 0 && Cout > 0 && HW > 0 && row0 >= 0 && col0 >= 0, MCD_E_ARG, "%s: bad shape", who);
    MCD_REQUIRE(mode >= MCD_POOL_AVG && mode <= MCD_POOL_NONE, MCD_E_ARG, "%s: bad mode %d", who, mode);
    if (ROWS) MCD_REQUIRE(rows && width >= Cout, MCD_E_ARG, "%s: rows is NULL or width %lld < Cout", who, (long long)width);
    if (B == 0) return MCD_OK;
    hipStream_t st = (hipStream_t)stream;
    if (mode == MCD_POOL_AVG || mode == MCD_POOL_MAX) {
        const int64_t planes = B * Cout;
        const unsigned grid = (unsigned)mcd_cdiv(planes, 4);
        const bool vec4 = (HW % 4 == 0) && (((uintptr_t)x) % 16 == 0);
        if (vec4)
            hipLaunchKernelGGL((pool_plane_kernel<true, ROWS>), dim3(grid), dim3(256), 0, st, x, planes, Cout, HW, mode, dst,
                               row0, col0, stride_n, stride_u, rows, width);
        else
            hipLaunchKernelGGL((pool_plane_kernel<false, ROWS>), dim3(grid), dim3(256), 0, st, x, planes, Cout, HW, mode, dst,
                               row0, col0, stride_n, stride_u, rows, width);
        MCD_LAUNCH_CHECK("pool_plane_kernel");
    } else {
        const int64_t bstride = (mode == MCD_POOL_CLS) ? HW * Cout : Cout;  // [B,T,F] token 0, or [B,F]
        const unsigned grid = (unsigned)mcd_cdiv(B * Cout, 256);
        hipLaunchKernelGGL(pool_copy_kernel<ROWS>, dim3(grid), dim3(256), 0, st, x, B, Cout, bstride, dst, row0, col0,
                           stride_n, stride_u, rows, width);
        MCD_LAUNCH_CHECK("pool_copy_kernel");
    }
    return MCD_OK;
}

}  // namespace

extern "C" int mcd_hook_pool(const float* x, int64_t B, int64_t Cout, int64_t HW, int mode, float* dst, int64_t row0,
                             int64_t col0, int64_t stride_n, int64_t stride_u, mcd_stream_t stream) {
    return hook_pool<false>("mcd_hook_pool", x, B, Cout, HW, mode, dst, row0, col0, stride_n, stride_u, nullptr, 0, stream);
}

extern "C" int mcd_hook_pool_rows(const float* x, int64_t B, int64_t Cout, int64_t HW, int mode, float* dst, int64_t row0,
                                  int64_t col0, int64_t stride_n, int64_t stride_u, float* rows, int64_t width,
                                  mcd_stream_t stream) {
    return hook_pool<true>("mcd_hook_pool_rows", x, B, Cout, HW, mode, dst, row0, col0, stride_n, stride_u, rows, width, stream);
}
