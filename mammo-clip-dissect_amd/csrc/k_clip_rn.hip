// k_clip_rn.hip -- K20 / K21: the pieces of OpenAI-CLIP's anti-aliased ResNet (RN50 / RN101 dissectors) that the ResNet
// kernels of k_resnet.hip do not cover: the 2x2 average pooling it uses in place of every strided convolution and of the
// max pooling, and the token sequence of its attention-pooling head.  Its 3x3 / 2 image stem is K19, an instantiation of
// the stem kernel in k_resnet.hip; the 3x3 / 1 convolutions are K18, the 1x1 convolutions and the projections GEMMs on
// libmcd_blaslt.so, the attention itself K9C.
//   replaces  ModifiedResNet's avgpool, Bottleneck.avgpool / downsample."-1" and the first three lines of
//             AttentionPool2d.forward                                concept_vit/clip/model.py:113, :23, :35, :67-69
// The rules of K16-K19: fp32, no atomics, no split reduction, one fixed order per output element (an image's bits depend
// neither on the batch it is in nor on its place in it), an image addressed from a 64-bit base with 32-bit offsets inside
// it (the entries refuse an image of 2^31 bytes or more), no environment variable read.
#include "k_nhwc.h"

namespace {

// ---- K20: 2x2 average pooling, stride 2 ---------------------------------------------------------------------------------
// One thread per (output pixel, channel quad): four 16-byte loads, one 16-byte store.  The order
// (((x00 + x01) + x10) + x11) * 0.25f is ATen's (avg_pool2d in either memory format): the same bits.  An odd trailing row
// or column is dropped.
__device__ __forceinline__ float avg4(float a, float b, float c, float d) { return (((a + b) + c) + d) * 0.25f; }

__global__ __launch_bounds__(256) void avgpool2_kernel(const float* __restrict__ x, int W, int C, int Ho, int Wo,
                                                        int64_t in_img, float* __restrict__ y) {
    const int64_t b = blockIdx.y;
    const int nq = C >> 2;
    const int total = Ho * Wo * nq;
    const float4* xb = reinterpret_cast<const float4*>(x + b * in_img);
    float4* yb = reinterpret_cast<float4*>(y + b * Ho * Wo * C);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int q = i % nq, p = i / nq;
        const int oy = p / Wo, ox = p - oy * Wo;
        const int i00 = (2 * oy * W + 2 * ox) * nq + q;
        const float4 a = xb[i00], c = xb[i00 + nq], d = xb[i00 + W * nq], e = xb[i00 + W * nq + nq];
        yb[i] = make_float4(avg4(a.x, c.x, d.x, e.x), avg4(a.y, c.y, d.y, e.y), avg4(a.z, c.z, d.z, e.z),
                            avg4(a.w, c.w, d.w, e.w));
    }
}

// ---- K21: the token sequence of the attention pool ----------------------------------------------------------------------
// tok[b, 0, :] = mean_p x[b, p, :] + pos[0], tok[b, 1 + p, :] = x[b, p, :] + pos[1 + p].  A thread owns one channel quad
// of one image and walks the pixels once (a wave reads 1 KiB of consecutive channels per pixel): the mean is one
// ascending sum over p, times 1/HW (computed once, in fp32, by the entry), the position row added last.
__global__ __launch_bounds__(64) void attnpool_tokens_kernel(const float* __restrict__ x, int HW, int C,
                                                              const float* __restrict__ pos, float inv_hw,
                                                              float* __restrict__ tok) {
    const int nq = C >> 2;
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= nq) return;
    const int64_t b = blockIdx.y;
    const float4* xb = reinterpret_cast<const float4*>(x + b * HW * C);
    const float4* pp = reinterpret_cast<const float4*>(pos);
    float4* tb = reinterpret_cast<float4*>(tok + b * (HW + 1) * C);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4                                   // four pixels' loads in flight; the sum stays one ascending chain
    for (int p = 0; p < HW; ++p) {
        const float4 v = xb[p * nq + q], e = pp[(p + 1) * nq + q];
        s = make_float4(s.x + v.x, s.y + v.y, s.z + v.z, s.w + v.w);
        tb[(p + 1) * nq + q] = make_float4(v.x + e.x, v.y + e.y, v.z + e.z, v.w + e.w);
    }
    const float4 e0 = pp[q];
    tb[q] = make_float4(s.x * inv_hw + e0.x, s.y * inv_hw + e0.y, s.z * inv_hw + e0.z, s.w * inv_hw + e0.w);
}

}  // namespace

extern "C" int mcd_avgpool2_nhwc(const float* x, int64_t B, int64_t H, int64_t W, int64_t C, float* y,
                                 mcd_stream_t stream) {
    MCD_REQUIRE(x && y, MCD_E_ARG, "mcd_avgpool2_nhwc: NULL pointer");
    MCD_REQUIRE(B >= 0 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0, MCD_E_ARG,
                "mcd_avgpool2_nhwc: bad shape B=%lld H=%lld W=%lld C=%lld (C %% 4 == 0)", (long long)B, (long long)H,
                (long long)W, (long long)C);
    MCD_REQUIRE(aligned16(x) && aligned16(y), MCD_E_ARG, "mcd_avgpool2_nhwc: pointers must be 16-byte aligned");
    MCD_REQUIRE(H * W * C * 4 < kImageLimit && B <= kBatchLimit, MCD_E_UNSUPPORTED,
                "mcd_avgpool2_nhwc: one image's tensor reaches 2^31 bytes, or B > 65535");
    const int64_t Ho = H / 2, Wo = W / 2;
    if (B == 0 || Ho == 0 || Wo == 0) return MCD_OK;      // a one-pixel-wide image pools to an empty output: nothing to write
    MCD_REQUIRE(!overlaps(x, B * H * W * C * 4, y, B * Ho * Wo * C * 4), MCD_E_ARG, "mcd_avgpool2_nhwc: x overlaps y");
    hipLaunchKernelGGL(avgpool2_kernel, dim3(grid_for(Ho * Wo * (C / 4), 256, 4096), (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, x, (int)W, (int)C, (int)Ho, (int)Wo, H * W * C, y);
    MCD_LAUNCH_CHECK("avgpool2_kernel");
    return MCD_OK;
}

extern "C" int mcd_attnpool_tokens(const float* x, int64_t B, int64_t HW, int64_t C, const float* pos, float* tok,
                                   mcd_stream_t stream) {
    MCD_REQUIRE(x && pos && tok, MCD_E_ARG, "mcd_attnpool_tokens: NULL pointer");
    MCD_REQUIRE(B >= 0 && HW >= 1 && C >= 4 && C % 4 == 0, MCD_E_ARG,
                "mcd_attnpool_tokens: bad shape B=%lld HW=%lld C=%lld (C %% 4 == 0)", (long long)B, (long long)HW,
                (long long)C);
    MCD_REQUIRE(aligned16(x) && aligned16(pos) && aligned16(tok), MCD_E_ARG,
                "mcd_attnpool_tokens: pointers must be 16-byte aligned");
    MCD_REQUIRE(HW < ((int64_t)1 << 31) && (HW + 1) * C * 4 < kImageLimit && B <= kBatchLimit, MCD_E_UNSUPPORTED,
                "mcd_attnpool_tokens: one image's tokens reach 2^31 bytes, or B > 65535");
    if (B == 0) return MCD_OK;
    const int64_t out_bytes = B * (HW + 1) * C * 4;
    MCD_REQUIRE(!overlaps(x, B * HW * C * 4, tok, out_bytes) && !overlaps(pos, (HW + 1) * C * 4, tok, out_bytes), MCD_E_ARG,
                "mcd_attnpool_tokens: x or pos overlaps tok");
    const float inv_hw = 1.0f / (float)HW;
    hipLaunchKernelGGL(attnpool_tokens_kernel, dim3((unsigned)mcd_cdiv(C / 4, 64), (unsigned)B), dim3(64), 0,
                       (hipStream_t)stream, x, (int)HW, (int)C, pos, inv_hw, tok);
    MCD_LAUNCH_CHECK("attnpool_tokens_kernel");
    return MCD_OK;
}
