// k_clip_rn.hip -- K19 / K20 / K21: the pieces of OpenAI-CLIP's anti-aliased ResNet (RN50 / RN101 dissectors) that the
// ResNet kernels of k_resnet.hip do not cover: its 3x3 / 2 image stem, the 2x2 average pooling it uses in place of every
// strided convolution and of the max pooling, and the token sequence of its attention-pooling head.  The 3x3 / 1
// convolutions are K18, the 1x1 convolutions and the projections GEMMs on libmcd_blaslt.so, the attention itself K9C.
//   replaces  ModifiedResNet's conv1 + bn1 + relu, avgpool, Bottleneck.avgpool / downsample."-1" and the first three
//             lines of AttentionPool2d.forward                       concept_vit/clip/model.py:107-108, :113, :23, :35, :67-69
// The rules of K16-K18: fp32, no atomics, no split reduction, one fixed order per output element (an image's bits depend
// neither on the batch it is in nor on its place in it), an image addressed from a 64-bit base with 32-bit offsets inside
// it (the entries refuse an image of 2^31 bytes or more), no environment variable read.
#include "mcd_common.h"

namespace {

constexpr int64_t kImageLimit = (int64_t)1 << 31;   // bytes of one image's tensor

__device__ __forceinline__ float relu1(float v) { return v < 0.f ? 0.f : v; }      // keeps a NaN, like ATen's

inline bool aligned16(const void* p) { return ((uintptr_t)p) % 16 == 0; }
inline bool overlaps(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

inline unsigned grid_for(int64_t n, int64_t per_block, int64_t cap) {
    const int64_t g = mcd_cdiv(n, per_block);
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// ---- K19: 3x3 / 2 stem, pad 1, folded batch norm, optional ReLU ---------------------------------------------------------
// K16's design at another kernel size: a workgroup owns a 16 x 16 tile of output pixels of one image and stages its
// 33 x 33 x Cin input window in LDS (zeros outside the image = the padding).  A thread owns one pixel and CO output
// channels at a time (32, or 4 for a width that is no multiple of 32): the weight and bias indices depend on loop
// counters only, so they come through the scalar cache and every LDS read feeds CO FMAs.  One fmaf chain from 0 over
// (channel, row, column), then + bias, then the ReLU.
constexpr int S3_TILE = 16;
constexpr int S3_WIN = (S3_TILE - 1) * 2 + 3;      // 33

template <int CO>                                  // 32 when Cout % 32 == 0, else 4
__global__ __launch_bounds__(256) void conv3x3s2_kernel(const float* __restrict__ x, int Cin, int H, int W,
                                                         const float* __restrict__ w, const float* __restrict__ bias,
                                                         int Cout, int Ho, int Wo, int ntx, int relu,
                                                         float* __restrict__ y) {
    __shared__ float win[4 * S3_WIN * S3_WIN];
    const int64_t b = blockIdx.y;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int iy0 = ty * S3_TILE * 2 - 1, ix0 = tx * S3_TILE * 2 - 1;
    const float* xb = x + b * Cin * H * W;
    for (int i = threadIdx.x; i < Cin * S3_WIN * S3_WIN; i += 256) {
        const int ci = i / (S3_WIN * S3_WIN), r = i - ci * (S3_WIN * S3_WIN);
        const int ly = r / S3_WIN, lx = r - ly * S3_WIN;
        const int iy = iy0 + ly, ix = ix0 + lx;
        win[i] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? xb[(ci * H + iy) * W + ix] : 0.f;
    }
    __syncthreads();
    const int py = threadIdx.x >> 4, px = threadIdx.x & 15;
    const int oy = ty * S3_TILE + py, ox = tx * S3_TILE + px;
    const bool live = oy < Ho && ox < Wo;
    float* yp = y + b * Ho * Wo * Cout + (live ? (oy * Wo + ox) * Cout : 0);
    for (int c0 = 0; c0 < Cout; c0 += CO) {
        float acc[CO];
#pragma unroll
        for (int j = 0; j < CO; ++j) acc[j] = 0.f;
        for (int ci = 0; ci < Cin; ++ci)
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const float* wrow = win + (ci * S3_WIN + py * 2 + dy) * S3_WIN + px * 2;
                const float* wt = w + (int64_t)((ci * 3 + dy) * 3) * Cout + c0;
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const float v = wrow[dx];
#pragma unroll
                    for (int j = 0; j < CO; ++j) acc[j] = fmaf(wt[dx * Cout + j], v, acc[j]);
                }
            }
        if (live) {
#pragma unroll
            for (int j = 0; j < CO; j += 4) {
                float4 o = make_float4(acc[j] + bias[c0 + j], acc[j + 1] + bias[c0 + j + 1], acc[j + 2] + bias[c0 + j + 2],
                                       acc[j + 3] + bias[c0 + j + 3]);
                if (relu) o = make_float4(relu1(o.x), relu1(o.y), relu1(o.z), relu1(o.w));
                *reinterpret_cast<float4*>(yp + c0 + j) = o;
            }
        }
    }
}

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

extern "C" int mcd_conv3x3s2_nhwc(const float* x, int64_t B, int64_t Cin, int64_t H, int64_t W, const float* w,
                                  const float* bias, int64_t Cout, int relu, float* y, mcd_stream_t stream) {
    MCD_REQUIRE(x && w && bias && y, MCD_E_ARG, "mcd_conv3x3s2_nhwc: NULL pointer");
    MCD_REQUIRE(B >= 0 && Cin >= 1 && Cin <= 4 && H >= 1 && W >= 1 && Cout >= 4 && Cout % 4 == 0, MCD_E_ARG,
                "mcd_conv3x3s2_nhwc: bad shape B=%lld Cin=%lld H=%lld W=%lld Cout=%lld (Cin <= 4, Cout %% 4 == 0)",
                (long long)B, (long long)Cin, (long long)H, (long long)W, (long long)Cout);
    MCD_REQUIRE(((uintptr_t)x) % 4 == 0 && aligned16(w) && aligned16(bias) && aligned16(y), MCD_E_ARG,
                "mcd_conv3x3s2_nhwc: w, bias and y must be 16-byte aligned (x: 4-byte)");
    const int64_t Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    const int64_t ntx = mcd_cdiv(Wo, S3_TILE), nty = mcd_cdiv(Ho, S3_TILE);
    MCD_REQUIRE(Cin * H * W * 4 < kImageLimit && Ho * Wo * Cout * 4 < kImageLimit && B <= 65535 &&
                    ntx * nty < ((int64_t)1 << 31), MCD_E_UNSUPPORTED,
                "mcd_conv3x3s2_nhwc: one image's tensor reaches 2^31 bytes, or B > 65535");
    const int64_t ybytes = B * Ho * Wo * Cout * 4;
    MCD_REQUIRE(B == 0 || !(overlaps(x, B * Cin * H * W * 4, y, ybytes) || overlaps(w, Cin * 9 * Cout * 4, y, ybytes) ||
                            overlaps(bias, Cout * 4, y, ybytes)), MCD_E_ARG,
                "mcd_conv3x3s2_nhwc: x, w or bias overlaps y");
    if (B == 0) return MCD_OK;
    const dim3 grid((unsigned)(ntx * nty), (unsigned)B);
    if (Cout % 32 == 0)
        hipLaunchKernelGGL(conv3x3s2_kernel<32>, grid, dim3(256), 0, (hipStream_t)stream, x, (int)Cin, (int)H, (int)W, w,
                           bias, (int)Cout, (int)Ho, (int)Wo, (int)ntx, relu ? 1 : 0, y);
    else
        hipLaunchKernelGGL(conv3x3s2_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, x, (int)Cin, (int)H, (int)W, w,
                           bias, (int)Cout, (int)Ho, (int)Wo, (int)ntx, relu ? 1 : 0, y);
    MCD_LAUNCH_CHECK("conv3x3s2_kernel");
    return MCD_OK;
}

extern "C" int mcd_avgpool2_nhwc(const float* x, int64_t B, int64_t H, int64_t W, int64_t C, float* y,
                                 mcd_stream_t stream) {
    MCD_REQUIRE(x && y, MCD_E_ARG, "mcd_avgpool2_nhwc: NULL pointer");
    MCD_REQUIRE(B >= 0 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0, MCD_E_ARG,
                "mcd_avgpool2_nhwc: bad shape B=%lld H=%lld W=%lld C=%lld (C %% 4 == 0)", (long long)B, (long long)H,
                (long long)W, (long long)C);
    MCD_REQUIRE(aligned16(x) && aligned16(y), MCD_E_ARG, "mcd_avgpool2_nhwc: pointers must be 16-byte aligned");
    MCD_REQUIRE(H * W * C * 4 < kImageLimit && B <= 65535, MCD_E_UNSUPPORTED,
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
    MCD_REQUIRE(HW < ((int64_t)1 << 31) && (HW + 1) * C * 4 < kImageLimit && B <= 65535, MCD_E_UNSUPPORTED,
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
