// k_mbconv.hip -- K12 / K13 / K14 / K15 / K0n: the EfficientNet-B5 image tower's inference route on channels-last (NHWC)
// activations with batch norm folded into the weights (encoder-side, HBM-bound).  The 1x1 convolutions around these
// kernels (expand, project, head) are GEMMs on libmcd_blaslt.so; everything else of a block is here.
//   replaces  _conv_stem + _bn0 + swish, the MBConv body (_depthwise_conv + _bn1 + swish, the squeeze-excite branch and
//             its sigmoid scale), head swish + average pooling   model/modules/efficientnet_custom.py:109-119, :241, :257,
//             :273, :301 -- and the forward hook's pooling of a channels-last block output (concept_vit/utils.py:37-47).
// Every kernel addresses one image from a 64-bit base with 32-bit offsets inside it (the entries refuse an image of 2^31
// bytes or more), uses no atomics and no data of other images: an image's bits do not depend on its batch.
#include "k_nhwc.h"

namespace {

// SiLU and sigmoid with the accurate expf (no fast-math exp), as ATen computes them: x / (1 + exp(-x)), 1 / (1 + exp(-x))
__device__ __forceinline__ float silu(float v) { return v / (1.0f + expf(-v)); }
__device__ __forceinline__ float4 silu4(float4 v) { return make_float4(silu(v.x), silu(v.y), silu(v.z), silu(v.w)); }

// TF-SAME padding of _SameConv (concept_vit/data_utils.py): the total pad max((ceil(n/s)-1)*s + k - n, 0), its smaller
// half in front (top / left), the rest behind
inline int same_pad_front(int64_t n, int k, int s) {
    const int64_t o = (n + s - 1) / s;
    const int64_t p = (o - 1) * s + k - n;
    return p > 0 ? (int)(p / 2) : 0;
}

// ---- K12: stem ----------------------------------------------------------------------------------------------------
// One thread per (output pixel, 4 output channels): 9 * Cin taps from the NCHW image (neighbouring threads share them:
// L1 broadcast), the tap-major weight as float4, one 16-byte store into the NHWC output (the bytes that bound it).
__global__ __launch_bounds__(256) void conv_stem_kernel(const float* __restrict__ x, int Cin, int H, int W,
                                                         const float* __restrict__ w, const float* __restrict__ bias,
                                                         int Cout, int Ho, int Wo, int pt, int pl, float* __restrict__ y) {
    const int64_t b = blockIdx.y;
    const int nq = Cout >> 2;
    const int total = Ho * Wo * nq;
    const float* xb = x + b * Cin * H * W;
    float4* yb = reinterpret_cast<float4*>(y + b * Ho * Wo * Cout);
    const float4* w4 = reinterpret_cast<const float4*>(w);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int q = i % nq, p = i / nq;
        const int oy = p / Wo, ox = p - oy * Wo;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int ci = 0; ci < Cin; ++ci) {
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const int iy = oy * 2 - pt + dy;
                if (iy < 0 || iy >= H) continue;
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int ix = ox * 2 - pl + dx;
                    if (ix < 0 || ix >= W) continue;
                    const float v = xb[(ci * H + iy) * W + ix];
                    acc = fma4(w4[(ci * 9 + dy * 3 + dx) * nq + q], make_float4(v, v, v, v), acc);
                }
            }
        }
        yb[i] = silu4(add4(acc, reinterpret_cast<const float4*>(bias)[q]));
    }
}

// ---- K13: depthwise conv + folded BN + SiLU + SE partial sums -----------------------------------------------------
// A workgroup owns an 8 x 8 tile of output pixels and a slice of QS channel quads of one image.  It stages the tile's
// input window (halo included, zero outside the image = the TF-SAME padding) in LDS once, applying SiLU on the way in
// when x is the raw expand-GEMM output (SiLU(0) = 0, so the padding commutes).  Thread (pixel group pg, quad q) keeps
// its quad's k*k taps of the tap-major weight in registers and walks the pixels pg, pg + PG, ... of the tile; its
// running sum of the outputs, then the PG groups summed in order, is the tile's SE partial psum[b, tile, c].
constexpr int DW_TILE = 8;

template <int K, int S>
__global__ __launch_bounds__(256) void dwconv_kernel(const float* __restrict__ x, int H, int W, int C,
                                                      const float* __restrict__ w, const float* __restrict__ bias,
                                                      int pt, int pl, int silu_in, int Ho, int Wo, int QS, int ntx, int T,
                                                      float* __restrict__ y, float* __restrict__ psum) {
    extern __shared__ float4 lds[];
    constexpr int IT = (DW_TILE - 1) * S + K;      // input window edge
    const int tile = blockIdx.x, b = blockIdx.z;
    const int ty = tile / ntx, tx = tile - ty * ntx;
    const int nq = C >> 2;
    const int q0 = blockIdx.y * QS;
    const int qs = min(QS, nq - q0);
    const int iy0 = ty * DW_TILE * S - pt, ix0 = tx * DW_TILE * S - pl;
    const float4* xb = reinterpret_cast<const float4*>(x + (int64_t)b * H * W * C);
    for (int i = threadIdx.x; i < IT * IT * qs; i += 256) {
        const int q = i % qs, pix = i / qs;
        const int ly = pix / IT, lx = pix - ly * IT;
        const int iy = iy0 + ly, ix = ix0 + lx;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
            v = xb[(iy * W + ix) * nq + q0 + q];
            if (silu_in) v = silu4(v);
        }
        lds[i] = v;
    }
    __syncthreads();
    const int PG = 256 / qs;
    const int q = threadIdx.x % qs, pg = threadIdx.x / qs;
    float4 part = make_float4(0.f, 0.f, 0.f, 0.f);
    if (pg < PG) {
        float4 wr[K * K];
        const float4* wq = reinterpret_cast<const float4*>(w) + q0 + q;
#pragma unroll
        for (int t = 0; t < K * K; ++t) wr[t] = wq[t * nq];
        const float4 bq = reinterpret_cast<const float4*>(bias)[q0 + q];
        float4* yb = reinterpret_cast<float4*>(y + (int64_t)b * Ho * Wo * C);
        for (int p = pg; p < DW_TILE * DW_TILE; p += PG) {
            const int py = p / DW_TILE, px = p - py * DW_TILE;
            const int oy = ty * DW_TILE + py, ox = tx * DW_TILE + px;
            if (oy >= Ho || ox >= Wo) continue;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int dy = 0; dy < K; ++dy)
#pragma unroll
                for (int dx = 0; dx < K; ++dx)
                    acc = fma4(wr[dy * K + dx], lds[((py * S + dy) * IT + px * S + dx) * qs + q], acc);
            const float4 o = silu4(add4(acc, bq));
            yb[(oy * Wo + ox) * nq + q0 + q] = o;
            part = add4(part, o);
        }
    }
    __syncthreads();                                // the window is consumed: reuse LDS for the partial sums
    if (pg < PG) lds[pg * qs + q] = part;
    __syncthreads();
    if ((int)threadIdx.x < qs) {
        float4 s = lds[threadIdx.x];
        for (int g = 1; g < PG; ++g) s = add4(s, lds[g * qs + threadIdx.x]);
        reinterpret_cast<float4*>(psum + ((int64_t)b * T + tile) * C)[q0 + threadIdx.x] = s;
    }
}

// ---- K14: squeeze-excite gate ---------------------------------------------------------------------------------------
// One workgroup per image: the channel means from the tile partials (summed in tile order; the loads unrolled so that
// 16 are in flight per thread), the reduce GEMV (one wave per SE unit, lanes over channels, butterfly sum), SiLU, the
// expand GEMV (one thread per channel, the transposed weight [sq, C] read along the channels: coalesced), sigmoid.
__global__ __launch_bounds__(256) void se_gate_kernel(const float* __restrict__ psum, int T, int C, float hw,
                                                       const float* __restrict__ w_r, const float* __restrict__ b_r, int sq,
                                                       const float* __restrict__ w_et, const float* __restrict__ b_e,
                                                       float* __restrict__ s) {
    extern __shared__ float sm[];                   // [C] means, then [sq] reduced units
    const int64_t b = blockIdx.x;
    const float* pb = psum + b * T * C;
    for (int c = threadIdx.x; c < C; c += 256) {
        float acc = 0.f;
        int t = 0;
        for (; t + 16 <= T; t += 16) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = pb[(t + u) * C + c];
#pragma unroll
            for (int u = 0; u < 16; ++u) acc += v[u];
        }
        for (; t < T; ++t) acc += pb[t * C + c];
        sm[c] = acc / hw;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int j = wv; j < sq; j += 4) {
        float acc = 0.f;
        for (int c = lane; c < C; c += 64) acc = fmaf(w_r[(int64_t)j * C + c], sm[c], acc);
        acc = mcd_wave_sum(acc);
        if (lane == 0) sm[C + j] = silu(acc + b_r[j]);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float acc = 0.f;
        for (int j = 0; j < sq; ++j) acc = fmaf(w_et[(int64_t)j * C + c], sm[C + j], acc);
        s[b * C + c] = 1.0f / (1.0f + expf(-(acc + b_e[c])));
    }
}

// ---- K15: per-image channel scale, in place -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void channel_scale_kernel(float* __restrict__ y, int n4, int nq,
                                                             const float* __restrict__ s) {
    const int64_t b = blockIdx.y;
    float4* yb = reinterpret_cast<float4*>(y + b * n4 * 4);
    const float4* sb = reinterpret_cast<const float4*>(s + b * nq * 4);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        const float4 v = yb[i], g = sb[i % nq];
        yb[i] = make_float4(v.x * g.x, v.y * g.y, v.z * g.z, v.w * g.w);
    }
}

// ---- K0n: hook pooling of a channels-last [B, C, H, W] (memory [B, HW, C]) --------------------------------------------
// Bit-identical to K0 (k_pool.hip) on the NCHW-contiguous copy: for channel c, "lane" l here accumulates exactly what
// K0's lane l accumulates over the plane (float4 groups of 4 consecutive pixels when VEC4, else single pixels, l, l+64,
// ...), in the same order; the 64 partials are then combined in K0's xor-butterfly order (level o: partial l += partial
// l + o for l < o -- the value K0's lane l holds, fp addition and fmaxf being commutative), and a NaN anywhere in the
// plane makes the max NaN.  A wave covers 64 consecutive channels (256 contiguous bytes per pixel); the workgroup's four
// waves take the lanes l = wave, wave + 4, ...
template <bool VEC4>
__global__ __launch_bounds__(256) void pool_nhwc_kernel(const float* __restrict__ x, int C, int HW, int mode,
                                                         float* __restrict__ dst, int64_t row0, int64_t col0,
                                                         int64_t stride_n, int64_t stride_u) {
    __shared__ float ps[64][64];
    __shared__ float pm[64][64];
    __shared__ int pn[4][64];
    const int cl = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const int64_t b = blockIdx.y;
    const float* xb = x + b * HW * C;
    const bool act = mode == MCD_POOL_SILU_AVG;
    int has_nan = 0;
    for (int l = wv; l < 64; l += 4) {
        float s = 0.f, m = -INFINITY;
        if (c < C) {
            if constexpr (VEC4) {
#pragma unroll 4
                for (int i = l; i < (HW >> 2); i += 64) {
                    const float* p = xb + (4 * i) * C + c;
                    float4 v = make_float4(p[0], p[C], p[2 * C], p[3 * C]);
                    if (act) v = silu4(v);
                    s += (v.x + v.y) + (v.z + v.w);
                    m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
                    has_nan |= (v.x != v.x) | (v.y != v.y) | (v.z != v.z) | (v.w != v.w);
                }
            } else {
#pragma unroll 4
                for (int i = l; i < HW; i += 64) {
                    float v = xb[i * C + c];
                    if (act) v = silu(v);
                    s += v;
                    m = fmaxf(m, v);
                    has_nan |= (v != v);
                }
            }
        }
        ps[l][cl] = s;
        pm[l][cl] = m;
    }
    pn[wv][cl] = has_nan;
    __syncthreads();
    if (wv == 0 && c < C) {
        for (int o = 32; o > 0; o >>= 1)
            for (int l = 0; l < o; ++l) {
                ps[l][cl] = ps[l][cl] + ps[l + o][cl];
                pm[l][cl] = fmaxf(pm[l][cl], pm[l + o][cl]);
            }
        float r;
        if (mode == MCD_POOL_MAX)
            r = (pn[0][cl] | pn[1][cl] | pn[2][cl] | pn[3][cl]) ? __uint_as_float(0x7fc00000u) : pm[0][cl];
        else
            r = ps[0][cl] / (float)HW;
        dst[(row0 + b) * stride_n + (col0 + c) * stride_u] = r;
    }
}

}  // namespace

extern "C" int mcd_conv_stem_nhwc(const float* x, int64_t B, int64_t Cin, int64_t H, int64_t W, const float* w,
                                  const float* bias, int64_t Cout, float* y, mcd_stream_t stream) {
    MCD_REQUIRE(x && w && bias && y, MCD_E_ARG, "mcd_conv_stem_nhwc: NULL pointer");
    MCD_REQUIRE(B >= 0 && Cin >= 1 && Cin <= 4 && H >= 1 && W >= 1 && Cout >= 4 && Cout % 4 == 0, MCD_E_ARG,
                "mcd_conv_stem_nhwc: bad shape B=%lld Cin=%lld H=%lld W=%lld Cout=%lld (Cin <= 4, Cout %% 4 == 0)",
                (long long)B, (long long)Cin, (long long)H, (long long)W, (long long)Cout);
    MCD_REQUIRE(aligned16(w, bias, y), MCD_E_ARG, "mcd_conv_stem_nhwc: w, bias and y must be 16-byte aligned");
    const int64_t Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    MCD_REQUIRE(Cin * H * W * 4 < kImageLimit && Ho * Wo * Cout * 4 < kImageLimit && B <= kBatchLimit, MCD_E_UNSUPPORTED,
                "mcd_conv_stem_nhwc: one image's tensor reaches 2^31 bytes, or B > 65535");
    if (B == 0) return MCD_OK;
    const int pt = same_pad_front(H, 3, 2), pl = same_pad_front(W, 3, 2);
    hipLaunchKernelGGL(conv_stem_kernel, dim3(grid_for(Ho * Wo * (Cout / 4), 256, 2048), (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, x, (int)Cin, (int)H, (int)W, w, bias, (int)Cout, (int)Ho, (int)Wo, pt, pl, y);
    MCD_LAUNCH_CHECK("conv_stem_kernel");
    return MCD_OK;
}

extern "C" int mcd_dwconv_bn_silu(const float* x, int64_t B, int64_t H, int64_t W, int64_t C, const float* w,
                                  const float* bias, int k, int stride, int silu_in, float* y, float* psum, int64_t T,
                                  mcd_stream_t stream) {
    MCD_REQUIRE(x && w && bias && y && psum, MCD_E_ARG, "mcd_dwconv_bn_silu: NULL pointer");
    MCD_REQUIRE(B >= 0 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0, MCD_E_ARG,
                "mcd_dwconv_bn_silu: bad shape B=%lld H=%lld W=%lld C=%lld (C %% 4 == 0)", (long long)B, (long long)H,
                (long long)W, (long long)C);
    MCD_REQUIRE((k == 3 || k == 5) && (stride == 1 || stride == 2), MCD_E_UNSUPPORTED,
                "mcd_dwconv_bn_silu: k=%d stride=%d (k in {3, 5}, stride in {1, 2})", k, stride);
    MCD_REQUIRE(aligned16(x, w, bias, y, psum), MCD_E_ARG, "mcd_dwconv_bn_silu: pointers must be 16-byte aligned");
    const int64_t Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
    const int64_t ntx = mcd_cdiv(Wo, DW_TILE), nty = mcd_cdiv(Ho, DW_TILE);
    MCD_REQUIRE(T == ntx * nty, MCD_E_ARG, "mcd_dwconv_bn_silu: T=%lld, the %lld x %lld output has %lld tiles of 8 x 8",
                (long long)T, (long long)Ho, (long long)Wo, (long long)(ntx * nty));
    MCD_REQUIRE(H * W * C * 4 < kImageLimit && T * C * 4 < kImageLimit && B <= kBatchLimit && T < (1LL << 31),
                MCD_E_UNSUPPORTED, "mcd_dwconv_bn_silu: one image's tensor reaches 2^31 bytes, or B > 65535");
    if (B == 0) return MCD_OK;
    const int nq = (int)(C / 4);
    const int it = (DW_TILE - 1) * stride + k;
    int qmax = 40960 / (it * it * 16);              // input window <= 40 KB of LDS
    qmax = qmax < 1 ? 1 : (qmax > 16 ? 16 : qmax);
    const int nslices = (int)mcd_cdiv(nq, qmax);
    const int QS = (int)mcd_cdiv(nq, nslices);
    const size_t lds = (size_t)16 * (it * it * QS > 256 ? it * it * QS : 256);
    const int pt = same_pad_front(H, k, stride), pl = same_pad_front(W, k, stride);
    const dim3 grid((unsigned)T, (unsigned)nslices, (unsigned)B);
#define MCD_DW(KK, SS)                                                                                                    \
    hipLaunchKernelGGL((dwconv_kernel<KK, SS>), grid, dim3(256), lds, (hipStream_t)stream, x, (int)H, (int)W, (int)C, w, \
                       bias, pt, pl, silu_in ? 1 : 0, (int)Ho, (int)Wo, QS, (int)ntx, (int)T, y, psum)
    if (k == 3 && stride == 1) MCD_DW(3, 1);
    else if (k == 3) MCD_DW(3, 2);
    else if (stride == 1) MCD_DW(5, 1);
    else MCD_DW(5, 2);
#undef MCD_DW
    MCD_LAUNCH_CHECK("dwconv_kernel");
    return MCD_OK;
}

extern "C" int mcd_se_gate(const float* psum, int64_t B, int64_t T, int64_t C, int64_t HW, const float* w_r,
                           const float* b_r, int64_t sq, const float* w_et, const float* b_e, float* s, mcd_stream_t stream) {
    MCD_REQUIRE(psum && w_r && b_r && w_et && b_e && s, MCD_E_ARG, "mcd_se_gate: NULL pointer");
    MCD_REQUIRE(B >= 0 && T >= 1 && C >= 4 && C % 4 == 0 && HW >= 1 && sq >= 1, MCD_E_ARG,
                "mcd_se_gate: bad shape B=%lld T=%lld C=%lld HW=%lld sq=%lld (C %% 4 == 0)", (long long)B, (long long)T,
                (long long)C, (long long)HW, (long long)sq);
    MCD_REQUIRE(C + sq <= 16384 && T * C * 4 < kImageLimit && sq * C * 4 < kImageLimit, MCD_E_UNSUPPORTED,
                "mcd_se_gate: C + sq = %lld > 16384 or a tensor past 2^31 bytes", (long long)(C + sq));
    if (B == 0) return MCD_OK;
    hipLaunchKernelGGL(se_gate_kernel, dim3((unsigned)B), dim3(256), (size_t)(C + sq) * 4, (hipStream_t)stream, psum,
                       (int)T, (int)C, (float)HW, w_r, b_r, (int)sq, w_et, b_e, s);
    MCD_LAUNCH_CHECK("se_gate_kernel");
    return MCD_OK;
}

extern "C" int mcd_channel_scale(float* y, int64_t B, int64_t HW, int64_t C, const float* s, mcd_stream_t stream) {
    MCD_REQUIRE(y && s, MCD_E_ARG, "mcd_channel_scale: NULL pointer");
    MCD_REQUIRE(B >= 0 && HW >= 1 && C >= 4 && C % 4 == 0, MCD_E_ARG,
                "mcd_channel_scale: bad shape B=%lld HW=%lld C=%lld (C %% 4 == 0)", (long long)B, (long long)HW, (long long)C);
    MCD_REQUIRE(aligned16(y, s), MCD_E_ARG, "mcd_channel_scale: pointers must be 16-byte aligned");
    MCD_REQUIRE(HW * C * 4 < kImageLimit && B <= kBatchLimit, MCD_E_UNSUPPORTED,
                "mcd_channel_scale: one image's tensor reaches 2^31 bytes, or B > 65535");
    if (B == 0) return MCD_OK;
    const int64_t n4 = HW * C / 4;
    hipLaunchKernelGGL(channel_scale_kernel, dim3(grid_for(n4, 256 * 4, 1024), (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, y, (int)n4, (int)(C / 4), s);
    MCD_LAUNCH_CHECK("channel_scale_kernel");
    return MCD_OK;
}

extern "C" int mcd_hook_pool_nhwc(const float* x, int64_t B, int64_t C, int64_t HW, int mode, float* dst, int64_t row0,
                                  int64_t col0, int64_t stride_n, int64_t stride_u, mcd_stream_t stream) {
    MCD_REQUIRE(x && dst, MCD_E_ARG, "mcd_hook_pool_nhwc: NULL pointer");
    MCD_REQUIRE(B >= 0 && C > 0 && HW > 0 && row0 >= 0 && col0 >= 0, MCD_E_ARG, "mcd_hook_pool_nhwc: bad shape");
    MCD_REQUIRE(mode == MCD_POOL_AVG || mode == MCD_POOL_MAX || mode == MCD_POOL_SILU_AVG, MCD_E_ARG,
                "mcd_hook_pool_nhwc: bad mode %d (avg, max or silu_avg)", mode);
    MCD_REQUIRE(HW * C * 4 < kImageLimit && B <= kBatchLimit, MCD_E_UNSUPPORTED,
                "mcd_hook_pool_nhwc: one image's tensor reaches 2^31 bytes, or B > 65535");
    if (B == 0) return MCD_OK;
    const dim3 grid((unsigned)mcd_cdiv(C, 64), (unsigned)B);
    if (HW % 4 == 0)      // K0's float4 grouping (its copy is always 16-byte aligned)
        hipLaunchKernelGGL(pool_nhwc_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, (int)C, (int)HW, mode, dst,
                           row0, col0, stride_n, stride_u);
    else
        hipLaunchKernelGGL(pool_nhwc_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, (int)C, (int)HW, mode, dst,
                           row0, col0, stride_n, stride_u);
    MCD_LAUNCH_CHECK("pool_nhwc_kernel");
    return MCD_OK;
}
