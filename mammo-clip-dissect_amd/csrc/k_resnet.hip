// k_resnet.hip -- K16 / K17 / K18 / K19: the ResNet targets' inference route on channels-last (NHWC) activations with
// batch norm folded into the weights, and the image stem of OpenAI-CLIP's ResNet, which is K16's kernel at another size.
// The stride-1 1x1 convolutions around these kernels (conv1, conv3 + skip + ReLU, the stride-1 downsample) are GEMMs on
// libmcd_blaslt.so; the stems, the pooling and every convolution whose rows are not a strided matrix (3x3, 1x1 / 2) are
// here.
//   replaces  conv1 (raw: it is a hook point), bn1 + relu + maxpool, and Bottleneck.conv2 + bn2 + relu /
//             downsample[0] + downsample[1] of the torchvision layout    concept_vit/data_utils.py:85-93 (resnet50)
//             ModifiedResNet's conv1 + bn1 + relu                        concept_vit/clip/model.py:107-108, :136-138
// ResNet's symmetric padding: out = (n + 2p - k) / s + 1 (floor).  Every kernel addresses an image from a 64-bit base
// with 32-bit offsets inside it (the entries refuse an image of 2^31 bytes or more), uses no atomics and never splits a
// reduction: each output element is one fmaf chain in a fixed order (K16, K19: channel, row, column; K18: tap, then
// channel), so an image's bits depend neither on the batch it is in nor on its place in it.
#include "k_nhwc.h"
#include "../../include/mcd_stem.h"

namespace {

// ---- K16 / K19: the KS x KS / 2 image stems, pad KS / 2 -------------------------------------------------------------
// K16 = <7, CO, false>: the ResNet stem, raw sums (conv1 is a hook point).  K19 = <3, CO, true>: CLIP's anti-aliased
// stem, + bias (the folded batch norm), then the optional ReLU.  <7, CO, true>: the stem of transformers' ResNet
// (mcd_conv7x7s2_bias_relu_nhwc, include/mcd_stem.h), K16's chain with K19's epilogue.
// A workgroup owns a 16 x 16 tile of output pixels of one image and stages its ST_WIN x ST_WIN x Cin input window (37 or
// 33 wide) in LDS (zeros outside the image = the padding).  A thread owns one pixel and CO output channels at a time (32,
// or 4 for a width that is no multiple of 32): the weight and bias indices depend on loop counters only, so they come
// through the scalar cache and every LDS read feeds CO FMAs.  One fmaf chain from 0 over (channel, row, column).
constexpr int ST_TILE = 16;

template <int KS, int CO, bool EPI>                // CO: 32 when Cout % 32 == 0, else 4
__global__ __launch_bounds__(256) void stem_conv_kernel(const float* __restrict__ x, int Cin, int H, int W,
                                                         const float* __restrict__ w, const float* __restrict__ bias,
                                                         int Cout, int Ho, int Wo, int ntx, int relu,
                                                         float* __restrict__ y) {
    constexpr int ST_WIN = (ST_TILE - 1) * 2 + KS, PAD = KS / 2;
    __shared__ float win[4 * ST_WIN * ST_WIN];
    const int64_t b = blockIdx.y;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int iy0 = ty * ST_TILE * 2 - PAD, ix0 = tx * ST_TILE * 2 - PAD;
    const float* xb = x + b * Cin * H * W;
    for (int i = threadIdx.x; i < Cin * ST_WIN * ST_WIN; i += 256) {
        const int ci = i / (ST_WIN * ST_WIN), r = i - ci * (ST_WIN * ST_WIN);
        const int ly = r / ST_WIN, lx = r - ly * ST_WIN;
        const int iy = iy0 + ly, ix = ix0 + lx;
        win[i] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? xb[(ci * H + iy) * W + ix] : 0.f;
    }
    __syncthreads();
    const int py = threadIdx.x >> 4, px = threadIdx.x & 15;
    const int oy = ty * ST_TILE + py, ox = tx * ST_TILE + px;
    const bool live = oy < Ho && ox < Wo;
    float* yp = y + b * Ho * Wo * Cout + (live ? (oy * Wo + ox) * Cout : 0);
    for (int c0 = 0; c0 < Cout; c0 += CO) {
        float acc[CO];
#pragma unroll
        for (int j = 0; j < CO; ++j) acc[j] = 0.f;
        // One window row of one channel.  A macro, so that both loops below hold the very text the two kernels had: as a
        // lambda or a __forceinline__ function the same lines compile to other registers and another schedule.
#define MCD_STEM_ROW                                                                         \
    {                                                                                        \
        const float* wrow = win + (ci * ST_WIN + py * 2 + dy) * ST_WIN + px * 2;             \
        const float* wt = w + (int64_t)((ci * KS + dy) * KS) * Cout + c0;                    \
        _Pragma("unroll") for (int dx = 0; dx < KS; ++dx) {                                  \
            const float v = wrow[dx];                                                        \
            _Pragma("unroll") for (int j = 0; j < CO; ++j) acc[j] = fmaf(wt[dx * Cout + j], v, acc[j]); \
        }                                                                                    \
    }
        // the rows of a 3 x 3 are unrolled, those of a 7 x 7 left to the compiler's heuristic (`unroll 1` is not the same)
        for (int ci = 0; ci < Cin; ++ci) {
            if constexpr (KS == 3) {
#pragma unroll
                for (int dy = 0; dy < KS; ++dy) MCD_STEM_ROW
            } else {
                for (int dy = 0; dy < KS; ++dy) MCD_STEM_ROW
            }
        }
#undef MCD_STEM_ROW
        if (live) {
#pragma unroll
            for (int j = 0; j < CO; j += 4) {
                float4 o = make_float4(acc[j], acc[j + 1], acc[j + 2], acc[j + 3]);
                if constexpr (EPI) {
                    o = add4(o, make_float4(bias[c0 + j], bias[c0 + j + 1], bias[c0 + j + 2], bias[c0 + j + 3]));
                    if (relu) o = relu4(o);
                }
                *reinterpret_cast<float4*>(yp + c0 + j) = o;
            }
        }
    }
}

// ---- K17: batch norm + ReLU + 3x3 / 2 max pooling (pad 1) ----------------------------------------------------------
// One thread per (output pixel, channel quad).  The padding never wins: the window always holds a real pixel.
__global__ __launch_bounds__(256) void bn_relu_maxpool_kernel(const float* __restrict__ x, int H, int W, int C,
                                                               const float* __restrict__ scale,
                                                               const float* __restrict__ shift, int Ho, int Wo,
                                                               float* __restrict__ y) {
    const int64_t b = blockIdx.y;
    const int nq = C >> 2;
    const int total = Ho * Wo * nq;
    const float4* xb = reinterpret_cast<const float4*>(x + b * H * W * C);
    float4* yb = reinterpret_cast<float4*>(y + b * Ho * Wo * C);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int q = i % nq, p = i / nq;
        const int oy = p / Wo, ox = p - oy * Wo;
        const float4 sc = reinterpret_cast<const float4*>(scale)[q], sh = reinterpret_cast<const float4*>(shift)[q];
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int iy = oy * 2 - 1 + dy;
            if (iy < 0 || iy >= H) continue;
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int ix = ox * 2 - 1 + dx;
                if (ix < 0 || ix >= W) continue;
                const float4 v = xb[(iy * W + ix) * nq + q];
                const float4 r = relu4(make_float4(fmaf(v.x, sc.x, sh.x), fmaf(v.y, sc.y, sh.y), fmaf(v.z, sc.z, sh.z),
                                                   fmaf(v.w, sc.w, sh.w)));
                m.x = (r.x > m.x || r.x != r.x) ? r.x : m.x;      // a NaN wins, as in ATen's max pooling
                m.y = (r.y > m.y || r.y != r.y) ? r.y : m.y;
                m.z = (r.z > m.z || r.z != r.z) ? r.z : m.z;
                m.w = (r.w > m.w || r.w != r.w) ? r.w : m.w;
            }
        }
        yb[i] = m;
    }
}

// ---- K18: implicit-GEMM convolution on the exact-fp32 MFMA ----------------------------------------------------------
//   D[cout, pixel] = sum over k = (tap, cin) of Wt[cout, k] * act_in(X[pixel's tap, cin])
// GEMM columns are the flattened output pixels B*Ho*Wo (a tile may span images), GEMM rows the output channels: the
// 32 x 32 accumulator of v_mfma_f32_32x32x2_f32 then has its pixel on the lane and four consecutive output channels in
// registers 4g .. 4g+3, which is a 16-byte NHWC store.  A workgroup (4 waves) owns IG_BP pixels x BC channels and walks k
// in steps of one tap x 32 channels; both slices are staged k-major in LDS ([32][tile + 4]: the MFMA operand reads are
// 32 consecutive floats, the staging writes hit 64 distinct banks), double-buffered with the next step's global loads
// in flight under the MFMAs.  Wave (wp, wc) owns pixels wp*64.. and channels wc*(BC/2)..: 2 x (BC/64) accumulators.
// k runs tap-major then channel in ascending order for every output element; a padded tap contributes fma(w, 0, acc).
// The order of one output element, whatever its tile, image or batch: k is cut into chunks of 256 consecutive values
// (IG_CHUNK steps); a chunk is one fmaf chain from 0 in ascending k (the MFMA's own arithmetic), the chunks' partial
// sums are added to the total in ascending order, the bias last.  One chain over all of k = 4 608 (layer4) measured
// 2.0e-6 of the output's maximum against float64, eight times ATen's error; the two-level sum keeps the rounding
// error near sqrt(256) + sqrt(18) ulps instead of sqrt(4 608) and costs 64 additions per wave and chunk.
// RES (mcd_conv_igemm_res_nhwc, a BasicBlock's conv2 + bn2 + skip + ReLU): a residual operand res [B, Ho, Wo, Cout] in the
// epilogue, y = act_out((total + bias) + res).  It is the same 16-byte NHWC piece the store writes, so a lane loads one
// float4 per store; a pixel tile's loads (4 * TC of them, under the stores' two guards) are issued together ahead of
// the adds.  Without RES the kernel is the code it was: the main loop is shared and the epilogue's extra lines are
// compiled out.
constexpr int IG_BP = 128;
constexpr int IG_BK = 32;
constexpr int IG_LDP = IG_BP + 4;
constexpr int IG_CHUNK = 8;                        // k-steps (of 32) per partial sum: 256 consecutive k

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int BC, int KS, bool RES>
__global__ __launch_bounds__(256, 2) void conv_igemm_kernel(const float* __restrict__ x, int H, int W, int Cin,
                                                          const float* __restrict__ wt, const float* __restrict__ bias,
                                                          const float* __restrict__ res, int Cout, int stride, int pad,
                                                          int Ho, int Wo, int64_t Mtot, int nct, int relu_in,
                                                          int relu_out, float* __restrict__ y) {
    constexpr int LDC = BC + 4;
    constexpr int TC = BC / 64;                     // accumulator tiles per wave along the channels
    constexpr int NW = BC / 64;                     // weight rows per thread and step
    extern __shared__ float lds[];                  // 2 x (Xs [32][IG_LDP] + Ws [32][LDC])
    constexpr int STAGE = IG_BK * (IG_LDP + LDC);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ct = blockIdx.x % nct;
    const int64_t pt = blockIdx.x / nct;
    const int c_base = ct * BC;
    const int64_t m_base = pt * IG_BP;
    const int K = KS * KS * Cin;
    const int HoWo = Ho * Wo;

    // staging role: 16 rows x 4 quads per wave and pass; rows r_lo + 16 * (2 * wv + j), quads q_lo + 4 * qh
    const int r_lo = lane & 15, q_lo = lane >> 4;
    const float* ximg[2];
    int iyb[2], ixb[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int64_t m = m_base + r_lo + 16 * (2 * wv + j);
        if (m < Mtot) {
            const int64_t b = m / HoWo;
            const int r = (int)(m - b * HoWo);
            const int oy = r / Wo, ox = r - oy * Wo;
            ximg[j] = x + b * H * W * Cin;
            iyb[j] = oy * stride - pad;
            ixb[j] = ox * stride - pad;
        } else {
            ximg[j] = x;
            iyb[j] = -(1 << 20);                    // every tap falls outside: zeros
            ixb[j] = 0;
        }
    }
    const float* wrow[NW];
    bool wlive[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const int n = c_base + r_lo + 16 * (NW * wv + j);
        wlive[j] = n < Cout;
        wrow[j] = wt + (int64_t)(wlive[j] ? n : 0) * K;
    }

    float4 xr[2][2], wr[NW][2];
    const int csteps = Cin / IG_BK;
    const int nsteps = KS * KS * csteps;

    auto load_step = [&](int s) {
        const int tap = s / csteps, c0 = (s - tap * csteps) * IG_BK;
        const int dy = tap / KS, dx = tap - dy * KS;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int iy = iyb[j] + dy, ix = ixb[j] + dx;
            const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
            const float* p = ximg[j] + (in ? (iy * W + ix) * Cin + c0 : 0);
#pragma unroll
            for (int qh = 0; qh < 2; ++qh) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (in) v = *reinterpret_cast<const float4*>(p + 4 * (q_lo + 4 * qh));
                xr[j][qh] = relu_in ? relu4(v) : v;
            }
        }
        const int k0 = tap * Cin + c0;
#pragma unroll
        for (int j = 0; j < NW; ++j)
#pragma unroll
            for (int qh = 0; qh < 2; ++qh) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (wlive[j]) v = *reinterpret_cast<const float4*>(wrow[j] + k0 + 4 * (q_lo + 4 * qh));
                wr[j][qh] = v;
            }
    };
    auto store_step = [&](int buf) {
        float* Xs = lds + buf * STAGE;
        float* Ws = Xs + IG_BK * IG_LDP;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int qh = 0; qh < 2; ++qh) {
                float* d = Xs + 4 * (q_lo + 4 * qh) * IG_LDP + r_lo + 16 * (2 * wv + j);
                d[0] = xr[j][qh].x;
                d[IG_LDP] = xr[j][qh].y;
                d[2 * IG_LDP] = xr[j][qh].z;
                d[3 * IG_LDP] = xr[j][qh].w;
            }
#pragma unroll
        for (int j = 0; j < NW; ++j)
#pragma unroll
            for (int qh = 0; qh < 2; ++qh) {
                float* d = Ws + 4 * (q_lo + 4 * qh) * LDC + r_lo + 16 * (NW * wv + j);
                d[0] = wr[j][qh].x;
                d[LDC] = wr[j][qh].y;
                d[2 * LDC] = wr[j][qh].z;
                d[3 * LDC] = wr[j][qh].w;
            }
    };

    const int wp = wv & 1, wc = wv >> 1;
    const int l31 = lane & 31, lh = lane >> 5;
    f32x16 acc[TC][2], tot[TC][2];
#pragma unroll
    for (int a = 0; a < TC; ++a)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][p][r] = tot[a][p][r] = 0.f;

    load_step(0);
    store_step(0);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        if (s + 1 < nsteps) load_step(s + 1);
        const float* Xs = lds + (s & 1) * STAGE + lh * IG_LDP + wp * 64 + l31;
        const float* Ws = lds + (s & 1) * STAGE + IG_BK * IG_LDP + lh * LDC + wc * (BC / 2) + l31;
#pragma unroll
        for (int kk = 0; kk < IG_BK / 2; ++kk) {
            float av[TC], bv[2];
#pragma unroll
            for (int a = 0; a < TC; ++a) av[a] = Ws[2 * kk * LDC + a * 32];
#pragma unroll
            for (int p = 0; p < 2; ++p) bv[p] = Xs[2 * kk * IG_LDP + p * 32];
#pragma unroll
            for (int a = 0; a < TC; ++a)
#pragma unroll
                for (int p = 0; p < 2; ++p)
                    acc[a][p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[p], acc[a][p], 0, 0, 0);
        }
        if ((s & (IG_CHUNK - 1)) == IG_CHUNK - 1 || s + 1 == nsteps) {      // close the chunk: total += partial, in k order
#pragma unroll
            for (int a = 0; a < TC; ++a)
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    tot[a][p] = tot[a][p] + acc[a][p];
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[a][p][r] = 0.f;
                }
        }
        if (s + 1 < nsteps) store_step((s + 1) & 1);
        __syncthreads();
    }

    // epilogue: lane = pixel (column), registers 4g .. 4g+3 = channels 8g + 4*lh + 0..3 of the 32-row tile
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int64_t m = m_base + wp * 64 + p * 32 + l31;
        if (m >= Mtot) continue;
        const int64_t b = m / HoWo;
        const int64_t poff = b * HoWo * Cout + (int)(m - b * HoWo) * Cout;     // the pixel's place in y, and in res
        float* yp = y + poff;
        float4 rq[RES ? TC : 1][4];
        if constexpr (RES) {                        // the pixel tile's residual pieces, all in flight before the first add
#pragma unroll
            for (int a = 0; a < TC; ++a)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int n = c_base + wc * (BC / 2) + a * 32 + 8 * g + 4 * lh;
                    rq[a][g] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (n < Cout) rq[a][g] = *reinterpret_cast<const float4*>(res + poff + n);
                }
        }
#pragma unroll
        for (int a = 0; a < TC; ++a)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = c_base + wc * (BC / 2) + a * 32 + 8 * g + 4 * lh;
                if (n >= Cout) continue;
                const float4 bq = *reinterpret_cast<const float4*>(bias + n);
                float4 o = make_float4(tot[a][p][4 * g] + bq.x, tot[a][p][4 * g + 1] + bq.y, tot[a][p][4 * g + 2] + bq.z,
                                       tot[a][p][4 * g + 3] + bq.w);
                if constexpr (RES) o = make_float4(o.x + rq[a][g].x, o.y + rq[a][g].y, o.z + rq[a][g].z, o.w + rq[a][g].w);
                if (relu_out) o = relu4(o);
                *reinterpret_cast<float4*>(yp + n) = o;
            }
    }
}

template <int BC, int KS, bool RES>
int launch_igemm(const float* x, int64_t B, int64_t H, int64_t W, int64_t Cin, const float* wt, const float* bias,
                 const float* res, int64_t Cout, int stride, int pad, int64_t Ho, int64_t Wo, int relu_in, int relu_out,
                 float* y, hipStream_t st) {
    constexpr size_t lds = (size_t)2 * IG_BK * (IG_LDP + BC + 4) * sizeof(float);
    MCD_RESERVE_LDS_ONCE((conv_igemm_kernel<BC, KS, RES>), lds, "mcd_conv_igemm_nhwc: cannot reserve %zu bytes of LDS", lds);
    const int64_t Mtot = B * Ho * Wo;
    const int64_t nct = mcd_cdiv(Cout, BC), npt = mcd_cdiv(Mtot, IG_BP);
    MCD_REQUIRE(nct * npt < ((int64_t)1 << 31), MCD_E_UNSUPPORTED, "mcd_conv_igemm_nhwc: %lld tiles exceed the grid",
                (long long)(nct * npt));
    hipLaunchKernelGGL((conv_igemm_kernel<BC, KS, RES>), dim3((unsigned)(nct * npt)), dim3(256), lds, st, x, (int)H, (int)W,
                       (int)Cin, wt, bias, res, (int)Cout, stride, pad, (int)Ho, (int)Wo, Mtot, (int)nct, relu_in ? 1 : 0,
                       relu_out ? 1 : 0, y);
    MCD_LAUNCH_CHECK("conv_igemm_kernel");
    return MCD_OK;
}

// The checks and the dispatch of the stem entries (`name` is the entry's, for the messages).  k = 7 without epi: K16, raw,
// no bias; k = 3 with epi: K19, with its epilogue; k = 7 with epi: the stem of transformers' ResNet, whose convolution,
// batch norm and ReLU are one module.
int stem_conv_entry(const char* name, int k, bool epi, const float* x, int64_t B, int64_t Cin, int64_t H, int64_t W,
                    const float* w, const float* bias, int64_t Cout, int relu, float* y, mcd_stream_t stream) {
    MCD_REQUIRE(x && w && y && (bias || !epi), MCD_E_ARG, "%s: NULL pointer", name);
    MCD_REQUIRE(B >= 0 && Cin >= 1 && Cin <= 4 && H >= 1 && W >= 1 && Cout >= 4 && Cout % 4 == 0, MCD_E_ARG,
                "%s: bad shape B=%lld Cin=%lld H=%lld W=%lld Cout=%lld (Cin <= 4, Cout %% 4 == 0)", name, (long long)B,
                (long long)Cin, (long long)H, (long long)W, (long long)Cout);
    MCD_REQUIRE((!epi || ((uintptr_t)x) % 4 == 0) && aligned16(w, bias, y), MCD_E_ARG,
                "%s: w, bias and y must be 16-byte aligned (x: 4-byte)", name);
    const int pad = k / 2;
    const int64_t Ho = (H + 2 * pad - k) / 2 + 1, Wo = (W + 2 * pad - k) / 2 + 1;
    const int64_t ntx = mcd_cdiv(Wo, ST_TILE), nty = mcd_cdiv(Ho, ST_TILE);
    MCD_REQUIRE(Cin * H * W * 4 < kImageLimit && Ho * Wo * Cout * 4 < kImageLimit && B <= kBatchLimit &&
                    ntx * nty < ((int64_t)1 << 31), MCD_E_UNSUPPORTED,
                "%s: one image's tensor reaches 2^31 bytes, or B > 65535", name);
    if (B == 0) return MCD_OK;
    const int64_t ybytes = B * Ho * Wo * Cout * 4;
    MCD_REQUIRE(!overlaps(x, B * Cin * H * W * 4, y, ybytes) && !overlaps(w, Cin * k * k * Cout * 4, y, ybytes) &&
                    !(bias && overlaps(bias, Cout * 4, y, ybytes)), MCD_E_ARG, "%s: x, w or bias overlaps y", name);
    const dim3 grid((unsigned)(ntx * nty), (unsigned)B);
#define MCD_STEM(KS, CO, EPI)                                                                                            \
    hipLaunchKernelGGL((stem_conv_kernel<KS, CO, EPI>), grid, dim3(256), 0, (hipStream_t)stream, x, (int)Cin, (int)H,   \
                       (int)W, w, bias, (int)Cout, (int)Ho, (int)Wo, (int)ntx, relu ? 1 : 0, y)
    if (k == 3) {
        if (Cout % 32 == 0) MCD_STEM(3, 32, true);
        else MCD_STEM(3, 4, true);
    } else if (epi) {
        if (Cout % 32 == 0) MCD_STEM(7, 32, true);
        else MCD_STEM(7, 4, true);
    } else {
        if (Cout % 32 == 0) MCD_STEM(7, 32, false);
        else MCD_STEM(7, 4, false);
    }
#undef MCD_STEM
    MCD_LAUNCH_CHECK("stem_conv_kernel");
    return MCD_OK;
}

}  // namespace

extern "C" int mcd_conv7x7s2_nhwc(const float* x, int64_t B, int64_t Cin, int64_t H, int64_t W, const float* w,
                                  int64_t Cout, float* y, mcd_stream_t stream) {
    return stem_conv_entry("mcd_conv7x7s2_nhwc", 7, false, x, B, Cin, H, W, w, nullptr, Cout, 0, y, stream);
}

extern "C" int mcd_conv3x3s2_nhwc(const float* x, int64_t B, int64_t Cin, int64_t H, int64_t W, const float* w,
                                  const float* bias, int64_t Cout, int relu, float* y, mcd_stream_t stream) {
    return stem_conv_entry("mcd_conv3x3s2_nhwc", 3, true, x, B, Cin, H, W, w, bias, Cout, relu, y, stream);
}

extern "C" int mcd_conv7x7s2_bias_relu_nhwc(const float* x, int64_t B, int64_t Cin, int64_t H, int64_t W, const float* w,
                                            const float* bias, int64_t Cout, int relu, float* y, mcd_stream_t stream) {
    return stem_conv_entry("mcd_conv7x7s2_bias_relu_nhwc", 7, true, x, B, Cin, H, W, w, bias, Cout, relu, y, stream);
}

extern "C" int mcd_bn_relu_maxpool_nhwc(const float* x, int64_t B, int64_t H, int64_t W, int64_t C, const float* scale,
                                        const float* shift, float* y, mcd_stream_t stream) {
    MCD_REQUIRE(x && scale && shift && y, MCD_E_ARG, "mcd_bn_relu_maxpool_nhwc: NULL pointer");
    MCD_REQUIRE(B >= 0 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0, MCD_E_ARG,
                "mcd_bn_relu_maxpool_nhwc: bad shape B=%lld H=%lld W=%lld C=%lld (C %% 4 == 0)", (long long)B,
                (long long)H, (long long)W, (long long)C);
    MCD_REQUIRE(aligned16(x, scale, shift, y), MCD_E_ARG, "mcd_bn_relu_maxpool_nhwc: pointers must be 16-byte aligned");
    MCD_REQUIRE(H * W * C * 4 < kImageLimit && B <= kBatchLimit, MCD_E_UNSUPPORTED,
                "mcd_bn_relu_maxpool_nhwc: one image's tensor reaches 2^31 bytes, or B > 65535");
    if (B == 0) return MCD_OK;
    const int64_t Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    hipLaunchKernelGGL(bn_relu_maxpool_kernel, dim3(grid_for(Ho * Wo * (C / 4), 256, 4096), (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, x, (int)H, (int)W, (int)C, scale, shift, (int)Ho, (int)Wo, y);
    MCD_LAUNCH_CHECK("bn_relu_maxpool_kernel");
    return MCD_OK;
}

namespace {

// The checks and the dispatch of both K18 entries (`name` is the entry's, for the messages).  res == NULL: the
// instantiations without a residual, whichever entry was called.
int conv_igemm_entry(const char* name, const float* x, int64_t B, int64_t H, int64_t W, int64_t Cin, const float* w,
                     const float* bias, const float* res, int64_t Cout, int k, int stride, int relu_in, int relu_out,
                     float* y, mcd_stream_t stream) {
    MCD_REQUIRE(x && w && bias && y, MCD_E_ARG, "%s: NULL pointer", name);
    MCD_REQUIRE(B >= 0 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, MCD_E_ARG,
                "%s: bad shape B=%lld H=%lld W=%lld Cin=%lld Cout=%lld", name, (long long)B, (long long)H, (long long)W,
                (long long)Cin, (long long)Cout);
    MCD_REQUIRE(((k == 3 && (stride == 1 || stride == 2)) || (k == 1 && stride == 2)) && Cin % 32 == 0 && Cout % 32 == 0,
                MCD_E_UNSUPPORTED, "%s: k=%d stride=%d Cin=%lld Cout=%lld (3x3 / 1 or 2, 1x1 / 2; Cin, Cout %% 32 == 0)",
                name, k, stride, (long long)Cin, (long long)Cout);
    MCD_REQUIRE(aligned16(x, w, bias, y, res), MCD_E_ARG, "%s: pointers must be 16-byte aligned", name);
    const int pad = k == 3 ? 1 : 0;
    const int64_t Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    MCD_REQUIRE(H * W * Cin * 4 < kImageLimit && Ho * Wo * Cout * 4 < kImageLimit && (int64_t)k * k * Cin * Cout * 4 < kImageLimit &&
                    B <= kBatchLimit, MCD_E_UNSUPPORTED,
                "%s: one image's tensor (or the weight) reaches 2^31 bytes, or B > 65535", name);
    if (res) {      // every workgroup reads its residual pieces before it stores, but another may have stored there already
        const int64_t bytes = B * Ho * Wo * Cout * 4;
        MCD_REQUIRE(res != y && !overlaps(res, bytes, y, bytes), MCD_E_ARG, "%s: res overlaps y", name);
    }
    if (B == 0) return MCD_OK;
    hipStream_t st = (hipStream_t)stream;
    const bool wide = Cout % 128 == 0;
#define MCD_IGEMM(BC, KS, RES) \
    launch_igemm<BC, KS, RES>(x, B, H, W, Cin, w, bias, res, Cout, stride, pad, Ho, Wo, relu_in, relu_out, y, st)
    if (res) {
        if (k == 3) return wide ? MCD_IGEMM(128, 3, true) : MCD_IGEMM(64, 3, true);
        return wide ? MCD_IGEMM(128, 1, true) : MCD_IGEMM(64, 1, true);
    }
    if (k == 3) return wide ? MCD_IGEMM(128, 3, false) : MCD_IGEMM(64, 3, false);
    return wide ? MCD_IGEMM(128, 1, false) : MCD_IGEMM(64, 1, false);
#undef MCD_IGEMM
}

}  // namespace

extern "C" int mcd_conv_igemm_nhwc(const float* x, int64_t B, int64_t H, int64_t W, int64_t Cin, const float* w,
                                   const float* bias, int64_t Cout, int k, int stride, int relu_in, int relu_out, float* y,
                                   mcd_stream_t stream) {
    return conv_igemm_entry("mcd_conv_igemm_nhwc", x, B, H, W, Cin, w, bias, nullptr, Cout, k, stride, relu_in, relu_out,
                            y, stream);
}

extern "C" int mcd_conv_igemm_res_nhwc(const float* x, int64_t B, int64_t H, int64_t W, int64_t Cin, const float* w,
                                       const float* bias, const float* res, int64_t Cout, int k, int stride, int relu_in,
                                       int relu_out, float* y, mcd_stream_t stream) {
    return conv_igemm_entry("mcd_conv_igemm_res_nhwc", x, B, H, W, Cin, w, bias, res, Cout, k, stride, relu_in, relu_out,
                            y, stream);
}
