// k_swin.hip -- K31 (include/mcd_swin.h): attention inside Swin's shifted windows on the fused q|k|v projection's output.
//   replaces  SwinLayer.forward between layernorm_before and the output projection (transformers modeling_swin.py):
//             F.pad, torch.roll, window_partition (view / permute / contiguous), three transpose_for_scores, bmm, the
//             gathered [heads, w^2, w^2] bias add, the [nW, w^2, w^2] mask add, softmax, bmm, window_reverse, torch.roll
//             back and the crop -- about a dozen passes over the activations.
// The op moves 4 x 128 bytes per token and head (q, k, v in, the head's output out) for 2 x w^2 x 32 multiply-adds: it is
// bound by memory, so everything that only renames positions is index arithmetic on the way in and out.
// One wave owns one (window, head, image): grid (windows, heads, B), 64 threads.
//   * K and V of the window's w^2 tokens are staged in LDS with 16-byte loads, eight lanes per token, so one wave
//     instruction reads eight whole 128-byte rows; the head's column of the bias table, (2w-1)^2 values times log2(e),
//     and the tokens' mask regions go beside them.  A padded token's rows come from pad_qkv.
//   * lane = query token (in-window order).  Its q lives in 32 registers, scaled by log2(e)/sqrt(32).
//   * keys are visited one window row (w keys) at a time: w scores from LDS broadcast reads of K (every lane reads the same
//     address), the bias by in-window distance, the mask by region, a running maximum, exp2 in the log2 domain as K9 does,
//     then P.V from broadcast reads of V.  The order is fixed: the bits of a window do not depend on where it is.
//   * the lane stores its 128 bytes at the token's original position; lanes of padded tokens store nothing.
// w is a template parameter (1 .. 8): the divisions by w and the w-key group unroll at compile time.
#include "mcd_common.h"
#include "../../include/mcd_swin.h"

namespace {

constexpr float SW_LOG2E = 1.44269504088896340736f;
constexpr float SW_QSCALE = 0.17677669529663688110f * 1.44269504088896340736f;      // log2(e) / sqrt(32)
constexpr float SW_MASK = -100.0f * 1.44269504088896340736f;                         // transformers' -100, log2 domain

template <int W>
__global__ __launch_bounds__(64) void window_attention_kernel(const float* __restrict__ qkv, const float* __restrict__ pad_qkv,
                                                              const float* __restrict__ table, int H, int Wd, int s, int heads,
                                                              float* __restrict__ out) {
    constexpr int NT = W * W, R = 2 * W - 1, NB = R * R;
    __shared__ float4 k_s[NT * 8];
    __shared__ float4 v_s[NT * 8];
    __shared__ float bias_s[NB];
    __shared__ int reg_s[NT];
    const int lane = threadIdx.x, h = blockIdx.y;
    const int nwc = (Wd + W - 1) / W, Hp = (H + W - 1) / W * W, Wp = nwc * W;
    const int r0 = (int)(blockIdx.x / nwc) * W, c0 = (int)(blockIdx.x % nwc) * W;       // the window's corner, rolled grid
    const int tok3 = 3 * heads * 32;                                                     // floats of one token of qkv
    const float* img = qkv + (int64_t)blockIdx.z * H * Wd * tok3;                        // in-image offsets fit an int (host)

    for (int i = lane; i < NB; i += 64) bias_s[i] = table[(int64_t)i * heads + h] * SW_LOG2E;
    for (int idx = lane; idx < NT * 8; idx += 64) {
        const int t = idx >> 3, part = idx & 7;
        int y = r0 + t / W + s, x = c0 + t % W + s;
        y = y >= Hp ? y - Hp : y;
        x = x >= Wp ? x - Wp : x;
        const float* src = (y < H && x < Wd ? img + (y * Wd + x) * tok3 : pad_qkv) + h * 32 + part * 4;
        k_s[idx] = *reinterpret_cast<const float4*>(src + heads * 32);
        v_s[idx] = *reinterpret_cast<const float4*>(src + 2 * heads * 32);
    }
    // this lane's token: position, region, q
    const bool active = lane < NT;
    const int t = active ? lane : 0, ti = t / W, tj = t % W;
    const int r = r0 + ti, c = c0 + tj;
    int y = r + s, x = c + s;
    y = y >= Hp ? y - Hp : y;
    x = x >= Wp ? x - Wp : x;
    const bool real = active && y < H && x < Wd;
    const int reg = s > 0 ? 3 * ((r >= Hp - W) + (r >= Hp - s)) + (c >= Wp - W) + (c >= Wp - s) : 0;
    if (active) reg_s[lane] = reg;
    float q[32];
    {
        const float4* qp = reinterpret_cast<const float4*>((real ? img + (y * Wd + x) * tok3 : (active && pad_qkv ? pad_qkv : img))
                                                           + h * 32);
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const float4 v = qp[p];
            q[4 * p] = v.x * SW_QSCALE, q[4 * p + 1] = v.y * SW_QSCALE, q[4 * p + 2] = v.z * SW_QSCALE, q[4 * p + 3] = v.w * SW_QSCALE;
        }
    }
    __syncthreads();
    if (!real) return;                      // a padded token's row is never stored, so it is not computed either

    float acc[32];
#pragma unroll
    for (int d = 0; d < 32; ++d) acc[d] = 0.f;
    float m = -INFINITY, l = 0.f;
    const int bq = (ti + W - 1) * R + (tj + W - 1);
    for (int ki = 0; ki < W; ++ki) {
        float sc[W];
        float cm = -INFINITY;
#pragma unroll
        for (int kj = 0; kj < W; ++kj) {
            const int n = ki * W + kj;
            float a = 0.f;
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const float4 kk = k_s[n * 8 + p];
                a = fmaf(q[4 * p], kk.x, a);
                a = fmaf(q[4 * p + 1], kk.y, a);
                a = fmaf(q[4 * p + 2], kk.z, a);
                a = fmaf(q[4 * p + 3], kk.w, a);
            }
            a += bias_s[bq - (ki * R + kj)];
            if (reg_s[n] != reg) a += SW_MASK;
            sc[kj] = a;
            cm = fmaxf(cm, a);
        }
        const float mn = fmaxf(m, cm);
        const float alpha = __builtin_amdgcn_exp2f(m - mn);               // first group: 2^-inf = 0
        m = mn;
        l *= alpha;
#pragma unroll
        for (int d = 0; d < 32; ++d) acc[d] *= alpha;
#pragma unroll
        for (int kj = 0; kj < W; ++kj) {
            const int n = ki * W + kj;
            const float pj = __builtin_amdgcn_exp2f(sc[kj] - m);
            l += pj;
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const float4 vv = v_s[n * 8 + p];
                acc[4 * p] = fmaf(pj, vv.x, acc[4 * p]);
                acc[4 * p + 1] = fmaf(pj, vv.y, acc[4 * p + 1]);
                acc[4 * p + 2] = fmaf(pj, vv.z, acc[4 * p + 2]);
                acc[4 * p + 3] = fmaf(pj, vv.w, acc[4 * p + 3]);
            }
        }
    }
    const float inv = 1.0f / l;
    float4* op = reinterpret_cast<float4*>(out + ((int64_t)blockIdx.z * H * Wd + (y * Wd + x)) * (heads * 32) + h * 32);
#pragma unroll
    for (int p = 0; p < 8; ++p)
        op[p] = make_float4(acc[4 * p] * inv, acc[4 * p + 1] * inv, acc[4 * p + 2] * inv, acc[4 * p + 3] * inv);
}

}  // namespace

extern "C" int mcd_window_attention(const float* qkv, const float* pad_qkv, int64_t B, int64_t H, int64_t W, int64_t heads,
                                    int64_t w, int64_t s, const float* table, float* out, mcd_stream_t stream) {
    MCD_REQUIRE(qkv && out && table, MCD_E_ARG, "mcd_window_attention: NULL pointer");
    MCD_REQUIRE(B >= 0 && H >= 1 && W >= 1 && heads >= 1 && w >= 1, MCD_E_ARG,
                "mcd_window_attention: bad shape B=%lld H=%lld W=%lld heads=%lld w=%lld", (long long)B, (long long)H,
                (long long)W, (long long)heads, (long long)w);
    MCD_REQUIRE(w <= 8, MCD_E_UNSUPPORTED, "mcd_window_attention: window %lld holds more than 64 tokens", (long long)w);
    MCD_REQUIRE(s >= 0 && s < w, MCD_E_ARG, "mcd_window_attention: shift %lld outside [0, %lld)", (long long)s, (long long)w);
    MCD_REQUIRE(B <= 65535 && heads <= 65535, MCD_E_UNSUPPORTED, "mcd_window_attention: B=%lld or heads=%lld over 65535",
                (long long)B, (long long)heads);
    MCD_REQUIRE(H < (1 << 24) && W < (1 << 24) && H * W < (1LL << 31) && H * W * heads * 96 < (1LL << 29), MCD_E_UNSUPPORTED,
                "mcd_window_attention: one image's qkv spans 2^31 bytes or more");
    MCD_REQUIRE(pad_qkv || (H % w == 0 && W % w == 0), MCD_E_ARG,
                "mcd_window_attention: a %lldx%lld grid is padded for window %lld and pad_qkv is NULL", (long long)H,
                (long long)W, (long long)w);
    MCD_REQUIRE(((uintptr_t)qkv) % 16 == 0 && ((uintptr_t)out) % 16 == 0 && ((uintptr_t)pad_qkv) % 16 == 0 &&
                    ((uintptr_t)table) % 4 == 0,
                MCD_E_ARG, "mcd_window_attention: qkv, pad_qkv and out must be 16-byte aligned, table 4-byte aligned");
    if (B == 0) return MCD_OK;
    const dim3 grid((unsigned)(mcd_cdiv(H, w) * mcd_cdiv(W, w)), (unsigned)heads, (unsigned)B), block(64);
#define MCD_WA(WS)                                                                                                         \
    hipLaunchKernelGGL(window_attention_kernel<WS>, grid, block, 0, (hipStream_t)stream, qkv, pad_qkv, table, (int)H, (int)W, \
                       (int)s, (int)heads, out)
    switch (w) {
        case 1: MCD_WA(1); break;
        case 2: MCD_WA(2); break;
        case 3: MCD_WA(3); break;
        case 4: MCD_WA(4); break;
        case 5: MCD_WA(5); break;
        case 6: MCD_WA(6); break;
        case 7: MCD_WA(7); break;
        default: MCD_WA(8); break;
    }
#undef MCD_WA
    MCD_LAUNCH_CHECK("window_attention_kernel");
    return MCD_OK;
}
