// k_clsfold.hip -- K30 (include/mcd_clsfold.h): m[b, h, :] = sum_t softmax_t(u[b, h, :] . n[b, t, :]) n[b, t, :], what the
// class-token row of a ViT's last block needs from the other tokens once W_k and W_v are folded out of the block
// (data_utils._block_hip): 12 scores per token and 12 weighted sums of LN1(x) per image instead of a K|V projection of every
// token.
//
// One workgroup of four waves per image, so an image's sums never depend on B or on where it lands.  n is read twice
// (B*T*D*4 bytes each; the second pass mostly out of L2 / the Infinity Cache, an image's rows are 0.6 MB at 197 x 768); the
// arithmetic is 2*H*T*D multiply-adds per image.  Plain VALU: at 2 500 x 197 x 768, 12 heads, it takes 0.70-0.80 ms
// (1.9 TB/s on one read of n) where the K|V GEMM it replaces took 7.96 ms; the fp32 MFMA form (heads
// padded to 16, u in registers instead of LDS) could take about 0.4 ms more off and was not built.
//   scores  a wave takes four token rows at a time, one per 16-lane DPP row; lane `sub` of a row holds floats
//           4 sub + 64 j .. + 3 of the token (256 contiguous bytes per row and load instruction) and multiplies them into
//           HC heads' rows of u, which lie in LDS (every DPP row reads the same addresses: broadcast).  A 4-step DPP sum
//           finishes a score; they stay in LDS, [H][T].
//   softmax one wave per head: the maximum, p = 2^(s - max) written back, the sum l kept.
//   sums    thread c owns floats 4c .. 4c + 3 of the width (a wave reads 1 KiB of a token row), walks the tokens in
//           order with four loads in flight and keeps HC heads' float4 accumulators; p is an LDS broadcast.  The division
//           by l is the last operation.
// HC (heads per pass, a template argument so that the accumulators are registers) is the largest of 16, 12, 8, 4, 2, 1 that
// divides H and whose u rows fit LDS beside the scores; H > HC repeats the two passes per group of heads.
#include "mcd_common.h"
#include "../../include/mcd_clsfold.h"

namespace {

constexpr int CF_THREADS = 256;
constexpr int CF_WAVES = CF_THREADS / 64;
constexpr int CF_LDS_BYTES = 144 * 1024;      // of the CU's 160 KiB: HC*D floats of u, H*T scores, H sums
constexpr int CF_MAX_D = 2048;
constexpr int64_t CF_MAX_B = 65535;

// x + (x of the lane that the DPP control pairs this one with, inside its 16-lane row): K9C's reduction (k_attn.hip)
template <int CTRL>
__device__ __forceinline__ float cf_dpp_add(float x) {
    return x + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true));
}

// The sum over the 16 lanes of a DPP row, in every lane of it: lane ^ 1, lane ^ 2 (quad_perm), the other quad of the half
// row (row_half_mirror), the other half (row_mirror).
__device__ __forceinline__ float cf_row_sum(float x) {
    x = cf_dpp_add<0xB1>(x);
    x = cf_dpp_add<0x4E>(x);
    x = cf_dpp_add<0x141>(x);
    return cf_dpp_add<0x140>(x);
}

__device__ __forceinline__ float cf_dot4(float4 a, float4 b, float s) {
    return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, s))));
}

template <int HC>
__global__ __launch_bounds__(CF_THREADS) void cls_token_mix_kernel(const float* __restrict__ u, int64_t u_img,
                                                                   const float* __restrict__ n, int64_t n_row, int64_t n_img,
                                                                   int T, int H, int D, float* __restrict__ m, int64_t m_img) {
    extern __shared__ __align__(16) float cf_lds[];
    float* us = cf_lds;                 // [HC][D]  the u rows of the heads in work
    float* sc = us + HC * D;            // [H][T]   scores, then p
    float* ls = sc + H * T;             // [H]      sum_t p
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int sub = lane & 15, g = lane >> 4;
    const int J = D >> 6, D4 = D >> 2;
    const float* ub = u + (int64_t)blockIdx.x * u_img;
    const float* nb = n + (int64_t)blockIdx.x * n_img;
    float* mb = m + (int64_t)blockIdx.x * m_img;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);

    // ---- scores ----------------------------------------------------------------------------------------------------------
    for (int hb = 0; hb < H; hb += HC) {
        if (hb) __syncthreads();        // the previous group's readers of us are done
        for (int i = tid; i < HC * D4; i += CF_THREADS)
            reinterpret_cast<float4*>(us)[i] = reinterpret_cast<const float4*>(ub + (int64_t)hb * D)[i];
        __syncthreads();
        for (int t0 = wave * 4; t0 < T; t0 += 4 * CF_WAVES) {       // wave-uniform: every lane meets the DPP adds
            const int t = t0 + g;
            const bool ok = t < T;
            const float* np = nb + (int64_t)(ok ? t : T - 1) * n_row + 4 * sub;   // a row past T: row T - 1 again, not stored
            float s[HC];
#pragma unroll
            for (int i = 0; i < HC; ++i) s[i] = 0.f;
            for (int j0 = 0; j0 < J; j0 += 4) {
                float4 nv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) nv[k] = j0 + k < J ? *reinterpret_cast<const float4*>(np + 64 * (j0 + k)) : zero;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (j0 + k < J) {
                        const float* up = us + 4 * sub + 64 * (j0 + k);
#pragma unroll
                        for (int i = 0; i < HC; ++i) s[i] = cf_dot4(nv[k], *reinterpret_cast<const float4*>(up + i * D), s[i]);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < HC; ++i) {
                const float r = cf_row_sum(s[i]);
                if (ok && sub == 0) sc[(hb + i) * T + t] = r;
            }
        }
    }
    __syncthreads();

    // ---- softmax over the tokens, one wave per head: p in place of s, l = sum p ---------------------------------------
    for (int h = wave; h < H; h += CF_WAVES) {
        float* row = sc + h * T;
        float mx = -INFINITY;
        for (int t = lane; t < T; t += 64) mx = fmaxf(mx, row[t]);
        mx = mcd_wave_max(mx);
        float l = 0.f;
        for (int t = lane; t < T; t += 64) {
            const float p = __builtin_amdgcn_exp2f(row[t] - mx);
            row[t] = p;
            l += p;
        }
        l = mcd_wave_sum(l);
        if (lane == 0) ls[h] = l;
    }
    __syncthreads();

    // ---- sums ------------------------------------------------------------------------------------------------------------
    for (int hb = 0; hb < H; hb += HC) {
        const float* pr = sc + hb * T;
        for (int c4 = tid; c4 < D4; c4 += CF_THREADS) {
            const float* np = nb + 4 * c4;
            float4 acc[HC];
#pragma unroll
            for (int i = 0; i < HC; ++i) acc[i] = zero;
            int t = 0;
            for (; t + 4 <= T; t += 4) {
                float4 nv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) nv[k] = *reinterpret_cast<const float4*>(np + (int64_t)(t + k) * n_row);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
#pragma unroll
                    for (int i = 0; i < HC; ++i) {
                        const float p = pr[i * T + t + k];
                        acc[i].x = fmaf(p, nv[k].x, acc[i].x);
                        acc[i].y = fmaf(p, nv[k].y, acc[i].y);
                        acc[i].z = fmaf(p, nv[k].z, acc[i].z);
                        acc[i].w = fmaf(p, nv[k].w, acc[i].w);
                    }
                }
            }
            for (; t < T; ++t) {
                const float4 v = *reinterpret_cast<const float4*>(np + (int64_t)t * n_row);
#pragma unroll
                for (int i = 0; i < HC; ++i) {
                    const float p = pr[i * T + t];
                    acc[i].x = fmaf(p, v.x, acc[i].x);
                    acc[i].y = fmaf(p, v.y, acc[i].y);
                    acc[i].z = fmaf(p, v.z, acc[i].z);
                    acc[i].w = fmaf(p, v.w, acc[i].w);
                }
            }
#pragma unroll
            for (int i = 0; i < HC; ++i) {
                const float l = ls[hb + i];
                *reinterpret_cast<float4*>(mb + (int64_t)(hb + i) * D + 4 * c4) =
                    make_float4(acc[i].x / l, acc[i].y / l, acc[i].z / l, acc[i].w / l);
            }
        }
    }
}

bool cf_shape_ok(int64_t H, int64_t D) { return H >= 1 && D >= 1 && D <= CF_MAX_D && D % (64 * H) == 0; }

size_t cf_lds_bytes(int64_t hc, int64_t T, int64_t H, int64_t D) { return (size_t)(hc * D + H * T + H) * sizeof(float); }

// heads per pass: the largest instantiated count that divides H and fits LDS beside the scores (1 fits whenever T is accepted)
int cf_heads_per_pass(int64_t T, int64_t H, int64_t D) {
    for (int hc : {16, 12, 8, 4, 2})
        if (H % hc == 0 && cf_lds_bytes(hc, T, H, D) <= (size_t)CF_LDS_BYTES) return hc;
    return 1;
}

template <int HC>
int cf_launch(const float* u, int64_t u_img, const float* n, int64_t n_row, int64_t n_img, int64_t B, int64_t T, int64_t H,
              int64_t D, float* m, int64_t m_img, hipStream_t st) {
    MCD_RESERVE_LDS_ONCE(cls_token_mix_kernel<HC>, CF_LDS_BYTES, "mcd_cls_token_mix: cannot reserve %d bytes of LDS", CF_LDS_BYTES);
    hipLaunchKernelGGL(cls_token_mix_kernel<HC>, dim3((unsigned)B), dim3(CF_THREADS), cf_lds_bytes(HC, T, H, D), st, u, u_img, n,
                       n_row, n_img, (int)T, (int)H, (int)D, m, m_img);
    MCD_LAUNCH_CHECK("cls_token_mix_kernel");
    return MCD_OK;
}

}  // namespace

extern "C" int64_t mcd_cls_token_mix_max_t(int64_t H, int64_t D) {
    if (!cf_shape_ok(H, D)) return 0;
    return (CF_LDS_BYTES / (int64_t)sizeof(float) - D - H) / H;
}

extern "C" int mcd_cls_token_mix(const float* u, int64_t u_img, const float* n, int64_t n_row, int64_t n_img, int64_t B,
                                 int64_t T, int64_t H, int64_t D, float* m, int64_t m_img, mcd_stream_t stream) {
    MCD_REQUIRE(u && n && m, MCD_E_ARG, "mcd_cls_token_mix: NULL pointer");
    MCD_REQUIRE(B >= 0 && H >= 1 && D >= 1, MCD_E_ARG, "mcd_cls_token_mix: bad shape B=%lld H=%lld D=%lld", (long long)B,
                (long long)H, (long long)D);
    MCD_REQUIRE(cf_shape_ok(H, D), MCD_E_UNSUPPORTED, "mcd_cls_token_mix: D=%lld must be a multiple of 64*H=%lld, at most %d",
                (long long)D, (long long)(64 * H), CF_MAX_D);
    MCD_REQUIRE(T >= 1 && T <= mcd_cls_token_mix_max_t(H, D), MCD_E_UNSUPPORTED,
                "mcd_cls_token_mix: T=%lld tokens, between 1 and %lld for H=%lld D=%lld", (long long)T,
                (long long)mcd_cls_token_mix_max_t(H, D), (long long)H, (long long)D);
    MCD_REQUIRE(B <= CF_MAX_B, MCD_E_UNSUPPORTED, "mcd_cls_token_mix: B=%lld images, at most %lld", (long long)B,
                (long long)CF_MAX_B);
    MCD_REQUIRE(u_img >= H * D && m_img >= H * D && n_row >= D && n_img >= D, MCD_E_ARG,
                "mcd_cls_token_mix: a stride (u_img=%lld n_row=%lld n_img=%lld m_img=%lld) is below its row: H*D=%lld, D=%lld",
                (long long)u_img, (long long)n_row, (long long)n_img, (long long)m_img, (long long)(H * D), (long long)D);
    MCD_REQUIRE(((uintptr_t)u | (uintptr_t)n | (uintptr_t)m) % 16 == 0 && (u_img | n_row | n_img | m_img) % 4 == 0, MCD_E_ARG,
                "mcd_cls_token_mix: pointers must be 16-byte aligned and strides multiples of 4 floats");
    if (B == 0) return MCD_OK;
    hipStream_t st = (hipStream_t)stream;
    switch (cf_heads_per_pass(T, H, D)) {
#define MCD_CF(HC) case HC: return cf_launch<HC>(u, u_img, n, n_row, n_img, B, T, H, D, m, m_img, st)
        MCD_CF(16);
        MCD_CF(12);
        MCD_CF(8);
        MCD_CF(4);
        MCD_CF(2);
        default: MCD_CF(1);
#undef MCD_CF
    }
}
