// k_mask.hip -- K28 and K29 (include/mcd_mask.h): the two data movements of a masked autoencoder's forward
// (transformers ViTMAEForPreTraining, data_utils.HFMae).
//   K28 replaces  patch_embeddings over all patches + torch.gather(sequence, 1, ids_keep)    ViTMAEEmbeddings.forward
//   K29 replaces  mask_token.repeat, cat, gather over an expanded index, cat, + decoder_pos_embed   ViTMAEDecoder.forward
// Both are row gathers through a short int32 index list: one thread per 16-byte (K28 at P % 4 != 0: 8-byte) vector of the
// OUTPUT, so a wave instruction writes 1 KiB (512 B) of consecutive addresses and reads whole source rows -- pieces of
// P*4 bytes of one patch row (K28), a whole D*4-byte token row (K29).  The index of a row is read by every lane that works
// on the row: the same 4 bytes for the lanes of a wave, one cache line per 16 rows.  Nothing is reused, nothing is staged in
// LDS; the work is a few hundred KiB per call and the launch is what it costs.
// Every index is clamped before it forms an address: no read leaves the image (K28) or the source rows (K29) whatever the
// index list holds.
#include "mcd_common.h"
#include "../../include/mcd_mask.h"

namespace {

constexpr int MK_THREADS = 256;
constexpr int64_t MK_MAX_GRID = 1 << 20;

template <typename V> __device__ __forceinline__ V mask_zero();
template <> __device__ __forceinline__ float4 mask_zero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }
template <> __device__ __forceinline__ float2 mask_zero<float2>() { return make_float2(0.f, 0.f); }

// K11's index arithmetic with the patch number taken from keep.  R = 1 + Lk output rows an image.
template <typename V>
__global__ __launch_bounds__(MK_THREADS) void patchify_kept_kernel(const float* __restrict__ x,
                                                                   const int32_t* __restrict__ keep, int B, int Cin, int H,
                                                                   int W, int P, int Lk, float* __restrict__ out) {
    constexpr int N = sizeof(V) / sizeof(float);
    const int nW = W / P, nP = (H / P) * nW, F = Cin * P * P, FV = F / N, PV = P / N, R = 1 + Lk;
    const int64_t total = (int64_t)B * R * FV;
    for (int64_t i = (int64_t)blockIdx.x * MK_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * MK_THREADS) {
        const int fv = (int)(i % FV);
        const int64_t row = i / FV;
        const int r = (int)(row % R);
        const int64_t b = row / R;
        V v = mask_zero<V>();
        if (r > 0) {
            const int p = min(max(keep[b * Lk + (r - 1)], 0), nP - 1);
            const int py = p / nW, px = p % nW;
            const int dxv = fv % PV, dy = (fv / PV) % P, c = fv / (PV * P);
            v = *reinterpret_cast<const V*>(x + ((b * Cin + c) * H + (py * P + dy)) * (int64_t)W + px * P + dxv * N);
        }
        reinterpret_cast<V*>(out)[i] = v;
    }
}

// D4 = D / 4 float4 columns, R = 1 + L output rows an image.  FILL: rows with r >= Lk take `fill`; otherwise r is clamped.
template <bool FILL, bool ADD>
__global__ __launch_bounds__(MK_THREADS) void token_restore_kernel(const float* __restrict__ src, int64_t src_img,
                                                                   const int32_t* __restrict__ restore,
                                                                   const float* __restrict__ fill,
                                                                   const float* __restrict__ add, int B, int L, int Lk, int D4,
                                                                   float* __restrict__ dst) {
    const int R = 1 + L;
    const int64_t total = (int64_t)B * R * D4;
    for (int64_t i = (int64_t)blockIdx.x * MK_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * MK_THREADS) {
        const int c = (int)(i % D4);
        const int64_t row = i / D4;
        const int t = (int)(row % R);
        const int64_t b = row / R;
        const float* from = src + b * src_img;                       // row 0 of image b's source
        if (t > 0) {
            int r = max(restore[b * L + (t - 1)], 0);
            if (FILL) {
                from = r < Lk ? from + (int64_t)(1 + r) * 4 * D4 : fill;
            } else {
                r = min(r, Lk - 1);
                from += (int64_t)(1 + r) * 4 * D4;
            }
        }
        float4 v = reinterpret_cast<const float4*>(from)[c];
        if (ADD) {
            const float4 a = reinterpret_cast<const float4*>(add)[(int64_t)t * D4 + c];
            v = make_float4(v.x + a.x, v.y + a.y, v.z + a.z, v.w + a.w);
        }
        reinterpret_cast<float4*>(dst)[i] = v;
    }
}

unsigned mask_grid(int64_t total) {
    const int64_t g = mcd_cdiv(total, MK_THREADS);
    return (unsigned)(g < MK_MAX_GRID ? g : MK_MAX_GRID);
}

}  // namespace

extern "C" int mcd_patchify_kept(const float* x, const int32_t* keep, int64_t B, int64_t Cin, int64_t H, int64_t W, int64_t P,
                                 int64_t Lk, float* out, mcd_stream_t stream) {
    MCD_REQUIRE(B >= 0 && Lk >= 0, MCD_E_ARG, "mcd_patchify_kept: B=%lld Lk=%lld", (long long)B, (long long)Lk);
    if (B == 0) return MCD_OK;
    MCD_REQUIRE(x && out && (keep || Lk == 0), MCD_E_ARG, "mcd_patchify_kept: NULL pointer");
    MCD_REQUIRE(Cin > 0 && P >= 2 && P % 2 == 0 && H > 0 && W > 0 && H % P == 0 && W % P == 0, MCD_E_UNSUPPORTED,
                "mcd_patchify_kept: bad shape Cin=%lld H=%lld W=%lld P=%lld", (long long)Cin, (long long)H, (long long)W,
                (long long)P);
    MCD_REQUIRE(B < (1 << 30) && Lk < (1 << 30) && H < (1 << 30) && W < (1 << 30) && Cin < (1 << 30), MCD_E_UNSUPPORTED,
                "mcd_patchify_kept: B=%lld Lk=%lld too large", (long long)B, (long long)Lk);
    MCD_REQUIRE(Cin * H < (1LL << 31) && Cin * H * W < (1LL << 29) && Cin * P * P < (1LL << 29)
                    && (1 + Lk) * (Cin * P * P) < (1LL << 29),
                MCD_E_UNSUPPORTED, "mcd_patchify_kept: one image or its rows span 2^31 bytes or more");
    MCD_REQUIRE(((uintptr_t)x) % 16 == 0 && ((uintptr_t)out) % 16 == 0 && ((uintptr_t)keep) % 4 == 0, MCD_E_ARG,
                "mcd_patchify_kept: x and out must be 16-byte aligned, keep 4-byte aligned");
    const int nvec = P % 4 == 0 ? 4 : 2;                  // floats per thread
    const int64_t total = B * (1 + Lk) * (Cin * P * P / nvec);
    if (nvec == 4)
        hipLaunchKernelGGL(patchify_kept_kernel<float4>, dim3(mask_grid(total)), dim3(MK_THREADS), 0, (hipStream_t)stream, x,
                           keep, (int)B, (int)Cin, (int)H, (int)W, (int)P, (int)Lk, out);
    else
        hipLaunchKernelGGL(patchify_kept_kernel<float2>, dim3(mask_grid(total)), dim3(MK_THREADS), 0, (hipStream_t)stream, x,
                           keep, (int)B, (int)Cin, (int)H, (int)W, (int)P, (int)Lk, out);
    MCD_LAUNCH_CHECK("patchify_kept_kernel");
    return MCD_OK;
}

extern "C" int mcd_token_restore(const float* src, int64_t src_img, const int32_t* restore, const float* fill,
                                 const float* add, int64_t B, int64_t L, int64_t Lk, int64_t D, float* dst,
                                 mcd_stream_t stream) {
    MCD_REQUIRE(B >= 0 && L >= 0 && Lk >= 0, MCD_E_ARG, "mcd_token_restore: B=%lld L=%lld Lk=%lld", (long long)B, (long long)L,
                (long long)Lk);
    MCD_REQUIRE(D >= 4 && D % 4 == 0, MCD_E_ARG, "mcd_token_restore: D=%lld must be a positive multiple of 4", (long long)D);
    if (B == 0) return MCD_OK;
    MCD_REQUIRE(src && dst && (restore || L == 0), MCD_E_ARG, "mcd_token_restore: NULL pointer");
    MCD_REQUIRE(fill || Lk >= 1 || L == 0, MCD_E_ARG, "mcd_token_restore: no fill row and no source row (Lk=0, L=%lld)",
                (long long)L);
    MCD_REQUIRE(B < (1 << 30) && L < (1 << 30) && Lk < (1 << 30) && D < (1 << 30), MCD_E_UNSUPPORTED,
                "mcd_token_restore: B=%lld L=%lld Lk=%lld D=%lld too large", (long long)B, (long long)L, (long long)Lk,
                (long long)D);
    const int64_t src_rows = (1 + Lk) * D, dst_rows = (1 + L) * D;      // floats of one image
    MCD_REQUIRE(src_rows < (1LL << 29) && dst_rows < (1LL << 29), MCD_E_UNSUPPORTED,
                "mcd_token_restore: one image spans 2^31 bytes or more");
    MCD_REQUIRE(src_img == 0 || (src_img >= src_rows && src_img % 4 == 0 && src_img <= (INT64_MAX / 8) / B), MCD_E_ARG,
                "mcd_token_restore: src_img=%lld is neither 0 nor a multiple of 4 of at least (1+Lk)*D=%lld", (long long)src_img,
                (long long)src_rows);
    MCD_REQUIRE(((uintptr_t)src) % 16 == 0 && ((uintptr_t)dst) % 16 == 0 && ((uintptr_t)fill) % 16 == 0
                    && ((uintptr_t)add) % 16 == 0 && ((uintptr_t)restore) % 4 == 0,
                MCD_E_ARG, "mcd_token_restore: src, fill, add and dst must be 16-byte aligned, restore 4-byte aligned");
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + 4 * (uintptr_t)((B - 1) * src_img + src_rows);
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + 4 * (uintptr_t)(B * dst_rows);
    MCD_REQUIRE(d1 <= s0 || s1 <= d0, MCD_E_ARG, "mcd_token_restore: dst overlaps src");
    const int64_t total = B * (1 + L) * (D / 4);
    const dim3 grid(mask_grid(total)), block(MK_THREADS);
#define MCD_TR(F, A)                                                                                                        \
    hipLaunchKernelGGL((token_restore_kernel<F, A>), grid, block, 0, (hipStream_t)stream, src, src_img, restore, fill, add, \
                       (int)B, (int)L, (int)Lk, (int)(D / 4), dst)
    if (fill && add) MCD_TR(true, true);
    else if (fill) MCD_TR(true, false);
    else if (add) MCD_TR(false, true);
    else MCD_TR(false, false);
#undef MCD_TR
    MCD_LAUNCH_CHECK("token_restore_kernel");
    return MCD_OK;
}
