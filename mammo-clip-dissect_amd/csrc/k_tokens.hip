// k_tokens.hip -- K26: the mean over a range of tokens of every image (include/mcd_tokens.h), the pooling in front of
// CLIPForImageClassification's classifier.
//   replaces torch.mean(last_hidden_state[:, 1:, :], dim=1): a strided slice and ATen's reduction over the middle dimension
// Bandwidth-bound: every float of the token range is read once, B * D floats are written.  A workgroup of TM_WAVES waves owns
// one image and one block of 64 float4 columns (256 floats: a wave instruction reads 1 KiB of one token row, whole cache
// lines); wave w takes the rows w, w + TM_WAVES, ... of the range, TM_U 16-byte loads in flight before the first add, and adds
// them in ascending order.  The partial sums meet in LDS and wave 0 adds them in wave order, divides and stores.  The order of
// the additions is a function of the row count alone (mcd_tokens.h writes it down): no atomics, no split over the grid.
// K27 (include/mcd_sentence.h): the same reduction over the first L rows of a sequence, L per sequence, and the L2
// normalisation of the mean in the same launch -- sentence-transformers' Pooling(mean) + Normalize behind MPNetModel.
#include "mcd_common.h"
#include "../../include/mcd_tokens.h"
#include "../../include/mcd_sentence.h"

namespace {

constexpr int TM_WAVES = 4;                       // the four partial sums of the header
constexpr int TM_THREADS = TM_WAVES * MCD_WAVE;
constexpr int TM_U = 8;                           // float4 loads of a lane in flight
constexpr int MM_CB = 8;                          // K27: column blocks of 64 float4, D <= 2048 (K10's limit)

__device__ __forceinline__ void add4(float4& a, const float4 v) {
    a.x += v.x;
    a.y += v.y;
    a.z += v.z;
    a.w += v.w;
}

// Wave w's partial sum of one float4 column: the rows w, w + TM_WAVES, ... < n of col in ascending order, TM_U loads in flight.
__device__ __forceinline__ float4 wave_rows_sum(const float* col, int w, int n, int64_t x_tok) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int r = w;
    for (; r + (TM_U - 1) * TM_WAVES < n; r += TM_U * TM_WAVES) {
        float4 v[TM_U];
#pragma unroll
        for (int u = 0; u < TM_U; ++u) v[u] = *reinterpret_cast<const float4*>(col + (int64_t)(r + u * TM_WAVES) * x_tok);
#pragma unroll
        for (int u = 0; u < TM_U; ++u) add4(acc, v[u]);
    }
    for (; r < n; r += TM_WAVES) add4(acc, *reinterpret_cast<const float4*>(col + (int64_t)r * x_tok));
    return acc;
}

// x points at token t0 of image 0; n = T - t0 rows, D4 = D / 4 float4 columns.  grid (ceil(D4 / 64), B).
__global__ __launch_bounds__(TM_THREADS) void token_mean_kernel(const float* x, int n, int D4, int64_t x_img, int64_t x_tok,
                                                                float* out, int64_t out_img) {
    __shared__ float4 part[TM_WAVES - 1][MCD_WAVE];
    const int lane = threadIdx.x & (MCD_WAVE - 1);
    const int w = threadIdx.x / MCD_WAVE;
    const int c = blockIdx.x * MCD_WAVE + lane;
    const bool live = c < D4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) acc = wave_rows_sum(x + (int64_t)blockIdx.y * x_img + 4 * (int64_t)c, w, n, x_tok);
    if (w > 0) part[w - 1][lane] = acc;
    __syncthreads();
    if (w == 0 && live) {
#pragma unroll
        for (int k = 0; k < TM_WAVES - 1; ++k) add4(acc, part[k][lane]);
        const float d = (float)n;
        *reinterpret_cast<float4*>(out + (int64_t)blockIdx.y * out_img + 4 * (int64_t)c) =
            make_float4(acc.x / d, acc.y / d, acc.z / d, acc.w / d);
    }
}

// K27: one workgroup per sequence.  Column block cb (64 float4 columns) goes through K26's steps -- the four waves share the
// rows 0 .. L-1, the partial sums meet in LDS, wave 0 adds them in wave order and divides by L -- and wave 0 keeps the means of
// all MM_CB blocks in registers (D <= 2048: 8 float4 per lane).  The squared norm is then wave 0's alone: each lane adds the
// squares of its columns in ascending order, an xor butterfly over the 64 lanes leaves every lane the same sum.
__global__ __launch_bounds__(TM_THREADS) void masked_mean_l2_kernel(const float* x, int T, int D4, const int32_t* lens,
                                                                    int normalize, float* out) {
    __shared__ float4 part[TM_WAVES - 1][MCD_WAVE];
    const int lane = threadIdx.x & (MCD_WAVE - 1);
    const int w = threadIdx.x / MCD_WAVE;
    const int64_t b = blockIdx.x;
    int n = T;
    if (lens) n = min(max(lens[b], 1), T);
    const int64_t x_tok = 4 * (int64_t)D4;
    const float* xb = x + b * T * x_tok;
    const float d = (float)n;
    float4 mean[MM_CB];
#pragma unroll
    for (int cb = 0; cb < MM_CB; ++cb) {
        mean[cb] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (cb * MCD_WAVE < D4) {                              // uniform over the workgroup
            const int c = cb * MCD_WAVE + lane;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < D4) acc = wave_rows_sum(xb + 4 * (int64_t)c, w, n, x_tok);
            if (w > 0) part[w - 1][lane] = acc;
            __syncthreads();
            if (w == 0) {
#pragma unroll
                for (int k = 0; k < TM_WAVES - 1; ++k) add4(acc, part[k][lane]);
                mean[cb] = make_float4(acc.x / d, acc.y / d, acc.z / d, acc.w / d);
            }
            __syncthreads();                                   // part is free for the next block
        }
    }
    if (w != 0) return;
    float den = 1.f;
    if (normalize) {
        float ss = 0.f;
#pragma unroll
        for (int cb = 0; cb < MM_CB; ++cb) {                   // a column past D holds zero
            ss += mean[cb].x * mean[cb].x;
            ss += mean[cb].y * mean[cb].y;
            ss += mean[cb].z * mean[cb].z;
            ss += mean[cb].w * mean[cb].w;
        }
#pragma unroll
        for (int s = MCD_WAVE / 2; s >= 1; s >>= 1) ss += __shfl_xor(ss, s);
        den = fmaxf(sqrtf(ss), 1e-12f);
    }
#pragma unroll
    for (int cb = 0; cb < MM_CB; ++cb) {
        const int c = cb * MCD_WAVE + lane;
        if (c < D4) {
            float4 m = mean[cb];
            if (normalize) m = make_float4(m.x / den, m.y / den, m.z / den, m.w / den);
            *reinterpret_cast<float4*>(out + b * x_tok + 4 * (int64_t)c) = m;
        }
    }
}

}  // namespace

extern "C" int mcd_masked_mean_l2(const float* x, int B, int T, int D, const int32_t* lens, int normalize, float* out,
                                  mcd_stream_t stream) {
    MCD_REQUIRE(B >= 0, MCD_E_ARG, "mcd_masked_mean_l2: B=%d", B);
    if (B == 0) return MCD_OK;
    MCD_REQUIRE(x && out, MCD_E_ARG, "mcd_masked_mean_l2: NULL pointer");
    MCD_REQUIRE(D >= 4 && D % 4 == 0, MCD_E_ARG, "mcd_masked_mean_l2: D=%d must be a positive multiple of 4", D);
    MCD_REQUIRE(T >= 1, MCD_E_ARG, "mcd_masked_mean_l2: T=%d", T);
    MCD_REQUIRE(normalize == 0 || normalize == 1, MCD_E_ARG, "mcd_masked_mean_l2: normalize=%d is neither 0 nor 1", normalize);
    MCD_REQUIRE(((uintptr_t)x) % 16 == 0 && ((uintptr_t)out) % 16 == 0 && ((uintptr_t)lens) % 4 == 0, MCD_E_ARG,
                "mcd_masked_mean_l2: x and out must be 16-byte aligned, lens 4-byte aligned");
    MCD_REQUIRE(D <= 4 * MCD_WAVE * MM_CB, MCD_E_UNSUPPORTED, "mcd_masked_mean_l2: D=%d is over %d", D, 4 * MCD_WAVE * MM_CB);
    MCD_REQUIRE((int64_t)T * D < ((int64_t)1 << 29), MCD_E_UNSUPPORTED,
                "mcd_masked_mean_l2: one sequence spans %lld floats, 2^31 bytes or more", (long long)T * D);
    const uintptr_t x0 = (uintptr_t)x, x1 = x0 + 4 * (uintptr_t)((int64_t)B * T * D);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + 4 * (uintptr_t)((int64_t)B * D);
    MCD_REQUIRE(o1 <= x0 || x1 <= o0, MCD_E_ARG, "mcd_masked_mean_l2: out overlaps x");
    hipLaunchKernelGGL(masked_mean_l2_kernel, dim3((unsigned)B), dim3(TM_THREADS), 0, (hipStream_t)stream, x, T, D / 4, lens,
                       normalize, out);
    MCD_LAUNCH_CHECK("masked_mean_l2_kernel");
    return MCD_OK;
}

extern "C" int mcd_token_mean(const float* x, int B, int T, int D, int64_t x_img, int64_t x_tok, int t0, float* out,
                              int64_t out_img, mcd_stream_t stream) {
    MCD_REQUIRE(B >= 0, MCD_E_ARG, "mcd_token_mean: B=%d", B);
    if (B == 0) return MCD_OK;
    MCD_REQUIRE(x && out, MCD_E_ARG, "mcd_token_mean: NULL pointer");
    MCD_REQUIRE(D >= 4 && D % 4 == 0, MCD_E_ARG, "mcd_token_mean: D=%d must be a positive multiple of 4", D);
    MCD_REQUIRE(T >= 1 && t0 >= 0 && t0 < T, MCD_E_ARG, "mcd_token_mean: T=%d t0=%d (need 0 <= t0 < T)", T, t0);
    MCD_REQUIRE(x_tok >= D && out_img >= D, MCD_E_ARG, "mcd_token_mean: x_tok=%lld out_img=%lld are under D=%d",
                (long long)x_tok, (long long)out_img, D);
    MCD_REQUIRE(x_tok <= INT64_MAX / T, MCD_E_ARG, "mcd_token_mean: x_tok=%lld overflows with T=%d", (long long)x_tok, T);
    const int64_t image = (int64_t)(T - 1) * x_tok + D;                        // floats from an image's first to its last
    MCD_REQUIRE(x_img >= image, MCD_E_ARG, "mcd_token_mean: x_img=%lld is under (T-1)*x_tok+D=%lld", (long long)x_img,
                (long long)image);
    MCD_REQUIRE(x_img % 4 == 0 && x_tok % 4 == 0 && out_img % 4 == 0, MCD_E_ARG,
                "mcd_token_mean: x_img=%lld x_tok=%lld out_img=%lld must be multiples of 4 floats", (long long)x_img,
                (long long)x_tok, (long long)out_img);
    MCD_REQUIRE(((uintptr_t)x) % 16 == 0 && ((uintptr_t)out) % 16 == 0, MCD_E_ARG,
                "mcd_token_mean: x and out must be 16-byte aligned");
    MCD_REQUIRE(B <= 65535, MCD_E_UNSUPPORTED, "mcd_token_mean: B=%d is over 65535", B);
    MCD_REQUIRE(image < ((int64_t)1 << 29), MCD_E_UNSUPPORTED, "mcd_token_mean: one image spans %lld floats, 2^31 bytes or more",
                (long long)image);
    MCD_REQUIRE(x_img <= (INT64_MAX / 8) / B && out_img <= (INT64_MAX / 8) / B, MCD_E_ARG,
                "mcd_token_mean: x_img=%lld / out_img=%lld overflow with B=%d", (long long)x_img, (long long)out_img, B);
    const uintptr_t x0 = (uintptr_t)x, x1 = x0 + 4 * (uintptr_t)((int64_t)(B - 1) * x_img + image);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + 4 * (uintptr_t)((int64_t)(B - 1) * out_img + D);
    MCD_REQUIRE(o1 <= x0 || x1 <= o0, MCD_E_ARG, "mcd_token_mean: out overlaps x");
    const int D4 = D / 4;
    hipLaunchKernelGGL(token_mean_kernel, dim3((unsigned)mcd_cdiv(D4, MCD_WAVE), (unsigned)B), dim3(TM_THREADS), 0,
                       (hipStream_t)stream, x + (int64_t)t0 * x_tok, T - t0, D4, x_img, x_tok, out, out_img);
    MCD_LAUNCH_CHECK("token_mean_kernel");
    return MCD_OK;
}
