// k_ln.hip -- K10: fp32 LayerNorm over the last dimension for the ViT towers (encoder-side, HBM-bound).
//   replaces  nn.LayerNorm inside the encoder blocks (ViTLayer.layernorm_before/after, model/modules/image_encoder.py:37;
//             ln_1 / ln_2, concept_vit/clip/model.py:172-176) in the forwards that concept_vit/utils.py:117-148 drives.
// ATen's kernel runs at 4.0 TB/s on the [49 250, 768] activations of the headline bench (75 us, 960 calls per step).
// Here one wave owns a row: the row lives in registers (NV float4 per lane), mean and the centred sum of squares are
// two shuffle reductions over it (two-pass in registers: no E[x^2] - E[x]^2 cancellation), one read and one write of
// HBM per element.  y = (x - mean) / sqrt(var + eps) * gamma + beta, biased variance, like torch.
//
// K24 (mcd_text_embed_ln): the embedding rows of the BERT text tower in one launch,
//   replaces  BertEmbeddings.forward inside BertModel(**tokens) (model/modules/text_encoder.py:48): three gathers, two adds
//             and embeddings.LayerNorm -- six ATen kernels and three [rows, D] temporaries.
// out[r] = LayerNorm((word[ids[r]] + type[type_ids[r]]) + pos[r % T]): one wave gathers the three table rows into K10's
// registers and runs K10's row routine (ln_row) on them, so the result is K10's on ATen's sum, bit for bit.
//
// K32 (mcd_patch_merge_ln, include/mcd_swin.h): Swin's patch merging up to its LayerNorm in one launch,
//   replaces  SwinPatchMerging.forward up to .norm (transformers modeling_swin.py): F.pad to even sizes, four strided
//             slices, cat and nn.LayerNorm -- a [B, H/2 * W/2, 4C] temporary written and read again.
// One wave gathers the four neighbours' C values (zeros past an odd edge) into K10's registers and runs ln_row on them.
#include <type_traits>

#include "mcd_common.h"
#include "../../include/mcd_text.h"
#include "../../include/mcd_swin.h"

namespace {

// The row routine of K10 and K24: the row is in v (float4 q = lane + 64 i of it, zeros past nq = D / 4); writes row `row` of y.
template <int NV>
__device__ __forceinline__ void ln_row(const float4 (&v)[NV], int lane, int nq, int D, const float* __restrict__ gamma,
                                       const float* __restrict__ beta, float eps, float* __restrict__ y, int64_t row) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    const float mean = mcd_wave_sum(s) / (float)D;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (lane + 64 * i < nq) {
            const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
            ss += (a * a + b * b) + (c * c + d * d);
        }
    }
    const float rstd = 1.0f / sqrtf(mcd_wave_sum(ss) / (float)D + eps);
    float4* yr = reinterpret_cast<float4*>(y + row * D);
    const float4* g4 = reinterpret_cast<const float4*>(gamma);
    const float4* b4 = reinterpret_cast<const float4*>(beta);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int q = lane + 64 * i;
        if (q < nq) {
            const float4 g = g4[q], b = b4[q];
            yr[q] = make_float4((v[i].x - mean) * rstd * g.x + b.x, (v[i].y - mean) * rstd * g.y + b.y,
                                (v[i].z - mean) * rstd * g.z + b.z, (v[i].w - mean) * rstd * g.w + b.w);
        }
    }
}

template <int NV>
__global__ __launch_bounds__(256) void layer_norm_kernel(const float* __restrict__ x, int64_t rows, int D,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float eps, float* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float4* xr = reinterpret_cast<const float4*>(x + row * D);
    const int nq = D >> 2;
    float4 v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int q = lane + 64 * i;
        v[i] = q < nq ? xr[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    ln_row<NV>(v, lane, nq, D, gamma, beta, eps, y, row);
}

// K24: the row is gathered instead of read -- (word[id] + type[type id]) + pos[row % T], HF's order of the two adds
// (BertEmbeddings: inputs_embeds + token_type_embeddings, then + position_embeddings), one rounding each -- and goes
// through the same routine: what K10 gives on ATen's sum of the three gathers, bit for bit.  Ids are clamped into their
// tables (the binding refuses a bad id on the host; the kernel never reads out of range).
template <int NV>
__global__ __launch_bounds__(256) void text_embed_ln_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ type_ids,
                                                             const float* __restrict__ word, const float* __restrict__ pos,
                                                             const float* __restrict__ type, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps, int64_t rows, int T,
                                                             int D, int64_t vocab, int64_t n_type, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    int64_t id = ids[row], tid = type_ids ? type_ids[row] : 0;
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    tid = tid < 0 ? 0 : (tid >= n_type ? n_type - 1 : tid);
    const float4* wr = reinterpret_cast<const float4*>(word + id * D);
    const float4* tr = reinterpret_cast<const float4*>(type + tid * D);
    const float4* pr = reinterpret_cast<const float4*>(pos + (row % T) * D);
    const int nq = D >> 2;
    float4 v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int q = lane + 64 * i;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < nq) {
            const float4 w = wr[q], t = tr[q], p = pr[q];
            v[i] = make_float4((w.x + t.x) + p.x, (w.y + t.y) + p.y, (w.z + t.z) + p.z, (w.w + t.w) + p.w);
        }
    }
    ln_row<NV>(v, lane, nq, D, gamma, beta, eps, out, row);
}

// K32: output row (b, oy, ox) is x[b, 2oy, 2ox] | x[b, 2oy+1, 2ox] | x[b, 2oy, 2ox+1] | x[b, 2oy+1, 2ox+1]; float4 q of
// the row lies in piece q / (C/4) -- pieces 1 and 3 one grid row down, pieces 2 and 3 one column right.
template <int NV>
__global__ __launch_bounds__(256) void patch_merge_ln_kernel(const float* __restrict__ x, int64_t rows, int H, int W, int C,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              float eps, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int Ho = (H + 1) >> 1, Wo = (W + 1) >> 1, cq = C >> 2, nq = C;        // nq = 4C / 4
    const int ox = (int)(row % Wo), oy = (int)((row / Wo) % Ho);
    const float* img = x + (row / ((int64_t)Ho * Wo)) * H * W * C;               // in-image offsets fit an int (host)
    float4 v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int q = lane + 64 * i;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < nq) {
            const int piece = q / cq, y = 2 * oy + (piece & 1), xx = 2 * ox + (piece >> 1);
            if (y < H && xx < W) v[i] = reinterpret_cast<const float4*>(img + (y * W + xx) * C)[q % cq];
        }
    }
    ln_row<NV>(v, lane, nq, 4 * C, gamma, beta, eps, out, row);
}

// The instantiated NV (float4 per lane) of a row of nq float4: the smallest of 1, 2, 3, 4, 6, 8 that holds it (nq <= 512).
int ln_nv(int64_t nq) {
    const int nv = (int)mcd_cdiv(nq, 64);
    return nv <= 1 ? 1 : nv <= 4 ? nv : nv <= 6 ? 6 : 8;
}

// launch(NV as a compile-time constant) for the rows of K10, K24 and K32: the one place that lists the instantiations.
template <typename Launch>
void ln_dispatch(int64_t nq, Launch launch) {
    switch (ln_nv(nq)) {
        case 1: return launch(std::integral_constant<int, 1>());
        case 2: return launch(std::integral_constant<int, 2>());
        case 3: return launch(std::integral_constant<int, 3>());
        case 4: return launch(std::integral_constant<int, 4>());
        case 6: return launch(std::integral_constant<int, 6>());
        default: return launch(std::integral_constant<int, 8>());
    }
}

}  // namespace

extern "C" int mcd_patch_merge_ln(const float* x, int64_t B, int64_t H, int64_t W, int64_t C, const float* gamma,
                                  const float* beta, float eps, float* out, mcd_stream_t stream) {
    MCD_REQUIRE(x && out && gamma && beta, MCD_E_ARG, "mcd_patch_merge_ln: NULL pointer");
    MCD_REQUIRE(B >= 0 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0, MCD_E_ARG,
                "mcd_patch_merge_ln: bad shape B=%lld H=%lld W=%lld C=%lld (C a positive multiple of 4)", (long long)B,
                (long long)H, (long long)W, (long long)C);
    MCD_REQUIRE(4 * C <= 2048, MCD_E_UNSUPPORTED, "mcd_patch_merge_ln: 4C=%lld is over 2048", (long long)(4 * C));
    MCD_REQUIRE(H < (1 << 24) && W < (1 << 24) && H * W * C < (1LL << 29) && B < (1LL << 31), MCD_E_UNSUPPORTED,
                "mcd_patch_merge_ln: one image spans 2^31 bytes or more");
    MCD_REQUIRE(((uintptr_t)x) % 16 == 0 && ((uintptr_t)out) % 16 == 0 && ((uintptr_t)gamma) % 16 == 0 && ((uintptr_t)beta) % 16 == 0,
                MCD_E_ARG, "mcd_patch_merge_ln: pointers must be 16-byte aligned");
    if (B == 0) return MCD_OK;
    const int64_t rows = B * ((H + 1) / 2) * ((W + 1) / 2);
    MCD_REQUIRE(mcd_cdiv(rows, 4) < (1LL << 31), MCD_E_UNSUPPORTED, "mcd_patch_merge_ln: %lld output rows", (long long)rows);
    const unsigned grid = (unsigned)mcd_cdiv(rows, 4);
    ln_dispatch(C, [&](auto nv) {      // a row of 4C floats
        hipLaunchKernelGGL(patch_merge_ln_kernel<decltype(nv)::value>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, rows,
                           (int)H, (int)W, (int)C, gamma, beta, eps, out);
    });
    MCD_LAUNCH_CHECK("patch_merge_ln_kernel");
    return MCD_OK;
}

extern "C" int mcd_layer_norm(const float* x, int64_t rows, int64_t D, const float* gamma, const float* beta, float eps,
                              float* y, mcd_stream_t stream) {
    MCD_REQUIRE(x && y && gamma && beta, MCD_E_ARG, "mcd_layer_norm: NULL pointer");
    MCD_REQUIRE(rows >= 0 && D >= 4 && D % 4 == 0 && D <= 2048, MCD_E_UNSUPPORTED,
                "mcd_layer_norm: D=%lld must be a multiple of 4 in [4, 2048]", (long long)D);
    MCD_REQUIRE(((uintptr_t)x) % 16 == 0 && ((uintptr_t)y) % 16 == 0 && ((uintptr_t)gamma) % 16 == 0 && ((uintptr_t)beta) % 16 == 0,
                MCD_E_ARG, "mcd_layer_norm: pointers must be 16-byte aligned");
    if (rows == 0) return MCD_OK;
    const unsigned grid = (unsigned)mcd_cdiv(rows, 4);
    ln_dispatch(D / 4, [&](auto nv) {
        hipLaunchKernelGGL(layer_norm_kernel<decltype(nv)::value>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, rows, (int)D,
                           gamma, beta, eps, y);
    });
    MCD_LAUNCH_CHECK("layer_norm_kernel");
    return MCD_OK;
}

extern "C" int mcd_text_embed_ln(const int64_t* ids, const int64_t* type_ids, const float* word, const float* pos,
                                 const float* type, const float* gamma, const float* beta, float eps, int64_t rows, int64_t T,
                                 int64_t D, int64_t vocab, int64_t n_type, float* out, mcd_stream_t stream) {
    MCD_REQUIRE(ids && word && pos && type && gamma && beta && out, MCD_E_ARG, "mcd_text_embed_ln: NULL pointer");
    MCD_REQUIRE(rows >= 0 && T >= 1 && vocab >= 1 && n_type >= 1 && T <= INT32_MAX, MCD_E_ARG,
                "mcd_text_embed_ln: bad shape rows=%lld T=%lld vocab=%lld n_type=%lld", (long long)rows, (long long)T,
                (long long)vocab, (long long)n_type);
    MCD_REQUIRE(D >= 4 && D % 4 == 0 && D <= 2048, MCD_E_UNSUPPORTED,
                "mcd_text_embed_ln: D=%lld must be a multiple of 4 in [4, 2048]", (long long)D);
    MCD_REQUIRE(((uintptr_t)word) % 16 == 0 && ((uintptr_t)pos) % 16 == 0 && ((uintptr_t)type) % 16 == 0 &&
                    ((uintptr_t)gamma) % 16 == 0 && ((uintptr_t)beta) % 16 == 0 && ((uintptr_t)out) % 16 == 0 &&
                    ((uintptr_t)ids) % 8 == 0 && ((uintptr_t)type_ids) % 8 == 0,
                MCD_E_ARG, "mcd_text_embed_ln: float pointers must be 16-byte aligned, id pointers 8-byte aligned");
    if (rows == 0) return MCD_OK;
    const unsigned grid = (unsigned)mcd_cdiv(rows, 4);
    ln_dispatch(D / 4, [&](auto nv) {
        hipLaunchKernelGGL(text_embed_ln_kernel<decltype(nv)::value>, dim3(grid), dim3(256), 0, (hipStream_t)stream, ids, type_ids,
                           word, pos, type, gamma, beta, eps, rows, (int)T, (int)D, vocab, n_type, out);
    });
    MCD_LAUNCH_CHECK("text_embed_ln_kernel");
    return MCD_OK;
}

// ---- K11: patch extraction for the ViT patch embedding ---------------------------------------------------------
//   replaces  the Conv2d(3, dim, P, stride P) of the patch embedding (ViTPatchEmbeddings / conv1, the same reference
//             sites as K9; Dinov2PatchEmbeddings at P = 14) by its GEMM form: rows of P*P*Cin pixels per patch, times
//             the [dim, Cin*P*P] weight.
// out is [B, 1 + nP, Cin*P*P]: row 0 of every image is zero (the class-token slot: the GEMM that follows adds the
// residual operand there), row 1 + (py*nW + px) is patch (py, px) in (c, dy, dx) order -- the order of the conv
// weight viewed as [dim, Cin*P*P].  A pure permutation: one thread per vector V of the output, coalesced writes.
//   P % 4 == 0: V = float4.  A patch row starts at float ((b*Cin + c)*H + y)*W + px*P of x, and W is a multiple of P:
//               every term is a multiple of 4 floats, so each 16-byte piece of a patch row is 16-byte aligned.
//   other even P (14 for DINOv2: a patch row is 56 bytes): V = float2.  W is a multiple of P, hence even, so the same
//               sum is a multiple of 2 floats and so is every piece's offset 2*dx inside the row: 8-byte aligned
//               wherever x is (16 bytes are asked of it).  On the output side Cin*P*P is a multiple of 4 for any even P.
// Odd P would need 4-byte accesses and is refused.
namespace {

template <typename V> __device__ __forceinline__ V patchify_zero();
template <> __device__ __forceinline__ float4 patchify_zero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }
template <> __device__ __forceinline__ float2 patchify_zero<float2>() { return make_float2(0.f, 0.f); }

template <typename V>
__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ x, int B, int Cin, int H, int W, int P,
                                                        float* __restrict__ out) {
    constexpr int N = sizeof(V) / sizeof(float);
    const int nW = W / P, nP = (H / P) * nW, F = Cin * P * P, FV = F / N, PV = P / N;
    const int64_t total = (int64_t)B * (1 + nP) * FV;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int fv = (int)(i % FV);
        const int64_t row = i / FV;
        const int r = (int)(row % (1 + nP));
        const int64_t b = row / (1 + nP);
        V v = patchify_zero<V>();
        if (r > 0) {
            const int p = r - 1, py = p / nW, px = p % nW;
            const int dxv = fv % PV, dy = (fv / PV) % P, c = fv / (PV * P);
            v = *reinterpret_cast<const V*>(x + ((b * Cin + c) * H + (py * P + dy)) * (int64_t)W + px * P + dxv * N);
        }
        reinterpret_cast<V*>(out)[i] = v;
    }
}

}  // namespace

extern "C" int mcd_patchify(const float* x, int64_t B, int64_t Cin, int64_t H, int64_t W, int64_t P, float* out,
                            mcd_stream_t stream) {
    MCD_REQUIRE(x && out, MCD_E_ARG, "mcd_patchify: NULL pointer");
    MCD_REQUIRE(B >= 0 && Cin > 0 && P >= 2 && P % 2 == 0 && H > 0 && W > 0 && H % P == 0 && W % P == 0,
                MCD_E_UNSUPPORTED, "mcd_patchify: bad shape B=%lld Cin=%lld H=%lld W=%lld P=%lld", (long long)B,
                (long long)Cin, (long long)H, (long long)W, (long long)P);
    MCD_REQUIRE(B < (1 << 30) && Cin * H * W < (1LL << 31), MCD_E_UNSUPPORTED, "mcd_patchify: image too large");
    MCD_REQUIRE(((uintptr_t)x) % 16 == 0 && ((uintptr_t)out) % 16 == 0, MCD_E_ARG, "mcd_patchify: pointers must be 16-byte aligned");
    if (B == 0) return MCD_OK;
    const int nvec = P % 4 == 0 ? 4 : 2;                  // floats per thread
    const int64_t total = B * (1 + (H / P) * (W / P)) * (Cin * P * P / nvec);
    const unsigned grid = (unsigned)(mcd_cdiv(total, 256) < (1 << 20) ? mcd_cdiv(total, 256) : (1 << 20));
    if (nvec == 4)
        hipLaunchKernelGGL(patchify_kernel<float4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (int)B, (int)Cin, (int)H,
                           (int)W, (int)P, out);
    else
        hipLaunchKernelGGL(patchify_kernel<float2>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (int)B, (int)Cin, (int)H,
                           (int)W, (int)P, out);
    MCD_LAUNCH_CHECK("patchify_kernel");
    return MCD_OK;
}
