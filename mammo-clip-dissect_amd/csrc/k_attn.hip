// k_attn.hip -- K9: fp32 self-attention of the ViT image tower, one launch per encoder block.
//   replaces, inside the encoder forwards that the extraction loop drives (concept_vit/utils.py:117-148):
//     model/modules/image_encoder.py:37  ViTModel(...)  -> softmax(q k^T / sqrt(64)) v  per head
//     concept_vit/clip/model.py:171-183  nn.MultiheadAttention(x, x, x, need_weights=False) without a mask
// 11 % of the GPU time of the headline bench was PyTorch's generic fp32 SDPA kernel (0.68 ms per call at 250 images
// x 12 heads x 197 tokens, 43 TFLOP/s); the matrix pipe can do the 29.8 GFLOP in 0.19 ms.
//
// One workgroup per (image, head), one wave per 32 queries (7 waves at T = 197), flash style over 32-key tiles.
// The K and V tiles ([32, 64] fp32 = 8 KB each) go global -> LDS by global_load_lds_dwordx4 (no staging registers)
// into a ring of four tiles, in pairs: the pair after the one being consumed is in flight.  A dedicated LOADER wave
// (the last one) issues the sixteen 1 KB pieces of a tile and waits for them; everybody meets at one s_barrier per
// pair.  The compute waves never issue a memory instruction inside the loop: the compiler puts an s_waitcnt
// vmcnt(0) in front of LDS reads that follow a DMA in the same wave (it must assume they alias), which would drain
// the ring every tile.  64 KB of LDS and 128 registers: two workgroups per CU.
// A DMA piece lands contiguously, so rows cannot be padded; instead the 16-byte chunk c of tile row r is kept at
// chunk position c ^ (r & 15), which makes both fragment reads (32 keys x one chunk for K, one key x 32 floats for
// V) bank-conflict free.  Keys past T are clamped to the last row (their scores are masked, so p = 0).
// Everything in fp32 on v_mfma_f32_32x32x2_f32:
//   S^T[key, q]  = K_tile . Q^T     A = K rows from LDS, B = Q (32 registers per lane, pre-scaled by log2(e)/8)
//   the MFMA C layout gives a lane ONE query (q = lane & 31) and 16 keys, so the running max / sum of the online
//   softmax are per-lane scalars plus one exchange between the two lane halves; p = 2^(s - m) on v_exp_f32;
//   O^T[d, q]   += V^T . P^T        B = P straight from the S^T accumulator registers: register r of lane half h is
//   key (r&3) + 8(r>>2) + 4h, and a 32x32x2 step may pair ANY two keys as long as the A operand (V from LDS) uses
//   the same two -- no transpose of P through LDS.
// On this part VALU instructions and fp32 MFMAs do not overlap, not even from different waves of a SIMD
// (scripts/micro/mfma_rate.hip: 16 MFMAs + 2N VALU instructions take 1024 + 8N cycles at any occupancy), so every
// non-MFMA instruction in the tile loop costs matrix time: ~150 per tile now (exp2, max, sum, rescale, swizzled
// addresses) against 4096 MFMA cycles.
// qkv is the [B, T, 3, H, 64] output of the fused qkv projection, out is [B, T, H*64] (what the output projection
// reads): no permute / contiguous copies around the call.
//
// K9L (mcd_vit_attention_long): the same workgroup body (attn_block) for the high-resolution towers, T up to 32 768
// (1024 x 1024 at patch 16 is 4 097 tokens, Mammo-CLIP's 1520 x 912 is 5 416): one workgroup per block of 256 queries
// of a head, each streaming all of the head's key tiles.  At T = 4 097 attention is half of the tower's flops; PyTorch's
// fp32 SDPA (its memory-efficient kernel) ran the same shapes at 0.56-0.60 of the fp32 MFMA peak, K9L at 0.68-0.71.
//
// K9M (mcd_vit_attention_keylen): K9 with a key count per sequence, for the BERT text tower's padded batches
//     model/modules/text_encoder.py:48  BertModel(**tokens) under a key-padding attention_mask (ones, then zeros)
// Sequence b attends to keys 0 .. L-1, L = clamp(lens[b], 1, T) -- lens lives on the device, the host cannot see it, so
// the clamp is the kernel's.  The same workgroup body with L as the key count: ceil(L / 32) tiles (a short sequence in a
// long batch skips its padded tiles), the loader clamps to row L-1, so no K or V row >= L is read and a NaN there reaches
// nothing.  Rows 0 .. L-1 are K9's bits on the sequence truncated to L tokens; the padded query rows are computed too
// (BertModel and SDPA do the same).  A NaN in q reaches that output row of that head only; +-Inf inputs: unspecified.
//
// K9A (mcd_vit_attention_causal, include/mcd_clip.h): K9 under a causal mask, for OpenAI CLIP's text transformer
//     concept_vit/clip/model.py:181-183, :324-330  nn.MultiheadAttention under attn_mask = triu(-inf, 1)
// Query t attends to keys 0 .. t.  Compute wave w (queries 32w .. 32w+31) needs the key tiles 0 .. w only: its tile loop
// ends after tile w, where the keys above the lane's own query get -inf in place of K9's end-of-sequence mask, and it then
// meets the loader at the remaining pair barriers with nothing between them.  Tile count, masked key set and online-softmax
// steps of row t are those of K9 on the sequence truncated to t + 1 tokens: the same bits, whatever follows token t.
//
// K9C (mcd_vit_attention_cls): attention for ONE query row per image -- the class token of the last encoder block, the
// only row of that block anything downstream reads (concept_vit/data_utils.py, cls_tail_route).  2 * 64 flops per 512
// bytes of K and V: a streaming kernel, bound by reading every K and V head row once (2 * B * T * H * 256 bytes), not
// by the matrix pipe.  No MFMA, no LDS staging: a 16-lane DPP row holds one 256-byte head row (float4 per lane), so one
// wave instruction reads four whole rows; the 64-term dot product is 4 fmas per lane and 4 DPP adds inside the row.
// Each 16-lane row keeps its own online-softmax stream (running max, sum and a float4 of the output) over the key rows
// it sees, AC_U loads of K and of V in flight per wave; the 4 (T <= 512) or 16 streams of an (image, head) pair meet
// once, through 4 KB of LDS.  q, k and v come with their own row / image strides: the [B, T, 2, H, 64] output of a
// K|V-only projection and a plain [B, T, 3, H, 64] qkv are both addressed in place.
#include "mcd_common.h"
#include "../../include/mcd_text.h"
#include "../../include/mcd_clip.h"
#include "../../include/mcd_sentence.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int AT_D = 64;           // head dimension
constexpr int AT_MAX_T = 256;      // 8 compute waves + the loader
constexpr int AT_LONG_MAX_T = 32768;   // the long form (2048 x 2048 at patch 16 is 16 385 tokens)
constexpr int AT_HALF = 32 * 256;  // bytes of a K (or V) tile
constexpr int AT_STAGE = 2 * AT_HALF;
constexpr int AT_NSTAGE = 4;       // ring of tiles: two pairs
constexpr int AT_REL = 2 * AT_MAX_T + 32;   // K9B's staged biases: 2T-1 distances + the masked keys of a short last tile

// The workgroup body of both forms: queries q0 .. q0 + 32 * ncw - 1 of head h of image b, one compute wave per 32 of
// them (waves 0 .. ncw-1), wave ncw the loader; all ntile key tiles of (b, h) go through the LDS ring.  Which block a
// query sits in does not enter its arithmetic: the long form gives K9's bits wherever both run.
// KEYLEN (K9M): the keys are rows 0 .. L-1 of the sequence (1 <= L <= T, uniform over the workgroup) -- L takes T's place
// in the tile count, in the loader's clamp and in the mask of the last tile, so no K or V row >= L is read; T keeps the
// row strides and the query count.  Without KEYLEN the key count IS T (L is not looked at): K9 and K9L as they were.
// CAUSAL (K9A): query q sees keys 0 .. q.  The loader stages every tile as always; compute wave w walks tiles
// 0 .. (q0 / 32) + w, masks the keys above each lane's query in the last of them, and idles through the pair barriers left.
// BIAS (K9B): rel points at this head's 2T-1 biases, one per key-minus-query distance d = -(T-1) .. T-1.  All waves stage
// them once, times log2(e) (the scores live in the log2 domain), into at_rel[d + T - 1], and the tile loop adds
// at_rel[key - q + T - 1] to every score in front of the mask.  Only the distances |d| <= L-1 of the sequence's own L keys
// are read from global memory: a padded query row t >= L takes the bias of d = -(L-1) for the distances below it, and the
// slots that only masked keys of the last tile address (d up to L + 30) hold zero.  A query lane past T works on row T-1,
// as its q fragment does.  Lanes 0 .. 31 of a read address 32 consecutive floats: no bank conflict.
template <bool KEYLEN, bool CAUSAL = false, bool BIAS = false>
__device__ __forceinline__ void attn_block(const float* __restrict__ qkv, int T, int H, int64_t b, int h, int q0, int ncw,
                                           int L, float* __restrict__ out, const float* __restrict__ rel = nullptr) {
    __shared__ __attribute__((aligned(1024))) char at_lds[AT_NSTAGE * AT_STAGE];   // [stage][K | V][32 rows x 256 B]
    const float* rel_s = nullptr;
    if constexpr (BIAS) {
        __shared__ float at_rel[AT_REL];
        for (int i = threadIdx.x; i < AT_REL; i += blockDim.x) {
            const int d = i - (T - 1);
            at_rel[i] = d < L ? rel[max(d, 1 - L) + T - 1] * 1.44269504088896340736f : 0.f;
        }
        rel_s = at_rel;
        __syncthreads();
    }
    const int TK = KEYLEN ? L : T;     // keys
    const int ntile = (TK + 31) >> 5;
    const int64_t row_stride = (int64_t)3 * H * AT_D;                 // floats between two tokens of qkv
    const float* base = qkv + b * T * row_stride + (int64_t)h * AT_D;  // q of token 0; k at +H*64, v at +2*H*64
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ql = lane & 31, half = lane >> 5;
    const int q = q0 + wave * 32 + ql;

    if (wave == ncw) {
        // ---- loader wave: DMA of tile kt into its ring slot; piece p (0..7) = tile rows 4p..4p+3 of K and of V ----
        // BUFFER-load DMA (SGPR descriptor of this image's qkv block + one 32-bit VGPR offset per lane): beside waves that
        // keep the matrix pipe busy, global_load_lds with a 64-bit address pair per lane issues 3-4x slower
        // (scripts/micro/ldsdma_rate.hip).  One image's block is T * 3 * H * 64 floats (1.8 MB at ViT-B/16, 151 MB at
        // T = 16 385): 32-bit offsets; the image's base address is formed in 64 bits.
        auto stage = [&](int kt) {
            __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(qkv + b * T * row_stride), 0,
                                                                            (int)(T * row_stride * 4), 0x00020000);
            char* dst = at_lds + (kt % AT_NSTAGE) * AT_STAGE;
            const int v_off = H * AT_D * 4;                               // bytes from a token's k to its v
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int r = 4 * p + (lane >> 4);
                const int c = (lane & 15) ^ (r & 15);
                int key = kt * 32 + r;
                if (key >= TK) key = TK - 1;
                const unsigned off = (unsigned)(((int64_t)key * row_stride + (int64_t)(h + H) * AT_D + c * 4) * 4);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(dst + p * 1024), 16, off, 0, 0, 0);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(dst + AT_HALF + p * 1024), 16, off,
                                                         v_off, 0, 0);
            }
        };
        // Tiles travel in pairs (one barrier per 64 keys): pair g is in flight while pair g-1 is consumed.
        stage(0);
        if (ntile > 1) stage(1);
        for (int kt = 0; kt < ntile; kt += 2) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the pair kt, kt+1 has landed
            __builtin_amdgcn_s_barrier();                      // ... and everyone is done with the pair before it,
            asm volatile("" ::: "memory");                     // whose two slots the next pair refills
            if (kt + 2 < ntile) stage(kt + 2);
            if (kt + 3 < ntile) stage(kt + 3);
        }
        return;
    }

    // Q fragment: step s = 4j + e of the S^T product uses d = 8j + 4*half + e.  Scores are kept in the log2 domain.
    const float qs = 0.125f * 1.44269504088896340736f;
    float Qr[32];
    const float* qrow = base + (int64_t)(q < T ? q : T - 1) * row_stride + 4 * half;   // rows past T: computed, not stored
    float4 qv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) qv[j] = *reinterpret_cast<const float4*>(qrow + 8 * j);   // eight loads in flight
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float4 t = qv[j];
        Qr[4 * j + 0] = t.x * qs;
        Qr[4 * j + 1] = t.y * qs;
        Qr[4 * j + 2] = t.z * qs;
        Qr[4 * j + 3] = t.w * qs;
    }

    // per-lane parts of the swizzled fragment addresses
    const int kx = ql & 15;                              // K: chunk (2j + half) of row ql sits at (2j + half) ^ kx
    const int k_off = ql * 256;
    const int v_row = 4 * half * 256 + (ql & 3) * 4;     // V: key k0 + 4*half, float 32i + ql -> chunk 8i + (ql >> 2)
    const int va = (ql >> 2) ^ (half << 2);              //    at ((8i) ^ (key & 8)) | (va ^ (k0 & 3))

    f32x16 o[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
    float m = -INFINITY, l = 0.f;
    const int rel_q = T - 1 - (q < T ? q : T - 1) + 4 * half;   // BIAS: at_rel index of this lane's key 0 of tile 0

    // CAUSAL: the diagonal tile is this wave's last (it exists: wave < ncw and q0 + 32 * wave < T for every launched wave)
    const int ntile_w = CAUSAL ? min(ntile, (q0 >> 5) + wave + 1) : ntile;
    for (int kt = 0; kt < ntile_w; ++kt) {
        if ((kt & 1) == 0) __builtin_amdgcn_s_barrier();   // the loader says tiles kt and kt+1 are in LDS
        asm volatile("" ::: "memory");
        const char* kb = at_lds + (kt % AT_NSTAGE) * AT_STAGE;
        const char* vb = kb + AT_HALF;
        // the swizzled offsets are recomputed every tile (a xor and an add each): hoisted out of the loop they cost
        // a dozen registers and the kernel spills at the 128 it may use
        int kx_t = kx, va_t = va;
        asm volatile("" : "+v"(kx_t), "+v"(va_t));
        int v_off[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v_off[e] = v_row + ((va_t ^ e) << 4);

        f32x16 c;
#pragma unroll
        for (int r = 0; r < 16; ++r) c[r] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float4 ka = *reinterpret_cast<const float4*>(kb + k_off + (((2 * j + half) ^ kx_t) << 4));
            c = __builtin_amdgcn_mfma_f32_32x32x2f32(ka.x, Qr[4 * j + 0], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x2f32(ka.y, Qr[4 * j + 1], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x2f32(ka.z, Qr[4 * j + 2], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x2f32(ka.w, Qr[4 * j + 3], c, 0, 0, 0);
        }
        if constexpr (BIAS) {
            const float* rb = rel_s + rel_q + kt * 32;
#pragma unroll
            for (int r = 0; r < 16; ++r) c[r] += rb[(r & 3) + 8 * (r >> 2)];
        }
        if constexpr (CAUSAL) {
            // the diagonal tile: key 32 kt + j is above query 32 kt + ql when j > ql.  That covers the keys past T of a
            // short last tile (a stored row has q < T <= key), so K9's mask is not needed beside it; key 32 kt itself is
            // never masked and the running maximum stays finite.
            if (kt == ntile_w - 1) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if ((r & 3) + 8 * (r >> 2) + 4 * half > ql) c[r] = -INFINITY;
            }
        } else {
            const int nk = TK - kt * 32;   // valid keys in this tile (>= 1)
            if (nk < 32) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if ((r & 3) + 8 * (r >> 2) + 4 * half >= nk) c[r] = -INFINITY;
            }
        }
        float mt = c[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mt = fmaxf(mt, c[r]);
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float m_new = fmaxf(m, mt);                       // finite: key kt*32 is valid (lane half 0 holds it)
        const float alpha = __builtin_amdgcn_exp2f(m - m_new);  // first tile: 2^-inf = 0
        float ls = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            c[r] = __builtin_amdgcn_exp2f(c[r] - m_new);
            ls += c[r];
        }
        l = l * alpha + ls;                                     // per lane half; the halves are added at the end
        m = m_new;
        // (rescaling only when some lane's maximum moves by more than 2^8 -- "lazy rescaling" -- measured no gain)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
        // step r pairs the keys k0 and k0 + 4 (k0 = (r&3) + 8(r>>2)); row k0 + 4*half, and (key & 8) = (k0 & 8):
        // chunk 8i + .. of that row sits at ((8i) ^ (k0 & 8)) | ..   A clamped key past T has p = 0.
        auto pv_step = [&](int r) {
            const int k0 = (r & 3) + 8 * (r >> 2);
            const char* vr = vb + k0 * 256 + v_off[r & 3];
            const float v0 = *reinterpret_cast<const float*>(vr + ((0 ^ (k0 & 8)) << 4));
            const float v1 = *reinterpret_cast<const float*>(vr + ((8 ^ (k0 & 8)) << 4));
            o[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(v0, c[r], o[0], 0, 0, 0);
            o[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(v1, c[r], o[1], 0, 0, 0);
        };
        // No branch around the steps, not even for a short last tile (its masked keys have p = 0): a branch per step
        // makes the compiler wait for each MFMA result and copy the accumulators, a branch per tile still costs a
        // copy of all 32 accumulator registers where the two paths meet.
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if ((r & 3) == 0 && r) asm volatile("" ::: "memory");   // keep the V reads of later groups from piling up
            pv_step(r);
        }
    }

    l = l + __shfl_xor(l, 32);
    if (q < T) {
        const float inv = 1.0f / l;
        float* dst = out + (b * T + q) * (int64_t)H * AT_D + (int64_t)h * AT_D + 4 * half;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {   // registers 4g..4g+3 = d 32i + 8g + 4*half + 0..3
                const float4 t = make_float4(o[i][4 * g + 0] * inv, o[i][4 * g + 1] * inv, o[i][4 * g + 2] * inv,
                                             o[i][4 * g + 3] * inv);
                *reinterpret_cast<float4*>(dst + 32 * i + 8 * g) = t;
            }
    }
    if constexpr (CAUSAL) {
        // the pair barriers of the tiles above the diagonal: a second, empty loop -- the loader counts on every wave at
        // every barrier, and a branch around the tile loop's body would cost what the comment on pv_step says
        for (int kt = (ntile_w + 1) & ~1; kt < ntile; kt += 2) __builtin_amdgcn_s_barrier();
    }
}

// K9: one workgroup per (image, head), one compute wave per 32 queries (T <= 256) + the loader.
__global__ __launch_bounds__(576, 4) void vit_attention_kernel(const float* __restrict__ qkv, int T, int H,
                                                                float* __restrict__ out) {
    const int ntile = (T + 31) >> 5;
    const int h = blockIdx.x;
    const int64_t b = blockIdx.y;
    attn_block<false>(qkv, T, H, b, h, 0, ntile, T, out);
}

// K9M: K9's grid and waves (one compute wave per 32 QUERIES, so ceil(T / 32) of them + the loader) with a key count per
// sequence: L = clamp(lens[b], 1, T), T without lens.  Every query row t < T is computed and stored, rows >= L included
// (they attend to the L valid keys, as SDPA's rows under a key-padding mask do).
__global__ __launch_bounds__(576, 4) void vit_attention_keylen_kernel(const float* __restrict__ qkv, int T, int H,
                                                                       const int32_t* __restrict__ lens,
                                                                       float* __restrict__ out) {
    const int ncw = (T + 31) >> 5;
    const int h = blockIdx.x;
    const int64_t b = blockIdx.y;
    int L = T;
    if (lens) L = min(max(lens[b], 1), T);
    attn_block<true>(qkv, T, H, b, h, 0, ncw, __builtin_amdgcn_readfirstlane(L), out);
}

// K9B: K9M with the per-head relative-position bias of MPNet's attention added to every score (include/mcd_sentence.h).
//     transformers MPNetSelfAttention.forward: attention_scores / 8 + position_bias (+ the key mask)
// The bias of MPNetEncoder.compute_position_bias is a function of head and key - query alone -- a Toeplitz matrix per head,
// the same in every layer and for every sequence -- so the operand is the [H, 2T-1] table of its diagonals, never [H, T, T].
__global__ __launch_bounds__(576, 4) void vit_attention_relbias_kernel(const float* __restrict__ qkv, int T, int H,
                                                                        const int32_t* __restrict__ lens,
                                                                        const float* __restrict__ rel,
                                                                        float* __restrict__ out) {
    const int ncw = (T + 31) >> 5;
    const int h = blockIdx.x;
    const int64_t b = blockIdx.y;
    int L = T;
    if (lens) L = min(max(lens[b], 1), T);
    attn_block<true, false, true>(qkv, T, H, b, h, 0, ncw, __builtin_amdgcn_readfirstlane(L), out,
                                  rel + (int64_t)h * (2 * T - 1));
}

// K9A: K9's grid and waves under the causal mask.
__global__ __launch_bounds__(576, 4) void vit_attention_causal_kernel(const float* __restrict__ qkv, int T, int H,
                                                                       float* __restrict__ out) {
    const int ntile = (T + 31) >> 5;
    const int h = blockIdx.x;
    const int64_t b = blockIdx.y;
    attn_block<false, true>(qkv, T, H, b, h, 0, ntile, T, out);
}

// K9L, the long form: one workgroup per (image, head, block of 32 * ncw queries), ncw = min(8, ceil(T / 32)).  Every
// workgroup streams all of its (image, head)'s key tiles, so the nqb query blocks of one (image, head) read the same
// K / V (2.1 MB at T = 4 097).  Placement, for speed only: workgroups are dealt round-robin over the 8 XCDs, so
// workgroup w runs on XCD slot w % 8.  The npairs = B * H * nqb (group, query block) pairs, group-major, are cut into
// 8 runs of per_xcd consecutive pairs, and slot x takes run x in order: the blocks of a group share one XCD's L2 (a
// group at a run's edge spans two), the load is even to one block, and at any moment each XCD works on one or two
// groups.  The <= 7 workgroups past npairs return at once, before any barrier.  A last block that reaches past T
// computes its surplus waves on clamped query rows (as K9's last wave does) and stores nothing for them: every wave
// meets the loader at every barrier.
__global__ __launch_bounds__(576, 4) void vit_attention_long_kernel(const float* __restrict__ qkv, int T, int H, int nqb,
                                                                     int npairs, int per_xcd, float* __restrict__ out) {
    const int pair = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
    if (pair >= npairs) return;
    const int grp = pair / nqb;                    // b * H + h
    const int ncw = min(8, (T + 31) >> 5);
    attn_block<false>(qkv, T, H, grp / H, grp % H, (pair - grp * nqb) * 32 * ncw, ncw, T, out);
}

// ---- K9C ----------------------------------------------------------------------------------------------------------------
constexpr int AC_WAVES = 4;        // waves per workgroup
constexpr int AC_U = 4;            // four-row loads of K (and of V) in flight per wave
constexpr int AC_SPLIT_T = 512;    // longer sequences: the four waves of a workgroup share one (image, head) pair
constexpr int AC_MAX_T = 32768;

// x + (x of the lane that the DPP control pairs this one with, inside its 16-lane row)
template <int CTRL>
__device__ __forceinline__ float ac_dpp_add(float x) {
    return x + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true));
}

// The sum over the 16 lanes of a DPP row, in every lane of it: lane ^ 1, lane ^ 2 (quad_perm), then the other quad of the
// half row (row_half_mirror) and the other half (row_mirror) -- after each step the lanes it pairs hold equal sums.
__device__ __forceinline__ float ac_row_sum(float x) {
    x = ac_dpp_add<0xB1>(x);
    x = ac_dpp_add<0x4E>(x);
    x = ac_dpp_add<0x141>(x);
    return ac_dpp_add<0x140>(x);
}

// One workgroup = AC_WAVES waves; S of them (1 or 4) share an (image, head) pair.  Key row j of a pair belongs to wave
// slice (j / 4) % S, lane row j % 4; lane `sub` of a row holds floats 4 sub .. 4 sub + 3 of the 64.
__global__ __launch_bounds__(64 * AC_WAVES) void vit_attention_cls_kernel(
    const float* __restrict__ q, int64_t q_img, const float* __restrict__ k, int64_t k_row, int64_t k_img,
    const float* __restrict__ v, int64_t v_row, int64_t v_img, int T, int H, int64_t npairs, int S, float* __restrict__ out) {
    __shared__ float4 st_acc[AC_WAVES * 4][16];
    __shared__ float st_m[AC_WAVES * 4], st_l[AC_WAVES * 4];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sub = lane & 15, g = lane >> 4;
    const int64_t pair = (int64_t)blockIdx.x * (AC_WAVES / S) + wave / S;   // b * H + h
    const int slice = wave % S;
    const bool live = pair < npairs;

    // a finite floor instead of -inf: a stream that has seen no key yet (T < 4 S: it never will) keeps alpha = 2^0 = 1
    float m = -1e30f, l = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
        const int64_t b = pair / H;
        const int h = (int)(pair - b * H);
        const float qs = 0.125f * 1.44269504088896340736f;   // scores in the log2 domain, like K9
        float4 qv = *reinterpret_cast<const float4*>(q + b * q_img + (int64_t)h * AT_D + 4 * sub);
        qv.x *= qs; qv.y *= qs; qv.z *= qs; qv.w *= qs;
        const int r0 = slice * 4 + g;
        const float* kp = k + b * k_img + (int64_t)r0 * k_row + (int64_t)h * AT_D + 4 * sub;
        const float* vp = v + b * v_img + (int64_t)r0 * v_row + (int64_t)h * AT_D + 4 * sub;
        const int64_t kstep = (int64_t)4 * S * k_row, vstep = (int64_t)4 * S * v_row;
        for (int rb = slice * 4; rb < T; rb += 4 * S * AC_U) {
            float4 kk[AC_U], vv[AC_U];
            bool ok[AC_U];
#pragma unroll
            for (int u = 0; u < AC_U; ++u) {
                ok[u] = rb + u * 4 * S + g < T;
                kk[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                vv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ok[u]) {
                    kk[u] = *reinterpret_cast<const float4*>(kp + u * kstep);
                    vv[u] = *reinterpret_cast<const float4*>(vp + u * vstep);
                }
            }
            kp += AC_U * kstep;
            vp += AC_U * vstep;
            float s[AC_U];
            float mt = m;
#pragma unroll
            for (int u = 0; u < AC_U; ++u) {
                const float d = fmaf(kk[u].w, qv.w, fmaf(kk[u].z, qv.z, fmaf(kk[u].y, qv.y, kk[u].x * qv.x)));
                const float r = ac_row_sum(d);     // in every lane: the DPP adds read their row's other lanes
                s[u] = ok[u] ? r : -INFINITY;      // a row past T gets p = 0
                mt = fmaxf(mt, s[u]);
            }
            const float alpha = __builtin_amdgcn_exp2f(m - mt);
            m = mt;
            l *= alpha;
            acc.x *= alpha; acc.y *= alpha; acc.z *= alpha; acc.w *= alpha;
#pragma unroll
            for (int u = 0; u < AC_U; ++u) {
                const float p = __builtin_amdgcn_exp2f(s[u] - mt);
                l += p;
                acc.x = fmaf(p, vv[u].x, acc.x);
                acc.y = fmaf(p, vv[u].y, acc.y);
                acc.z = fmaf(p, vv[u].z, acc.z);
                acc.w = fmaf(p, vv[u].w, acc.w);
            }
        }
    }
    st_acc[wave * 4 + g][sub] = acc;
    if (sub == 0) {
        st_m[wave * 4 + g] = m;
        st_l[wave * 4 + g] = l;
    }
    __syncthreads();
    if (live && slice == 0) {
        // this pair's 4 S streams are those of waves wave .. wave + S - 1; lane d of the slice-0 wave finishes float d
        const int s0 = wave * 4, ns = 4 * S;
        float mx = st_m[s0];
        for (int i = 1; i < ns; ++i) mx = fmaxf(mx, st_m[s0 + i]);   // finite: key 0 is in stream s0
        float num = 0.f, den = 0.f;
        const float* accf = reinterpret_cast<const float*>(&st_acc[s0][0]);
        for (int i = 0; i < ns; ++i) {
            const float w = __builtin_amdgcn_exp2f(st_m[s0 + i] - mx);
            num = fmaf(accf[i * 64 + lane], w, num);
            den = fmaf(st_l[s0 + i], w, den);
        }
        out[pair * AT_D + lane] = num / den;
    }
}

// The checks and the launch of K9, K9M, K9B and K9A (`name` is the entry's, for the messages).  lens and rel are the extra
// operands of K9M and K9B (NULL elsewhere, and NULL is aligned), `aligned` the entry's sentence about all of them.
// launch(grid, block) starts the entry's kernel and returns that kernel's name.
template <typename Launch>
int attention_entry(const char* name, const float* qkv, int64_t B, int64_t T, int64_t H, const int32_t* lens, const float* rel,
                    const char* aligned, float* out, Launch launch) {
    MCD_REQUIRE(qkv && out, MCD_E_ARG, "%s: NULL pointer", name);
    MCD_REQUIRE(B >= 0 && T >= 1 && H >= 1, MCD_E_ARG, "%s: bad shape B=%lld T=%lld H=%lld", name, (long long)B, (long long)T,
                (long long)H);
    MCD_REQUIRE(T <= AT_MAX_T, MCD_E_UNSUPPORTED, "%s: T=%lld tokens, at most %d (one wave per 32 queries, 8 waves)", name,
                (long long)T, AT_MAX_T);
    MCD_REQUIRE(B <= 65535 && H <= 65535, MCD_E_UNSUPPORTED, "%s: B and H must be <= 65535", name);
    MCD_REQUIRE(((uintptr_t)qkv) % 16 == 0 && ((uintptr_t)out) % 16 == 0 && ((uintptr_t)lens) % 4 == 0 &&
                    ((uintptr_t)rel) % 16 == 0,
                MCD_E_ARG, "%s: %s", name, aligned);
    if (B == 0) return MCD_OK;
    const int nwaves = (int)((T + 31) / 32) + 1;   // one per 32 queries + the loader
    const char* kernel = launch(dim3((unsigned)H, (unsigned)B), dim3(64 * nwaves));
    MCD_LAUNCH_CHECK(kernel);
    return MCD_OK;
}

}  // namespace

extern "C" int mcd_vit_attention(const float* qkv, int64_t B, int64_t T, int64_t H, float* out, mcd_stream_t stream) {
    const auto launch = [&](dim3 grid, dim3 block) {
        hipLaunchKernelGGL(vit_attention_kernel, grid, block, 0, (hipStream_t)stream, qkv, (int)T, (int)H, out);
        return "vit_attention_kernel";
    };
    return attention_entry("mcd_vit_attention", qkv, B, T, H, nullptr, nullptr, "qkv and out must be 16-byte aligned", out, launch);
}

extern "C" int mcd_vit_attention_keylen(const float* qkv, int64_t B, int64_t T, int64_t H, const int32_t* lens, float* out,
                                        mcd_stream_t stream) {
    const auto launch = [&](dim3 grid, dim3 block) {
        hipLaunchKernelGGL(vit_attention_keylen_kernel, grid, block, 0, (hipStream_t)stream, qkv, (int)T, (int)H, lens, out);
        return "vit_attention_keylen_kernel";
    };
    return attention_entry("mcd_vit_attention_keylen", qkv, B, T, H, lens, nullptr,
                           "qkv and out must be 16-byte aligned, lens 4-byte aligned", out, launch);
}

extern "C" int mcd_vit_attention_relbias(const float* qkv, int64_t B, int64_t T, int64_t H, const int32_t* lens,
                                         const float* rel, float* out, mcd_stream_t stream) {
    const auto launch = [&](dim3 grid, dim3 block) {
        if (!rel) {   // no bias: K9M's own kernel, K9M's bits
            hipLaunchKernelGGL(vit_attention_keylen_kernel, grid, block, 0, (hipStream_t)stream, qkv, (int)T, (int)H, lens, out);
            return "vit_attention_keylen_kernel";
        }
        hipLaunchKernelGGL(vit_attention_relbias_kernel, grid, block, 0, (hipStream_t)stream, qkv, (int)T, (int)H, lens, rel, out);
        return "vit_attention_relbias_kernel";
    };
    return attention_entry("mcd_vit_attention_relbias", qkv, B, T, H, lens, rel,
                           "qkv, out and rel must be 16-byte aligned, lens 4-byte aligned", out, launch);
}

extern "C" int mcd_vit_attention_causal(const float* qkv, int64_t B, int64_t T, int64_t H, float* out, mcd_stream_t stream) {
    const auto launch = [&](dim3 grid, dim3 block) {
        hipLaunchKernelGGL(vit_attention_causal_kernel, grid, block, 0, (hipStream_t)stream, qkv, (int)T, (int)H, out);
        return "vit_attention_causal_kernel";
    };
    return attention_entry("mcd_vit_attention_causal", qkv, B, T, H, nullptr, nullptr, "qkv and out must be 16-byte aligned", out,
                           launch);
}

extern "C" int mcd_vit_attention_long(const float* qkv, int64_t B, int64_t T, int64_t H, float* out, mcd_stream_t stream) {
    MCD_REQUIRE(qkv && out, MCD_E_ARG, "mcd_vit_attention_long: NULL pointer");
    MCD_REQUIRE(B >= 0 && T >= 1 && H >= 1, MCD_E_ARG, "mcd_vit_attention_long: bad shape B=%lld T=%lld H=%lld",
                (long long)B, (long long)T, (long long)H);
    MCD_REQUIRE(T <= AT_LONG_MAX_T, MCD_E_UNSUPPORTED, "mcd_vit_attention_long: T=%lld tokens, at most %d", (long long)T,
                AT_LONG_MAX_T);
    MCD_REQUIRE(B <= INT32_MAX && H <= 65535, MCD_E_UNSUPPORTED, "mcd_vit_attention_long: B must be < 2^31, H <= 65535");
    MCD_REQUIRE(T * 3 * H * AT_D * 4 <= INT32_MAX, MCD_E_UNSUPPORTED,
                "mcd_vit_attention_long: one image's qkv block (T=%lld x H=%lld heads) must stay under 2^31 bytes",
                (long long)T, (long long)H);
    MCD_REQUIRE(((uintptr_t)qkv) % 16 == 0 && ((uintptr_t)out) % 16 == 0, MCD_E_ARG,
                "mcd_vit_attention_long: qkv and out must be 16-byte aligned");
    if (B == 0) return MCD_OK;
    const int64_t ncw = std::min<int64_t>(8, (T + 31) / 32);   // compute waves per workgroup
    const int64_t nqb = mcd_cdiv((T + 31) / 32, ncw);            // query blocks per (image, head)
    const int64_t npairs = B * H * nqb;
    MCD_REQUIRE(npairs <= INT32_MAX / 576 - 8, MCD_E_UNSUPPORTED,
                "mcd_vit_attention_long: B=%lld x H=%lld x %lld query blocks is too large a grid", (long long)B,
                (long long)H, (long long)nqb);
    const int64_t per_xcd = mcd_cdiv(npairs, 8);
    hipLaunchKernelGGL(vit_attention_long_kernel, dim3((unsigned)(8 * per_xcd)), dim3(64 * (unsigned)(ncw + 1)), 0,
                       (hipStream_t)stream, qkv, (int)T, (int)H, (int)nqb, (int)npairs, (int)per_xcd, out);
    MCD_LAUNCH_CHECK("vit_attention_long_kernel");
    return MCD_OK;
}

extern "C" int mcd_vit_attention_cls(const float* q, int64_t q_img, const float* k, int64_t k_row, int64_t k_img,
                                     const float* v, int64_t v_row, int64_t v_img, int64_t B, int64_t T, int64_t H,
                                     float* out, mcd_stream_t stream) {
    MCD_REQUIRE(q && k && v && out, MCD_E_ARG, "mcd_vit_attention_cls: NULL pointer");
    MCD_REQUIRE(B >= 0 && T >= 1 && H >= 1, MCD_E_ARG, "mcd_vit_attention_cls: bad shape B=%lld T=%lld H=%lld", (long long)B,
                (long long)T, (long long)H);
    MCD_REQUIRE(T <= AC_MAX_T, MCD_E_UNSUPPORTED, "mcd_vit_attention_cls: T=%lld tokens, at most %d", (long long)T, AC_MAX_T);
    MCD_REQUIRE(H <= 65535 && B <= INT32_MAX / 65535, MCD_E_UNSUPPORTED,
                "mcd_vit_attention_cls: H must be <= 65535 and B * 65535 < 2^31");
    const int64_t W = H * AT_D;
    MCD_REQUIRE(q_img >= W && k_row >= W && v_row >= W && k_img >= W && v_img >= W, MCD_E_ARG,
                "mcd_vit_attention_cls: a stride (q_img=%lld k_row=%lld k_img=%lld v_row=%lld v_img=%lld) is below H*64=%lld",
                (long long)q_img, (long long)k_row, (long long)k_img, (long long)v_row, (long long)v_img, (long long)W);
    MCD_REQUIRE(((uintptr_t)q) % 16 == 0 && ((uintptr_t)k) % 16 == 0 && ((uintptr_t)v) % 16 == 0 && ((uintptr_t)out) % 16 == 0 &&
                    q_img % 4 == 0 && k_row % 4 == 0 && k_img % 4 == 0 && v_row % 4 == 0 && v_img % 4 == 0,
                MCD_E_ARG, "mcd_vit_attention_cls: pointers must be 16-byte aligned and strides multiples of 4 floats");
    if (B == 0) return MCD_OK;
    const int S = T > AC_SPLIT_T ? AC_WAVES : 1;
    const int64_t npairs = B * H;
    const int64_t nwg = mcd_cdiv(npairs, (int64_t)(AC_WAVES / S));
    hipLaunchKernelGGL(vit_attention_cls_kernel, dim3((unsigned)nwg), dim3(64 * AC_WAVES), 0, (hipStream_t)stream, q, q_img, k,
                       k_row, k_img, v, v_row, v_img, (int)T, (int)H, npairs, S, out);
    MCD_LAUNCH_CHECK("vit_attention_cls_kernel");
    return MCD_OK;
}
