/*
 * mcd_hip.h -- C ABI of libmcd_hip.so: the MI355X (gfx950) dissection core of
 * Mammo-CLIP-Dissect, hand-written HIP.
 *
 * The reference is pure Python: its "operator interface" for this path is the set of torch
 * calls inside concept_vit/similarity.py and around it in concept_vit/utils.py and the
 * describe_*_neurons.py drivers.  Each entry point below replaces one of those call sites
 * (file:line relative to the reference root).  Plain pointers and sizes only: every pointer
 * is a DEVICE pointer (HBM) unless stated, the caller owns every buffer, nothing is
 * allocated or synchronised inside, every call is asynchronous on `stream`
 * (a hipStream_t passed as void*; NULL = the default stream) and is hipGraph-capturable.
 *
 * Return value: 0 on success; negative on error (MCD_E_*), with a human readable message in
 * mcd_last_error() (thread local).  No call ever falls back to a CPU path.
 *
 * Layout vocabulary:
 *   N images, C concepts, D embedding width, U neurons (of one layer or of all layers
 *   concatenated), K = top_k activating images per neuron.
 *   "image-major"  [N, U]: element (n,u) at base[n*ld + u]   (what torch.cat of hook outputs gives)
 *   "neuron-major" [U, N]: element (n,u) at base[u*ld + n]   (what the fused pipeline keeps in HBM)
 *
 * The text tower's entries of this library -- K9M mcd_vit_attention_keylen (K9 with a key count per sequence) and K24
 * mcd_text_embed_ln (BERT's embedding rows in one launch) -- are declared in mcd_text.h, which includes this header and
 * follows every convention above.  They are additive: mcd_abi_version() stays 9.
 * The OpenAI-CLIP entries -- K9A mcd_vit_attention_causal (K9 under a causal mask) and K25 mcd_quick_gelu -- are declared in
 * mcd_clip.h in the same way.
 */
#ifndef MCD_HIP_H
#define MCD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mcd_stream_t; /* hipStream_t */

enum {
    MCD_OK = 0,
    MCD_E_ARG = -1,     /* bad shape / stride / alignment / NULL pointer */
    MCD_E_RANGE = -2,   /* k out of range (torch: "selected index k out of range") */
    MCD_E_WORKSPACE = -3,
    MCD_E_LAUNCH = -4,  /* hipGetLastError() after a launch */
    MCD_E_UNSUPPORTED = -5
};

/* GEMM arithmetic modes for mcd_embed_gemm */
enum {
    MCD_GEMM_F32 = 0,     /* v_mfma_f32_32x32x2_f32: exact fp32 fma chains over MKL's K-blocks (parity mode:
                             bit-identical to torch's CPU matmul for D <= 768 and D = 1024) */
    MCD_GEMM_BF16X3 = 1,  /* split-bf16 hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16, fp32 accumulate */
    MCD_GEMM_BF16 = 2     /* single-pass bf16 MFMA (stress config only; no parity claim) */
};

/* bits of the `soft` argument of mcd_wpmi_score */
enum { MCD_WPMI_SOFT = 1, MCD_WPMI_FAST_LOG = 2, MCD_WPMI_S_IS_PROB = 4 };

/* hook pooling modes for mcd_hook_pool */
enum { MCD_POOL_AVG = 0, MCD_POOL_MAX = 1, MCD_POOL_CLS = 2, MCD_POOL_NONE = 3,
       MCD_POOL_SILU_AVG = 4 /* mcd_hook_pool_nhwc only: mean over HW of SiLU(x) */ };

const char* mcd_last_error(void);
int mcd_abi_version(void);

/* ---------------------------------------------------------------------------------------------
 * K1a  rows of x scaled to unit L2 norm:  y[r,:] = x[r,:] / sqrt(sum_k x[r,k]^2)
 * replaces  image_features /= image_features.norm(dim=-1, keepdim=True)   concept_vit/utils.py:577
 *           text_features  /= text_features.norm(dim=-1, keepdim=True)    concept_vit/utils.py:578
 *           (same lines: og_utils.py:485-486, CLIP_og_utils.py:158-159)
 * y may alias x (the reference normalises in place).
 * ------------------------------------------------------------------------------------------- */
int mcd_normalize_rows(const float* x, int64_t ldx, int64_t n, int64_t d, float* y, int64_t ldy,
                       mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K7   per row r (length n):  d = x - mean(x);  c = d^3;  y = c / max(||c||_2, min_norm)
 * replaces  x - mean(dim=0); x**3; x / clip(norm(dim=0), min_norm)         concept_vit/similarity.py:15-22
 *           (cos_similarity_cubed; rows here are the reference's columns: the matrices are passed
 *           neuron-major / concept-major so that the image axis is contiguous).  y may alias x.
 * ------------------------------------------------------------------------------------------- */
int mcd_center_cube_normalize_rows(const float* x, int64_t ldx, int64_t rows, int64_t n, float min_norm,
                                   float* y, int64_t ldy, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K1a / K7 on rows that arrive in pieces: the rank-major message of an all-gather of neuron-major activation shards.
 *      src holds G blocks, block g at src + g*ld_block; row u of block g at + u*ld_src, its first counts[g] floats valid.
 *      The LOGICAL row u of length n = sum(counts) is the concatenation of its G pieces in block order.  For the rows
 *      row0 <= u < row1 the prepared logical row is written densely to dst + (u - row0)*ldd:
 *        mode 0: y = x / ||x||_2                                    bit-equal to mcd_normalize_rows on the logical row
 *        mode 1: d = x - mean(x); c = d^3; y = c / max(||c||, min_norm)   bit-equal to mcd_center_cube_normalize_rows
 *      (the same partition of logical indices over lanes, the same reduction trees, the same final division, for any
 *      G and counts, empty pieces included).  Every element is read and written without an intermediate copy.
 *      counts is a HOST array of G values (1 <= G <= 64); G = 1 with src = a neuron-major matrix is the plain
 *      row preparation.  dst must not overlap src.
 * replaces  the column normalisation of cos_similarity / cos_similarity_cubed   concept_vit/similarity.py:15-22, :40-41
 *           on activations sharded over the images (pipeline.Dissector.finish with more than one rank)
 * ------------------------------------------------------------------------------------------- */
int mcd_prepare_rows_gathered(const float* src, int64_t ld_src, int64_t ld_block, int G, const int64_t* counts,
                              int64_t n, int64_t row0, int64_t row1, int mode, float min_norm, float* dst, int64_t ldd,
                              mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K1   P[n,c] = sum_k I[n,k] * T[c,k]      (I: [N,D] ld ldi, T: [C,D] ld ldt, P: [N,C] ld ldp)
 * replaces  clip_feats = image_features @ text_features.T                 concept_vit/utils.py:594
 *           (og_utils.py:501, CLIP_og_utils.py:160)
 * ws: optional scratch of mcd_embed_gemm_workspace() bytes (0 for MCD_GEMM_F32 and for small problems).  With
 * it, the bf16 modes convert the operands to bf16 once and run the 256x256-tile kernel (the stress shape);
 * without it (NULL / fewer bytes than that / not 16-byte aligned) they run the 128x128 kernel that converts while staging and
 * leave ws alone -- same results per mode (MCD_OK either way: a workspace is never an error of this entry).
 * ------------------------------------------------------------------------------------------- */
size_t mcd_embed_gemm_workspace(int64_t N, int64_t C, int64_t D, int mode);
int mcd_embed_gemm(const float* I, int64_t ldi, const float* T, int64_t ldt, int64_t N, int64_t C, int64_t D,
                   int mode, float* P, int64_t ldp, void* ws, size_t ws_bytes, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K2   S[n,c] = softmax_c(a * P[n,c]);  columns C..lds-1 of S are written as 0 (padding).
 * replaces  clip_feats = torch.nn.functional.softmax(a*clip_feats, dim=1)  concept_vit/similarity.py:54, :80
 * ------------------------------------------------------------------------------------------- */
int mcd_row_softmax(const float* P, int64_t ldp, int64_t N, int64_t C, float a, float* S, int64_t lds,
                    mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K3   per neuron u: the K largest activations over the N images, sorted descending; ties go to
 *      the lower image index; NaN ranks above +inf (torch.topk's rule).
 * replaces  inds = torch.topk(target_feats, dim=0, k=top_k)[1]             concept_vit/similarity.py:55, :82
 *           _, top_ids = torch.topk(target_feats, k=5, dim=0)              describe_clip_neurons.py:66
 *                                                                          describe_og_neurons.py:100
 *                                                                          describe_broad_neurons.py:102
 * A element (n,u) at A[n*stride_n + u*stride_u]; exactly one of the strides must be 1
 * (image-major: stride_u == 1; neuron-major: stride_n == 1).
 * Outputs are NEURON-major: vals[u*ldo + j], idx[u*ldo + j], j < K (either may be NULL).
 * ws: mcd_col_topk_workspace() bytes, 16-byte aligned, for either layout: one "left to the streaming kernel" word per neuron
 * (rounded up to 256 bytes), which the entry writes before it reads it, and behind them, for image-major input, the [U, ceil4(N)]
 * transposed copy.  ws == NULL or ws_bytes too small: MCD_E_WORKSPACE; ws not 16-byte aligned: MCD_E_ARG; nothing is written.
 * Returns MCD_E_RANGE when K > N (torch raises "selected index k out of range").
 * ------------------------------------------------------------------------------------------- */
size_t mcd_col_topk_workspace(int64_t N, int64_t U, int64_t stride_n, int64_t stride_u, int K);
int mcd_col_topk(const float* A, int64_t N, int64_t U, int64_t stride_n, int64_t stride_u, int K, float* vals,
                 int32_t* idx, int64_t ldo, void* ws, size_t ws_bytes, mcd_stream_t stream);

/* image-major [N,U] -> neuron-major [U,N] (dst ld ldd >= N).  Used by K3 and by the activation cache. */
int mcd_transpose(const float* src, int64_t lds, int64_t N, int64_t U, float* dst, int64_t ldd,
                  mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K4   pdge[u,c] = sum_{j<K} log(w_j),  g = S[idx[u,j], c]
 *        soft != 0:  w_j = (1 + p[j]*(g - 1)) + min_prob      concept_vit/similarity.py:59-65
 *        soft == 0:  w_j = g + min_prob                        concept_vit/similarity.py:84-88
 *      every fp32 operation rounded on its own (no contraction); the sum over j follows
 *      torch.sum(dim=0) on CPU: columns c < split in ATen's cascade order, columns c >= split in
 *      its row_sum order (4 interleaved partials).  split < 0 selects ATen's rule for C
 *      ((C/32)*32 for C >= 8, (C/4)*4 below).
 * replaces the Python loop `for orig_id in tqdm(range(target_feats.shape[1]))` with its
 *      gather / log / sum(dim=0) / cat.
 * idx is neuron-major int32 [U, K] (ld ldidx), every entry in [0, N); p is [K] (ignored for hard WPMI).
 * `soft` is a bit set: bit 0 = soft-WPMI terms; bit 1 (MCD_WPMI_FAST_LOG) = use the v_log_f32 based log
 * (<= ~1.5 ulp) instead of the default accurate log (near correctly rounded, like the reference's MKL vsLn);
 * bit 2 (MCD_WPMI_S_IS_PROB) = the caller promises that S holds probabilities in [0,1] (a softmax output) and p
 * lies in [0,1], which lets the kernel skip the range check in front of its log table.  NaN entries of S (softmax
 * rows of NaN/inf similarities) are allowed: they propagate as NaN through the arithmetic.  Finite values outside [0,1]
 * break the promise and yield unspecified results.
 * ------------------------------------------------------------------------------------------- */
int mcd_wpmi_score(const float* S, int64_t ldS, int64_t N, int64_t C, const int32_t* idx, int64_t ldidx, int64_t U,
                   int K, const float* p, float min_prob, int soft, int split, float* pdge, int64_t ldo,
                   mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K1s + K4s  the STRESS chain (BASELINE configs[4]: 10 000 concepts, bf16 MFMA similarity; no parity claim).
 * K1 and K2 in one kernel that never writes fp32 P:
 *      E[n,c]  = bf16( exp(a * (P[n,c] - 1)) ),  P = I_hat @ T_hat^T on the bf16 MFMA (fp32 accumulate)
 *      rinv[n] = 1 / sum_c exp(a * (P[n,c] - 1))
 *   so that softmax(a*P)[n,c] = E[n,c] * rinv[n].  I and T must be row-normalised (|P| <= 1: no row maximum is needed),
 *   or raw with MCD_GEMM_EXP_NORMALIZE in `flags`;
 *   E is [N, ldE] bf16, ldE a multiple of 16 (anything else: MCD_E_UNSUPPORTED; K4s wants a multiple of 128), columns
 *   C..ldE-1 written as 0; rinv[n] = 1 / (the sum of row n's STORED bf16 values), so E * rinv sums to 1 over a row; ws of
 *   mcd_embed_gemm_exp_workspace() bytes, 16-byte aligned, holds the bf16 operands and the per-tile partial row sums (the entry
 *   writes every byte it later reads, the zero padding of the operand image included); ws == NULL, ws_bytes too small or ws not
 *   16-byte aligned: MCD_E_WORKSPACE, nothing is written.  mcd_wpmi_score_bf16: ws of mcd_wpmi_score_bf16_workspace() bytes,
 *   8-byte aligned; NULL, too small or misaligned: MCD_E_WORKSPACE, nothing is written.
 * replaces  clip_feats = image_features @ text_features.T                 concept_vit/utils.py:594
 *           clip_feats = torch.nn.functional.softmax(a*clip_feats, dim=1)  concept_vit/similarity.py:54, :80
 * K4 on that representation:
 *      pdge[u,c] = sum_j log(w_j),  g = E[idx[u,j], c] * rinv[idx[u,j]],  w_j as in mcd_wpmi_score;
 *   v_log_f32-based log, sums kept in the log2 domain.  ldE % 128 == 0.
 * replaces  the Python loop of soft_wpmi / wpmi                            concept_vit/similarity.py:59-65, :84-88
 * ------------------------------------------------------------------------------------------- */
enum { MCD_GEMM_EXP_NORMALIZE = 1 };  /* flags: I and T are RAW embeddings; rows are L2-normalised while they are converted
                                         to bf16 (utils.py:577-578 folded in; D <= 2048) */
size_t mcd_embed_gemm_exp_workspace(int64_t N, int64_t C, int64_t D);
int mcd_embed_gemm_exp(const float* I, int64_t ldi, const float* T, int64_t ldt, int64_t N, int64_t C, int64_t D,
                       float a, int flags, uint16_t* E, int64_t ldE, float* rinv, void* ws, size_t ws_bytes,
                       mcd_stream_t stream);
/* Measurement hook (bench.py; not on the data path): after mcd_embed_gemm_exp_time_kernel(reps), reps > 0, mcd_embed_gemm_exp
 * launches its GEMM kernel `reps` times back to back (same arguments, same output) between a pair of HIP events on its stream --
 * the kernel alone, not the bf16 conversion in front of it nor the row-sum finish behind it; mcd_embed_gemm_exp_kernel_ms() waits
 * for the pair of the calling thread's current device and returns the elapsed milliseconds PER LAUNCH of the last timed call
 * (< 0: none recorded).  One launch between two events reads 10-25 us long (marker packets, dispatch gaps): use reps >= 8.
 * reps = 0 (the default) turns it off: the entry point then neither creates events nor synchronises, and stays capturable in a
 * hipGraph.  (One kernel serves every shape since round 5; the quotient uses the number of launches actually issued.) */
int mcd_embed_gemm_exp_time_kernel(int reps);
float mcd_embed_gemm_exp_kernel_ms(void);
size_t mcd_wpmi_score_bf16_workspace(int64_t U, int K);   /* {row, p_j * rinv[row]} per (neuron, j): 8 U K bytes */
int mcd_wpmi_score_bf16(const uint16_t* E, int64_t ldE, int64_t N, int64_t C, const float* rinv, const int32_t* idx,
                        int64_t ldidx, int64_t U, int K, const float* p, float min_prob, int soft, float* pdge,
                        int64_t ldo, void* ws, size_t ws_bytes, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K5   per segment s (= one layer, rows seg[s]..seg[s+1]-1 of pdge), per column c:
 *        prob_d = logsumexp_u(pdge[u,c]) - log(U_s);   out[u,c] = pdge[u,c] - lam*prob_d
 * replaces  prob_d = torch.logsumexp(prob_d_given_e, dim=0, keepdim=True) - torch.log(U*ones([1]))
 *           mutual_info = prob_d_given_e - lam*prob_d                     concept_vit/similarity.py:70-72, :92-96
 * seg_offsets is a HOST array of n_seg+1 ascending row offsets (n_seg <= 64; a segment without rows is skipped); out may alias pdge.
 * ws: device scratch of mcd_logsumexp_sub_workspace(total rows, C, n_seg) bytes (column maxima and the
 * 16-row partial sums that ATen's summation order chains), aligned for float; only the three-pass path (a segment of more than
 * 3840 rows) uses it, and it writes what it reads.  ws == NULL or ws_bytes too small: MCD_E_WORKSPACE on either path, nothing is
 * written.  seg_offsets is read during the call only (a captured graph keeps no pointer to it).
 * ------------------------------------------------------------------------------------------- */
size_t mcd_logsumexp_sub_workspace(int64_t U_total, int64_t C, int n_seg);
int mcd_logsumexp_sub(const float* pdge, int64_t ld, int64_t C, const int64_t* seg_offsets, int n_seg, float lam,
                      int split, float* out, int64_t ldo, void* ws, size_t ws_bytes, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K6   per row u of sim [U,C]: the k largest entries, sorted descending, ties to the lower
 *      concept index.  k = 1 is torch.max(dim=1).  k <= 16.
 * replaces  vals, ids = torch.max(similarities, dim=1)                    describe_clip_neurons.py:64
 *           vals, ids = torch.topk(similarities, k=10, dim=1)             describe_og_neurons.py:99
 *                                                                         describe_broad_neurons.py:101
 * vals/idx are [U,k] contiguous.
 * ------------------------------------------------------------------------------------------- */
int mcd_row_topk(const float* sim, int64_t ld, int64_t U, int64_t C, int k, float* vals, int32_t* idx,
                 mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K0   forward-hook pooling written straight into the activation matrix.
 *      x is the hooked tensor: [B, Cout, HW] for AVG/MAX (mean / amax over HW),
 *      [B, T, F] for CLS (token 0: x[b,0,:], Cout = F, HW = T), [B, F] for NONE (HW = 1).
 *      Result (b, ch) goes to dst[(row0+b)*stride_n + (col0+ch)*stride_u].
 * replaces  get_activation(outputs, mode) hook bodies                     concept_vit/utils.py:27-52
 *           (og_utils.py:31-56, CLIP_og_utils.py:13-36) and the later torch.cat (utils.py:143).
 * ------------------------------------------------------------------------------------------- */
int mcd_hook_pool(const float* x, int64_t B, int64_t Cout, int64_t HW, int mode, float* dst, int64_t row0,
                  int64_t col0, int64_t stride_n, int64_t stride_u, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K8   rank_reorder scoring of one layer.
 *      tvals/tidx are neuron-major [U, top_n] (ld ldt): the top_n largest activations of every neuron in
 *      descending order and their image indices (mcd_col_topk's output); perms is int32 [U, n_perm, top_n],
 *      the random permutations of the baseline (the reference draws them with torch.randperm on the global CPU
 *      generator, 5 per neuron in neuron order -- the host mirror does the same so a seeded run reproduces the
 *      reference); baseline_ws is caller-owned scratch of U floats (no ws_bytes: NULL is MCD_E_ARG), written before it is read.
 *      out[u,c] = -( mean_j |t_j - st[rank_jc]|^p / baseline_u ) / mean_j(P[idx_j, c])^scale_p
 * replaces  the per-neuron Python loop of rank_reorder                    concept_vit/similarity.py:107-132
 * ------------------------------------------------------------------------------------------- */
int mcd_rank_reorder(const float* P, int64_t ldP, int64_t N, int64_t C, const float* tvals, const int32_t* tidx,
                     int64_t ldt, int64_t U, int top_n, const int32_t* perms, int n_perm, float p, float scale_p,
                     float* baseline_ws, float* out, int64_t ldo, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K9   fp32 multi-head self-attention of the ViT image tower (head dimension 64, no mask, T <= 256 tokens).
 *      qkv is the fused projection's output [B, T, 3, H, 64] (q, k, v of a token adjacent), out is [B, T, H*64]:
 *      out[b, t, h, :] = softmax_j(q[b,t,h].k[b,j,h] / 8) v[b,j,h].  One workgroup per (image, head), K and V in
 *      LDS, flash-style online softmax, v_mfma_f32_32x32x2_f32 for both products.  Both pointers 16-byte aligned.
 *      Encoder-side op (the forwards that the extraction loop drives, concept_vit/utils.py:117-148): fp32-accurate
 *      (<= 2e-6 from torch's SDPA), no bit-exactness claim -- the reference's own encoders run on whatever
 *      backend torch picks.  A NaN propagates as in the reference (in q: that output row of that head; in k: every
 *      query of that image and head; in v: that column of them) and reaches nothing else; results for +-Inf inputs
 *      are unspecified (K9, K9L and K9C alike: a masked key multiplies the clamped last V row by p = 0).
 * replaces  the attention inside ViTModel(...)                             model/modules/image_encoder.py:37
 *           nn.MultiheadAttention(x, x, x, need_weights=False)            concept_vit/clip/model.py:171-183
 * ------------------------------------------------------------------------------------------- */
int mcd_vit_attention(const float* qkv, int64_t B, int64_t T, int64_t H, float* out, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K9L  the same attention for long sequences: 1 <= T <= 32 768 tokens (2048 x 2048 at patch 16 is 16 385), the same
 *      layout, arithmetic and alignment as K9, and one image's qkv block (T * 3 * H * 64 floats) under 2^31 bytes
 *      (MCD_E_UNSUPPORTED past either limit; the whole batch may be larger).  One workgroup per (image, head, block of
 *      256 queries) streams all of that head's 32-key tiles through K9's LDS ring; a query's arithmetic is K9's, in
 *      the same order, so for T <= 256 the result is K9's, bit for bit, and it does not depend on the query block or
 *      the batch.  No T x T buffer.  The query blocks of one (image, head) are placed on one XCD (speed only).
 * replaces  the attention inside ViTModel(...) at high resolution          model/modules/image_encoder.py:37
 *           nn.MultiheadAttention(x, x, x, need_weights=False)            concept_vit/clip/model.py:171-183
 * ------------------------------------------------------------------------------------------- */
int mcd_vit_attention_long(const float* qkv, int64_t B, int64_t T, int64_t H, float* out, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K9C  the same attention for ONE query row per image (the class token of the last encoder block, whose other rows
 *      nothing reads): out[b, h, :] = softmax_j(q[b,h].k[b,j,h] / 8) v[b,j,h], fp32 throughout, head dimension 64,
 *      1 <= T <= 32 768.  q is one row of H*64 floats per image, q_img floats apart; token j of image b of k (of v) is
 *      at k + b*k_img + j*k_row (v + b*v_img + j*v_row), H*64 floats; out is [B, H*64], contiguous.  So a
 *      [B, T, 2, H, 64] K|V projection (k_row = 2*H*64, v = k + H*64) and a plain [B, T, 3, H, 64] qkv (q_img = T*3*H*64,
 *      k = qkv + H*64, v = qkv + 2*H*64, rows 3*H*64 apart) are both read in place.  Every stride >= H*64 and a multiple
 *      of 4 floats, all pointers 16-byte aligned (MCD_E_ARG), T past the limit MCD_E_UNSUPPORTED.
 *      A streaming kernel: every K and V head row is read once (2*B*T*H*256 bytes), 16 lanes x float4 per row, online
 *      softmax per 16-lane row, no T-sized scratch.  K9's accuracy contract; not K9's bits (another summation order).
 * replaces  row 0 of the attention inside the last ViTLayer                 model/modules/image_encoder.py:37
 *           (all that output[:, 0] / encode_image read)                     concept_vit/utils.py:39-49, model/clip.py:49-52
 * ------------------------------------------------------------------------------------------- */
int mcd_vit_attention_cls(const float* q, int64_t q_img, const float* k, int64_t k_row, int64_t k_img, const float* v,
                          int64_t v_row, int64_t v_img, int64_t B, int64_t T, int64_t H, float* out, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K10  fp32 LayerNorm over the last dimension (biased variance, like torch): rows x D contiguous, D a multiple of 4
 *      up to 2048, pointers 16-byte aligned.  One wave per row, the row register-resident, two-pass statistics.
 *      Encoder-side op, fp32-accurate (<= 1e-6 relative from torch's), no bit-exactness claim.
 * replaces  nn.LayerNorm inside the ViT blocks                              model/modules/image_encoder.py:37
 *           (ViTLayer.layernorm_before / layernorm_after), ln_1 / ln_2      concept_vit/clip/model.py:172-176
 * ------------------------------------------------------------------------------------------- */
int mcd_layer_norm(const float* x, int64_t rows, int64_t D, const float* gamma, const float* beta, float eps, float* y,
                   mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K11  patch extraction for the ViT patch embedding: x [B, Cin, H, W] -> out [B, 1 + (H/P)(W/P), Cin*P*P], row 0 of
 *      every image zero (class-token slot), row 1 + patch in (c, dy, dx) order, so that the Conv2d(Cin, dim, P, P) is
 *      the GEMM  out . weight.view(dim, Cin*P*P)^T.  A permutation of the pixels: exact.  P is any even size >= 2 that
 *      divides H and W (16 for ViT-B/16, 14 for DINOv2): 16-byte accesses when P % 4 == 0, 8-byte ones otherwise (W is
 *      a multiple of P, so every piece of a patch row is aligned to its size); an odd P is MCD_E_UNSUPPORTED.  Pointers
 *      16-byte aligned.
 * replaces  the patch-embedding convolution of the image tower              model/modules/image_encoder.py:37
 *           (ViTPatchEmbeddings.projection), conv1                          concept_vit/clip/model.py:206-223
 *           Dinov2PatchEmbeddings.projection of the `dino` targets          concept_vit/data_utils.py:24,63-69
 * ------------------------------------------------------------------------------------------- */
int mcd_patchify(const float* x, int64_t B, int64_t Cin, int64_t H, int64_t W, int64_t P, float* out, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * EfficientNet-B5 image tower, inference route (K12-K15, K0n): channels-last (NHWC) activations, batch norm (eval,
 * running statistics) folded into the weights as W' = W * g / sqrt(var + eps) per output channel and
 * b' = beta - mean * g / sqrt(var + eps); the 1x1 convolutions are GEMMs on libmcd_blaslt.so.  fp32, SiLU and sigmoid
 * with the accurate exp.  Every kernel addresses one image from a 64-bit base with 32-bit offsets inside it: a tensor
 * of one image of 2^31 bytes or more, or B > 65535, is MCD_E_UNSUPPORTED (the caller takes the ATen route).  No
 * atomics: an image's bits do not depend on the batch it is in.  Encoder-side ops, fp32-accurate, no bit-exactness
 * claim against the reference's backend (K0n excepted: bit-equal to K0, below).  TF-SAME padding throughout: for n
 * input rows, kernel k and stride s the output has ceil(n/s) rows and the pad max((ceil(n/s)-1)*s + k - n, 0) is split
 * with its smaller half on top (left).  Float pointers 16-byte aligned.
 *
 * K12  stem: x NCHW [B, Cin, H, W] (Cin <= 4) -> y NHWC [B, ceil(H/2), ceil(W/2), Cout] = SiLU(conv3x3/2(x, W') + b'),
 *      w tap-major [Cin, 3, 3, Cout], Cout % 4 == 0.
 * replaces  _conv_stem + _bn0 + swish                          model/modules/efficientnet_custom.py:241, :273
 * ------------------------------------------------------------------------------------------- */
int mcd_conv_stem_nhwc(const float* x, int64_t B, int64_t Cin, int64_t H, int64_t W, const float* w, const float* bias,
                       int64_t Cout, float* y, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K13  depthwise k x k (k in {3, 5}), stride 1 or 2, on NHWC x [B, H, W, C] (C % 4 == 0):
 *        y[b, oy, ox, c] = SiLU( sum_taps w[dy*k + dx, c] * a(x[b, iy, ix, c]) + bias[c] ),  y [B, ceil(H/s), ceil(W/s), C]
 *      a = SiLU when silu_in != 0 (x is the raw expand-GEMM output; the zero padding commutes: SiLU(0) = 0), the
 *      identity otherwise.  w is tap-major [k*k, C].  Also writes the squeeze-excite partial sums
 *      psum[b, t, c] = sum of y[b, ., ., c] over output tile t, for the T = ceil(Ho/8) * ceil(Wo/8) tiles of 8 x 8
 *      output pixels (row-major; the tiling depends on (Ho, Wo) only).  One workgroup per (tile, channel slice, image)
 *      stages the tile's input window in LDS once.
 * replaces  _depthwise_conv + _bn1 + swish + adaptive_avg_pool2d  model/modules/efficientnet_custom.py:109-115
 * ------------------------------------------------------------------------------------------- */
int mcd_dwconv_bn_silu(const float* x, int64_t B, int64_t H, int64_t W, int64_t C, const float* w, const float* bias,
                       int k, int stride, int silu_in, float* y, float* psum, int64_t T, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K14  squeeze-excite gate, one workgroup per image:  mean[c] = (sum_t psum[b, t, c], in t order) / HW,
 *        s[b, c] = sigmoid( b_e[c] + sum_j w_et[j, c] * SiLU( b_r[j] + sum_c' w_r[j, c'] * mean[c'] ) )
 *      w_r [sq, C] (_se_reduce's weight), w_et [sq, C] (_se_expand's weight TRANSPOSED), any SE width sq >= 1,
 *      C + sq <= 16384.
 * replaces  _se_reduce, swish, _se_expand, sigmoid             model/modules/efficientnet_custom.py:116-119
 * ------------------------------------------------------------------------------------------- */
int mcd_se_gate(const float* psum, int64_t B, int64_t T, int64_t C, int64_t HW, const float* w_r, const float* b_r,
                int64_t sq, const float* w_et, const float* b_e, float* s, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K15  y[b, p, c] *= s[b, c] in place on NHWC y [B, HW, C] (C % 4 == 0), 16-byte accesses: the same bits as
 *      y * s[:, None, None, :].  (hipBLASLt cannot scale a GEMM's reduction dimension per image: a pass of its own.)
 * replaces  torch.sigmoid(x_squeezed) * x                      model/modules/efficientnet_custom.py:119
 * ------------------------------------------------------------------------------------------- */
int mcd_channel_scale(float* y, int64_t B, int64_t HW, int64_t C, const float* s, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K0n  K0 for a channels-last [B, C, H, W] (memory [B, HW, C]): mean (MCD_POOL_AVG) or amax (MCD_POOL_MAX) over HW
 *      into dst exactly as mcd_hook_pool writes it, BIT-IDENTICAL to mcd_hook_pool on the NCHW-contiguous copy (K0's
 *      per-lane partials -- its float4 grouping when HW % 4 == 0, its scalar walk otherwise -- combined in K0's
 *      xor-butterfly order; a NaN in a plane makes its max NaN).  MCD_POOL_SILU_AVG: mean over HW of SiLU(x), the
 *      tower's head (mcd_hook_pool rejects that mode).
 * replaces  output.mean/amax(dim=[2,3]) of the hook body        concept_vit/utils.py:37-47
 *           head swish + average pooling                       model/modules/efficientnet_custom.py:257, :301
 * ------------------------------------------------------------------------------------------- */
int mcd_hook_pool_nhwc(const float* x, int64_t B, int64_t C, int64_t HW, int mode, float* dst, int64_t row0,
                       int64_t col0, int64_t stride_n, int64_t stride_u, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * ResNet-50 target, inference route (K16-K18): channels-last (NHWC) activations, batch norm (eval, running statistics)
 * folded as for the B5 tower; the stride-1 1x1 convolutions are GEMMs on libmcd_blaslt.so.  fp32.  ResNet's symmetric
 * padding: for n input rows, kernel k, stride s and pad p the output has (n + 2p - k) / s + 1 rows (floor).  One image's
 * tensor of 2^31 bytes or more, B > 65535 or a width a kernel does not take is MCD_E_UNSUPPORTED (the caller takes the
 * ATen route).  No atomics and no split reduction: every output element is one fmaf chain in a fixed order, so an
 * image's bits depend neither on the batch it is in nor on its place in it.  Float pointers 16-byte aligned.
 *
 * K16  stem, raw: x NCHW [B, Cin, H, W] (Cin <= 4) -> y NHWC [B, Ho, Wo, Cout] = conv7x7/2, pad 3 (x, w); no bias, no
 *      batch norm, no ReLU (conv1 is a hook point: the hook sees the convolution's own output).  w tap-major
 *      [Cin, 7, 7, Cout], Cout % 4 == 0.  An x or a w that overlaps y is MCD_E_ARG.
 * replaces  conv1 of the torchvision ResNet-50                    concept_vit/data_utils.py:85-93
 * ------------------------------------------------------------------------------------------- */
int mcd_conv7x7s2_nhwc(const float* x, int64_t B, int64_t Cin, int64_t H, int64_t W, const float* w, int64_t Cout,
                       float* y, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K17  NHWC x [B, H, W, C] (C % 4 == 0) -> y [B, Ho, Wo, C]: max over the 3x3 / stride 2 / pad 1 window of
 *      relu(fma(x, scale[c], shift[c])); the padding never wins (the window always holds a real pixel).  With
 *      scale = 1, shift = 0 bit-equal to max_pool2d(relu(x), 3, 2, 1).
 * replaces  bn1 + relu + maxpool of the torchvision ResNet-50     concept_vit/data_utils.py:85-93
 * ------------------------------------------------------------------------------------------- */
int mcd_bn_relu_maxpool_nhwc(const float* x, int64_t B, int64_t H, int64_t W, int64_t C, const float* scale,
                             const float* shift, float* y, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K18  implicit-GEMM convolution on v_mfma_f32_32x32x2_f32 (exact fp32), no im2col buffer: x NHWC [B, H, W, Cin],
 *      w [Cout, k*k*Cin] tap-major then channel, bias [Cout], y NHWC [B, Ho, Wo, Cout]:
 *        y = act_out( bias + sum over (tap, cin) of w * act_in(x) ),  act_in / act_out = ReLU when relu_in / relu_out
 *      (relu(0) = 0: the zero padding commutes with relu_in).  k = 3 with stride 1 or 2 (pad 1), k = 1 with stride 2
 *      (pad 0); Cin % 32 == 0 and Cout % 32 == 0; anything else is MCD_E_UNSUPPORTED.  GEMM rows are the flattened
 *      output pixels B*Ho*Wo (a tile may span images).  The reduction of every output element runs tap-major, then
 *      channel, in ascending order: chunks of 256 consecutive k, each a k-ordered fmaf chain from 0 (the MFMA's
 *      arithmetic), the chunks' partial sums added in ascending order, the bias last -- the same order for every
 *      element whatever its tile, image or batch (a single chain over k = 4 608 is 8 x less accurate than ATen).
 * replaces  Bottleneck.conv2 + bn2 + relu (and the relu after bn1 on the way in), downsample[0] + downsample[1] of a
 *           stride-2 block                                        concept_vit/data_utils.py:85-93
 * ------------------------------------------------------------------------------------------- */
int mcd_conv_igemm_nhwc(const float* x, int64_t B, int64_t H, int64_t W, int64_t Cin, const float* w, const float* bias,
                        int64_t Cout, int k, int stride, int relu_in, int relu_out, float* y, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K18 with a residual operand in its epilogue: everything of mcd_conv_igemm_nhwc (shapes, layouts, alignment, size limits
 *      and return codes), and res NHWC [B, Ho, Wo, Cout], contiguous and 16-byte aligned:
 *        y = act_out( (bias + sum over (tap, cin) of w * act_in(x)) + res )
 *      The order per output element is fixed: (1) K18's chunked sum as above, (2) + bias, (3) + res, (4) the ReLU when
 *      relu_out is set.  The ReLU acts on the whole sum: a residual that drives it negative gives 0.  res must not
 *      overlap y (MCD_E_ARG).  res == NULL means no residual: the call is mcd_conv_igemm_nhwc, bit for bit; and
 *      mcd_conv_igemm_nhwc returns the bits it returned before this entry existed.  The residual is the 16-byte NHWC
 *      piece a lane stores, one float4 load per store under the store's guards; nothing else of the kernel changes, so
 *      an image's bits still depend neither on its batch nor on its place in it.
 * replaces  BasicBlock.conv2 + bn2 + (+= identity) + relu of the torchvision ResNet-18 / -34 (and resnet18_places)
 *                                                                 concept_vit/data_utils.py:70-89
 * ------------------------------------------------------------------------------------------- */
int mcd_conv_igemm_res_nhwc(const float* x, int64_t B, int64_t H, int64_t W, int64_t Cin, const float* w,
                            const float* bias, const float* res, int64_t Cout, int k, int stride, int relu_in,
                            int relu_out, float* y, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * OpenAI-CLIP's anti-aliased ResNet (the RN50 / RN101 dissectors), inference route (K19-K21, with K18, K9C, K0n and the
 * GEMMs of libmcd_blaslt.so): the rules of K16-K18 -- fp32, channels-last activations, folded batch norm, no atomics, no
 * split reduction, one fixed order per output element (an image's bits depend neither on its batch nor on its place in
 * it), one image's tensor of 2^31 bytes or more or B > 65535 is MCD_E_UNSUPPORTED; NULL, misaligned (16 bytes; K19's x:
 * 4) or overlapping input / output pointers, C % 4 != 0 and Cin > 4 are MCD_E_ARG.  No entry reads the environment.
 *
 * K19  stem: x NCHW [B, Cin, H, W] (Cin <= 4) -> y NHWC [B, Ho, Wo, Cout] = act(conv3x3/2, pad 1 (x, w) + bias),
 *      Ho = (H + 2 - 3) / 2 + 1; w tap-major [Cin, 3, 3, Cout] with the batch norm folded in, Cout % 4 == 0; act = ReLU
 *      when relu != 0 (it keeps a NaN).  K16's kernel: a 16 x 16 output tile per workgroup, its 33 x 33 x Cin window in
 *      LDS, weights through the scalar cache, 32 output channels per pass (4 when Cout % 32).  Per output element: one
 *      fmaf chain from 0 over (channel, row, column), then + bias, then the ReLU.
 * replaces  visual.conv1 + bn1 + relu of ModifiedResNet           concept_vit/clip/model.py:107-108, :136-138
 * ------------------------------------------------------------------------------------------- */
int mcd_conv3x3s2_nhwc(const float* x, int64_t B, int64_t Cin, int64_t H, int64_t W, const float* w, const float* bias,
                       int64_t Cout, int relu, float* y, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K20  nn.AvgPool2d(2) on NHWC x [B, H, W, C] (C % 4 == 0) -> y [B, H/2, W/2, C] (floor: an odd trailing row or column
 *      is dropped; H == 1 or W == 1 is an empty output: MCD_OK, nothing is written).  One thread per (output pixel,
 *      channel quad).  y = (((x00 + x01) + x10) + x11) * 0.25f: bit-equal to F.avg_pool2d(x, 2) in either memory format.
 * replaces  the stem's avgpool, a stride-2 Bottleneck's avgpool     concept_vit/clip/model.py:113, :139, :23, :45,
 *           and downsample."-1"                                     :35
 * ------------------------------------------------------------------------------------------- */
int mcd_avgpool2_nhwc(const float* x, int64_t B, int64_t H, int64_t W, int64_t C, float* y, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K21  the attention pool's token sequence: x NHWC [B, HW, C], pos [HW + 1, C] -> tok [B, HW + 1, C] (C % 4 == 0),
 *        tok[b, 0, :] = mean_p x[b, p, :] + pos[0],    tok[b, 1 + p, :] = x[b, p, :] + pos[1 + p]
 *      A thread owns a channel quad of one image.  The mean is one ascending sum over p, times 1/HW (computed once, in
 *      fp32), the position row added last; rows 1.. are a single fp32 add (torch's bits).
 * replaces  reshape / permute, cat(mean, x), + positional_embedding  concept_vit/clip/model.py:67-69
 *           of AttentionPool2d.forward
 * ------------------------------------------------------------------------------------------- */
int mcd_attnpool_tokens(const float* x, int64_t B, int64_t HW, int64_t C, const float* pos, float* tok,
                        mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K22  probe-image preprocessing in one launch: src packed RGB uint8 [n, H, W, 3] (n images of ONE source size) ->
 *      dst fp32 [n, 3, OH, OW], image i at dst + i * dst_img (dst_img >= 3*OH*OW elements; the gap is not written).
 *      PIL's 8-bit two-pass resampler (Resample.c, PRECISION_BITS = 22) to RH x RW, a crop window of OH x OW at
 *      (top, left) inside it, then one look-up per byte:
 *        t[y][o] = clip8((2^21 + sum_j src[y][first_o + j] * coef_o[j]) >> 22)      horizontal, per channel
 *        r[o][x] = clip8((2^21 + sum_j   t[first_o + j][x] * coef_o[j]) >> 22)      vertical, on the uint8 t
 *        dst[i][c][y][x] = lut[c][ r[top + y][left + x][c] ]
 *      int32 accumulation (|sum| <= 255 * sum|coef| + 2^21 < 2^31 for tables whose rows sum to 2^22), arithmetic
 *      shift, clip8 clamps to 0..255: bit for bit Image.resize((RW, RH), BILINEAR | BICUBIC) on an RGB image.  No
 *      floating-point operation runs on the device; lut [3][256] fp32 carries ToTensor / Normalize (the caller computes
 *      v / 255, (. - mean) / std once per byte value).  Only the crop window is computed.
 *      xtab [RW][2 + kx], ytab [RH][2 + ky] int32: row o = {first, count, coef[0 .. k)}, zero padded, count <= k, as
 *      PIL's precompute_coeffs + normalize_coeffs_8bpc give them (first non-decreasing in o).  A NULL table skips that
 *      pass and needs RW == W (RH == H).  Rows that name pixels outside the image are clamped into it (a wrong
 *      picture, no access outside src).
 *      Limits: H*W*3 and 3*OH*OW*4 under 2^31 and at most 128 coefficients per table row (bicubic up to ratio 31,
 *      bilinear up to 63), else MCD_E_UNSUPPORTED and nothing is written.  lut, dst and the tables 4-byte aligned.
 *      No aliasing: src, lut or a table overlapping dst is MCD_E_ARG.  n == 0 is MCD_OK.
 * replaces  Resize(256) + CenterCrop(224) + ToTensor + Normalize   concept_vit/data_utils.py:95-100
 *           CLIP's _transform (bicubic 224, crop, normalise)       concept_vit/clip/clip.py:79-86
 *           Resize((1520, 912)) + ToTensor of the EMBED sets       concept_vit/data_utils.py:176-179
 *           ToTensor + Normalize of imagenet_subsets               concept_vit/data_utils.py:111
 * ------------------------------------------------------------------------------------------- */
int mcd_image_preprocess(const uint8_t* src, int64_t n, int64_t H, int64_t W, const int32_t* xtab, int64_t kx, int64_t RW,
                         const int32_t* ytab, int64_t ky, int64_t RH, int64_t top, int64_t left, int64_t OH, int64_t OW,
                         const float* lut, float* dst, int64_t dst_img, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K23  per-image min-max normalisation, the transform of the mammogram probe sets: src uint8, n images of ONE size packed
 *      back to back, channels == 3: [n, H, W, 3] (what .convert('RGB') gives), channels == 1: [n, H, W] (a mode-L PNG,
 *      which .convert('RGB') only replicates) -> dst fp32 [n, 3, H, W], image i at dst + i * dst_img (dst_img >= 3*H*W
 *      elements; the gap is not written).  With channels == 1 the three planes are identical.
 *        MCD_IMG_MINMAX  mn, mx = the smallest and the largest byte of image i over ALL of its channels,
 *                        out = ((f32(v) - f32(mn)) / f32(mx - mn) - mean) / std
 *                        four IEEE fp32 operations, each rounded once, both divisions real divisions; mx == mn gives
 *                        NaN in the whole image (0 / 0), which is the reference's result
 *        MCD_IMG_RAW     out = f32(v); mean and std are ignored, ws may be NULL
 *      Two launches, no atomics, no memset: (a) grid (chunks, n), a workgroup reduces one chunk of
 *      MCD_IMAGE_MINMAX_CHUNK bytes of image i (doubled until an image has at most 256 chunks) to an int32 (min, max)
 *      pair in ws[i][chunk], 16-byte loads on the aligned body, bytes at the chunk's head and tail, nothing outside the
 *      image is read; (b) grid (tiles, n), every workgroup folds its image's pairs, builds the 256-entry fp32 table in
 *      LDS (thread v computes entry v) and streams its tile through it.  Wide path (dword loads of 4 pixels, one 16-byte
 *      store per plane): H*W % 16 == 0, dst_img % 4 == 0, dst 16-byte and src 4-byte aligned; every other shape takes
 *      scalar accesses.  min and max are integers: an image's bits depend neither on its batch nor on its place in it.
 *      The workspace function gives the bytes ws needs (0 for a shape the entry refuses).
 *      MCD_E_ARG: NULL src or dst, channels not 1 or 3, an unknown mode, H or W < 1, n < 0, dst_img < 3*H*W, dst not 4-byte or ws
 *      not 8-byte aligned, src or ws overlapping dst, MCD_IMG_MINMAX with ws == NULL.  MCD_E_WORKSPACE: ws_bytes too small.
 *      MCD_E_UNSUPPORTED: n > 65535, one image's source or output of 2^31 bytes or more.  n == 0 is MCD_OK.  On any
 *      error nothing is written.  No environment variable is read.
 * replaces  img.astype('float32'); img -= img.min(); img /= img.max(); (img - mean) / std
 *                                                 data/dataset/image_classification_zs.py:57-96 (:81-84)
 *           the vindr / vindr_alt loaders          concept_vit/data_utils.py:114-158, data/datamodule.py:53-98,
 *                                                 data/data_utils.py:25-67 (load_transform: None at 1520 x 912)
 *           images.permute(0, 3, 1, 2)            concept_vit/utils.py:176
 *           np.array(Image.open(path), dtype=np.float32), repeat to 3 channels, ToTensor (csaw, csaw_all_splits)
 *                                                 data/dataset/CSAW_dataset.py:41-68, concept_vit/data_utils.py:254-298
 * ------------------------------------------------------------------------------------------- */
#define MCD_IMG_MINMAX 0
#define MCD_IMG_RAW 1
#define MCD_IMAGE_MINMAX_CHUNK 16384
size_t mcd_image_minmax_workspace(int64_t n, int64_t H, int64_t W, int64_t channels);
int mcd_image_minmax_normalize(const uint8_t* src, int64_t n, int64_t H, int64_t W, int64_t channels, int mode, float mean,
                               float std, float* dst, int64_t dst_img, void* ws, size_t ws_bytes, mcd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MCD_HIP_H */
