/*
 * mcd_sentence.h -- the sentence-encoder entries of libmcd_hip.so (K9B, K27): the two kernels that the MPNet sentence
 * encoder behind get_cos_similarity (data_utils.MPNetSentenceEncoder: transformers.MPNetModel + sentence-transformers'
 * Pooling(mean) + Normalize, i.e. all-mpnet-base-v2) needs beside the BERT tower's.  Same library, same conventions as
 * include/mcd_hip.h, which this header includes for mcd_stream_t and the MCD_E_* codes: plain device pointers, the caller
 * owns every buffer, nothing is allocated or synchronised inside, no workspace, no environment read, every call is
 * asynchronous on `stream` and is hipGraph-capturable (tests/test_gpu_mpnet.py holds both entries to the stream and
 * capture contracts).
 * Additive to ABI version 9: mcd_abi_version() is unchanged.  The ctypes rows are _lib.SENTENCE_SIGNATURES.
 */
#ifndef MCD_SENTENCE_H
#define MCD_SENTENCE_H

#include "mcd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * K9B  K9M (include/mcd_text.h) with an additive score bias that depends on the head and on the key-minus-query distance
 *      alone: MPNet's relative-position bias.  qkv [B, T, 3, H, 64], lens (B int32 on the device, or NULL = every length
 *      is T) and out [B, T, H*64] are K9M's, the clamp L = clamp(lens[b], 1, T) included; 1 <= T <= 256.
 *      rel is [H, 2T-1] fp32, contiguous, 16-byte aligned: rel[h, d + T - 1] is the bias of head h at distance
 *      d = key - query, -(T-1) <= d <= T-1.  For a valid query row t < L and every key j < L
 *          score(b, h, t, j) = q[b,t,h].k[b,j,h] / 8 + rel[h, (j - t) + T - 1],
 *          out[b, t, h, :]   = softmax_{j < L}(score) v[b,j,h].
 *      The [H, T, T] bias is never formed: it is Toeplitz and the same for every sequence, so a workgroup stages its head's
 *      row in LDS once and the score loop indexes it by distance.
 *      rel == NULL gives K9M's output bit for bit (K9M's kernel runs).  An all-zero rel gives K9M's output bit for bit as
 *      well: the kernel keeps scores in the log2 domain, the bias is multiplied by log2(e) like the 1/8 scale is, zero
 *      stays zero, and adding it changes no finite score.
 *      Reads.  No K or V row >= L is read.  Of rel, sequence b reads the distances |d| <= L - 1 of its head rows and
 *      nothing else: entries with |d| >= the batch's longest L are never read, a NaN there reaches nothing.
 *      Padded query rows t >= L are computed and stored, as K9M's are, but nothing may depend on them: they attend to
 *      the L valid keys under the bias of max(j - t, -(L-1)) -- the distances below -(L-1) take that entry's value --
 *      which is NOT what MPNetModel computes for its padded rows.  Rows t < L equal a B = 1, T = L call on sequence b
 *      with the matching 2L-1 entries of every rel row, bit for bit: neither padding nor batch neighbours change them.
 *      NaN propagation for q, k and v is K9M's; a NaN in a rel entry that is read reaches every query row of that head at
 *      that distance.  Results for +-Inf inputs are unspecified.
 *      MCD_E_ARG: NULL qkv / out, B < 0, T < 1, H < 1, a pointer that is not aligned as said.  MCD_E_UNSUPPORTED: T > 256,
 *      B or H over 65535.  B == 0 returns MCD_OK.  Every argument check precedes the first HIP call.
 * replaces  MPNetSelfAttention.forward under position_bias and the key mask        transformers modeling_mpnet.py
 * ------------------------------------------------------------------------------------------- */
int mcd_vit_attention_relbias(const float* qkv, int64_t B, int64_t T, int64_t H, const int32_t* lens,
                              const float* rel /* may be NULL = K9M */, float* out, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K27  The masked mean of the token rows of every sequence and its L2 normalisation, in fp32, one launch:
 *          m[b, :]   = (sum over t < L of x[b, t, :]) / L,        L = clamp(lens[b], 1, T)  (lens NULL: L = T),
 *          out[b, :] = m / max(||m||_2, 1e-12)   with normalize = 1,      out[b, :] = m   with normalize = 0.
 *      x is [B, T, D] and out [B, D], both contiguous and 16-byte aligned; lens is B int32 on the device or NULL.
 *      D is a multiple of 4, at most 2048 (K10's limit).  No row t >= L is read: a NaN there reaches nothing.
 *      The bits of row b depend on its own L and on D alone -- not on B, not on its neighbours, not on T:
 *        1. the mean is K26's (include/mcd_tokens.h) with n = L: four partial sums p_w over the rows w, w + 4, ... < L in
 *           ascending order, s = ((p_0 + p_1) + p_2) + p_3, m = s / (float)L, every step one fp32 rounding;
 *        2. lane l (0 .. 63) adds the squares of its columns -- 4 (64 cb + l) + e for cb = 0 .. 7, e = 0 .. 3, in that
 *           order, each square and each add rounded once, columns >= D counting as zero -- from +0;
 *        3. the 64 lane sums meet in an xor butterfly (partners 32, 16, 8, 4, 2, 1 apart);
 *        4. den = max(sqrtf(sum), 1e-12f), out = m / den, one correctly rounded division per element.
 *      An all-zero sequence gives zeros (0 / 1e-12), not NaN.
 *      MCD_E_ARG: B < 0; with B > 0 a NULL x or out, D < 4, D % 4 != 0, T < 1, normalize neither 0 nor 1, a pointer that
 *      is not aligned as said, out overlapping x.  MCD_E_UNSUPPORTED: D > 2048, or one sequence of 2^31 bytes or more.
 *      B == 0 returns MCD_OK and looks at nothing else.  On any error nothing is written.
 * replaces  sentence-transformers Pooling(pooling_mode_mean_tokens) + Normalize:
 *           sum(x * mask[..., None], 1) / clamp(mask.sum(1), 1e-9), then F.normalize(., p=2, dim=1)
 * ------------------------------------------------------------------------------------------- */
int mcd_masked_mean_l2(const float* x, int B, int T, int D, const int32_t* lens /* may be NULL */, int normalize,
                       float* out, mcd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MCD_SENTENCE_H */
