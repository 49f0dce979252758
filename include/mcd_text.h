/*
 * mcd_text.h -- the text-tower entries of libmcd_hip.so (K9M, K24): the encoder-side kernels of the BERT text tower
 * that mirrors the reference's BreastClip.text_encoder (model/clip.py:17: HuggingfaceTextEncoder around
 * transformers.BertModel, model/modules/text_encoder.py:48).  Same library, same conventions as include/mcd_hip.h,
 * which this header includes for mcd_stream_t and the MCD_E_* codes: plain device pointers, the caller owns every
 * buffer, nothing is allocated or synchronised inside, every call is asynchronous on `stream` and is
 * hipGraph-capturable (tests/test_gpu_text_tower.py holds both entries to the stream and capture contracts).
 * Additive to ABI version 9: mcd_abi_version() is unchanged.  The ctypes rows are _lib.TEXT_SIGNATURES.
 */
#ifndef MCD_TEXT_H
#define MCD_TEXT_H

#include "mcd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * K9M  K9 with a key count per sequence: the self-attention of a padded text batch (head dimension 64, 1 <= T <= 256).
 *      Layout and alignment are K9's: qkv [B, T, 3, H, 64], out [B, T, H*64], both 16-byte aligned.  lens points to B
 *      int32 on the device, or is NULL (every length is T: the whole output is then K9's, bit for bit).  Sequence b
 *      attends to keys 0 .. L-1, L = clamp(lens[b], 1, T): the values are on the device, the host cannot refuse them,
 *      so the clamp is part of the contract (lens[b] <= 0 acts as 1, lens[b] > T as T).
 *      out[b, t, h, :] = softmax_{j < L}(q[b,t,h].k[b,j,h] / 8) v[b,j,h]  for EVERY t < T -- the padded query rows
 *      t >= L are computed and stored too, attending to the L valid keys, which is what BertModel / SDPA give under a
 *      key-padding mask.  No K or V row >= L is read (the loader clamps to row L-1, the tile count is ceil(L / 32)):
 *      a NaN in a padded K or V row reaches nothing.  Rows t < L equal mcd_vit_attention on sequence b truncated to L
 *      tokens, bit for bit, so neither padding nor batch neighbours change a valid row.  No workspace.
 *      A NaN propagates as in K9 (in q: that output row of that head; in a valid k row: every query of that sequence
 *      and head; in a valid v row: that column of them); results for +-Inf inputs are unspecified.  No causal mask.
 * replaces  the attention inside BertModel(**x) under attention_mask         model/modules/text_encoder.py:48
 * ------------------------------------------------------------------------------------------- */
int mcd_vit_attention_keylen(const float* qkv, int64_t B, int64_t T, int64_t H, const int32_t* lens, float* out,
                             mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K24  the embedding rows of the BERT text tower in one launch:
 *      out[r] = LayerNorm((word[ids[r]] + type[type_ids[r]]) + pos[r % T])   for r < rows = B * T,
 *      the two adds in BertEmbeddings' order, one fp32 rounding each, the normalisation K10's row routine: the result
 *      is bit-identical to mcd_layer_norm on ATen's sum of the three gathers.  word [vocab, D], type [n_type, D],
 *      pos [>= T, D] (the caller guarantees the T rows: the entry cannot see the table's size), gamma / beta [D], out
 *      [rows, D], all contiguous and 16-byte aligned; ids / type_ids [rows] int64, type_ids may be NULL (= row 0 of
 *      type for every token).  K10's limits: D a multiple of 4 up to 2048.  An id outside [0, vocab) or [0, n_type) is
 *      clamped into the table -- never read out of range; the Python binding refuses such ids on the host.
 * replaces  BertEmbeddings.forward inside BertModel(**x)                      model/modules/text_encoder.py:48
 * ------------------------------------------------------------------------------------------- */
int mcd_text_embed_ln(const int64_t* ids, const int64_t* type_ids /* may be NULL = row 0 */, const float* word,
                      const float* pos, const float* type, const float* gamma, const float* beta, float eps, int64_t rows,
                      int64_t T, int64_t D, int64_t vocab, int64_t n_type, float* out, mcd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MCD_TEXT_H */
