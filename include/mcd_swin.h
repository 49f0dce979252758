/*
 * mcd_swin.h -- the Swin entries of libmcd_hip.so (K31, K32): the two operations of a Swin image tower
 * (data_utils.SwinTower: transformers.SwinModel, the reference's `source: huggingface, model_type: swin` image encoder,
 * model/modules/image_encoder.py:27-28) that no other tower has -- attention inside shifted windows under a 2-D
 * relative-position bias, and 2x2 patch merging in front of a LayerNorm.  Same library, same conventions as
 * include/mcd_hip.h, which this header includes for mcd_stream_t and the MCD_E_* codes: plain device pointers, the caller
 * owns every buffer, nothing is allocated or synchronised inside, no workspace, no environment read, no atomics, every
 * call is asynchronous on `stream` and is hipGraph-capturable (tests/test_gpu_swin.py holds both entries to the stream and
 * capture contracts).  Every argument check precedes the first HIP call.
 * Additive to ABI version 9: mcd_abi_version() is unchanged.  The ctypes rows are _lib.SWIN_SIGNATURES.
 */
#ifndef MCD_SWIN_H
#define MCD_SWIN_H

#include "mcd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * K31  Swin's window attention on the fused projection's output, one launch: cyclic shift, zero padding of the token grid,
 *      window partition, relative-position bias, shift mask, softmax, P.V, window reverse and un-shift are index
 *      arithmetic; no [nW, w^2, w^2] mask and no [heads, w^2, w^2] bias exists in memory.
 *      qkv     [B, H*W, 3, heads, 32] fp32, contiguous, 16-byte aligned: q | k | v of every token of the H x W grid in
 *              token (row-major) order, heads 32 wide.
 *      pad_qkv [3, heads, 32], 16-byte aligned: q | k | v of a padded token (the projection of a zero row: its bias).  The
 *              grid is padded on the bottom and right to Hp x Wp, the multiples of w; NULL is allowed only when
 *              H % w == 0 and W % w == 0.  Padded tokens are keys like any other; they are read from pad_qkv and their
 *              output rows are never stored.
 *      w       the window's side, 1 .. 8 (at most 64 tokens, one per lane of a wave); s the shift, 0 .. w-1.
 *      table   [(2w-1)^2, heads] fp32, contiguous, 4-byte aligned, as the checkpoint stores relative_position_bias_table.
 *      out     [B, H*W, heads*32], contiguous, 16-byte aligned, token order.
 *      The window grid lies on roll(x, (-s, -s)): rolled position (r, c) holds the token of ((r+s) mod Hp, (c+s) mod Wp).
 *      For the tokens (i, j) and (i', j') of one window (in-window coordinates) of head h
 *          score = q.k / sqrt(32) + table[(i-i'+w-1)(2w-1) + (j-j'+w-1), h] + mask,
 *      mask = -100 (transformers' value, not -inf) when s > 0 and the two tokens' (row region, column region) differ --
 *      a rolled row r is in region 0, 1 or 2 for r < Hp-w, r < Hp-s, or otherwise; columns likewise with Wp -- else 0;
 *      out = softmax over the window's w^2 keys, times v, written to the token's original position.
 *      Arithmetic: fp32; q is scaled by log2(e)/sqrt(32) and the table by log2(e) once, scores live in the log2 domain
 *      (exp2, as K9); dot products are fused multiply-adds over the 32 dimensions in ascending order; keys are visited in
 *      window order in groups of w (one window row) under a running maximum; the sum is divided out at the end.
 *      The bits of a window's rows depend on that window's q, k, v, its mask pattern (which tokens differ in region) and
 *      the head's table column alone: not on B, the image index, the window's place in the grid or its neighbours.
 *      A NaN in a token's k or v reaches every stored row of that token's (shifted) window in that head and nothing else.
 *      Results for +-Inf inputs are unspecified.
 *      MCD_E_ARG: NULL qkv / out / table, B < 0, H < 1, W < 1, heads < 1, w < 1, s < 0 or s >= w, a pointer that is not
 *      aligned as said, pad_qkv NULL with a padded grid.  MCD_E_UNSUPPORTED: w > 8, B or heads over 65535, one image's
 *      qkv of 2^31 bytes or more.  B == 0 returns MCD_OK (after the checks).
 * replaces  SwinLayer.forward between layernorm_before and the output projection: pad, roll, window_partition,
 *           SwinSelfAttention (bias gather, mask add, softmax, matmul), window_reverse, roll back, crop
 *           (transformers modeling_swin.py)
 * ------------------------------------------------------------------------------------------- */
int mcd_window_attention(const float* qkv, const float* pad_qkv /* may be NULL */, int64_t B, int64_t H, int64_t W,
                         int64_t heads, int64_t w, int64_t s, const float* table, float* out, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K32  Swin's patch merging up to its LayerNorm, one launch: x [B, H*W, C] -> out [B, ceil(H/2)*ceil(W/2), 4C],
 *          row(b, oy, ox) = x[b, 2oy, 2ox] | x[b, 2oy+1, 2ox] | x[b, 2oy, 2ox+1] | x[b, 2oy+1, 2ox+1]
 *      (transformers' order), a neighbour past an odd edge reading as zeros; out = LayerNorm over the 4C values with
 *      gamma, beta, eps.  One wave gathers the row into K10's registers and runs K10's row routine on it: the result is
 *      mcd_layer_norm's on the gathered row, bit for bit.  x, out, gamma and beta are contiguous and 16-byte aligned.
 *      MCD_E_ARG: a NULL pointer, B < 0, H < 1, W < 1, C < 4, C % 4 != 0, a pointer that is not aligned as said.
 *      MCD_E_UNSUPPORTED: 4C > 2048 (K10's limit), one image of x of 2^31 bytes or more.  B == 0 returns MCD_OK.
 * replaces  SwinPatchMerging.forward up to .norm: pad, four strided slices, cat, LayerNorm (the reduction GEMM follows)
 * ------------------------------------------------------------------------------------------- */
int mcd_patch_merge_ln(const float* x, int64_t B, int64_t H, int64_t W, int64_t C, const float* gamma, const float* beta,
                       float eps, float* out, mcd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MCD_SWIN_H */
