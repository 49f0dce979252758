/*
 * mcd_tokens.h -- the token-reduction entry of libmcd_hip.so (K26): the mean over the patch tokens that the head of
 * transformers' CLIPForImageClassification (data_utils.HFClip) reads.  Same library, same conventions as
 * include/mcd_hip.h, which this header includes for mcd_stream_t and the MCD_E_* codes: plain device pointers, the caller
 * owns every buffer, nothing is allocated or synchronised inside, the call is asynchronous on `stream` and is
 * hipGraph-capturable (tests/test_gpu_hf_clip.py holds it to the stream and capture contracts).
 * Additive to ABI version 9: mcd_abi_version() is unchanged.  The ctypes row is _lib.TOKEN_SIGNATURES.
 */
#ifndef MCD_TOKENS_H
#define MCD_TOKENS_H

#include "mcd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * K26  The mean of the tokens t0 .. T-1 of every image, in fp32, one launch, no workspace, no environment read:
 *          out[b*out_img + d] = (sum over t = t0 .. T-1 of x[b*x_img + t*x_tok + d]) / (T - t0)     b < B, d < D.
 *      x is [B, T, D] with a unit inner stride, tokens x_tok floats and images x_img floats apart; out is [B, D] with
 *      rows out_img floats apart.  Floats between two tokens, between two images and between two rows of out are
 *      neither read nor written.
 *      The order of the sum depends on n = T - t0 alone -- not on B, not on where an image stands in the batch, not on
 *      the grid -- so the row of image b has the same bits whatever its neighbours are.  With row r = t - t0:
 *        1. four partial sums p_w (w = 0 .. 3), each starting from +0: p_w takes the rows r = w, w + 4, w + 8, ... < n in
 *           ascending order, one fp32 add per row (no fused multiply-add);
 *        2. s = ((p_0 + p_1) + p_2) + p_3   (a p_w that took no row is +0);
 *        3. out = s / (float)n, one correctly rounded fp32 division.
 *      Every column d goes through the same steps (a lane holds four adjacent columns).
 *      MCD_E_ARG: B < 0; with B > 0 a NULL pointer, D < 4, D % 4 != 0, T < 1, t0 < 0, t0 >= T, x_tok < D, out_img < D,
 *        x_img < (T-1)*x_tok + D, a stride that is no multiple of 4 floats, a pointer that is not 16-byte aligned, or out
 *        overlapping x (the spans [x, x + (B-1)*x_img + (T-1)*x_tok + D) and [out, out + (B-1)*out_img + D)).
 *      MCD_E_UNSUPPORTED: B > 65535, or one image -- (T-1)*x_tok + D floats -- of 2^31 bytes or more.
 *      B == 0 returns MCD_OK and looks at nothing else.  On any error nothing is written; every argument check precedes
 *      the first HIP call.
 * replaces  torch.mean(last_hidden_state[:, 1:, :], dim=1)      transformers CLIPForImageClassification.forward
 *           (t0 = 1; the same reduction stands in Dinov2ForImageClassification.forward)
 * ------------------------------------------------------------------------------------------- */
int mcd_token_mean(const float* x, int B, int T, int D, int64_t x_img, int64_t x_tok, int t0,
                   float* out, int64_t out_img, mcd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MCD_TOKENS_H */
