/*
 * mcd_clip.h -- the OpenAI-CLIP entries of libmcd_hip.so (K9A, K25): the two encoder-side kernels that the mirror of the
 * reference's CLIP (concept_vit/clip/model.py:239-383, data_utils.OpenAIClip) adds to the ViT tower's -- the causal
 * attention of its text transformer and the QuickGELU of both towers.  Same library, same conventions as
 * include/mcd_hip.h, which this header includes for mcd_stream_t and the MCD_E_* codes: plain device pointers, the caller
 * owns every buffer, nothing is allocated or synchronised inside, every call is asynchronous on `stream` and is
 * hipGraph-capturable (tests/test_gpu_tower_openai_clip.py holds both entries to the stream and capture contracts).
 * Additive to ABI version 9: mcd_abi_version() is unchanged.  The ctypes rows are _lib.CLIP_SIGNATURES.
 */
#ifndef MCD_CLIP_H
#define MCD_CLIP_H

#include "mcd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * K9A  K9 under a causal mask: the self-attention of CLIP's text transformer (head dimension 64, 1 <= T <= 256).
 *      Layout, limits and alignment are K9's: qkv [B, T, 3, H, 64], out [B, T, H*64], both 16-byte aligned, B and H at
 *      most 65535, no workspace.
 *      out[b, t, h, :] = softmax_{j <= t}(q[b,t,h].k[b,j,h] / 8) v[b,j,h]  for every t < T.
 *      Row t equals row t of mcd_vit_attention on sequence b truncated to t + 1 tokens, bit for bit: the wave of a
 *      32-query block walks the key tiles up to its own and no further, with the tile count, the masked keys and the
 *      online-softmax steps of that truncated call.  So a row depends neither on later tokens nor on batch neighbours.
 *      Inputs must be finite.  A NaN in token j may reach every row of j's 32-query block (0 * NaN in the P.V product,
 *      as in ATen) and every later row; it reaches no row of an earlier 32-query block -- those waves never touch tile
 *      j / 32.  Results for +-Inf inputs are unspecified.
 * replaces  nn.MultiheadAttention(x, x, x, need_weights=False, attn_mask=triu(-inf, 1))
 *           concept_vit/clip/model.py:181-183, the mask of :324-330
 * ------------------------------------------------------------------------------------------- */
int mcd_vit_attention_causal(const float* qkv, int64_t B, int64_t T, int64_t H, float* out, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K25  QuickGELU, elementwise in fp32:  out[i] = x[i] * (1 / (1 + exp(-(1.702f * x[i]))))  for i < n.
 *      x and out are 16-byte aligned and either the same pointer or disjoint (out == x works in place); n >= 0, and
 *      n = 0 is a no-op that returns 0 (the pointers are then not looked at).  The body moves float4s, the n % 4 tail
 *      goes element by element.  exp is v_exp_f32 on the argument times log2(e).  Every finite x gives a finite result:
 *      a large negative x gives -0 or 0 (exp overflows to +inf, 1 / inf = 0), never NaN; a NaN stays a NaN.
 * replaces  QuickGELU.forward: x * torch.sigmoid(1.702 * x), three launches      concept_vit/clip/model.py:162-164
 * ------------------------------------------------------------------------------------------- */
int mcd_quick_gelu(const float* x, int64_t n, float* out, mcd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MCD_CLIP_H */
