/*
 * mcd_mask.h -- the masked-autoencoder entries of libmcd_hip.so (K28, K29): the two data movements that transformers'
 * ViTMAEForPreTraining (data_utils.HFMae) adds to the ViT tower's -- the patch rows of the KEPT patches only, in front of
 * the embedding GEMM, and the decoder's mask-token fill, un-shuffle and position add.  Same library, same conventions as
 * include/mcd_hip.h, which this header includes for mcd_stream_t and the MCD_E_* codes: plain device pointers, the caller
 * owns every buffer, nothing is allocated or synchronised inside, every call is asynchronous on `stream` and is
 * hipGraph-capturable (tests/test_gpu_mae.py holds both entries to the stream and capture contracts).
 * Additive to ABI version 9: mcd_abi_version() is unchanged.  The ctypes rows are _lib.MASK_SIGNATURES.
 */
#ifndef MCD_MASK_H
#define MCD_MASK_H

#include "mcd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * K28  K11 with an index list: the patch rows of Lk chosen patches of every image.
 *      x [B, Cin, H, W] fp32 contiguous; keep [B, Lk] int32 contiguous, patch numbers row-major over the
 *      (H/P) x (W/P) patch grid, L = (H/P)*(W/P) of them; out [B, 1 + Lk, Cin*P*P] contiguous.
 *          out[b, 0, :]     = 0                                  (the class-token slot, as in K11)
 *          out[b, 1 + j, :] = patch clamp(keep[b, j], 0, L-1) of image b in K11's (c, dy, dx) order
 *      A permutation of pixels: exact.  An index outside [0, L-1] is clamped, so nothing outside image b is read whatever
 *      keep holds.  P, H and W have K11's constraints (P even and >= 2, H and W multiples of P) and K11's accesses:
 *      16-byte pieces of a patch row at P % 4 == 0, 8-byte pieces at any other even P.  Lk >= 0 (Lk = 0: the zero rows
 *      alone); Lk may exceed L (indices may repeat).
 *      MCD_E_ARG: B < 0 or Lk < 0; with B > 0 a NULL x or out, a NULL keep with Lk > 0, x or out not 16-byte aligned,
 *        keep not 4-byte aligned.
 *      MCD_E_UNSUPPORTED: Cin < 1, P < 2, P odd, H or W < 1 or no multiple of P, B >= 2^30, Lk >= 2^30, one image
 *        (Cin*H*W floats) or one image's rows ((1 + Lk)*Cin*P*P floats) of 2^31 bytes or more.
 *      B == 0 returns MCD_OK and looks at nothing else but the signs of B and Lk.  On any error nothing is written;
 *      every argument check precedes the first HIP call.
 * replaces  patch_embeddings(pixel_values) over ALL patches followed by torch.gather(sequence, 1, ids_keep...)
 *           transformers ViTMAEEmbeddings.forward / random_masking -- the embedding GEMM then has 1 + Lk rows an image
 * ------------------------------------------------------------------------------------------- */
int mcd_patchify_kept(const float* x, const int32_t* keep, int64_t B, int64_t Cin, int64_t H, int64_t W, int64_t P,
                      int64_t Lk, float* out, mcd_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K29  Token restore: rows gathered through an index list, a fill row for the indices past the source, an optional
 *      table added, one launch, fp32, D % 4 == 0, 16-byte accesses along D.
 *      src: 1 + Lk rows of D floats per image, images src_img floats apart (src_img = 0: ONE table shared by all
 *      images); restore [B, L] int32 contiguous; fill [D] or NULL; add [1 + L, D] contiguous or NULL;
 *      dst [B, 1 + L, D] contiguous.  With r = restore[b, t-1]:
 *          dst[b, 0, :] = src[b, 0, :] + add[0, :]
 *          dst[b, t, :] = (r < Lk ? src[b, 1 + max(r, 0), :] : fill) + add[t, :]            1 <= t <= L
 *      fill == NULL: no row is filled and r is clamped to Lk - 1 (needs Lk >= 1 when L >= 1).  add == NULL: nothing is
 *      added (the rows are copied bit for bit).  With add, one fp32 add per element, the gathered row first.
 *      Whatever restore holds, only the 1 + Lk rows of image b's src (or of the shared table) are read.
 *      The decoder of a masked autoencoder: src = decoder_embed's output [B, 1 + Lk, D], restore = ids_restore, fill =
 *      mask_token, add = decoder_pos_embed.  The encoder's position rows: src = the position table [1 + L', D] with
 *      src_img = 0 and Lk = L', restore = the kept patch numbers, fill = add = NULL -> [B, 1 + kept, D].
 *      MCD_E_ARG: B, L or Lk < 0; D < 4 or D % 4 != 0; with B > 0 a NULL src or dst, a NULL restore with L > 0, fill ==
 *        NULL with Lk == 0 and L > 0, src_img < 0, src_img neither 0 nor at least (1 + Lk)*D, src_img % 4 != 0, src, fill,
 *        add or dst not 16-byte aligned, restore not 4-byte aligned, or dst overlapping src (the spans
 *        [src, src + (B-1)*src_img + (1 + Lk)*D) and [dst, dst + B*(1 + L)*D)).
 *      MCD_E_UNSUPPORTED: B >= 2^30, or (1 + L)*D or (1 + Lk)*D floats of 2^31 bytes or more.
 *      B == 0 returns MCD_OK after the sign and D checks.  On any error nothing is written; every argument check
 *      precedes the first HIP call.
 * replaces  mask_token.repeat, cat, gather over an expanded index, cat, + decoder_pos_embed
 *           transformers ViTMAEDecoder.forward
 * ------------------------------------------------------------------------------------------- */
int mcd_token_restore(const float* src, int64_t src_img, const int32_t* restore, const float* fill, const float* add,
                      int64_t B, int64_t L, int64_t Lk, int64_t D, float* dst, mcd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MCD_MASK_H */
