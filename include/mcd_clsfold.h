/*
 * mcd_clsfold.h -- the class-token fold entry of libmcd_hip.so (K30): what the class-token row of a ViT's last block
 * needs from the other tokens once the K and V projections are folded out of it (data_utils._block_hip).
 * Same library, same conventions as include/mcd_hip.h, which this header includes for mcd_stream_t and the MCD_E_* codes:
 * plain device pointers, the caller owns every buffer, nothing is allocated or synchronised inside, no workspace, the call
 * is asynchronous on `stream` and is hipGraph-capturable (tests/test_gpu_cls_fold.py holds it to both contracts).
 * Additive to ABI version 9: mcd_abi_version() is unchanged.  The ctypes rows are _lib.CLSFOLD_SIGNATURES.
 */
#ifndef MCD_CLSFOLD_H
#define MCD_CLSFOLD_H

#include "mcd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * K30  Softmax-weighted mean of an image's token rows, one weighting per head.  fp32 throughout.
 *      u [B, H, D]: u[b, h, :] at u + b*u_img + h*D, the score vector of head h, ALREADY scaled by log2(e)/8 (the
 *        scores are taken in the log2 domain, on v_exp_f32, as K9 does);
 *      n [B, T, D]: n[b, t, :] at n + b*n_img + t*n_row;
 *      m [B, H, D]: m[b, h, :] at m + b*m_img + h*D.
 *          s[b, h, t] = u[b, h, :] . n[b, t, :]
 *          p[b, h, t] = 2^(s[b, h, t] - max_t s[b, h, :])
 *          m[b, h, :] = (sum_t p[b, h, t] * n[b, t, :]) / (sum_t p[b, h, t])
 *      With u[b, h, :] = W_k,h^T q[b, h, :] * log2(e)/8 and n = LN1(x), W_v,h m[b, h, :] + b_v,h is head h of
 *      softmax(q k^T / 8) v for the one query row q[b]: a key's bias term q . b_k,h is the same for every key and the
 *      softmax cancels it; sum_t p = 1 carries b_v,h through.
 *      One workgroup per image; an image's result depends on its own rows alone, never on B or on its neighbours.  n is
 *      read twice (scores, sums) when the u rows of all heads fit LDS beside the scores, which holds for D = 64*H up to
 *      H = 16 at a ViT's token counts; otherwise the heads are taken in groups and n is re-read per group.
 *      MCD_E_ARG: a NULL pointer; B < 0, H < 1 or D < 1; u, n or m not 16-byte aligned; a stride that is no multiple of
 *        4 floats; u_img or m_img below H*D, n_row or n_img below D.
 *      MCD_E_UNSUPPORTED: D no multiple of 64*H or D > 2048; T < 1 or T > mcd_cls_token_mix_max_t(H, D) (the scores
 *        of all heads stay in LDS: at least 1 024 for every accepted H and D); B > 65 535.
 *      B == 0 returns MCD_OK after these checks.  On any error nothing is written; every argument check precedes the
 *      first HIP call.
 * replaces  the K|V projection of all tokens (M = B*T, N = 2D, K = D) and K9C in the class-token-only last block
 * ------------------------------------------------------------------------------------------- */
int mcd_cls_token_mix(const float* u, int64_t u_img, const float* n, int64_t n_row, int64_t n_img, int64_t B, int64_t T,
                      int64_t H, int64_t D, float* m, int64_t m_img, mcd_stream_t stream);

/* The largest T mcd_cls_token_mix accepts for H heads of width D (0 when H and D themselves are refused). */
int64_t mcd_cls_token_mix_max_t(int64_t H, int64_t D);

#ifdef __cplusplus
}
#endif
#endif /* MCD_CLSFOLD_H */
