/*
 * mcd_stem.h -- the 7x7 / 2 image stem with its epilogue, of libmcd_hip.so: the first unit of transformers' ResNet
 * (data_utils.HFResNet: ResNetForImageClassification, the reference's `resnet` targets, concept_vit/data_utils.py:21-36,
 * :63-69), whose convolution, batch norm and ReLU are one module (ResNetConvLayer), so that the hook on it sees the tensor
 * behind the ReLU and K16's raw sums are of no use.  Same library, same conventions as include/mcd_hip.h, which this
 * header includes for mcd_stream_t and the MCD_E_* codes: plain device pointers, the caller owns every buffer, nothing is
 * allocated or synchronised inside, no workspace, no environment read, no atomics, the call is asynchronous on `stream`
 * and is hipGraph-capturable (tests/test_gpu_hf_resnet.py holds it to the stream and capture contracts).  Every argument
 * check precedes the first HIP call.
 * Additive to ABI version 9: mcd_abi_version() is unchanged.  The ctypes row is _lib.STEM_SIGNATURES.
 */
#ifndef MCD_STEM_H
#define MCD_STEM_H

#include "mcd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * The 7x7 / 2 stem with K19's epilogue: x NCHW [B, Cin, H, W] (Cin <= 4) -> y NHWC [B, Ho, Wo, Cout] =
 *      act(conv7x7/2, pad 3 (x, w) + bias), Ho = (H + 6 - 7) / 2 + 1; w tap-major [Cin, 7, 7, Cout] with the batch norm
 *      folded in, Cout % 4 == 0; bias [Cout]; act = ReLU when relu != 0 (it keeps a NaN).  K16's kernel with K19's
 *      epilogue (stem_conv_kernel<7, CO, true>, csrc/k_resnet.hip): a 16 x 16 output tile per workgroup, its
 *      37 x 37 x Cin window in LDS, weights through the scalar cache, 32 output channels per pass (4 when Cout % 32).
 *      Per output element: one fmaf chain from 0 over (channel, row, column) -- K16's chain, so with bias = 0 and
 *      relu = 0 the values are mcd_conv7x7s2_nhwc's (a -0 becomes +0: the epilogue adds +0) -- then + bias, then the
 *      ReLU.  An image's bits depend neither on the batch it is in nor on its place in it.
 *      K19's argument contract.  MCD_E_ARG: a NULL x / w / bias / y, B < 0, Cin < 1 or > 4, H < 1, W < 1, Cout < 4 or
 *      Cout % 4 != 0, w / bias / y not 16-byte aligned (x: 4), an x, w or bias that overlaps y.  MCD_E_UNSUPPORTED: one
 *      image of x or of y of 2^31 bytes or more, B > 65535.  B == 0 returns MCD_OK (after the checks).
 * replaces  resnet.embedder.embedder (convolution + normalization + activation) of transformers' ResNet
 *           (modeling_resnet.py, ResNetEmbeddings)
 * ------------------------------------------------------------------------------------------- */
int mcd_conv7x7s2_bias_relu_nhwc(const float* x, int64_t B, int64_t Cin, int64_t H, int64_t W, const float* w,
                                 const float* bias, int64_t Cout, int relu, float* y, mcd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MCD_STEM_H */
