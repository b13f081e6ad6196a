/* libcosnet_hip -- bank-head inference extensions of the C ABI (include/cosnet_hip.h,
 * include/cosnet_hip_infer.h).
 *
 * A convolution is linear in its input channels, so the reduce conv of the a-side head over
 * cat = [gate(Z_a) | V_a] (rgbd_segmentation_RAA.py:186-190, :235-242) splits into
 *     conv(W[..., :C], gate(Z_a)) + conv(W[..., C:], V_a)
 * whose second term depends on the target frame alone.  cn_conv_fwd_partial computes that term once
 * per frame of a feature bank, unrounded; cn_conv_fwd_affine_add computes the first term per
 * (target, reference) pair and adds the frame's partial in the GEMM epilogue, before the eval-mode
 * BatchNorm and the one rounding (model.set_head_split(), head_a_indexed(split=True)).  A header of
 * its own: the entry-point sets of the three headers above stay the sets their tests pin.  The
 * conventions, dtype codes and CN_ERR_* codes are the core header's; the entry points live in the
 * same library.
 */
#ifndef COSNET_HIP_INFER_HEAD_H
#define COSNET_HIP_INFER_HEAD_H
#include "cosnet_hip_infer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cn_conv_fwd whose output is the fp32 accumulator itself: y is always fp32 [M][Cout] with the row
 * stride ldy in floats and holds acc (+ bias[c]) with no rounding, whatever the operand dtype.
 * x, w, bias, OH / OW, the strided views, the bounds contract and the error codes are
 * cn_conv_fwd's.  dtype: bf16 or fp32 operands (else CN_ERR_UNSUPPORTED).  The product never
 * splits over K and takes no workspace. */
int cn_conv_fwd_partial(int dtype, const void* x, long long ldx, int N, int H, int W, int Cin,
                        const void* w, int Cout, int KH, int KW, int stride, int pad, int dil,
                        const float* bias, void* y, long long ldy, int OH, int OW,
                        hipStream_t stream);

/* cn_conv_fwd_affine with an fp32 addend, looked up per block of add_rows output rows, in front of
 * the affine.  With M = N * OH * OW output rows, per output element of row m and column c, in fp32:
 *     j = m / add_rows;  r = m % add_rows;  f = add_map ? add_map[j] : j
 *     t = acc (+ bias[c]);  t = t + add[(f * add_rows + r) * lda + c]
 *     t = fmaf(t, scale[c], shift[c]);  t = act(t)
 * and y is ONE round-to-nearest-even rounding of t (bf16) or t itself (fp32).  The first 19
 * parameters (x, w, bias, y, OH / OW: one contract for x, w and y), scale / shift, act and prelu are
 * cn_conv_fwd_affine's.  add: fp32 rows of at least Cout floats, lda floats apart (64-bit row
 * addressing); a row that 16-byte loads cannot take (a ragged column edge, a view that is not
 * 16-byte aligned) is read element-wise.  add_map: null, or a device int32 array of M / add_rows
 * entries, 4-byte aligned, which the kernel does not range-check.  add null, add_rows <= 0,
 * M % add_rows != 0 or lda < Cout: CN_ERR_SHAPE; misaligned scale, shift (16 bytes) or add_map
 * (4 bytes): CN_ERR_ALIGN; a dtype other than bf16 / fp32, act outside 0..2 or 2 without prelu:
 * CN_ERR_UNSUPPORTED.  No residual operand, no split over K, no weight-stationary route.  Served:
 * the plain 1x1 product and the conv gather whose K tiles hold one tap each (Cin a multiple of 64
 * bf16 / 32 fp32 channels); any other gather, or a forced tile configuration without this
 * epilogue, is CN_ERR_UNSUPPORTED. */
int cn_conv_fwd_affine_add(int dtype, const void* x, long long ldx, int N, int H, int W, int Cin,
                           const void* w, int Cout, int KH, int KW, int stride, int pad, int dil,
                           const float* bias, void* y, long long ldy, int OH, int OW,
                           const float* scale, const float* shift,
                           const float* add, long long lda, const int* add_map, int add_rows,
                           int act, const float* prelu, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
