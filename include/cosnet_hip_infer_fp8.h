/* libcosnet_hip -- static-scale fp8 inference extensions of the C ABI (include/cosnet_hip.h,
 * include/cosnet_hip_infer.h).
 *
 * The conv2d + eval BatchNorm2d pair of cosnet_hip_infer.h on e4m3 operands under frozen scales
 * (cosnet_amd/fp8_infer.py, model.set_fp8_static(calibration, fold_bn=True)).  A header of its
 * own: the entry-point sets of the two headers above stay the sets their tests pin.  The
 * conventions, dtype codes and CN_ERR_* codes are the core header's; the entry point lives in
 * the same library.
 */
#ifndef COSNET_HIP_INFER_FP8_H
#define COSNET_HIP_INFER_FP8_H
#include "cosnet_hip_infer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cn_conv_fwd_affine on e4m3 operands: x8, w8, bias, x_state / w_state, the strided views and the
 * operand error codes are cn_conv_fwd_fp8's.  In fp32, per output element:
 *     t = acc * x_state[0] * w_state[0] (+ bias[c]);  t = fmaf(t, scale[c], shift[c]);
 *     t += res[row][c];  t = act(t)
 * y (bf16, nullable) is ONE round-to-nearest-even rounding of t.  y8 (nullable) is the e4m3 image
 * of the same t under the frozen state out_state = (scale, 1 / scale, ., .) of the output tensor:
 *     y8 = e4m3(clamp(t * out_state[1], -448, 448))
 * -- the bytes cn_bn_apply_q8 writes for that fp32 value and state; of t, not of the stored bf16.
 * No state is written.  act: 0 none, 1 ReLU, 2 PReLU with the slope prelu[0]; outside 0..2, or 2
 * without prelu: CN_ERR_UNSUPPORTED.  scale / shift: the fp32 [Cout] arrays of cn_bn_fold_table,
 * 16-byte aligned (null: CN_ERR_SHAPE, misaligned: CN_ERR_ALIGN).  res: null, or a bf16 [M][Cout]
 * view with its own row stride ldr.  At least one of y / y8 (else CN_ERR_SHAPE); y8 needs
 * out_state (CN_ERR_SHAPE), Cout % 8 == 0, ldy8 % 8 == 0 (bytes) and an 8-byte aligned base
 * (CN_ERR_ALIGN); either output may be a column slice of a wider buffer.  No workspace: fp8
 * products do not split over K. */
int cn_conv_fwd_fp8_affine(const void* x8, long long ldx, int N, int H, int W, int Cin,
                           const void* w8, int Cout, int KH, int KW, int stride, int pad, int dil,
                           const float* bias, const float* x_state, const float* w_state,
                           const float* scale, const float* shift,
                           const void* res, long long ldr, int act, const float* prelu,
                           void* y, long long ldy, void* y8, long long ldy8, const float* out_state,
                           int OH, int OW, hipStream_t st);

#ifdef __cplusplus
}
#endif
#endif
