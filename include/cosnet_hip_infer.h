/* libcosnet_hip -- inference extensions of the C ABI (include/cosnet_hip.h).
 *
 * Launches that replace a *pair* of reference calls, conv2d + eval BatchNorm2d: in eval mode a
 * BatchNorm2d is a frozen per-channel affine, so the conv GEMM's epilogue applies it (with the
 * block's residual add and activation) and the raw conv output never exists in memory.  The
 * conventions, dtype codes and CN_ERR_* codes are the core header's; the entry points live in
 * the same library.  Feature-bank inference (cosnet_amd/bn_fold.py) is their only caller.
 */
#ifndef COSNET_HIP_INFER_H
#define COSNET_HIP_INFER_H
#include "cosnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* scale[c] = gamma[c] * invstd[c], shift[c] = beta[c] - run_mean[c] * scale[c] with
 * invstd[c] = 1 / sqrt(run_var[c] + eps) as cn_bn_eval_params computes it: the affine that
 * cn_bn_apply forms from (mean, invstd, gamma, beta) on every call, in the same fp32 arithmetic.
 * gamma / beta may be null (a BatchNorm2d without affine parameters: 1 and 0).  nn.BatchNorm2d
 * in eval mode: deeplab/residual_net.py:80,84,88,158 ; deeplab/deeplabv3_encoder.py:59,64,81 ;
 * rgbd_segmentation_RAA.py:190,242.  One launch, at set-up time. */
int cn_bn_fold_table(const float* run_mean, const float* run_var, const float* gamma,
                     const float* beta, int C, float eps, float* scale, float* shift,
                     hipStream_t stream);

/* y = act(fma(conv2d(x, w) + bias, scale, shift) + res): nn.Conv2d.forward followed by an
 * eval-mode nn.BatchNorm2d.forward, the residual add and the activation in one launch
 * (deeplab/residual_net.py:79-96 a bottleneck's three pairs, :157-159 the stem ;
 * deeplab/deeplabv3_encoder.py:58-60,63-65,80-82 the ASPP ; rgbd_segmentation_RAA.py:189-190,
 * 241-242 the reduce convs).  In fp32, per output element:
 *     t = acc (+ bias[c]);  t = fmaf(t, scale[c], shift[c]);  t += res[row][c];  t = act(t)
 * and y is ONE round-to-nearest-even rounding of t (bf16) or t itself (fp32).  act: 0 none,
 * 1 ReLU, 2 PReLU with the slope prelu[0] (cn_bn_apply's convention).  scale / shift: fp32
 * [Cout] device arrays, 16-byte aligned (cn_bn_fold_table).  res: null, or a [M][Cout] view of
 * y's dtype with its own row stride ldr.  x, w, bias, y, OH / OW, the strided views and the
 * bounds contract are cn_conv_fwd's; y may be a column slice of a wider buffer.  ws / ws_floats
 * as cn_conv_fwd_ws (cn_conv_fwd_workspace_floats): a shape that splits over K applies the affine
 * in its reduce. */
int cn_conv_fwd_affine(int dtype, const void* x, long long ldx, int N, int H, int W, int Cin,
                       const void* w, int Cout, int KH, int KW, int stride, int pad, int dil,
                       const float* bias, void* y, long long ldy, int OH, int OW,
                       const float* scale, const float* shift, const void* res, long long ldr,
                       int act, const float* prelu, float* ws, size_t ws_floats,
                       hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
