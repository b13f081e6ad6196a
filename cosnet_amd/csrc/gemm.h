// Argument block of the generic implicit-GEMM kernel (gemm.hip).
#pragma once
#include "common.h"

enum LoadKind { L_KC_DENSE = 0, L_KC_CONV = 1, L_MC_DENSE = 2, L_MC_CONV = 3,
                L_KC_CONV_G = 4 };   // KC_CONV whose K tiles may straddle taps (C % BK != 0);
                                     // picked by cn_gemm_dispatch, callers pass L_KC_CONV

// Gather geometry.  For a KC_CONV A operand the GEMM row m is an output pixel (n, oy, ox)
// over the (OH, OW) grid and k = (r, s, ci); the source element is
//   src[n, oy*st + off_y + r*step_y, ox*st + off_x + s*step_x, ci]  (zero outside H x W).
// Forward conv:  st = stride, off = -pad, step = +dilation.
// Dgrad (stride 1): src = dY, off = +pad, step = -dilation, weights in [Cin][kh][kw][Cout].
// For an MC_CONV B operand (wgrad) k is the output pixel and n = (r, s, ci).
struct ConvGeom {
  int N, H, W, C;
  int OH, OW;
  int KH, KW;
  int st;
  int off_y, off_x, step_y, step_x;
  FastDiv div_C, div_KW, div_OW, div_OHW;
};

// Grouped launch: blockIdx.z = problem g (nsplit 1) takes its A / B / C from these arrays
// instead of the a_bs / b_bs / c_bs strides (independent products of one shape, e.g. the weight
// gradients of the bottlenecks of a layer).
constexpr int GEMM_MAXG = 24;
struct GemmGroup {
  const void* A[GEMM_MAXG];
  const void* B[GEMM_MAXG];
  void* C[GEMM_MAXG];
  // fp8 operands: per-problem dequantisation scales (null: the launch-wide scale_a / scale_b)
  const float* SA[GEMM_MAXG];
  const float* SB[GEMM_MAXG];
};

struct GemmArgs {
  int M, N, K;
  int ka_lim, kb_lim;          // k validity bound of each operand (zero beyond)
  const void* A; long long lda, a_bs;
  const void* B; long long ldb, b_bs;
  void* C; long long ldc, c_bs;
  const float* bias;           // [N] fp32 or null
  ConvGeom ga, gb;
  int k_chunk, nsplit;         // split-K: blockIdx.z = batch * nsplit + split
  int row_map;                 // 1: stride-2 dgrad scatter of output rows
  FastDiv rm_div_OW, rm_div_OHW;
  int rm_H, rm_W;
  int c_mode;                  // 0 store, 1 fp32 atomic add, 2 read-add-store,
                               // 3 split-K slab store (C + split * slab)
  long long slab;              // elements between split-K slabs (c_mode 3)
  float alpha;
  const float* scale_a;        // fp8 operands: device per-tensor dequantisation scales (C *= sa * sb)
  const float* scale_b;
  int cfg;                     // tile configuration (gemm.hip kCfg), -1 = shape heuristic
  // BatchNorm epilogues (st_mode != 0: one problem -- batch == 1, never a grouped launch --
  // nsplit == 1, row_map == 0, c_mode 0 only):
  //  st_mode 1: per-(M-tile, column) statistics of the STORED C for train-mode BN: planes
  //             [K, sum(c-K), sum((c-K)^2)] for the tile's first segment (rows < the next
  //             multiple of st_seg_rows) and [sum, sumsq] for the second, K = the tile's first
  //             row (a per-tile shift); plane stride st_plane floats, row = M-tile, col = n.
  //  st_mode 2: BN backward reduce of the stored C (= dy of a BN + ReLU whose pre-BN input is
  //             br_x): dz = dy * (br_x * k1 + sf > 0), xh = (br_x - mu) * is;
  //             planes [sum dz, sum dz * xh].  k1 = gamma * is, sf = beta - mu * k1.
  //  st_mode 4: eval-mode BN folded into a forward conv (cn_conv_fwd_affine; no statistics):
  //             C = act(fma(acc + bias, br_gamma[n], br_beta[n]) + br_x[m][n]),
  //             br_gamma / br_beta = the folded scale / shift, br_x / br_ldx = the residual rows
  //             (C's type, nullable), act / prelu below.  With e4m3 operands (bf16 C;
  //             cn_conv_fwd_fp8_affine) the same fp32 value t is also written as its saturating
  //             e4m3 image under a frozen state, c8 = e4m3(clamp(t * q_state[1], +-448)) -- of t
  //             itself, not of the stored bf16 -- and either of C / c8 may be null.
  int st_mode;
  float* st_ws;
  long long st_plane;
  int st_seg_rows;
  const void* br_x; long long br_ldx;
  const float* br_mean; const float* br_invstd; const float* br_gamma; const float* br_beta;
  int ngroup;                  // > 0: grouped launch (GemmGroup), batch = ngroup, nsplit 1,
                               // st_mode 0; the problems differ in their operands only
  GemmGroup grp;
  int wt;                      // C stores: 4 non-temporal, 0 plain (other: write-through, sc1);
                               // set by cn_gemm_dispatch
  int act;                     // st_mode 4 / 5: 0 none, 1 ReLU, 2 PReLU with the slope prelu[0]
  const float* prelu;
  // st_mode 4 with e4m3 operands: the e4m3 output image [M][N] (nullable), its row stride in
  // bytes, and the frozen state of the output tensor (q_state[1] = 1 / scale; only read)
  unsigned char* c8; long long ldc8;
  const float* q_state;
  // st_mode 5: st_mode 4 with an fp32 addend in front of the affine instead of the residual behind
  //            it (cn_conv_fwd_affine_add; bf16 / fp32 operands):
  //            C = act(fma(acc + bias + add[f * add_rows + r][n], br_gamma[n], br_beta[n])) for
  //            row m = j * add_rows + r, f = add_map ? add_map[j] : j.  add: fp32 rows add_ld floats
  //            apart (64-bit row addressing); add_map: device int32, one entry per block of
  //            add_rows output rows, not range-checked; add_div = fastdiv_make(add_rows).
  const float* add; long long add_ld;
  const int* add_map;
  int add_rows;
  FastDiv add_div;
};

int cn_gemm_dispatch(const GemmArgs& a, int dtype, int c_f32, int la, int lb, int batch, hipStream_t st);
// Tile configuration the dispatcher picks for a bf16 problem, and its block count.
int cn_gemm_pick(int M, int N, int K, int batch_splits);
long long cn_gemm_cfg_blocks(int cfg, int M, int N);
// Tile rows (BM) of the configuration cn_gemm_dispatch uses for a problem (BN epilogues size
// their per-M-tile partials with it).
int cn_gemm_bm(int dtype, int M, int N, int K, int cfg_or_minus1);
// Weight-stationary persistent kernel (gemm_ws.hip) for bf16 KC_DENSE x KC_DENSE products with
// K in {64, 128, 256, 512}: shape / alignment conditions, and the launch.  `walkers_per_xcd` > 0
// caps the M walkers of each XCD (0: as many as the CUs allow).
bool cn_gemm_ws_supports(const GemmArgs& a);
int cn_gemm_ws_launch(const GemmArgs& a, int walkers_per_xcd, hipStream_t st);
int cn_splitk_reduce_impl(const float* ws, int nsplit, long long slab, long long n, float* out,
                          int accumulate, hipStream_t st);
