// Shared by the flash co-attention forward / PV kernels (coatt_fused.hip, coatt_dsplit.hip):
// tile geometry and the launch arguments; the padding and key-split rules also serve
// coatt_flash.hip and coatt_f8.hip (rgbd_segmentation_RAA.py:160-170, :213-221).
#pragma once
#include "common.h"

constexpr int FD = 256;              // feature channels (all_channel)
constexpr int FBQ = 128;             // query rows per workgroup
constexpr int FBK = 32;              // keys per tile
constexpr int FROWB = FD * 2;        // bytes per key row in LDS
constexpr int FTILE = FBK * FROWB;   // 16 KB per K (or V) tile
constexpr int FQB = FBQ * FROWB;     // 64 KB Q block

struct FusedDir {
  const bf16* q; const bf16* k; const bf16* v; bf16* o;
  long long ldq, ldk, ldv, ldo;
  float* lse;          // MODE 0 (optional): log2-sum-exp2 of each query row's logits x log2(e),
                       //   [B][HWp] (rows HW..HWp-1 get +inf)
  const float* klse;   // MODE 1: per-KEY normaliser in the same units, [B][HWp], +inf padded
  // Indexed operands (cn_coatt_fused_fwd_idx): q / k / v are banks [T*HW][ld] and pair b reads
  // its query frame qi[b] and its key AND value frame kvi[b] (K and V always share the frame);
  // NULL: frame b, the dense stack.  Outputs, lse and partial slots stay addressed by b.
  const int* qi;
  const int* kvi;
};
struct FusedArgs {
  FusedDir dir[2];
  int HW, HWp, ndir, nrb, nwork, accumulate;
  // tail key split (MODE 0, no-grad forward).  Items = (row block, batch x direction); the
  // first nfull items run whole, one workgroup each (full rounds of the chip); each of the
  // remaining items is split over nsplit workgroups, split s covering key tiles
  // [s tps, (s+1) tps), which write their un-normalised O (fp32) and row (max, sum) to the
  // partials that coatt_merge_k folds in split order -- the last, partial round of workgroups
  // becomes a short round of short workgroups.
  int nitems, nfull, nsplit, tps;
  float* opart;    // [nsplit][nitems - nfull][128][256]
  float* mlpart;   // [nsplit][nitems - nfull][128][2]
  // coatt_q48_k (stream-K): key tiles per item, partial slots per item, per-item arrival counters
  int ntiles, smax;
  int* cnt;
};

// row statistics (lse, klse) are padded to whole 32-key tiles
static inline int hw_pad32(int HW) { return (HW + 31) / 32 * 32; }

// Key splits for `idle` work items that would leave CUs idle at one workgroup per CU (idle < 256):
// 256 / idle splits, at most 8, each of at least 16 key tiles.  1: unsplit.
static inline int key_splits(int idle, int ntiles) {
  int s = 256 / idle;
  if (s > 8) s = 8;
  while (s > 1 && ntiles / s < 16) --s;
  return s;
}

// coatt_dsplit.hip: the d-split wave-pair variant (kernel variant 4) of the forward / PV kernel
int coatt_dsplit_launch(int mode, const FusedArgs& a, dim3 grid, hipStream_t st);

// coatt_q48.hip: 48 query rows per wave on 16x16x32 MFMA tiles (kernel variant 5), 192-row items,
// stream-K work split.  coatt_q48_launch takes a.dir / HW / HWp / accumulate; with a workspace of
// coatt_q48_workspace_bytes (and merge_ok: 16-byte output rows) it cuts items across 256
// workgroups, else it runs one workgroup per item.
int coatt_q48_rows();
size_t coatt_q48_workspace_bytes(int items, int ntiles);
int coatt_q48_launch(int mode, FusedArgs& a, int B, int nd, bool merge_ok, void* ws,
                     size_t ws_bytes, hipStream_t st);
