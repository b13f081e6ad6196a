// Device helpers shared by the implicit-GEMM kernels (gemm.hip, gemm_ws.hip): the buffer-form
// LDS-DMA, the barrier that does not drain it, and the bf16 fragment read of a k-contiguous tile.
#pragma once
#include "common.h"

// Buffer-descriptor form of the LDS-DMA (buffer_load_dwordx4 ... lds): address = base +
// soffset (SGPR, wave-uniform: the K position of the tile) + voffset (VGPR, constant per chunk
// over a whole tap / the whole K loop).  The hardware range check covers voffset only (not
// soffset): a chunk with no source (padding row / column, conv tap outside the image, k past the
// end) gets voffset = BUF_OOB and reads zeros -- no zero page, no per-chunk select, no 64-bit
// address arithmetic in the K loop.
constexpr unsigned BUF_OOB = 0x80000000u;   // = num_records of every operand descriptor
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* base) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)BUF_OOB, 0x00020000);
}
__device__ __forceinline__ void blds16(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff,
                                       char* lds_wave_base) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds_wave_base,
                                           16, (int)voff, (int)soff, 0, 0);
}

// Workgroup barrier that does NOT drain the LDS-DMA queue (unlike __syncthreads(), whose
// fence emits vmcnt(0)); the asm memory clobbers keep the compiler from moving LDS accesses
// across it.
__device__ __forceinline__ void raw_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// bf16 fragment of a k-contiguous tile ([rows][128 B], 16-byte chunk c of row r in slot
// c ^ (r & 7)) for k-piece p (32 k values): lane l -> row/col (l & 15), k = 32p + 8(l >> 4) + j
__device__ __forceinline__ bf16x8 read_frag_kc_bf16(const char* lds, int rowbase, int p, int lane) {
  const int row = rowbase + (lane & 15);
  const int c = 4 * p + (lane >> 4);
  return *(const bf16x8*)(lds + row * 128 + ((c ^ (row & 7)) << 4));
}
