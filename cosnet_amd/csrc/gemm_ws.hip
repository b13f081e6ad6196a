// Weight-stationary persistent GEMM for the shallow-K 1x1 products (K <= 512, bf16):
//
//   C[m][n] (+)= sum_k A[m][k] * B[n][k]      A, B row-major with k contiguous, fp32 accumulation
//
// With K = 256 a tile of the generic kernel (gemm.hip) runs four K steps: every block pays a
// pipeline fill, re-fetches the B panel its column shares with every other M-tile, and stores
// its C tile with nothing else in flight.  Here a block keeps one BN-column slice of B in LDS for
// the whole launch and walks a contiguous range of M in BM-row tiles:
//
//   prologue  B slice + A tile 0 by LDS-DMA (and the old C rows of tile 0 for read-add-store)
//   tile t    issue the DMA of A tile t+1 into the other ring stage (and fetch tile t+1's old C)
//             MFMAs of tile t over the whole K (no barrier inside)
//             epilogue of tile t: each wave stages its own accumulators through a private LDS
//             patch and stores whole 16-byte row pieces
//             counted wait: everything but tile t's own stores has landed; one barrier
//
// so the C stores of tile t drain while tile t+1's MFMAs run and tile t+2's A is in flight, the
// per-tile LDS fill is A alone, and there is neither a per-tile prologue nor a partial last round
// of blocks.  Blocks never talk to each other.
//
// Counted waits: gfx9 retires vector memory operations in issue order on one counter (vmcnt),
// loads, LDS-DMA and stores alike.  Every store and every old-C load of the tile loop is therefore
// issued UNCONDITIONALLY -- rows or columns without a destination get the out-of-range buffer
// offset (the store is dropped) or a harmless address (the load is ignored) -- so the number of
// operations younger than the A prefetch is a compile-time constant.  The old-C loads are inline
// assembly (the compiler drains the DMA queue for ordinary loads beside an LDS-DMA); their
// registers are tied to the hand-placed wait.
//
// Numerics are those of gemm_kernel: v_mfma_f32_16x16x32_bf16 with A as the A operand, one
// accumulator chain per element over ascending k with the same k-to-lane assignment, fp32 add of
// the old C and one bf16 rounding -- the results are bitwise the generic kernel's.
#include "common.h"
#include "gemm.h"
#include "gemm_dev.h"
#include "../../include/cosnet_hip.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace {

struct WsArgs {
  int M, N;
  const bf16* A; long long lda;
  const bf16* B; long long ldb;
  bf16* C; long long ldc;
  int nslices;   // BN-column slices of B
  int wpx;       // M walkers per XCD (each walker = nslices blocks, one per slice)
  int wt;        // C store policy (GemmArgs::wt)
  // FOLD (eval-mode BN fold, GemmArgs st_mode 4): C = act(fma(acc, scale[n], shift[n]) + res[m][n])
  const bf16* res; long long ldr;   // residual rows (FOLD 2)
  const float* scale; const float* shift;
  int act;       // 0 none, 1 ReLU
};

__device__ __forceinline__ u32x4 load16_asm(const void* p) {
  u32x4 v;
  asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(v) : "v"(p) : "memory");
  return v;
}

// Everything but the youngest KEEP vector memory operations of this wave has landed; the old-C
// registers (TIE) are tied to the wait so no use of them can be scheduled above it.
template <int KEEP, bool TIE, int N>
__device__ __forceinline__ void wait_keep(u32x4 (&x)[N]) {
  static_assert(KEEP < 64, "vmcnt is 6 bits");
  asm volatile("s_waitcnt vmcnt(%0)" :: "n"(KEEP) : "memory");
  if constexpr (TIE) {
#pragma unroll
    for (int i = 0; i < N; ++i) asm volatile("" : "+v"(x[i]));
  }
}

// KT = K / 64 k-tiles; BM x BN block tile, WM x WN waves; MODE2: read-add-store (c_mode 2);
// BREG: B fragments in registers; FOLD: the eval-mode BN fold before the one rounding -- 1 the
// per-column affine and the activation, 2 also the residual rows, which take the old-C rows'
// prefetch slots (as many loads per tile, issued as unconditionally: the counted waits are MODE2's).
// LDS: [B slice: KT x BN x 128 B][A ring: 2 x KT x BM x 128 B][per-wave fp32 staging patches].
template <int KT, int BM, int BN, int WM, int WN, bool MODE2, bool BREG, int FOLD = 0>
__global__ __launch_bounds__(WM * WN * 64, 1) void gemm_ws_kernel(WsArgs p) {
  static_assert(!(MODE2 && FOLD), "the fold stores, it does not accumulate");
  constexpr bool PRE = MODE2 || FOLD == 2;   // rows prefetched under the counted wait
  constexpr int NT = WM * WN * 64;
  constexpr int BBYTES = KT * BN * 128, ASTG = KT * BM * 128;
  constexpr int TM = BM / WM, TN = BN / WN;   // wave tile
  constexpr int RM = TM / 16, RN = TN / 16;
  constexpr int NCA = BM * 8 / NT, NCB = BN * 8 / NT;   // 16-byte chunks per thread per k-tile
  constexpr int RSTEP = NT / 8;
  constexpr int CSB = TM * TN * 4;                      // staging patch of one wave
  constexpr int GPR = TN / 8, RPP = 64 / GPR, IT = TM / RPP;   // epilogue: 8-column groups, rows per pass
  static_assert(NCA >= 1 && NCA * NT == BM * 8 && NCB * NT == BN * 8, "tiles fill whole chunk rounds");
  static_assert(RSTEP % 8 == 0, "a thread's chunks share row & 7");
  static_assert(IT >= 1 && IT * RPP == TM && (RN & (RN - 1)) == 0, "epilogue passes");
  static_assert(BBYTES + 2 * ASTG + WM * WN * CSB <= 160 * 1024, "LDS budget");
  __shared__ __attribute__((aligned(16))) char smem[BBYTES + 2 * ASTG + WM * WN * CSB];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;

  // Placement (speed only): under round-robin dispatch block b runs on XCD b & 7; the nslices
  // blocks of one walker sit on one XCD, so an A tile comes from HBM once and hits that XCD's L2
  // for the other slices.
  const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
  const int slice = j % p.nslices;
  const int walker = xcd * p.wpx + j / p.nslices, nwalk = 8 * p.wpx;
  const int n0 = slice * BN;
  // this walker's rows: the 16-row granules of M dealt evenly, so a partial last tile costs
  // MFMA time only (its missing rows are neither fetched nor stored)
  const int m16 = (p.M + 15) >> 4;
  const int r0 = (int)((long long)m16 * walker / nwalk) * 16;
  const int r1 = min(p.M, (int)((long long)m16 * (walker + 1) / nwalk) * 16);
  if (r0 >= r1) return;
  const int ntiles = (r1 - r0 + BM - 1) / BM;

  // FOLD: this lane's eight scale / shift values (its columns are fixed for the launch), loaded
  // before any LDS-DMA is in flight
  float fsc[FOLD ? 8 : 1], fsh[FOLD ? 8 : 1];
  if constexpr (FOLD != 0) {
    const int fc = n0 + wn * TN + (lane % (TN / 8)) * 8;
    const bool in = fc < p.N;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const f32x4 s0 = in ? *(const f32x4*)(p.scale + fc) : z, s1 = in ? *(const f32x4*)(p.scale + fc + 4) : z;
    const f32x4 h0 = in ? *(const f32x4*)(p.shift + fc) : z, h1 = in ? *(const f32x4*)(p.shift + fc + 4) : z;
#pragma unroll
    for (int e = 0; e < 4; ++e) { fsc[e] = s0[e]; fsc[4 + e] = s1[e]; fsh[e] = h0[e]; fsh[4 + e] = h1[e]; }
  }

  char* Bs = smem;
  char* As = smem + BBYTES;
  float* cs = (float*)(smem + BBYTES + 2 * ASTG + wave * CSB);
  const int wbase = __builtin_amdgcn_readfirstlane((tid & ~63) * 16);   // the wave's chunks of a round

  // chunk geometry of the fills: chunk q = tid + NT i lands at byte 16 q of a k-tile; the XOR
  // swizzle lives in the source address (gemm.hip Loader)
  const int kcol = ((tid & 7) ^ ((tid >> 3) & 7)) * 8;
  const int rl0 = tid >> 3;

  {  // B slice, once
    const __amdgpu_buffer_rsrc_t rb = buf_rsrc(p.B + (long long)n0 * p.ldb);
#pragma unroll
    for (int i = 0; i < NCB; ++i) {
      const int rl = rl0 + RSTEP * i;
      const unsigned voff = n0 + rl < p.N ? (unsigned)((rl * p.ldb + kcol) * 2) : BUF_OOB;
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) blds16(rb, voff, kt * 128, Bs + kt * BN * 128 + wbase + i * NT * 16);
    }
  }
  auto issue_a = [&](int t, char* stg) {
    const int m0 = r0 + t * BM;
    const __amdgpu_buffer_rsrc_t ra = buf_rsrc(p.A + (long long)m0 * p.lda);
#pragma unroll
    for (int i = 0; i < NCA; ++i) {
      const int rl = rl0 + RSTEP * i;
      const unsigned voff = m0 + rl < r1 ? (unsigned)((rl * p.lda + kcol) * 2) : BUF_OOB;
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) blds16(ra, voff, kt * 128, stg + kt * BM * 128 + wbase + i * NT * 16);
    }
  };
  // epilogue geometry: lane -> 8 columns (lane % GPR) of rows lane / GPR + RPP it of the wave tile
  const int erow = wm * TM + lane / GPR, ecol = n0 + wn * TN + (lane % GPR) * 8;
  const bool col_ok = ecol < p.N;   // N % 8 == 0: a column group is whole or absent
  u32x4 xnx[PRE ? IT : 1], xpf[PRE ? IT : 1];
  const bf16* const pre_base = FOLD == 2 ? p.res : p.C;
  const long long pre_ld = FOLD == 2 ? p.ldr : p.ldc;
  auto fetch_c = [&](int t) {   // old C (FOLD 2: residual) rows of tile t (always IT loads)
    const int m0 = r0 + t * BM;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int row = m0 + erow + it * RPP;
      const bf16* src = (row < r1 && col_ok) ? pre_base + (long long)row * pre_ld + ecol : pre_base;
      xnx[it] = load16_asm(src);
    }
  };
  issue_a(0, As);
  if constexpr (PRE) fetch_c(0);
  wait_keep<0, PRE>(xnx);
  raw_barrier();

  // BREG: the wave's B fragments (its TN columns over the whole K) live in registers for the
  // launch, so a tile reads only its A fragments from LDS
  bf16x8 breg[BREG ? KT * 2 : 1][RN];
  if constexpr (BREG) {
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int pc = 0; pc < 2; ++pc)
#pragma unroll
        for (int jj = 0; jj < RN; ++jj)
          breg[kt * 2 + pc][jj] = read_frag_kc_bf16(Bs + kt * BN * 128, wn * TN + jj * 16, pc, lane);
  }

  auto epilogue = [&](int t, auto aux_c, const f32x4 (&acc)[RM][RN]) {
    constexpr int AUX = decltype(aux_c)::value;
    const int m0 = r0 + t * BM;
    const __amdgpu_buffer_rsrc_t rc = buf_rsrc(p.C + (long long)m0 * p.ldc);
    const int g = lane >> 4;
    // lane holds C[16 i + 4 g + r][16 j + (l & 15)] of the wave tile; the 16-column groups of a
    // row are XOR-swizzled by g so the four row groups of one store hit distinct banks
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int jj = 0; jj < RN; ++jj)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          cs[(i * 16 + 4 * g + r) * TN + (((jj ^ (g & (RN - 1))) << 4) | (lane & 15))] = acc[i][jj][r];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // wave-private patch: no barrier
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int rr = lane / GPR + it * RPP;
      const int c0 = ((lane % GPR) * 8) ^ ((((rr >> 2) & 3) & (RN - 1)) << 4);
      float v[8];
      *(f32x4*)&v[0] = *(const f32x4*)&cs[rr * TN + c0];
      *(f32x4*)&v[4] = *(const f32x4*)&cs[rr * TN + c0 + 4];
      if constexpr (MODE2) {
        float q[8];
        Chunk<bf16>::unpack(xpf[it], q);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += q[e];
      }
      if constexpr (FOLD != 0) {   // gemm_kernel's EPI 4 arithmetic
        float q[8];
        if constexpr (FOLD == 2) Chunk<bf16>::unpack(xpf[it], q);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float u = fmaf(v[e], fsc[e], fsh[e]);
          if constexpr (FOLD == 2) u += q[e];
          v[e] = p.act == 1 ? fmaxf(u, 0.f) : u;
        }
      }
      const int row = erow + it * RPP;   // within the tile
      const unsigned off = (m0 + row < r1 && col_ok) ? (unsigned)(((long long)row * p.ldc + ecol) * 2) : BUF_OOB;
      __builtin_amdgcn_raw_buffer_store_b128(Chunk<bf16>::pack(v), rc, (int)off, 0, AUX);
    }
    asm volatile("" ::: "memory");
  };

#pragma unroll 1
  for (int t = 0; t < ntiles; ++t) {
    char* cur = As + (t & 1) * ASTG;
    if constexpr (PRE) {
#pragma unroll
      for (int it = 0; it < IT; ++it) xpf[it] = xnx[it];
    }
    // the other stage held tile t-1: every wave passed the barrier that ended it
    if (t + 1 < ntiles) {
      issue_a(t + 1, As + ((t + 1) & 1) * ASTG);
      if constexpr (PRE) fetch_c(t + 1);
    }
    f32x4 acc[RM][RN];
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int jj = 0; jj < RN; ++jj) acc[i][jj] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int pc = 0; pc < 2; ++pc) {
        bf16x8 af[RM], bfr[RN];
#pragma unroll
        for (int i = 0; i < RM; ++i) af[i] = read_frag_kc_bf16(cur + kt * BM * 128, wm * TM + i * 16, pc, lane);
#pragma unroll
        for (int jj = 0; jj < RN; ++jj) {
          if constexpr (BREG) bfr[jj] = breg[kt * 2 + pc][jj];
          else bfr[jj] = read_frag_kc_bf16(Bs + kt * BN * 128, wn * TN + jj * 16, pc, lane);
        }
#pragma unroll
        for (int i = 0; i < RM; ++i)
#pragma unroll
          for (int jj = 0; jj < RN; ++jj)
            acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[jj], acc[i][jj], 0, 0, 0);
      }
    // C store policy as in gemm_kernel: 4 non-temporal, other non-zero write-through (sc1), 0 plain
    if (p.wt == 4) epilogue(t, std::integral_constant<int, 2>{}, acc);
    else if (p.wt) epilogue(t, std::integral_constant<int, 16>{}, acc);
    else epilogue(t, std::integral_constant<int, 0>{}, acc);
    if (t + 1 < ntiles) {
      // tile t+1's A (and old C) are older than tile t's IT stores: leave only those in flight
      wait_keep<IT, PRE>(xnx);
      raw_barrier();
    }
  }
}

template <int KT, int BM, int BN, int WM, int WN, bool BREG>
int launch_ws(const GemmArgs& a, int cus, int cap, hipStream_t st) {
  WsArgs w;
  w.M = a.M; w.N = a.N;
  w.A = (const bf16*)a.A; w.lda = a.lda;
  w.B = (const bf16*)a.B; w.ldb = a.ldb;
  w.C = (bf16*)a.C; w.ldc = a.ldc;
  w.nslices = (a.N + BN - 1) / BN;
  w.wt = a.wt;
  w.res = (const bf16*)a.br_x; w.ldr = a.br_ldx;
  w.scale = a.br_gamma; w.shift = a.br_beta;
  w.act = a.act;
  const int per_xcd = cus / 8;
  // no more walkers than 16-row granules of M
  const int want = (int)((((long long)a.M + 15) / 16 + 7) / 8);
  w.wpx = std::min(per_xcd / w.nslices, std::max(want, 1));
  if (cap > 0) w.wpx = std::min(w.wpx, cap);
  if (w.wpx < 1) return CN_ERR_UNSUPPORTED;
  const dim3 grid(8 * w.wpx * w.nslices), block(WM * WN * 64);
  if (a.st_mode == 4 && a.br_x)
    hipLaunchKernelGGL((gemm_ws_kernel<KT, BM, BN, WM, WN, false, BREG, 2>), grid, block, 0, st, w);
  else if (a.st_mode == 4)
    hipLaunchKernelGGL((gemm_ws_kernel<KT, BM, BN, WM, WN, false, BREG, 1>), grid, block, 0, st, w);
  else if (a.c_mode == 2)
    hipLaunchKernelGGL((gemm_ws_kernel<KT, BM, BN, WM, WN, true, BREG>), grid, block, 0, st, w);
  else
    hipLaunchKernelGGL((gemm_ws_kernel<KT, BM, BN, WM, WN, false, BREG>), grid, block, 0, st, w);
  CN_CHECK_LAUNCH();
  return 0;
}

int device_cus() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return v;
  }();
  return n;
}

int ws_bn(int K) { return K == 512 ? 64 : 128; }

}  // namespace

// Can the weight-stationary kernel run this problem?  (Operand kinds, batch, epilogue and split
// conditions are cn_gemm_dispatch's; here: the shape and the 16-byte row pieces of C.)
bool cn_gemm_ws_supports(const GemmArgs& a) {
  if (a.K != 64 && a.K != 128 && a.K != 256 && a.K != 512) return false;
  if (a.ka_lim < a.K || a.kb_lim < a.K) return false;
  if (a.N % 8 || a.ldc % 8 || (uintptr_t)a.C % 16) return false;
  if (a.lda % 8 || a.ldb % 8 || (uintptr_t)a.A % 16 || (uintptr_t)a.B % 16) return false;
  if (256 * a.ldc * 2 >= 0x80000000ll) return false;   // 32-bit store offsets within a tile
  if (a.st_mode == 4) {   // the fold: ReLU or none, 16-byte pieces of the tables and the residual rows
    if (a.act == 2 || (uintptr_t)a.br_gamma % 16 || (uintptr_t)a.br_beta % 16) return false;
    if (a.br_x && (a.br_ldx % 8 || (uintptr_t)a.br_x % 16)) return false;
  }
  const int cus = device_cus();
  return cus >= 8 && (a.N + ws_bn(a.K) - 1) / ws_bn(a.K) <= cus / 8;
}

// Tiles by measurement (profiles/r07_gemm_ws_classes.txt, cold operands): 8 waves with the B
// fragments in registers; 128-row tiles where the A stage is small (K <= 128) except for the
// K = 64 read-add-store, which ran faster on 64 rows; K = 512 leaves room for a 32 x 64 tile only
// and is slower than the generic kernel (not routed by default).
int cn_gemm_ws_launch(const GemmArgs& a, int walkers_per_xcd, hipStream_t st) {
  const int cus = device_cus();
  switch (a.K) {
    case 64:
      if (a.c_mode == 2) return launch_ws<1, 64, 128, 2, 2, true>(a, cus, walkers_per_xcd, st);
      return launch_ws<1, 128, 128, 4, 2, true>(a, cus, walkers_per_xcd, st);
    case 128: return launch_ws<2, 128, 128, 4, 2, true>(a, cus, walkers_per_xcd, st);
    case 256: return launch_ws<4, 64, 128, 2, 4, true>(a, cus, walkers_per_xcd, st);
    case 512: return launch_ws<8, 32, 64, 2, 2, false>(a, cus, walkers_per_xcd, st);
    default: return CN_ERR_UNSUPPORTED;
  }
}
