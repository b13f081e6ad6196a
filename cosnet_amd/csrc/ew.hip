// Memory-bound kernels of the hot path: layout conversion, weight preparation, pooling,
// gating, decoder head, bilinear upsample + sigmoid, loss, SGD.  All NHWC [P][C] with row
// stride ld; 16-byte vector accesses wherever channels are contiguous.
#include "common.h"
#include "../../include/cosnet_hip.h"

namespace {

template <class T> __device__ __forceinline__ void ldv(const T* p, float* f) {
  Chunk<T>::unpack(*(const u32x4*)p, f);
}
template <class T> __device__ __forceinline__ void stv(T* p, const float* f) {
  *(u32x4*)p = Chunk<T>::pack(f);
}

// ---- input: NCHW fp32 -> NHWC T with channels zero-padded to Cp ------------------------
template <class T>
__global__ void nchw_to_nhwc_k(const float* __restrict__ x, int N, int C, int H, int W, int Cp,
                               T* __restrict__ y) {
  // one pixel per thread: coalesced channel-plane reads, the pixel's Cp (% VEC == 0) channels
  // written as whole 16-byte chunks
  constexpr int V = VecOf<T>::N;
  long long total = (long long)N * H * W;
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < total;
       p += (long long)gridDim.x * blockDim.x) {
    long long n = p / ((long long)H * W), hw = p - n * H * W;
    for (int c0 = 0; c0 < Cp; c0 += V) {
      float f[V];
#pragma unroll
      for (int v = 0; v < V; ++v) f[v] = c0 + v < C ? x[(n * C + c0 + v) * H * W + hw] : 0.f;
      *(u32x4*)(y + p * Cp + c0) = Chunk<T>::pack(f);
    }
  }
}

// ---- weights: fp32 [Cout][KHW][Cin] -> T [Cout][KHW][Cp] and T [Cin][KHW][Cout] ---------
template <class T>
__global__ void weight_prep_k(const float* __restrict__ w, int Cout, int KHW, int Cin, int Cp,
                              T* __restrict__ wf, T* __restrict__ wt) {
  long long total = (long long)Cout * KHW * Cp;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    int ci = (int)(i % Cp);
    long long rest = i / Cp;
    int t = (int)(rest % KHW);
    int co = (int)(rest / KHW);
    float v = ci < Cin ? w[((long long)co * KHW + t) * Cin + ci] : 0.f;
    wf[i] = fromf<T>(v);
    if (wt && ci < Cin) wt[((long long)ci * KHW + t) * Cout + co] = fromf<T>(v);
  }
}

// ---- max pool 3x3 / s2 / p1 / ceil_mode (deeplab/residual_net.py:109) -------------------
template <class T>
__global__ void maxpool_fwd_k(const T* __restrict__ x, int N, int H, int W, int C, int OH, int OW,
                              int k, int s, int pad, T* __restrict__ y, unsigned char* __restrict__ am) {
  constexpr int V = VecOf<T>::N;
  const int CPR = C / V;
  long long total = (long long)N * OH * OW * CPR;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    int cc = (int)(i % CPR);
    long long p = i / CPR;
    int ox = (int)(p % OW);
    long long q = p / OW;
    int oy = (int)(q % OH);
    int n = (int)(q / OH);
    float best[V];
    int bi[V];
#pragma unroll
    for (int v = 0; v < V; ++v) { best[v] = -INFINITY; bi[v] = 0; }
    if (k == 3) {
      // the stem's 3x3 window: all nine 16-byte loads issued before the first compare (taps
      // outside the image are skipped exactly as below: scan order and tie-breaking unchanged)
      u32x4 raw[9];
      bool in[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int yy = oy * s - pad + t / 3, xx = ox * s - pad + t % 3;
        in[t] = yy >= 0 && yy < H && xx >= 0 && xx < W;
        raw[t] = in[t] ? *(const u32x4*)(x + (((long long)n * H + yy) * W + xx) * C + cc * V)
                       : u32x4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        if (!in[t]) continue;
        float f[V];
        Chunk<T>::unpack(raw[t], f);
#pragma unroll
        for (int v = 0; v < V; ++v)
          if (f[v] > best[v] || (f[v] != f[v])) { best[v] = f[v]; bi[v] = t; }
      }
    } else {
      for (int r = 0; r < k; ++r) {
        int yy = oy * s - pad + r;
        if (yy < 0 || yy >= H) continue;
        for (int c = 0; c < k; ++c) {
          int xx = ox * s - pad + c;
          if (xx < 0 || xx >= W) continue;
          float f[V];
          ldv(x + (((long long)n * H + yy) * W + xx) * C + cc * V, f);
#pragma unroll
          for (int v = 0; v < V; ++v)
            if (f[v] > best[v] || (f[v] != f[v])) { best[v] = f[v]; bi[v] = r * k + c; }
        }
      }
    }
    stv(y + p * C + cc * V, best);
    // the V argmax bytes of this chunk in one store (V = 8: 8 B, V = 4: 4 B; C % V == 0)
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int v = 0; v < 4; ++v) lo |= (unsigned)(bi[v] & 0xff) << (8 * v);
    if constexpr (V == 8) {
#pragma unroll
      for (int v = 0; v < 4; ++v) hi |= (unsigned)(bi[4 + v] & 0xff) << (8 * v);
      *(u32x2*)(am + p * C + cc * V) = u32x2{lo, hi};
    } else {
      *(unsigned*)(am + p * C + cc * V) = lo;
    }
  }
}

// gather form: each input pixel sums the outputs whose argmax points at it (deterministic)
template <class T>
__global__ void maxpool_bwd_k(const T* __restrict__ dy, const unsigned char* __restrict__ am,
                              int N, int H, int W, int C, int OH, int OW, int k, int s, int pad,
                              T* __restrict__ dx) {
  constexpr int V = VecOf<T>::N;
  const int CPR = C / V;
  long long total = (long long)N * H * W * CPR;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    int cc = (int)(i % CPR);
    long long p = i / CPR;
    int xx = (int)(p % W);
    long long q = p / W;
    int yy = (int)(q % H);
    int n = (int)(q / H);
    float acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.f;
    // outputs oy with oy*s - pad <= yy <= oy*s - pad + k - 1
    int oy_lo = (yy + pad - (k - 1) + s - 1) / s; if (yy + pad - (k - 1) < 0) oy_lo = 0;
    int oy_hi = (yy + pad) / s; if (oy_hi > OH - 1) oy_hi = OH - 1;
    int ox_lo = (xx + pad - (k - 1) + s - 1) / s; if (xx + pad - (k - 1) < 0) ox_lo = 0;
    int ox_hi = (xx + pad) / s; if (ox_hi > OW - 1) ox_hi = OW - 1;
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
      int r = yy - (oy * s - pad);
      for (int ox = ox_lo; ox <= ox_hi; ++ox) {
        int c = xx - (ox * s - pad);
        int idx = r * k + c;
        long long o = (((long long)n * OH + oy) * OW + ox) * C + cc * V;
        float g[V];
        ldv(dy + o, g);
#pragma unroll
        for (int v = 0; v < V; ++v)
          if (am[o + v] == idx) acc[v] += g[v];
      }
    }
    stv(dx + p * C + cc * V, acc);
  }
}

// ---- global average pool over HW per image: T [N*HW][C] (ld) -> T [N][C] --------------
// grid (ceil(C/V/64), N, RS): block = 64 chunks x 4 row groups; each (row split z) writes its
// fp32 partial to ws [z][N][C]; avgpool_final_k sums the RS partials in a fixed order, so the
// result is deterministic and no zero-fill / atomics are needed (graph-capture friendly).
template <class T>
__global__ __launch_bounds__(256) void avgpool_partial_k(const T* __restrict__ x, long long ld, int HW,
                                                         int C, float* __restrict__ ws) {
  constexpr int V = VecOf<T>::N;
  const int cc = blockIdx.x * 64 + (threadIdx.x & 63);
  const int rg = threadIdx.x >> 6;
  const int n = blockIdx.y;
  const int per = (HW + gridDim.z - 1) / gridDim.z;
  const int r0 = blockIdx.z * per, r1 = min(HW, r0 + per);
  __shared__ float red[4][64][8];
  float acc[V];
#pragma unroll
  for (int v = 0; v < V; ++v) acc[v] = 0.f;
  if (cc * V < C) {
    // 4 rows' loads in flight per thread (rows past the range re-read row r and add +0), added
    // in row order as before: bitwise the same sums
    for (int r = r0 + rg; r < r1; r += 16) {
      float f[4][V];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int rr = r + 4 * u < r1 ? r + 4 * u : r;
        ldv(x + ((long long)n * HW + rr) * ld + cc * V, f[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] += r + 4 * u < r1 ? f[u][v] : 0.f;
    }
  }
#pragma unroll
  for (int v = 0; v < V; ++v) red[rg][threadIdx.x & 63][v] = acc[v];
  __syncthreads();
  if (rg == 0 && cc * V < C) {
    float* dst = ws + ((long long)blockIdx.z * gridDim.y + n) * C + cc * V;
#pragma unroll
    for (int v = 0; v < V; ++v)
      dst[v] = (red[0][threadIdx.x][v] + red[1][threadIdx.x][v]) +
               (red[2][threadIdx.x][v] + red[3][threadIdx.x][v]);
  }
}

template <class T>
__global__ void avgpool_final_k(const float* __restrict__ ws, int rs, long long n, float scale,
                                T* __restrict__ y) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int z = 0; z < rs; ++z) s += ws[(long long)z * n + i];
    y[i] = fromf<T>(s * scale);
  }
}

// broadcast T [N][C] over HW rows into dst (ld); scale applied (1 for fwd, 1/HW for avgpool bwd)
template <class T>
__global__ void bcast_rows_k(const T* __restrict__ src, int N, int HW, int C, float scale,
                             T* __restrict__ dst, long long ld, int accumulate) {
  constexpr int V = VecOf<T>::N;
  const int CPR = C / V;
  long long total = (long long)N * HW * CPR;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    int cc = (int)(i % CPR);
    long long p = i / CPR;
    int n = (int)(p / HW);
    float f[V];
    ldv(src + (long long)n * C + cc * V, f);
#pragma unroll
    for (int v = 0; v < V; ++v) f[v] *= scale;
    if (accumulate) {
      float q[V];
      ldv(dst + p * ld + cc * V, q);
#pragma unroll
      for (int v = 0; v < V; ++v) f[v] += q[v];
    }
    stv(dst + p * ld + cc * V, f);
  }
}

// ---- spatial gate: m = sigmoid(z . g + b); out = z * m  (rgbd_segmentation_RAA.py:177-184)
// one wave per pixel row
template <class T>
__global__ void gate_fwd_k(const T* __restrict__ z, long long ldz, int P, int C,
                           const float* __restrict__ g, const float* __restrict__ gb,
                           T* __restrict__ out, long long ldo, float* __restrict__ mask) {
  constexpr int V = VecOf<T>::N;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= P) return;
  const int CPR = C / V;
  float acc = 0.f;
  for (int cc = lane; cc < CPR; cc += 64) {
    float f[V];
    ldv(z + (long long)row * ldz + cc * V, f);
#pragma unroll
    for (int v = 0; v < V; ++v) acc = fmaf(f[v], g[cc * V + v], acc);
  }
  acc = warp_sum(acc);
  float m = 1.f / (1.f + expf(-(acc + (gb ? gb[0] : 0.f))));
  if (lane == 0 && mask) mask[row] = m;
  for (int cc = lane; cc < CPR; cc += 64) {
    float f[V];
    ldv(z + (long long)row * ldz + cc * V, f);
#pragma unroll
    for (int v = 0; v < V; ++v) f[v] *= m;
    stv(out + (long long)row * ldo + cc * V, f);
  }
}

// ---- gate + concat from a feature bank (rgbd_segmentation_RAA.py:177-186, :228-235): row
// p HW + r of out is [z row * m | bank row iv[p] HW + r], one wave per row, one launch for both
// halves.  A lane keeps its one 16-byte chunk of z in registers between the dot product and the
// scaling (C <= 64 chunks: the all_channel = 256 of every call site), so every element is read
// once and written once; the gate's arithmetic is gate_fwd_k's, in its order.
template <class T>
__global__ void gate_cat_idx_k(const T* __restrict__ z, long long ldz, const T* __restrict__ vbank,
                               long long ldb, const int* __restrict__ iv, int P, int HW, int C,
                               const float* __restrict__ g, const float* __restrict__ gb,
                               T* __restrict__ out, long long ldo) {
  constexpr int V = VecOf<T>::N;
  const int lane = threadIdx.x & 63;
  const long long row = blockIdx.x * 4ll + (threadIdx.x >> 6);
  if (row >= (long long)P * HW) return;
  const int p = (int)(row / HW), r = (int)(row - (long long)p * HW);
  const long long frame = iv ? (long long)iv[p] : p;
  const bool on = lane < C / V;
  float f[V];
  u32x4 vraw;
  float acc = 0.f;
  if (on) {
    vraw = *(const u32x4*)(vbank + (frame * HW + r) * ldb + lane * V);   // pass-through half, raw
    ldv(z + row * ldz + lane * V, f);
#pragma unroll
    for (int v = 0; v < V; ++v) acc = fmaf(f[v], g[lane * V + v], acc);
  }
  acc = warp_sum(acc);
  const float m = 1.f / (1.f + expf(-(acc + (gb ? gb[0] : 0.f))));
  if (on) {
#pragma unroll
    for (int v = 0; v < V; ++v) f[v] *= m;
    stv(out + row * ldo + lane * V, f);
    *(u32x4*)(out + row * ldo + C + lane * V) = vraw;
  }
}

// dz = dout*m + (sum_c dout*z) * m(1-m) * g ;  dg += sum_p (.)*z ; dgb += sum_p (.)
// one wave per row, rows grid-strided; dg / dgb reduced per block before one atomic each.
// ---- deterministic column reductions ------------------------------------------------------
// A 4-wave block whose lane l holds V column sums acc (columns l*V..l*V+V-1) and wave-0 lane 0 a
// scalar accb writes them as ONE row of partials: ws[blockIdx.x][0..C) and
// ws[gridDim.x * C + blockIdx.x] (the scalar); colreduce_k then sums the rows in block order.
// Fixed-order sums: results are bitwise repeatable run to run (no float atomics).
template <int V>
__device__ __forceinline__ void block_partials(const float* acc, float accb, bool on, int C,
                                               float* __restrict__ ws) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ float red[4][64][8];
  __shared__ float redb[4];
#pragma unroll
  for (int v = 0; v < V; ++v) red[wave][lane][v] = acc[v];
  if (lane == 0) redb[wave] = accb;
  __syncthreads();
  if (wave == 0 && on) {
    float* dst = ws + (long long)blockIdx.x * C + lane * V;
#pragma unroll
    for (int v = 0; v < V; ++v)
      dst[v] = (red[0][lane][v] + red[1][lane][v]) + (red[2][lane][v] + red[3][lane][v]);
  }
  if (threadIdx.x == 0)
    ws[(long long)gridDim.x * C + blockIdx.x] = (redb[0] + redb[1]) + (redb[2] + redb[3]);
}

// out[c] = scale * sum_{b < nb} part[b * C + c] / div.  Block = 64 columns x 4 row groups; row
// group w sums rows w, w+4, ... (4 loads in flight per step), then the 4 group sums are added in
// a fixed order: deterministic.  (div: the N-reference mean divides like the reference's
// `output_sum / sample_range`, test.py:305, instead of multiplying by a rounded 1/N.)
__global__ __launch_bounds__(256) void colreduce_k(const float* __restrict__ part, int nb, int C,
                                                   float scale, float div, float* __restrict__ out) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + l;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (c < C) {
    int b = w;
    for (; b + 12 < nb; b += 16) {
      s0 += part[(long long)b * C + c];
      s1 += part[(long long)(b + 4) * C + c];
      s2 += part[(long long)(b + 8) * C + c];
      s3 += part[(long long)(b + 12) * C + c];
    }
    for (; b < nb; b += 4) s0 += part[(long long)b * C + c];
  }
  __shared__ float red[4][64];
  red[w][l] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (w == 0 && c < C) out[c] = ((red[0][l] + red[1][l]) + (red[2][l] + red[3][l])) * scale / div;
}

template <class T>
__global__ __launch_bounds__(256) void gate_bwd_k(const T* __restrict__ z, long long ldz,
                                                  const T* __restrict__ dout, long long lddo,
                                                  const float* __restrict__ mask, int P, int C,
                                                  const float* __restrict__ g, int through_mask,
                                                  T* __restrict__ dz, long long lddz,
                                                  float* __restrict__ ws) {
  constexpr int V = VecOf<T>::N;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int CPR = C / V;  // <= 64 (checked by the launcher)
  const bool on = lane < CPR;
  float gv[V], acc[V];
#pragma unroll
  for (int v = 0; v < V; ++v) { gv[v] = on ? g[lane * V + v] : 0.f; acc[v] = 0.f; }
  float accb = 0.f;
  for (int row = blockIdx.x * 4 + wave; row < P; row += gridDim.x * 4) {
    float f[V], d[V];
    if (on) {
      ldv(z + (long long)row * ldz + lane * V, f);
      ldv(dout + (long long)row * lddo + lane * V, d);
    } else {
#pragma unroll
      for (int v = 0; v < V; ++v) f[v] = d[v] = 0.f;
    }
    float dm = 0.f;
    if (through_mask) {
#pragma unroll
      for (int v = 0; v < V; ++v) dm = fmaf(f[v], d[v], dm);
      dm = warp_sum(dm);
    }
    const float m = mask[row];
    const float dpre = dm * m * (1.f - m);
    accb += dpre;
    if (on) {
      float o[V];
#pragma unroll
      for (int v = 0; v < V; ++v) {
        o[v] = d[v] * m + dpre * gv[v];
        acc[v] = fmaf(dpre, f[v], acc[v]);
      }
      stv(dz + (long long)row * lddz + lane * V, o);
    }
  }
  if (!ws) return;
  block_partials<V>(acc, accb, on, C, ws);
}

// ---- decoder head: zr = relu(a [+ b]) (stored if zout), logit = zr . w + bias ---------------
template <class T>
__global__ void head_fwd_k(const T* __restrict__ a, long long lda, const T* __restrict__ b,
                           long long ldb, int P, int C, int relu, const float* __restrict__ w,
                           const float* __restrict__ bias, T* __restrict__ zout, long long ldz,
                           float* __restrict__ logit) {
  constexpr int V = VecOf<T>::N;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= P) return;
  const int CPR = C / V;
  float acc = 0.f;
  for (int cc = lane; cc < CPR; cc += 64) {
    float f[V];
    ldv(a + (long long)row * lda + cc * V, f);
    if (b) {
      float q[V];
      ldv(b + (long long)row * ldb + cc * V, q);
#pragma unroll
      for (int v = 0; v < V; ++v) f[v] += q[v];
    }
    if (relu) {
#pragma unroll
      for (int v = 0; v < V; ++v) f[v] = fmaxf(f[v], 0.f);
    }
    if (zout) stv(zout + (long long)row * ldz + cc * V, f);
#pragma unroll
    for (int v = 0; v < V; ++v) acc = fmaf(f[v], w[cc * V + v], acc);
  }
  acc = warp_sum(acc);
  if (lane == 0) logit[row] = acc + (bias ? bias[0] : 0.f);
}

template <class T>
__global__ __launch_bounds__(256) void head_bwd_k(const T* __restrict__ z, long long ldz,
                                                  const float* __restrict__ dlogit, int P, int C,
                                                  int relu, const float* __restrict__ w,
                                                  T* __restrict__ dz, long long lddz,
                                                  float* __restrict__ ws) {
  constexpr int V = VecOf<T>::N;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int CPR = C / V;  // <= 64 (checked by the launcher)
  const bool on = lane < CPR;
  float wv[V], acc[V];
#pragma unroll
  for (int v = 0; v < V; ++v) { wv[v] = on ? w[lane * V + v] : 0.f; acc[v] = 0.f; }
  float accb = 0.f;
  for (int row = blockIdx.x * 4 + wave; row < P; row += gridDim.x * 4) {
    const float dl = dlogit[row];
    accb += dl;
    if (!on) continue;
    float f[V], o[V];
    ldv(z + (long long)row * ldz + lane * V, f);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      o[v] = (!relu || f[v] > 0.f) ? dl * wv[v] : 0.f;
      acc[v] = fmaf(dl, f[v], acc[v]);
    }
    if (dz) stv(dz + (long long)row * lddz + lane * V, o);
  }
  if (!ws) return;
  block_partials<V>(acc, accb, on, C, ws);
}

// ---- bilinear upsample (align_corners=False, torch semantics) + sigmoid ----------------
__device__ __forceinline__ void src_index(int dst, int in, int out, float scale, int& i0, int& i1,
                                          float& l1) {
  float s = scale * ((float)dst + 0.5f) - 0.5f;
  if (s < 0.f) s = 0.f;
  i0 = (int)s;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = s - (float)i0;
}

__global__ void upsample_sigmoid_k(const float* __restrict__ in, int N, int h, int w, int H, int W,
                                   float sh, float sw, int apply_sigmoid, float* __restrict__ out) {
  long long total = (long long)N * H * W;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    int X = (int)(i % W);
    long long q = i / W;
    int Y = (int)(q % H);
    int n = (int)(q / H);
    int y0, y1, x0, x1;
    float ly, lx;
    src_index(Y, h, H, sh, y0, y1, ly);
    src_index(X, w, W, sw, x0, x1, lx);
    const float* b = in + (long long)n * h * w;
    float v = (1.f - ly) * ((1.f - lx) * b[y0 * w + x0] + lx * b[y0 * w + x1]) +
              ly * ((1.f - lx) * b[y1 * w + x0] + lx * b[y1 * w + x1]);
    out[i] = apply_sigmoid ? 1.f / (1.f + expf(-v)) : v;
  }
}

// d in[n,y,x] = sum over output pixels of dout * s(1-s) * wy * wx (gather; deterministic).
// One wave per input pixel: its lanes stride the (Y, X) window of output pixels whose source
// interval touches it (~17 x 17 at 60 -> 473), then a fixed xor-shuffle tree adds the lanes.
__global__ __launch_bounds__(256) void upsample_sigmoid_bwd_k(const float* __restrict__ dout,
                                                             const float* __restrict__ out, int N,
                                                             int h, int w, int H, int W, float sh,
                                                             float sw, int apply_sigmoid,
                                                             float* __restrict__ din) {
  const int lane = threadIdx.x & 63;
  long long total = (long long)N * h * w;
  for (long long i = blockIdx.x * 4ll + (threadIdx.x >> 6); i < total; i += gridDim.x * 4ll) {
    int x = (int)(i % w);
    long long q = i / w;
    int y = (int)(q % h);
    int n = (int)(q / h);
    // output rows Y whose source interval touches y: src(Y) in (y-1, y+1)
    int Ylo = (int)floorf(((float)y - 1.f + 0.5f) / sh - 0.5f) - 1;
    int Yhi = (int)ceilf(((float)y + 1.f + 0.5f) / sh - 0.5f) + 1;
    int Xlo = (int)floorf(((float)x - 1.f + 0.5f) / sw - 0.5f) - 1;
    int Xhi = (int)ceilf(((float)x + 1.f + 0.5f) / sw - 0.5f) + 1;
    if (Ylo < 0) Ylo = 0;
    if (Xlo < 0) Xlo = 0;
    if (Yhi > H - 1) Yhi = H - 1;
    if (Xhi > W - 1) Xhi = W - 1;
    const int nX = Xhi - Xlo + 1, nk = (Yhi - Ylo + 1) * nX;
    float acc = 0.f;
    for (int k = lane; k < nk; k += 64) {
      const int Y = Ylo + k / nX, X = Xlo + k % nX;
      int y0, y1, x0, x1;
      float ly, lx;
      src_index(Y, h, H, sh, y0, y1, ly);
      src_index(X, w, W, sw, x0, x1, lx);
      const float wy = (y0 == y ? 1.f - ly : 0.f) + (y1 == y ? ly : 0.f);
      const float wx = (x0 == x ? 1.f - lx : 0.f) + (x1 == x ? lx : 0.f);
      if (wy == 0.f || wx == 0.f) continue;
      const long long o = ((long long)n * H + Y) * W + X;
      float g = dout[o];
      if (apply_sigmoid) { float s = out[o]; g *= s * (1.f - s); }
      acc = fmaf(g, wy * wx, acc);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) din[i] = acc;
  }
}

// ---- loss: r*BCE + 0.8*L1 (train.py:176-216), gradient fused --------------------------
__global__ void zero_u64_k(unsigned long long* p, long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    p[i] = 0ull;
}

// #(gt >= thr): per-thread counts, a block reduction, ONE integer atomic per block (a few
// hundred blocks: same-address atomics serialise, so one per wave would dominate)
__global__ __launch_bounds__(256) void count_ge_k(const float* __restrict__ gt, long long n, float thr,
                                                 unsigned long long* cnt) {
  unsigned c = 0;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    c += gt[i] >= thr ? 1u : 0u;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  __shared__ unsigned wsum[4];
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long t = (unsigned long long)wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (t) atomicAdd(cnt, t);
  }
}

// partial[block] = sum of per-element loss; dpred = d loss / d pred (already / n, * gscale)
__global__ void bce_l1_k(const float* __restrict__ p, const float* __restrict__ y, long long n,
                         float weight, float l1w, float* __restrict__ partial,
                         float* __restrict__ dpred, const long long* __restrict__ pos_cnt,
                         double total) {
  if (pos_cnt) {  // weight = N*H*W / #(gt >= 0.5) from a device-side count (no host sync)
    long long c = *pos_cnt;
    weight = c > 0 ? (float)(total / (double)c) : 1.f;
  }
  float acc = 0.f;
  const float invn = 1.f / (float)n;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    float pv = p[i], yv = y[i];
    float lp = fmaxf(logf(pv), -100.f), l1p = fmaxf(logf(1.f - pv), -100.f);
    float bce = -weight * (yv * lp + (1.f - yv) * l1p);
    float d = pv - yv;
    acc += bce + l1w * fabsf(d);
    if (dpred) {
      float gb = weight * d / fmaxf((1.f - pv) * pv, 1e-12f);
      float gl = l1w * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
      dpred[i] = (gb + gl) * invn;
    }
  }
  acc = warp_sum(acc);
  __shared__ float s[4];
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}

__global__ void sum_partials_k(const float* __restrict__ partial, int n, float scale, float* out) {
  double a = 0;
  for (int i = threadIdx.x; i < n; i += 64) a += partial[i];
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if (threadIdx.x == 0) out[0] = (float)(a * scale);
}

// ---- SGD (torch.optim.SGD semantics: d = g + wd*p; buf = mom*buf + d (buf = d first);
//      p -= lr * buf), multi-tensor, fused with the refresh of the compute-dtype weight copies
//      the GEMMs read (wf [Cout][KHW][Cp], wt [Cin][KHW][Cout]) -------------------------------
// One record = one work item of one parameter: a flat element range (mode 0) or a range of
// 64x64 (co, ci) tiles of one tap (mode 1: coalesced fp32 reads/writes along ci, the new
// weights staged through LDS so the transposed copy is written coalesced along co).
struct SgdTensor {
  float* p;
  const float* g;
  float* buf;
  long long n;
  int group;
  int first;
  void* wf;
  void* wt;
  int cout, khw, cin, cp;
  int wdt;   // 0: no copy, 1: bf16 copies, 2: fp32 copies
  int mode;  // 0: elements [beg, end); 1: tiles [beg, end)
  long long beg, end;
};
static_assert(sizeof(SgdTensor) == 96, "SgdTensor layout is shared with cosnet_amd/optim.py");

__device__ __forceinline__ float sgd_upd(float& p, float g, float& b, float lr, float wd, float mom,
                                         int first) {
  float d = g + wd * p;
  b = first ? d : fmaf(mom, b, d);
  p -= lr * b;
  return p;
}

__device__ __forceinline__ void put_w(void* base, long long idx, float v, int wdt) {
  if (wdt == 1) ((bf16*)base)[idx] = (bf16)v;
  else ((float*)base)[idx] = v;
}

__global__ __launch_bounds__(256) void sgd_k(const SgdTensor* __restrict__ ts, int nt,
                                             const float* __restrict__ lrs, float wd, float mom) {
  __shared__ float tile[64][65];
  const int tid = threadIdx.x;
  for (int t = blockIdx.x; t < nt; t += gridDim.x) {
    const SgdTensor T = ts[t];
    if (!T.g) continue;
    const float lr = lrs[T.group];
    if (T.mode == 0) {
      if (T.wdt == 0 && (T.beg & 3) == 0 && ((T.end - T.beg) & 3) == 0 &&
          ((uintptr_t)T.p & 15) == 0 && ((uintptr_t)T.g & 15) == 0 && ((uintptr_t)T.buf & 15) == 0) {
        for (long long i = T.beg + 4 * tid; i < T.end; i += 4 * 256) {
          f32x4 p = *(const f32x4*)(T.p + i), g = *(const f32x4*)(T.g + i);
          f32x4 b = T.first ? (f32x4){0.f, 0.f, 0.f, 0.f} : *(const f32x4*)(T.buf + i);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float pe = p[e], be = b[e];
            sgd_upd(pe, g[e], be, lr, wd, mom, T.first);
            p[e] = pe;
            b[e] = be;
          }
          *(f32x4*)(T.p + i) = p;
          *(f32x4*)(T.buf + i) = b;
        }
      } else {
        for (long long i = T.beg + tid; i < T.end; i += 256) {
          float p = T.p[i], b = T.first ? 0.f : T.buf[i];
          float v = sgd_upd(p, T.g[i], b, lr, wd, mom, T.first);
          T.p[i] = p;
          T.buf[i] = b;
          if (T.wdt) {
            int ci = (int)(i % T.cin);
            long long r = i / T.cin;
            int tap = (int)(r % T.khw), co = (int)(r / T.khw);
            put_w(T.wf, ((long long)co * T.khw + tap) * T.cp + ci, v, T.wdt);
            if (T.wt) put_w(T.wt, ((long long)ci * T.khw + tap) * T.cout + co, v, T.wdt);
          }
        }
      }
      continue;
    }
    // mode 1: cin % 4 == 0
    const int ncob = (T.cout + 63) >> 6, ncib = (T.cin + 63) >> 6;
    for (long long tl = T.beg; tl < T.end; ++tl) {
      const int cib = (int)(tl % ncib);
      const long long r0 = tl / ncib;
      const int cob = (int)(r0 % ncob), tap = (int)(r0 / ncob);
      const int co0 = cob * 64, ci0 = cib * 64;
      const int rr = tid >> 4, c4 = (tid & 15) * 4;
      const int ci = ci0 + c4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int co = co0 + rr + 16 * j;
        if (co < T.cout && ci < T.cin) {
          const long long idx = ((long long)co * T.khw + tap) * T.cin + ci;
          f32x4 p = *(const f32x4*)(T.p + idx), g = *(const f32x4*)(T.g + idx);
          f32x4 b = T.first ? (f32x4){0.f, 0.f, 0.f, 0.f} : *(const f32x4*)(T.buf + idx);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float pe = p[e], be = b[e];
            sgd_upd(pe, g[e], be, lr, wd, mom, T.first);
            p[e] = pe;
            b[e] = be;
          }
          *(f32x4*)(T.p + idx) = p;
          *(f32x4*)(T.buf + idx) = b;
          const long long fo = ((long long)co * T.khw + tap) * T.cp + ci;
          if (T.wdt == 1) {
            bf16* w = (bf16*)T.wf + fo;
            w[0] = (bf16)p[0]; w[1] = (bf16)p[1]; w[2] = (bf16)p[2]; w[3] = (bf16)p[3];
          } else {
            float* w = (float*)T.wf + fo;
            w[0] = p[0]; w[1] = p[1]; w[2] = p[2]; w[3] = p[3];
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) tile[rr + 16 * j][c4 + e] = p[e];
        }
      }
      if (T.wt) {
        __syncthreads();
        // wt rows ci (64 per tile), 16 consecutive co per thread
        const int cil = tid >> 2, seg = (tid & 3) * 16;
        const int cw = ci0 + cil;
        if (cw < T.cin) {
          const long long ro = ((long long)cw * T.khw + tap) * T.cout;
          if (T.wdt == 1 && (T.cout & 7) == 0 && co0 + seg + 16 <= T.cout) {
            float v[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) v[e] = tile[seg + e][cil];
            u32x4* dst = (u32x4*)((bf16*)T.wt + ro + co0 + seg);
            dst[0] = Chunk<bf16>::pack(v);
            dst[1] = Chunk<bf16>::pack(v + 8);
          } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const int co = co0 + seg + e;
              if (co < T.cout) put_w(T.wt, ro + co, tile[seg + e][cil], T.wdt);
            }
          }
        }
        __syncthreads();
      }
    }
  }
}

// ---- generic helpers ------------------------------------------------------------------
template <class T>
__global__ void rowdot_k(const T* __restrict__ a, long long lda, const T* __restrict__ b,
                         long long ldb, int P, int C, int seg, int seg_ld, float* __restrict__ out) {
  constexpr int V = VecOf<T>::N;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= P) return;
  float acc = 0.f;
  for (int cc = lane; cc < C / V; cc += 64) {
    float f[V], q[V];
    ldv(a + (long long)row * lda + cc * V, f);
    ldv(b + (long long)row * ldb + cc * V, q);
#pragma unroll
    for (int v = 0; v < V; ++v) acc = fmaf(f[v], q[v], acc);
  }
  acc = warp_sum(acc);
  if (lane == 0) out[(long long)(row / seg) * seg_ld + row % seg] = acc;
}

// column sums of T [P][C] (ld) into fp32 [C] (atomic across row blocks)
template <class T>
__global__ void colsum_k(const T* __restrict__ x, long long ld, int P, int C, float* __restrict__ part) {
  // grid (ceil(C/V/64), gy): block (x, y) sums rows y*4+rg, y*4+rg + 4*gy, ... of its columns
  // into part[y][C] (fixed order; colreduce_k adds the gy rows)
  constexpr int V = VecOf<T>::N;
  int cc = blockIdx.x * 64 + (threadIdx.x & 63);
  int rg = threadIdx.x >> 6;
  float acc[V];
#pragma unroll
  for (int v = 0; v < V; ++v) acc[v] = 0.f;
  if (cc * V < C) {
    // 4 rows' loads in flight per thread (rows past P re-read row r and add +0), added in row
    // order as before: bitwise the same sums
    const int st = gridDim.y * 4;
    for (int r = blockIdx.y * 4 + rg; r < P; r += 4 * st) {
      float f[4][V];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int rr = r + u * st < P ? r + u * st : r;
        ldv(x + (long long)rr * ld + cc * V, f[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] += r + u * st < P ? f[u][v] : 0.f;
    }
  }
  __shared__ float red[4][64][8];
#pragma unroll
  for (int v = 0; v < V; ++v) red[rg][threadIdx.x & 63][v] = acc[v];
  __syncthreads();
  if (rg == 0 && cc * V < C) {
    float* dst = part + (long long)blockIdx.y * C + cc * V;
#pragma unroll
    for (int v = 0; v < V; ++v)
      dst[v] = (red[0][threadIdx.x][v] + red[1][threadIdx.x][v]) +
               (red[2][threadIdx.x][v] + red[3][threadIdx.x][v]);
  }
}

template <class TI, class TO>
__global__ void cast2d_k(const TI* __restrict__ x, long long ldx, int P, int C, TO* __restrict__ y,
                         long long ldy, int accumulate) {
  long long total = (long long)P * C;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    long long r = i / C;
    int c = (int)(i - r * C);
    float v = tof(x[r * ldx + c]);
    if (accumulate) v += tof(y[r * ldy + c]);
    y[r * ldy + c] = fromf<TO>(v);
  }
}

inline int nblocks(long long n, int per = 256) {
  long long b = (n + per - 1) / per;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace

extern "C" int cn_nchw_to_nhwc(int dtype, const float* x, int N, int C, int H, int W, int Cp,
                               void* y, hipStream_t st) {
  return with_dtype(dtype, [&](auto tag) {
    using T = tag_t<decltype(tag)>;
    if (Cp % VecOf<T>::N || misaligned(y)) return CN_ERR_ALIGN;
    long long n = (long long)N * H * W;
    hipLaunchKernelGGL(nchw_to_nhwc_k<T>, dim3(nblocks(n)), dim3(256), 0, st, x, N, C, H, W, Cp, (T*)y);
    CN_CHECK_LAUNCH();
    return 0;
  });
}

extern "C" int cn_weight_prep(int dtype, const float* w, int Cout, int KHW, int Cin, int Cp,
                              void* wf, void* wt, hipStream_t st) {
  return with_dtype(dtype, [&](auto tag) {
    using T = tag_t<decltype(tag)>;
    long long n = (long long)Cout * KHW * Cp;
    hipLaunchKernelGGL(weight_prep_k<T>, dim3(nblocks(n)), dim3(256), 0, st, w, Cout, KHW, Cin, Cp, (T*)wf, (T*)wt);
    CN_CHECK_LAUNCH();
    return 0;
  });
}

extern "C" int cn_maxpool_fwd(int dtype, const void* x, int N, int H, int W, int C, int OH, int OW,
                              int k, int s, int pad, void* y, unsigned char* argmax, hipStream_t st) {
  return with_dtype(dtype, [&](auto tag) {
    using T = tag_t<decltype(tag)>;
    if (C % VecOf<T>::N) return CN_ERR_ALIGN;
    long long n = (long long)N * OH * OW * (C / VecOf<T>::N);
    hipLaunchKernelGGL(maxpool_fwd_k<T>, dim3(nblocks(n)), dim3(256), 0, st, (const T*)x, N, H, W, C, OH, OW, k, s, pad, (T*)y, argmax);
    CN_CHECK_LAUNCH();
    return 0;
  });
}

extern "C" int cn_maxpool_bwd(int dtype, const void* dy, const unsigned char* argmax, int N, int H,
                              int W, int C, int OH, int OW, int k, int s, int pad, void* dx,
                              hipStream_t st) {
  return with_dtype(dtype, [&](auto tag) {
    using T = tag_t<decltype(tag)>;
    if (C % VecOf<T>::N) return CN_ERR_ALIGN;
    long long n = (long long)N * H * W * (C / VecOf<T>::N);
    hipLaunchKernelGGL(maxpool_bwd_k<T>, dim3(nblocks(n)), dim3(256), 0, st, (const T*)dy, argmax, N, H, W, C, OH, OW, k, s, pad, (T*)dx);
    CN_CHECK_LAUNCH();
    return 0;
  });
}

static int avgpool_splits(int N, int HW, int C, int V) {
  int gx = (C / V + 63) / 64;
  int rs = (HW + 255) / 256;
  if (rs * gx * N > 1024) rs = 1024 / (gx * N);
  return rs < 1 ? 1 : rs;
}

extern "C" size_t cn_avgpool_workspace_floats(int dtype, int N, int HW, int C) {
  return (size_t)avgpool_splits(N, HW, C, vec_of(dtype)) * N * C;
}

extern "C" int cn_avgpool(int dtype, const void* x, long long ld, int N, int HW, int C,
                          float scale, void* y, float* ws, hipStream_t st) {
  return with_dtype(dtype, [&](auto tag) {
    using T = tag_t<decltype(tag)>;
    constexpr int V = VecOf<T>::N;
    if (C % V) return CN_ERR_ALIGN;
    int gx = (C / V + 63) / 64;
    int rs = avgpool_splits(N, HW, C, V);
    hipLaunchKernelGGL(avgpool_partial_k<T>, dim3(gx, N, rs), dim3(256), 0, st, (const T*)x, ld, HW, C, ws);
    CN_CHECK_LAUNCH();
    long long n = (long long)N * C;
    hipLaunchKernelGGL(avgpool_final_k<T>, dim3(nblocks(n)), dim3(256), 0, st, ws, rs, n, scale, (T*)y);
    CN_CHECK_LAUNCH();
    return 0;
  });
}

extern "C" int cn_bcast_rows(int dtype, const void* src, int N, int HW, int C, float scale,
                             void* dst, long long ld, int accumulate, hipStream_t st) {
  return with_dtype(dtype, [&](auto tag) {
    using T = tag_t<decltype(tag)>;
    if (C % VecOf<T>::N) return CN_ERR_ALIGN;
    long long n = (long long)N * HW * (C / VecOf<T>::N);
    hipLaunchKernelGGL(bcast_rows_k<T>, dim3(nblocks(n)), dim3(256), 0, st, (const T*)src, N, HW, C, scale, (T*)dst, ld, accumulate);
    CN_CHECK_LAUNCH();
    return 0;
  });
}

extern "C" int cn_gate_fwd(int dtype, const void* z, long long ldz, int P, int C, const float* g,
                           const float* gb, void* out, long long ldo, float* mask, hipStream_t st) {
  return with_dtype(dtype, [&](auto tag) {
    using T = tag_t<decltype(tag)>;
    if (C % VecOf<T>::N) return CN_ERR_ALIGN;
    hipLaunchKernelGGL(gate_fwd_k<T>, dim3((P + 3) / 4), dim3(256), 0, st, (const T*)z, ldz, P, C, g, gb, (T*)out, ldo, mask);
    CN_CHECK_LAUNCH();
    return 0;
  });
}

extern "C" int cn_gate_cat_idx(int dtype, const void* z, long long ldz, const void* vbank,
                               long long ldv, const int* iv, int P, int HW, int C, const float* g,
                               const float* gb, void* out, long long ldo, hipStream_t st) {
  return with_dtype(dtype, [&](auto tag) {
    using T = tag_t<decltype(tag)>;
    constexpr int V = VecOf<T>::N;
    if (P <= 0 || HW <= 0 || C <= 0 || ldz < C || ldv < C || ldo < 2 * C) return CN_ERR_SHAPE;
    if (C % V || ldz % V || ldv % V || ldo % V) return CN_ERR_ALIGN;
    if (misaligned(z) || misaligned(vbank) || misaligned(out) || misaligned(iv, 4)) return CN_ERR_ALIGN;
    if (C / V > 64) return CN_ERR_UNSUPPORTED;   // one chunk per lane
    const long long rows = (long long)P * HW;
    if (rows > 0x7fffffffll) return CN_ERR_SHAPE;
    const dim3 grid((unsigned)((rows + 3) / 4));
    hipLaunchKernelGGL(gate_cat_idx_k<T>, grid, dim3(256), 0, st, (const T*)z, ldz, (const T*)vbank, ldv, iv, P, HW, C, g, gb, (T*)out, ldo);
    CN_CHECK_LAUNCH();
    return 0;
  });
}

// Column-partial workspace of cn_gate_bwd / cn_head_bwd / cn_colsum: [nb][C] row-block partials of
// the column sums, then [nb] partials of the scalar sum (gate / head backward only).
struct ColPart { int nb; float *cols, *scalar; size_t floats; };
static ColPart colpart_layout(int P, int C, float* ws) {
  const int nb = nblocks(P, 4 * 16);
  return {nb, ws, ws + (long long)nb * C, (size_t)nb * (size_t)(C + 1)};
}

extern "C" size_t cn_colpart_workspace_floats(int P, int C) {
  return colpart_layout(P, C, nullptr).floats;
}

static int colreduce(const float* ws, int nb, int C, float* out, hipStream_t st) {
  if (!out) return 0;
  hipLaunchKernelGGL(colreduce_k, dim3((C + 63) / 64), dim3(256), 0, st, ws, nb, C, 1.f, 1.f, out);
  CN_CHECK_LAUNCH();
  return 0;
}

// out[c] = (((x[0][c] + x[1][c]) + x[2][c]) + ...) / nrows: the reference's running fp32 sum
// `output_sum += output` over the references followed by `/ sample_range` (test.py:301-305),
// in the same order, so the mean is bit-identical given identical per-reference outputs.
__global__ void mean_rows_seq_k(const float* __restrict__ x, int nrows, int C, float* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s = x[c];
  for (int r = 1; r < nrows; ++r) s += x[(long long)r * C + c];
  out[c] = s / (float)nrows;
}

extern "C" int cn_mean_rows(const float* x, int nrows, int C, float* out, hipStream_t st) {
  if (nrows < 1 || C < 1) return CN_ERR_SHAPE;
  hipLaunchKernelGGL(mean_rows_seq_k, dim3((C + 255) / 256), dim3(256), 0, st, x, nrows, C, out);
  CN_CHECK_LAUNCH();
  return 0;
}

// out[g][c] = mean_rows_seq_k of rows g n .. g n + n - 1: one launch for every target of a sequence
// (test.py:301-305 per target), the same running sum and division, so bitwise cn_mean_rows per group.
__global__ void mean_groups_seq_k(const float* __restrict__ x, int n, int C, float* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float* xg = x + (long long)blockIdx.y * n * C;
  float s = xg[c];
  for (int r = 1; r < n; ++r) s += xg[(long long)r * C + c];
  out[(long long)blockIdx.y * C + c] = s / (float)n;
}

extern "C" int cn_mean_groups(const float* x, int ngroups, int n, int C, float* out, hipStream_t st) {
  if (ngroups < 1 || ngroups > 65535 || n < 1 || C < 1) return CN_ERR_SHAPE;
  hipLaunchKernelGGL(mean_groups_seq_k, dim3((C + 255) / 256, ngroups), dim3(256), 0, st, x, n, C, out);
  CN_CHECK_LAUNCH();
  return 0;
}

extern "C" int cn_sum_rows(const float* x, int nrows, int C, float* out, hipStream_t st) {
  if (nrows < 1 || C < 1) return CN_ERR_SHAPE;
  hipLaunchKernelGGL(colreduce_k, dim3((C + 63) / 64), dim3(256), 0, st, x, nrows, C, 1.f, 1.f, out);
  CN_CHECK_LAUNCH();
  return 0;
}

// out[i] = x[i] * s[0] (+ second tensor): the chain-rule scaling of a loss gradient by the
// incoming device scalar, without a host read of it.
__global__ void scale_dev_k(const float* __restrict__ x, long long n, const float* __restrict__ s,
                            float* __restrict__ out) {
  const float f = *s;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    out[i] = x[i] * f;
}

__global__ void scale_k(float* __restrict__ x, long long n, float s) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    x[i] *= s;
}

extern "C" int cn_scale(float* x, long long n, float s, hipStream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(scale_k, dim3(nblocks(n)), dim3(256), 0, st, x, n, s);
  CN_CHECK_LAUNCH();
  return 0;
}

extern "C" int cn_scale_dev(const float* x, long long n, const float* s, float* out, hipStream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(scale_dev_k, dim3(nblocks(n)), dim3(256), 0, st, x, n, s, out);
  CN_CHECK_LAUNCH();
  return 0;
}

extern "C" int cn_gate_bwd(int dtype, const void* z, long long ldz, const void* dout, long long lddo,
                           const float* mask, int P, int C, const float* g, int through_mask,
                           void* dz, long long lddz, float* dg, float* dgb, float* ws,
                           hipStream_t st) {
  return with_dtype(dtype, [&](auto tag) {
    using T = tag_t<decltype(tag)>;
    constexpr int V = VecOf<T>::N;
    if (C % V) return CN_ERR_ALIGN;
    if (C / V > 64) return CN_ERR_UNSUPPORTED;
    if ((dg || dgb) && !ws) return CN_ERR_SHAPE;
    const ColPart l = colpart_layout(P, C, ws);
    float* w = (dg || dgb) ? l.cols : nullptr;
    hipLaunchKernelGGL(gate_bwd_k<T>, dim3(l.nb), dim3(256), 0, st, (const T*)z, ldz, (const T*)dout, lddo, mask, P, C, g, through_mask, (T*)dz, lddz, w);
    CN_CHECK_LAUNCH();
    if (!w) return 0;
    int rc = colreduce(l.cols, l.nb, C, dg, st);
    if (rc) return rc;
    return colreduce(l.scalar, l.nb, 1, dgb, st);
  });
}

extern "C" int cn_head_fwd(int dtype, const void* a, long long lda, const void* b, long long ldb,
                           int P, int C, int relu, const float* w, const float* bias, void* zout,
                           long long ldz, float* logit, hipStream_t st) {
  return with_dtype(dtype, [&](auto tag) {
    using T = tag_t<decltype(tag)>;
    if (C % VecOf<T>::N) return CN_ERR_ALIGN;
    hipLaunchKernelGGL(head_fwd_k<T>, dim3((P + 3) / 4), dim3(256), 0, st, (const T*)a, lda, (const T*)b, ldb, P, C, relu, w, bias, (T*)zout, ldz, logit);
    CN_CHECK_LAUNCH();
    return 0;
  });
}

extern "C" int cn_head_bwd(int dtype, const void* z, long long ldz, const float* dlogit, int P, int C,
                           int relu, const float* w, void* dz, long long lddz, float* dw, float* db,
                           float* ws, hipStream_t st) {
  return with_dtype(dtype, [&](auto tag) {
    using T = tag_t<decltype(tag)>;
    constexpr int V = VecOf<T>::N;
    if (C % V) return CN_ERR_ALIGN;
    if (C / V > 64) return CN_ERR_UNSUPPORTED;
    if ((dw || db) && !ws) return CN_ERR_SHAPE;
    const ColPart l = colpart_layout(P, C, ws);
    float* wp = (dw || db) ? l.cols : nullptr;
    hipLaunchKernelGGL(head_bwd_k<T>, dim3(l.nb), dim3(256), 0, st, (const T*)z, ldz, dlogit, P, C, relu, w, (T*)dz, lddz, wp);
    CN_CHECK_LAUNCH();
    if (!wp) return 0;
    int rc = colreduce(l.cols, l.nb, C, dw, st);
    if (rc) return rc;
    return colreduce(l.scalar, l.nb, 1, db, st);
  });
}

extern "C" int cn_upsample_sigmoid(const float* in, int N, int h, int w, int H, int W,
                                   int apply_sigmoid, float* out, hipStream_t st) {
  float sh = (float)h / (float)H, sw = (float)w / (float)W;
  long long n = (long long)N * H * W;
  hipLaunchKernelGGL(upsample_sigmoid_k, dim3(nblocks(n)), dim3(256), 0, st, in, N, h, w, H, W, sh, sw, apply_sigmoid, out);
  CN_CHECK_LAUNCH();
  return 0;
}

extern "C" int cn_upsample_sigmoid_bwd(const float* dout, const float* out, int N, int h, int w,
                                       int H, int W, int apply_sigmoid, float* din, hipStream_t st) {
  float sh = (float)h / (float)H, sw = (float)w / (float)W;
  long long n = (long long)N * h * w;
  hipLaunchKernelGGL(upsample_sigmoid_bwd_k, dim3(nblocks(n, 4)), dim3(256), 0, st, dout, out, N, h, w, H, W, sh, sw, apply_sigmoid, din);
  CN_CHECK_LAUNCH();
  return 0;
}

extern "C" int cn_count_ge(const float* gt, long long n, float thr, unsigned long long* cnt, hipStream_t st) {
  hipLaunchKernelGGL(zero_u64_k, dim3(1), dim3(64), 0, st, cnt, 1ll);
  CN_CHECK_LAUNCH();
  hipLaunchKernelGGL(count_ge_k, dim3(nblocks(n, 256 * 16) < 256 ? nblocks(n, 256 * 16) : 256), dim3(256), 0, st, gt, n, thr, cnt);
  CN_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t cn_loss_workspace_floats(long long n) { return (size_t)nblocks(n, 1024); }

extern "C" int cn_bce_l1(const float* pred, const float* gt, long long n, float weight, float l1w,
                         float* ws, float* loss, float* dpred, hipStream_t st) {
  int nb = nblocks(n, 1024);
  hipLaunchKernelGGL(bce_l1_k, dim3(nb), dim3(256), 0, st, pred, gt, n, weight, l1w, ws, dpred,
                     (const long long*)nullptr, 0.0);
  CN_CHECK_LAUNCH();
  hipLaunchKernelGGL(sum_partials_k, dim3(1), dim3(64), 0, st, ws, nb, 1.0f / (float)n, loss);
  CN_CHECK_LAUNCH();
  return 0;
}

extern "C" int cn_bce_l1_devcount(const float* pred, const float* gt, long long n,
                                  const long long* pos_count, double total, float l1w, float* ws,
                                  float* loss, float* dpred, hipStream_t st) {
  int nb = nblocks(n, 1024);
  hipLaunchKernelGGL(bce_l1_k, dim3(nb), dim3(256), 0, st, pred, gt, n, 1.f, l1w, ws, dpred,
                     pos_count, total);
  CN_CHECK_LAUNCH();
  hipLaunchKernelGGL(sum_partials_k, dim3(1), dim3(64), 0, st, ws, nb, 1.0f / (float)n, loss);
  CN_CHECK_LAUNCH();
  return 0;
}

extern "C" int cn_sgd(const void* tensors, int nt, const float* lrs, float wd, float momentum,
                      hipStream_t st) {
  if (nt <= 0) return 0;
  dim3 grid(nt < 8192 ? nt : 8192);
  hipLaunchKernelGGL(sgd_k, grid, dim3(256), 0, st, (const SgdTensor*)tensors, nt, lrs, wd, momentum);
  CN_CHECK_LAUNCH();
  return 0;
}

extern "C" int cn_rowdot_seg(int dtype, const void* a, long long lda, const void* b, long long ldb,
                             int P, int C, int seg, int seg_ld, float* out, hipStream_t st) {
  return with_dtype(dtype, [&](auto tag) {
    using T = tag_t<decltype(tag)>;
    if (C % VecOf<T>::N) return CN_ERR_ALIGN;
    if (seg < 1 || seg_ld < seg) return CN_ERR_SHAPE;
    hipLaunchKernelGGL(rowdot_k<T>, dim3((P + 3) / 4), dim3(256), 0, st, (const T*)a, lda, (const T*)b, ldb, P, C, seg, seg_ld, out);
    CN_CHECK_LAUNCH();
    return 0;
  });
}

extern "C" int cn_rowdot(int dtype, const void* a, long long lda, const void* b, long long ldb,
                         int P, int C, float* out, hipStream_t st) {
  return cn_rowdot_seg(dtype, a, lda, b, ldb, P, C, P > 0 ? P : 1, P > 0 ? P : 1, out, st);
}

extern "C" int cn_colsum(int dtype, const void* x, long long ld, int P, int C, float* out, float* ws,
                         hipStream_t st) {
  return with_dtype(dtype, [&](auto tag) {
    using T = tag_t<decltype(tag)>;
    constexpr int V = VecOf<T>::N;
    if (C % V) return CN_ERR_ALIGN;
    const ColPart l = colpart_layout(P, C, ws);
    int gx = (C / V + 63) / 64;
    int gy = (P + 63) / 64;
    if (gy > 256) gy = 256;
    if (gy > l.nb) gy = l.nb;  // the partial rows fit the layout's [nb][C]
    hipLaunchKernelGGL(colsum_k<T>, dim3(gx, gy), dim3(256), 0, st, (const T*)x, ld, P, C, l.cols);
    CN_CHECK_LAUNCH();
    return colreduce(l.cols, gy, C, out, st);
  });
}

extern "C" int cn_cast2d(int dtype_in, int dtype_out, const void* x, long long ldx, int P, int C,
                         void* y, long long ldy, int accumulate, hipStream_t st) {
  return with_dtype(dtype_in, [&](auto tin) {
    return with_dtype(dtype_out, [&](auto tout) {
      using TI = tag_t<decltype(tin)>;
      using TO = tag_t<decltype(tout)>;
      int nb = nblocks((long long)P * C);
      hipLaunchKernelGGL((cast2d_k<TI, TO>), dim3(nb), dim3(256), 0, st, (const TI*)x, ldx, P, C, (TO*)y, ldy, accumulate);
      CN_CHECK_LAUNCH();
      return 0;
    });
  });
}
