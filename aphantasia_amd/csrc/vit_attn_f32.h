// fp32 multi-head attention of the EXACT ViT path (head dim 64, T <= 256 tokens), forward and input-gradient backward.
//
// qkv [S*T, 3D] f32 (q | k | v, head h at columns h*64), att / datt [S*T, D] f32, dqkv [S*T, 3D] f32, lse [S*heads*T] f32 =
// log-sum-exp of the scaled scores (the f16 kernels' convention), delta [S*heads*T] f32 scratch of the backward.
// Plain fp32 FMA chains on the vector ALU (the attention is ~1/40 of the GEMM work at ViT-B/32), accurate expf / logf, no
// atomics: every output element is one thread's fixed-order sum -- bitwise repeatable.
// A workgroup (4 waves) takes one (cut, head) and a block of kAtfRows rows; the whole head's other two operands are held in LDS
// (rows padded to 65 floats where lanes walk rows: conflict-free), at T = 256 about 150 KiB:
//   forward      (query block): K, V, the block's Q rows      -> att, lse      (causal variant: the text tower's, see the kernel)
//   backward dQ  (query block): K, V, the block's Q / dO rows -> dQ, delta_i = sum_j P_ij dP_ij
//   backward dKV (key block):   Q, dO, the block's K / V rows -> dK, dV   (reads lse and delta)
// A wave works one row at a time: lane j holds the scores of keys j, j + 64, ... (<= 4); the row's probabilities go through a
// per-wave LDS row, from which lane d forms output feature d.
// (The kernels are `inline`: two translation units include this header -- the product and the test entries; see vit_ops.h.)
#pragma once
#include "aph_device.h"

namespace aph {

constexpr int kAtfRows = 32;          // rows per workgroup
constexpr int kAtfPad = 65;           // padded row pitch (floats) of the operands lanes read row-wise

inline size_t attn_f32_smem(int T, int which) {     // which: 0 forward, 1 backward dQ, 2 backward dKV
  const size_t t = (size_t)T;
  if (which == 0) return 4 * (t * kAtfPad + t * 64 + kAtfRows * 64 + 4 * 256);
  if (which == 1) return 4 * (2 * t * kAtfPad + 2 * kAtfRows * 64 + 4 * 256);
  return 4 * (2 * t * kAtfPad + 2 * kAtfRows * 64 + 2 * 4 * 256 + 2 * t);
}

// rows [0, n) of one head's 64 columns at qkv column offset `col` -> LDS rows of pitch `pitch`
__device__ __forceinline__ void atf_stage(const float* __restrict__ src, int ld, int n, float* dst, int pitch) {
  for (int e = threadIdx.x; e < n * 64; e += blockDim.x) {
    const int r = e >> 6, d = e & 63;
    dst[r * pitch + d] = src[(size_t)r * ld + d];
  }
}

// CAUSAL (the text tower): query row i attends to the keys j <= i only.  The later keys never enter a score, the maximum, the sum or the
// P.V loop -- they are not masked after the fact, they are not read -- and only the i0 + nq K / V rows the block's rows can see are staged.
// The non-causal instantiation runs the same statements with T keys for every row.
template <bool CAUSAL>
__global__ __launch_bounds__(256) void attn_fwd_f32_kernel(const float* __restrict__ qkv, float* __restrict__ att, float* __restrict__ lse,
                                                           int T, int heads) {
  APH_DYN_SMEM(smem);
  const int nb = (T + kAtfRows - 1) / kAtfRows;
  const int item = blockIdx.x / nb, i0 = (blockIdx.x - item * nb) * kAtfRows;
  const int s = item / heads, h = item - s * heads, D = heads * 64, ld = 3 * D;
  const int nq = T - i0 < kAtfRows ? T - i0 : kAtfRows;
  float* Ks = reinterpret_cast<float*>(smem);           // [T][65]
  float* Vs = Ks + T * kAtfPad;                         // [T][64]
  float* Qs = Vs + T * 64;                              // [kAtfRows][64]
  float* Ps = Qs + kAtfRows * 64;                       // [4 waves][256]
  const float* base = qkv + (size_t)s * T * ld + h * 64;
  const int ns = CAUSAL ? i0 + nq : T;                  // K / V rows staged
  atf_stage(base + D, ld, ns, Ks, kAtfPad);
  atf_stage(base + 2 * D, ld, ns, Vs, 64);
  atf_stage(base + (size_t)i0 * ld, ld, nq, Qs, 64);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* P = Ps + wave * 256;
  for (int r = wave; r < nq; r += 4) {
    const float* q = Qs + r * 64;
    const int nk = CAUSAL ? i0 + r + 1 : T;             // keys of this row
    float sc[4];
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = lane + 64 * c;
      float a = 0.f;
      if (j < nk) {
        const float* k = Ks + j * kAtfPad;
        for (int d = 0; d < 64; ++d) a = fmaf(q[d], k[d], a);
        mx = a > mx ? a : mx;
      }
      sc[c] = a;
    }
    mx = wave_max(mx);
    float l = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = lane + 64 * c;
      if (j < nk) {
        const float p = expf((sc[c] - mx) * 0.125f);
        sc[c] = p;
        l += p;
      }
    }
    l = wave_sum(l);
    const float il = 1.0f / l;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = lane + 64 * c;
      if (j < nk) P[j] = sc[c] * il;
    }
    wave_lds_fence();
    float o = 0.f;
    for (int j = 0; j < nk; ++j) o = fmaf(P[j], Vs[j * 64 + lane], o);
    const int i = i0 + r;
    att[((size_t)s * T + i) * D + h * 64 + lane] = o;
    if (lane == 0) lse[((size_t)s * heads + h) * T + i] = mx * 0.125f + logf(l);
    wave_lds_fence();          // P is rewritten by this wave's next row
  }
}

// dQ_i = 1/8 sum_j dS_ij K_j,  dS_ij = P_ij (dP_ij - delta_i),  dP_ij = dO_i . V_j,  P_ij = exp(S_ij / 8 - lse_i)
inline __global__ __launch_bounds__(256) void attn_bwd_dq_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ datt, const float* __restrict__ lse,
                                                              float* __restrict__ delta, float* __restrict__ dqkv, int T, int heads) {
  APH_DYN_SMEM(smem);
  const int nb = (T + kAtfRows - 1) / kAtfRows;
  const int item = blockIdx.x / nb, i0 = (blockIdx.x - item * nb) * kAtfRows;
  const int s = item / heads, h = item - s * heads, D = heads * 64, ld = 3 * D;
  const int nq = T - i0 < kAtfRows ? T - i0 : kAtfRows;
  float* Ks = reinterpret_cast<float*>(smem);           // [T][65]
  float* Vs = Ks + T * kAtfPad;                         // [T][65]
  float* Qs = Vs + T * kAtfPad;                         // [kAtfRows][64]
  float* Gs = Qs + kAtfRows * 64;                       // [kAtfRows][64]  dO rows
  float* Ps = Gs + kAtfRows * 64;                       // [4 waves][256]  dS row
  const float* base = qkv + (size_t)s * T * ld + h * 64;
  atf_stage(base + D, ld, T, Ks, kAtfPad);
  atf_stage(base + 2 * D, ld, T, Vs, kAtfPad);
  atf_stage(base + (size_t)i0 * ld, ld, nq, Qs, 64);
  atf_stage(datt + ((size_t)s * T + i0) * D + h * 64, D, nq, Gs, 64);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* P = Ps + wave * 256;
  for (int r = wave; r < nq; r += 4) {
    const int i = i0 + r;
    const float* q = Qs + r * 64;
    const float* g = Gs + r * 64;
    const float L = lse[((size_t)s * heads + h) * T + i];
    float pv[4], dp[4];
    float dsum = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = lane + 64 * c;
      pv[c] = 0.f; dp[c] = 0.f;
      if (j < T) {
        const float* k = Ks + j * kAtfPad;
        const float* v = Vs + j * kAtfPad;
        float a = 0.f, b = 0.f;
        for (int d = 0; d < 64; ++d) { a = fmaf(q[d], k[d], a); b = fmaf(g[d], v[d], b); }
        pv[c] = expf(a * 0.125f - L);
        dp[c] = b;
        dsum = fmaf(pv[c], b, dsum);
      }
    }
    const float Di = wave_sum(dsum);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = lane + 64 * c;
      if (j < T) P[j] = pv[c] * (dp[c] - Di);
    }
    wave_lds_fence();
    float o = 0.f;
    for (int j = 0; j < T; ++j) o = fmaf(P[j], Ks[j * kAtfPad + lane], o);
    dqkv[((size_t)s * T + i) * ld + h * 64 + lane] = o * 0.125f;
    if (lane == 0) delta[((size_t)s * heads + h) * T + i] = Di;
    wave_lds_fence();
  }
}

// dK_j = 1/8 sum_i dS_ij Q_i,  dV_j = sum_i P_ij dO_i   (key block j0 .. j0 + kAtfRows)
inline __global__ __launch_bounds__(256) void attn_bwd_dkv_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ datt, const float* __restrict__ lse,
                                                               const float* __restrict__ delta, float* __restrict__ dqkv, int T, int heads) {
  APH_DYN_SMEM(smem);
  const int nb = (T + kAtfRows - 1) / kAtfRows;
  const int item = blockIdx.x / nb, j0 = (blockIdx.x - item * nb) * kAtfRows;
  const int s = item / heads, h = item - s * heads, D = heads * 64, ld = 3 * D;
  const int nk = T - j0 < kAtfRows ? T - j0 : kAtfRows;
  float* Qs = reinterpret_cast<float*>(smem);           // [T][65]
  float* Gs = Qs + T * kAtfPad;                         // [T][65]  dO
  float* Kb = Gs + T * kAtfPad;                         // [kAtfRows][64]
  float* Vb = Kb + kAtfRows * 64;                       // [kAtfRows][64]
  float* Ps = Vb + kAtfRows * 64;                       // [4 waves][256]  P column
  float* Ss = Ps + 4 * 256;                             // [4 waves][256]  dS column
  float* Ls = Ss + 4 * 256;                             // [T] lse
  float* Ds = Ls + T;                                   // [T] delta
  const float* base = qkv + (size_t)s * T * ld + h * 64;
  atf_stage(base, ld, T, Qs, kAtfPad);
  atf_stage(datt + (size_t)s * T * D + h * 64, D, T, Gs, kAtfPad);
  atf_stage(base + (size_t)j0 * ld + D, ld, nk, Kb, 64);
  atf_stage(base + (size_t)j0 * ld + 2 * D, ld, nk, Vb, 64);
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    Ls[t] = lse[((size_t)s * heads + h) * T + t];
    Ds[t] = delta[((size_t)s * heads + h) * T + t];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* P = Ps + wave * 256;
  float* dS = Ss + wave * 256;
  for (int r = wave; r < nk; r += 4) {
    const int j = j0 + r;
    const float* k = Kb + r * 64;
    const float* v = Vb + r * 64;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = lane + 64 * c;
      if (i < T) {
        const float* q = Qs + i * kAtfPad;
        const float* g = Gs + i * kAtfPad;
        float a = 0.f, b = 0.f;
        for (int d = 0; d < 64; ++d) { a = fmaf(q[d], k[d], a); b = fmaf(g[d], v[d], b); }
        const float p = expf(a * 0.125f - Ls[i]);
        P[i] = p;
        dS[i] = p * (b - Ds[i]);
      }
    }
    wave_lds_fence();
    float dk = 0.f, dv = 0.f;
    for (int i = 0; i < T; ++i) {
      dk = fmaf(dS[i], Qs[i * kAtfPad + lane], dk);
      dv = fmaf(P[i], Gs[i * kAtfPad + lane], dv);
    }
    float* o = dqkv + ((size_t)s * T + j) * ld + h * 64 + lane;
    o[D] = dk * 0.125f;
    o[2 * D] = dv;
    wave_lds_fence();
  }
}

template <bool CAUSAL = false>
void launch_attn_fwd_f32(const float* qkv, float* att, float* lse, int S, int T, int heads, hipStream_t st) {
  const size_t smem = attn_f32_smem(T, 0);
  APH_ALLOW_SMEM(attn_fwd_f32_kernel<CAUSAL>, smem);
  APH_LAUNCH(attn_fwd_f32_kernel<CAUSAL>, dim3(S * heads * ((T + kAtfRows - 1) / kAtfRows)), dim3(256), smem, st, qkv, att, lse, T, heads);
}
inline void launch_attn_bwd_f32(const float* qkv, const float* datt, const float* lse, float* delta, float* dqkv, int S, int T, int heads,
                                hipStream_t st) {
  const dim3 grid(S * heads * ((T + kAtfRows - 1) / kAtfRows));
  const size_t s1 = attn_f32_smem(T, 1), s2 = attn_f32_smem(T, 2);
  APH_ALLOW_SMEM(attn_bwd_dq_f32_kernel, s1);
  APH_ALLOW_SMEM(attn_bwd_dkv_f32_kernel, s2);
  APH_LAUNCH(attn_bwd_dq_f32_kernel, grid, dim3(256), s1, st, qkv, datt, lse, delta, dqkv, T, heads);
  APH_LAUNCH(attn_bwd_dkv_f32_kernel, grid, dim3(256), s2, st, qkv, datt, lse, (const float*)delta, dqkv, T, heads);
}

}  // namespace aph
