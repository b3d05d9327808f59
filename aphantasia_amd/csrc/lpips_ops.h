// The LPIPS term's kernels around the convolutions (lpips_conv.h): the half-size bicubic resize with the input scaling and its adjoint,
// the 2x2 max-pool, the merge of the backward streams at a tap, and the head (channel norm, difference, lin weights, spatial mean).
// Everything here is fp32 arithmetic on f16 NHWC activations; spatial sums go through fp64 block partials in a fixed order.
#pragma once
#include "aph_device.h"
#include "aph_host.h"

namespace aph {
namespace lpips {

constexpr float kEps = 1e-10f;
constexpr float kF16Max = 65504.f;
constexpr int kHeadBlocks = 512;         // most workgroups (= fp64 partials) of one head launch

// ---- bicubic, align_corners = True, A = -0.75, border taps clamped (torch upsample_bicubic2d) -------------------------------------------------
// Output index o of `out` samples reads source coordinate o (in - 1) / (out - 1): the whole part i0 and the fraction are taken from the integer
// division, so the fraction is one rounding away from exact at any size.  Taps i0 - 1 .. i0 + 2 with weights w[0 .. 3].
__device__ __forceinline__ void cubic_taps(int o, int in, int out, int& i0, float w[4]) {
  const int num = o * (in - 1), den = out - 1;
  i0 = num / den;
  const float t = (float)(num - i0 * den) / (float)den;
  // the outer taps A (x^3 - 5 x^2 + 8 x - 4) at x = 1 + t factor as A t (1 - t)^2: evaluated as the product, not as a Horner chain whose terms
  // of size 8 |A| x cancel down to a weight below 0.15
  const float A = -0.75f, u = 1.f - t;
  w[0] = A * t * u * u;
  w[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
  w[2] = ((A + 2.f) * u - (A + 3.f)) * u * u + 1.f;
  w[3] = A * u * t * t;
}
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__device__ __forceinline__ float cubic_sample(const float* __restrict__ src, int W, int H, int y0, const float wy[4], int x0, const float wx[4]) {
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float* row = src + (size_t)clampi(y0 - 1 + i, H - 1) * W;
    float r = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) r += wx[j] * row[clampi(x0 - 1 + j, W - 1)];
    acc += wy[i] * r;
  }
  return acc;
}

// out [3][Ho][Wo] = resize(in [3][H][W])
static __global__ __launch_bounds__(256) void resize_fwd_kernel(const float* __restrict__ in, int H, int W, float* __restrict__ out, int Ho, int Wo) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= Ho * Wo) return;
  const int oy = idx / Wo, ox = idx - oy * Wo;
  int y0, x0; float wy[4], wx[4];
  cubic_taps(oy, H, Ho, y0, wy);
  cubic_taps(ox, W, Wo, x0, wx);
  for (int c = 0; c < 3; ++c) out[(size_t)c * Ho * Wo + idx] = cubic_sample(in + (size_t)c * H * W, W, H, y0, wy, x0, wx);
}

// The same taps in fp64 for the network's input (below)
__device__ __forceinline__ void cubic_taps64(int o, int in, int out, int& i0, double w[4]) {
  const int num = o * (in - 1), den = out - 1;
  i0 = num / den;
  const double t = (double)(num - i0 * den) / (double)den, A = -0.75, u = 1.0 - t;
  w[0] = A * t * u * u;
  w[1] = ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0;
  w[2] = ((A + 2.0) * u - (A + 3.0)) * u * u + 1.0;
  w[3] = A * u * t * t;
}

// The network's input: x [Ho][Wo][8] f16 = ((2 resize(rgb) - 1) - shift_c) / scale_c in channels 0 .. 2, zeros in 3 .. 7.  Resize and scaling
// in fp64 and ONE rounding to f16: the stored value is the correctly rounded one, not an fp32 result rounded again (a double rounding lands on
// the other f16 neighbour now and then, and every such flip travels through the whole network).  48 fp64 multiply-adds per pixel: nothing.
static __global__ __launch_bounds__(256) void prep_kernel(const float* __restrict__ in, int H, int W, half_t* __restrict__ x, int Ho, int Wo) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= Ho * Wo) return;
  const int oy = idx / Wo, ox = idx - oy * Wo;
  int y0, x0; double wy[4], wx[4];
  cubic_taps64(oy, H, Ho, y0, wy);
  cubic_taps64(ox, W, Wo, x0, wx);
  const double shift[3] = {-0.030, -0.088, -0.188}, scale[3] = {0.458, 0.448, 0.450};
  half8 v;
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = (half_t)0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* src = in + (size_t)c * H * W;
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float* row = src + (size_t)clampi(y0 - 1 + i, H - 1) * W;
      double r = 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j) r += wx[j] * (double)row[clampi(x0 - 1 + j, W - 1)];
      acc += wy[i] * r;
    }
    v[c] = (half_t)(((2.0 * acc - 1.0) - shift[c]) / scale[c]);
  }
  *reinterpret_cast<half8*>(x + (size_t)idx * 8) = v;
}

// The adjoint as a gather: grad [3][H][W] += coef_c * sum over the output samples whose (clamped) taps land on (y, x) of weight * g [3][Ho][Wo].
// coef_c = coef * (chain ? 2 / scale_c : 1) * (*d_weight if given).  One thread per input pixel, candidates in ascending (oy, ox): a fixed order.
static __global__ __launch_bounds__(256) void resize_adj_kernel(const float* __restrict__ g, int Ho, int Wo, float* __restrict__ grad, int H, int W, float coef,
                                                         int chain, const float* __restrict__ d_weight) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= H * W) return;
  const int y = idx / W, x = idx - y * W;
  // samples whose first tap row i0 - 1 .. i0 + 2 can reach y: i0 in [y - 2, y + 1]; one extra candidate either side costs a comparison
  const int oy_lo = clampi((int)(((long long)(y - 2) * (Ho - 1)) / (H - 1)) - 1, Ho - 1), oy_hi = clampi((int)(((long long)(y + 2) * (Ho - 1)) / (H - 1)) + 1, Ho - 1);
  const int ox_lo = clampi((int)(((long long)(x - 2) * (Wo - 1)) / (W - 1)) - 1, Wo - 1), ox_hi = clampi((int)(((long long)(x + 2) * (Wo - 1)) / (W - 1)) + 1, Wo - 1);
  float acc[3] = {0.f, 0.f, 0.f};
  for (int oy = oy_lo; oy <= oy_hi; ++oy) {
    int y0; float wy[4];
    cubic_taps(oy, H, Ho, y0, wy);
    float ay = 0.f; bool hit_y = false;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (clampi(y0 - 1 + i, H - 1) == y) { ay += wy[i]; hit_y = true; }
    if (!hit_y) continue;
    for (int ox = ox_lo; ox <= ox_hi; ++ox) {
      int x0; float wx[4];
      cubic_taps(ox, W, Wo, x0, wx);
      float ax = 0.f; bool hit_x = false;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (clampi(x0 - 1 + j, W - 1) == x) { ax += wx[j]; hit_x = true; }
      if (!hit_x) continue;
      const float wgt = ay * ax;
      const size_t o = (size_t)oy * Wo + ox;
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += wgt * g[(size_t)c * Ho * Wo + o];
    }
  }
  const float scale[3] = {0.458f, 0.448f, 0.450f};
  const float wgt = d_weight ? *d_weight : 1.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) grad[(size_t)c * H * W + idx] += acc[c] * (coef * (chain ? 2.f / scale[c] : 1.f) * wgt);
}

// ---- 2x2 stride-2 floor max-pool on [H][W][C] f16, C % 8 == 0 ----------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void pool_fwd_kernel(const half_t* __restrict__ in, int H, int W, int C, half_t* __restrict__ out) {
  const int Hp = H / 2, Wp = W / 2, c8 = C / 8;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)Hp * Wp * c8) return;
  const int v = (int)(idx % c8);
  const size_t p = idx / c8;
  const int py = (int)(p / Wp), px = (int)(p - (size_t)py * Wp);
  const half_t* s = in + ((size_t)(2 * py) * W + 2 * px) * C + v * 8;
  half8 m = *reinterpret_cast<const half8*>(s);
  const half8 b = *reinterpret_cast<const half8*>(s + C), c = *reinterpret_cast<const half8*>(s + (size_t)W * C), d = *reinterpret_cast<const half8*>(s + (size_t)W * C + C);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (b[k] > m[k]) m[k] = b[k];
    if (c[k] > m[k]) m[k] = c[k];
    if (d[k] > m[k]) m[k] = d[k];
  }
  *reinterpret_cast<half8*>(out + p * C + v * 8) = m;
}

// The backward stream at the stored activation act [H][W][C]:  out f16 = sat(((dpool routed to the window's first maximum) + head) x (act > 0)).
//   dpool [H/2][W/2][C] f16 or null (no pool above this activation); the argmax is recomputed from act, first maximum in row-major window
//   order; a trailing odd row / column is in no window and receives nothing from dpool
//   head  [H][W][C] fp32 or null (no tap here);  relu == 0: no mask (the pool test entry)
static __global__ __launch_bounds__(256) void grad_merge_kernel(const half_t* __restrict__ act, int H, int W, int C, const half_t* __restrict__ dpool,
                                                         const float* __restrict__ head, int relu, half_t* __restrict__ out) {
  const int Hp = H / 2, Wp = W / 2, c8 = C / 8;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)H * W * c8) return;
  const int v = (int)(idx % c8);
  const size_t p = idx / c8;
  const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
  const size_t o = p * C + v * 8;
  const half8 a = *reinterpret_cast<const half8*>(act + o);
  float g[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) g[k] = head ? head[o + k] : 0.f;
  const int py = y >> 1, px = x >> 1;
  if (dpool && py < Hp && px < Wp) {
    const half_t* s = act + ((size_t)(2 * py) * W + 2 * px) * C + v * 8;
    const half8 w0 = *reinterpret_cast<const half8*>(s), w1 = *reinterpret_cast<const half8*>(s + C);
    const half8 w2 = *reinterpret_cast<const half8*>(s + (size_t)W * C), w3 = *reinterpret_cast<const half8*>(s + (size_t)W * C + C);
    const half8 d = *reinterpret_cast<const half8*>(dpool + ((size_t)py * Wp + px) * C + v * 8);
    const int me = (y & 1) * 2 + (x & 1);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      int arg = 0; half_t m = w0[k];
      if (w1[k] > m) { m = w1[k]; arg = 1; }
      if (w2[k] > m) { m = w2[k]; arg = 2; }
      if (w3[k] > m) { m = w3[k]; arg = 3; }
      if (arg == me) g[k] += (float)d[k];
    }
  }
  half8 r;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float t = (!relu || (float)a[k] > 0.f) ? g[k] : 0.f;
    t = t > kF16Max ? kF16Max : (t < -kF16Max ? -kF16Max : t);
    r[k] = (half_t)t;
  }
  *reinterpret_cast<half8*>(out + o) = r;
}

// ---- head --------------------------------------------------------------------------------------------------------------------------------------
// Eight lanes per pixel, lane j of the group takes the 8-channel vectors j, j + 8, ...; the group's sums are xor-shuffles (every lane of the
// workgroup runs every iteration, so the shuffles are whole-wave).
__device__ __forceinline__ float group8_sum(float v) {
  v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
  return v;
}

// ny [P][C] fp32 = f / (sqrt(sum_c f^2) + eps): the constant side of the head
static __global__ __launch_bounds__(256) void unit_norm_kernel(const half_t* __restrict__ f, int P, int C, float* __restrict__ ny) {
  const int j = threadIdx.x & 7, nv = C / 8;
  for (size_t base = (size_t)blockIdx.x * 32; base < (size_t)P; base += (size_t)gridDim.x * 32) {
    const size_t p = base + (threadIdx.x >> 3);
    const bool ok = p < (size_t)P;
    float ss = 0.f;
    if (ok)
      for (int v = j; v < nv; v += 8) {
        const half8 h = *reinterpret_cast<const half8*>(f + p * C + v * 8);
#pragma unroll
        for (int k = 0; k < 8; ++k) ss += (float)h[k] * (float)h[k];
      }
    ss = group8_sum(ss);
    const float inv = 1.f / (sqrtf(ss) + kEps);
    if (ok)
      for (int v = j; v < nv; v += 8) {
        const half8 h = *reinterpret_cast<const half8*>(f + p * C + v * 8);
#pragma unroll
        for (int k = 0; k < 8; ++k) ny[p * C + v * 8 + k] = (float)h[k] * inv;
      }
  }
}

// d(p) = sum_c lin_c (n_c - ny_c)^2, n = f / (s + eps), s = sqrt(sum_c f^2);  partial[block] = this workgroup's sum_p d(p) in fp64.
// hg [P][C] (or null) = gcoef * dd/df:  dd/df_k = q_k / (s + eps) - f_k (sum_c q_c f_c) / (s (s + eps)^2),  q_c = 2 lin_c (n_c - ny_c);
// the second term is 0 at s = 0 (f = 0).
static __global__ __launch_bounds__(256) void head_kernel(const half_t* __restrict__ f, const float* __restrict__ ny, const float* __restrict__ lin, int P, int C,
                                                   float gcoef, float* __restrict__ hg, double* __restrict__ partial) {
  __shared__ double red[16];
  const int j = threadIdx.x & 7, nv = C / 8;
  double mine = 0.0;
  for (size_t base = (size_t)blockIdx.x * 32; base < (size_t)P; base += (size_t)gridDim.x * 32) {
    const size_t p = base + (threadIdx.x >> 3);
    const bool ok = p < (size_t)P;
    float ss = 0.f;
    if (ok)
      for (int v = j; v < nv; v += 8) {
        const half8 h = *reinterpret_cast<const half8*>(f + p * C + v * 8);
#pragma unroll
        for (int k = 0; k < 8; ++k) ss += (float)h[k] * (float)h[k];
      }
    ss = group8_sum(ss);
    const float s = sqrtf(ss), inv = 1.f / (s + kEps);
    float val = 0.f, dot = 0.f;
    if (ok)
      for (int v = j; v < nv; v += 8) {
        const half8 h = *reinterpret_cast<const half8*>(f + p * C + v * 8);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int c = v * 8 + k;
          const float fk = (float)h[k], d = fk * inv - ny[p * C + c], l = lin[c];
          val += l * d * d;
          dot += 2.f * l * d * fk;
        }
      }
    val = group8_sum(val);
    dot = group8_sum(dot);
    if (ok && j == 0) mine += (double)val;
    if (ok && hg) {
      const float back = s > 0.f ? dot * inv * inv / s : 0.f;
      for (int v = j; v < nv; v += 8) {
        const half8 h = *reinterpret_cast<const half8*>(f + p * C + v * 8);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int c = v * 8 + k;
          const float fk = (float)h[k], d = fk * inv - ny[p * C + c];
          hg[p * C + c] = gcoef * (2.f * lin[c] * d * inv - fk * back);
        }
      }
    }
  }
  const double tot = block_sum(mine, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// value = sum_l (sum of tap l's partials) / P_l in fp64, taps and partials in index order; *d_value (nullable) = value, *d_loss (nullable) +=
// *d_weight * value.  One workgroup.
struct HeadSums { const double* partial[5]; int count[5]; int P[5]; };
static __global__ __launch_bounds__(256) void head_finish_kernel(HeadSums hs, const float* __restrict__ d_weight, float* __restrict__ d_value, float* __restrict__ d_loss) {
  __shared__ double red[16];
  double total = 0.0;
  for (int l = 0; l < 5; ++l) {
    double a = 0.0;
    for (int i = threadIdx.x; i < hs.count[l]; i += blockDim.x) a += hs.partial[l][i];
    total += block_sum(a, red) / (double)hs.P[l];
  }
  if (threadIdx.x == 0) {
    const float v = (float)total;
    if (d_value) *d_value = v;
    if (d_loss) *d_loss += *d_weight * v;
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------------
static inline unsigned blocks_for(size_t n, int per) { return (unsigned)((n + per - 1) / per); }
static inline int head_blocks(int P) { const int b = (P + 31) / 32; return b > kHeadBlocks ? kHeadBlocks : b; }

static inline void launch_resize_fwd(const float* in, int H, int W, float* out, int Ho, int Wo, hipStream_t st) {
  APH_LAUNCH(resize_fwd_kernel, dim3(blocks_for((size_t)Ho * Wo, 256)), dim3(256), 0, st, in, H, W, out, Ho, Wo);
}
static inline void launch_prep(const float* in, int H, int W, half_t* x, int Ho, int Wo, hipStream_t st) {
  APH_LAUNCH(prep_kernel, dim3(blocks_for((size_t)Ho * Wo, 256)), dim3(256), 0, st, in, H, W, x, Ho, Wo);
}
static inline void launch_resize_adj(const float* g, int Ho, int Wo, float* grad, int H, int W, float coef, int chain, const float* d_weight, hipStream_t st) {
  APH_LAUNCH(resize_adj_kernel, dim3(blocks_for((size_t)H * W, 256)), dim3(256), 0, st, g, Ho, Wo, grad, H, W, coef, chain, d_weight);
}
static inline void launch_pool_fwd(const half_t* in, int H, int W, int C, half_t* out, hipStream_t st) {
  APH_LAUNCH(pool_fwd_kernel, dim3(blocks_for((size_t)(H / 2) * (W / 2) * (C / 8), 256)), dim3(256), 0, st, in, H, W, C, out);
}
static inline void launch_grad_merge(const half_t* act, int H, int W, int C, const half_t* dpool, const float* head, int relu, half_t* out, hipStream_t st) {
  APH_LAUNCH(grad_merge_kernel, dim3(blocks_for((size_t)H * W * (C / 8), 256)), dim3(256), 0, st, act, H, W, C, dpool, head, relu, out);
}
static inline void launch_unit_norm(const half_t* f, int P, int C, float* ny, hipStream_t st) {
  APH_LAUNCH(unit_norm_kernel, dim3(head_blocks(P)), dim3(256), 0, st, f, P, C, ny);
}
static inline void launch_head(const half_t* f, const float* ny, const float* lin, int P, int C, float gcoef, float* hg, double* partial, hipStream_t st) {
  APH_LAUNCH(head_kernel, dim3(head_blocks(P)), dim3(256), 0, st, f, ny, lin, P, C, gcoef, hg, partial);
}

}  // namespace lpips
}  // namespace aph
