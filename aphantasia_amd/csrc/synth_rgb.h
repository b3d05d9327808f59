// Image parameteriser, from raw to rgb: the fp64 statistics (sum / sum-of-squares accumulator, partial and finalize kernels), the 3x3 colour
// mix + sigmoid (to_valid_rgb) with its adjoint, and the element-wise std-normalisation adjoint of the spatial parameterisers.
// Included by synth.hip.
#pragma once
#include "aph_device.h"
#include "aph_host.h"

namespace aph {

// (sum, sum of squares) of fp32 values in fp64: a thread's share, then the block's total as a pair of doubles
struct SumSq {
  double s1 = 0.0, s2 = 0.0;
  __device__ __forceinline__ void add(float v) { s1 += v; s2 += (double)v * v; }
  __device__ __forceinline__ void add(const double* __restrict__ pair) { s1 += pair[0]; s2 += pair[1]; }
  // every thread gets the block's totals; `red` = LDS scratch of >= 16 doubles
  __device__ __forceinline__ void block_total(double* red) {
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
  }
  __device__ __forceinline__ void store_block_total(double* red, double* __restrict__ pair) {
    block_total(red);
    if (threadIdx.x == 0) { pair[0] = s1; pair[1] = s2; }
  }
  // mean and unbiased std of the n values summed   (image.py:174 `image.std()`)
  __device__ __forceinline__ void mean_std(double n, double& mean, double& sd) const {
    mean = s1 / n;
    double var = (s2 - s1 * mean) / (n - 1.0);
    if (var < 0) var = 0;
    sd = sqrt(var);
  }
};

// per-block partial (sum, sumsq) of plane blockIdx.y of x [gridDim.y][n]  ->  partials[blockIdx.y][gridDim.x][2]
// (one plane: the pixel / DWT parameterisers' global std; three: the RGB priors' per-channel statistics)
__global__ void stats_partial_kernel(const float* __restrict__ x, size_t n, double* __restrict__ partials) {
  __shared__ double red[16];
  x += (size_t)blockIdx.y * n;
  SumSq s;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) s.add(x[i]);
  s.store_block_total(red, partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2);
}

// stats[0] = mean, stats[1] = unbiased std
__global__ void stats_finalize_kernel(const double* __restrict__ partials, int nparts, double n, float* __restrict__ stats) {
  __shared__ double red[16];
  SumSq s;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) s.add(partials + 2 * i);
  s.block_total(red);
  if (threadIdx.x == 0) {
    double mean, sd;
    s.mean_std(n, mean, sd);
    stats[0] = (float)mean;
    stats[1] = (float)sd;
  }
}

// bstats = {A, B, mean} for  d raw = A * dn + B * (raw - mean):
//   y = c x / s ;  dL/dx_i = (c/s) g_i - c (sum_j g_j x_j) / (s^3 (N-1)) (x_i - mean)
// fixed_div > 0 selects pixel_image's `fixcontrast` branch (image.py:115-116): y = c x / fixed_div.
__global__ void bstats_finalize_kernel(const double* __restrict__ partials, int nparts, double n,
                                       const float* __restrict__ stats, float contrast, float fixed_div,
                                       float* __restrict__ bstats) {
  __shared__ double red[16];
  double sg = 0.0;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) sg += partials[i];
  sg = block_sum(sg, red);
  if (threadIdx.x == 0) {
    if (fixed_div > 0.f) {
      bstats[0] = contrast / fixed_div; bstats[1] = 0.f; bstats[2] = 0.f;
    } else {
      const double s = stats[1], c = contrast;
      bstats[0] = (float)(c / s);
      bstats[1] = (float)(-c * sg / (s * s * s * (n - 1.0)));
      bstats[2] = stats[0];
    }
  }
}

// ---------------------------------------------------------------------------------
// colour decorrelation + sigmoid (to_valid_rgb), and adjoint
// ---------------------------------------------------------------------------------
struct ColorMat {
  float m[9];  // colcorr_t[c][d], row-major
  // z[d] = sum_c n[c] m[c][d]
  __device__ __forceinline__ void mix(float n0, float n1, float n2, float& z0, float& z1, float& z2) const {
    z0 = n0 * m[0] + n1 * m[3] + n2 * m[6];
    z1 = n0 * m[1] + n1 * m[4] + n2 * m[7];
    z2 = n0 * m[2] + n1 * m[5] + n2 * m[8];
  }
  // g[c] = sum_d m[c][d] d[d]   (the adjoint of mix)
  __device__ __forceinline__ void mix_t(float d0, float d1, float d2, float& g0, float& g1, float& g2) const {
    g0 = m[0] * d0 + m[1] * d1 + m[2] * d2;
    g1 = m[3] * d0 + m[4] * d1 + m[5] * d2;
    g2 = m[6] * d0 + m[7] * d1 + m[8] * d2;
  }
};

__global__ void rgb_fwd_kernel(const float* __restrict__ raw, const float* __restrict__ stats, float contrast,
                               float fixed_div, ColorMat cc, int decorrelate, float* __restrict__ rgb, size_t HW) {
  const float k = fixed_div > 0.f ? contrast / fixed_div : contrast / stats[1];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += (size_t)gridDim.x * blockDim.x) {
    const float n0 = raw[i] * k, n1 = raw[HW + i] * k, n2 = raw[2 * HW + i] * k;
    float z0 = n0, z1 = n1, z2 = n2;
    if (decorrelate) cc.mix(n0, n1, n2, z0, z1, z2);
    rgb[i] = 1.0f / (1.0f + expf(-z0));
    rgb[HW + i] = 1.0f / (1.0f + expf(-z1));
    rgb[2 * HW + i] = 1.0f / (1.0f + expf(-z2));
  }
}

// dn[c] = sum_d cc[c][d] * drgb[d] * rgb[d] (1 - rgb[d]);  partial sums of dn * raw (fp64)
__global__ void rgb_bwd_kernel(const float* __restrict__ drgb, const float* __restrict__ rgb,
                               const float* __restrict__ raw, ColorMat cc, int decorrelate, float gscale,
                               float* __restrict__ dn, double* __restrict__ partials, size_t HW) {
  __shared__ double red[16];
  double acc = 0.0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += (size_t)gridDim.x * blockDim.x) {
    const float r0 = rgb[i], r1 = rgb[HW + i], r2 = rgb[2 * HW + i];
    const float d0 = drgb[i] * gscale * r0 * (1.f - r0), d1 = drgb[HW + i] * gscale * r1 * (1.f - r1),
                d2 = drgb[2 * HW + i] * gscale * r2 * (1.f - r2);
    float g0 = d0, g1 = d1, g2 = d2;
    if (decorrelate) cc.mix_t(d0, d1, d2, g0, g1, g2);
    dn[i] = g0; dn[HW + i] = g1; dn[2 * HW + i] = g2;
    acc += (double)g0 * raw[i] + (double)g1 * raw[HW + i] + (double)g2 * raw[2 * HW + i];
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// elementwise std-normalisation adjoint (pixel / DWT parameterisers; the FFT path fuses it)
__global__ void norm_bwd_kernel(const float* __restrict__ dn, const float* __restrict__ raw,
                                const float* __restrict__ bstats, float* __restrict__ draw, size_t n) {
  const float A = bstats[0], Bc = bstats[1], mu = bstats[2];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    draw[i] = A * dn[i] + Bc * (raw[i] - mu);
}

}  // namespace aph
