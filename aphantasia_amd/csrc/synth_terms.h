// Image parameteriser, loss terms on rgb [3,H,W]: illustrip's RGB priors and the --sharp term, value and gradient.  Included by synth.hip.
#pragma once
#include "synth_rgb.h"

namespace aph {

// ---------------------------------------------------------------------------------
// illustrip's RGB priors (illustrip.py:438-440, `--gen RGB`):
//     loss += mean_c |mean_hw(rgb_c) - t_mean|  +  mean_c |std_hw(rgb_c) - t_std|        (unbiased std)
// Per-channel (sum, sumsq) in fp64 block partials (stats_partial_kernel, grid (kPriorBlocks, 3)), then value and gradient in one elementwise pass:
//     d/d rgb_c[p] = [sign(m_c - t_mean) / HW  +  sign(s_c - t_std) (rgb_c[p] - m_c) / ((HW - 1) s_c)] / 3
// ---------------------------------------------------------------------------------
constexpr int kPriorBlocks = 128;

// mean and unbiased std of channel c from its nb block partials (one thread, fixed order)
__device__ __forceinline__ void prior_channel_stats(const double* __restrict__ partials, int nb, int c, double n, double& mean, double& sd) {
  SumSq s;
  for (int i = 0; i < nb; ++i) s.add(partials + ((size_t)c * nb + i) * 2);
  s.mean_std(n, mean, sd);
  sd = sd > 0 ? sd : 0;      // (a non-finite channel: the priors take its std as 0, the global statistics above keep the NaN)
}

__global__ void rgb_prior_apply_kernel(const float* __restrict__ rgb, size_t HW, const double* __restrict__ partials, int nb,
                                       float t_mean, float t_std, float weight, float* __restrict__ loss, float* __restrict__ grgb) {
  __shared__ float ab[3];
  const int c = blockIdx.y;
  const double n = (double)HW;
  if (threadIdx.x == 0) {
    double m, sd;
    prior_channel_stats(partials, nb, c, n, m, sd);
    const double sm = m > t_mean ? 1.0 : (m < t_mean ? -1.0 : 0.0), ss = sd > t_std ? 1.0 : (sd < t_std ? -1.0 : 0.0);
    ab[0] = (float)(weight * sm / (3.0 * n));
    ab[1] = sd > 0 ? (float)(weight * ss / (3.0 * (n - 1.0) * sd)) : 0.f;
    ab[2] = (float)m;
    if (loss && blockIdx.x == 0 && c == 0) {          // one thread adds the value of all three channels (fixed order)
      double v = 0.0;
      for (int cc = 0; cc < 3; ++cc) {
        double m2, s2;
        prior_channel_stats(partials, nb, cc, n, m2, s2);
        v += fabs(m2 - t_mean) / 3.0 + fabs(s2 - t_std) / 3.0;
      }
      loss[0] += (float)(weight * v);
    }
  }
  __syncthreads();
  if (!grgb) return;
  const float a = ab[0], b = ab[1], mu = ab[2];
  const float* x = rgb + (size_t)c * HW;
  float* g = grgb + (size_t)c * HW;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += (size_t)gridDim.x * blockDim.x) g[i] += a + b * (x[i] - mu);
}

// ---------------------------------------------------------------------------------
// --sharp term (clip_fft.py:269-270): derivat(img, 'naiv') = 0.5 (mean |d/dx| + mean |d/dy|)  (utils.py:265-268)
// over rgb [3,H,W]; value and gradient (sub-gradient 0 at ties, as torch.abs) in two passes.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ float sgnf(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

__global__ void rgb_sharp_partial_kernel(const float* __restrict__ rgb, int H, int W, double* __restrict__ partials) {
  __shared__ double red[16];
  const size_t n = (size_t)3 * H * W;
  double sx = 0.0, sy = 0.0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const float v = rgb[i];
    if (x + 1 < W) sx += fabsf(rgb[i + 1] - v);
    if (y + 1 < H) sy += fabsf(rgb[i + W] - v);
  }
  sx = block_sum(sx, red);
  sy = block_sum(sy, red);
  if (threadIdx.x == 0) { partials[2 * blockIdx.x] = sx; partials[2 * blockIdx.x + 1] = sy; }
}

__global__ void rgb_sharp_apply_kernel(const float* __restrict__ rgb, int H, int W, const double* __restrict__ partials, int nb,
                                       float weight, float* __restrict__ loss, float* __restrict__ grgb) {
  const double nx = 3.0 * H * (W - 1), ny = 3.0 * (H - 1) * W;
  if (loss && blockIdx.x == 0 && threadIdx.x == 0) {
    double sx = 0.0, sy = 0.0;
    for (int i = 0; i < nb; ++i) { sx += partials[2 * i]; sy += partials[2 * i + 1]; }
    loss[0] += (float)(weight * 0.5 * (sx / nx + sy / ny));
  }
  if (!grgb) return;
  const float kx = (float)(0.5 * weight / nx), ky = (float)(0.5 * weight / ny);
  const size_t n = (size_t)3 * H * W;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const float v = rgb[i];
    float gx = 0.f, gy = 0.f;
    if (x > 0) gx += sgnf(v - rgb[i - 1]);
    if (x + 1 < W) gx -= sgnf(rgb[i + 1] - v);
    if (y > 0) gy += sgnf(v - rgb[i - W]);
    if (y + 1 < H) gy -= sgnf(rgb[i + W] - v);
    grgb[i] += kx * gx + ky * gy;
  }
}

}  // namespace aph
