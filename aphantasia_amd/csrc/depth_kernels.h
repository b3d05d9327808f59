// Kernels of the Depth-Anything-V2 estimator (depth.hip) that the ViT and LPIPS headers do not already have: forward only, f16 operands,
// fp32 accumulation.
//   attn_long_fwd_kernel   softmax attention for any T >= 1 (T = 1370 at 518 x 518, 2406 at 518 x 910), head dim 64, online softmax
//   dn_gemm_kernel         the neck's 1 x 1 convolutions and kernel = stride transpose convolutions: out channels of any multiple of 16, K of any
//                          multiple of 8 (the ring GEMM of vit_gemm.h wants N % 64 == 0 and K % 64 == 0; the neck has 48 and 32)
//   dn_ln_kernel           LayerNorm of rows of any width D <= 1024 (D % 4 == 0; DINOv2-S has 384, vit_ops.h holds multiples of 256) with eps as
//                          an argument, optionally dropping the class row (the four taps)
//   dn_patch_kernel, dn_cls_kernel, dn_resize_kernel, dn_subsample_kernel, dn_head_out_kernel, dn_minmax_*_kernel: the small ones
// Activations of the neck and head are f16 [B][H][W][C], channel-innermost, as lpips_conv.h reads them.
#pragma once
#include "aph_device.h"
#include "aph_host.h"
#include "vit_gemm.h"
#include "vit_attn.h"

namespace aph {
namespace depth {

constexpr int kPatch = 14;
constexpr int kPatchK = 3 * kPatch * kPatch;      // 588
constexpr int kPatchKP = 640;                     // ... padded with zeros to a multiple of the GEMM's 64

// ---- attention --------------------------------------------------------------------------------------------------------------------------
// grid (ceil(T / 64), heads, images), 4 waves: wave w owns queries 64 blockIdx.x + 16 w .. + 15, its Q fragment loaded once from global into
// registers; the workgroup walks the keys in tiles of 64 staged in LDS: K row-major (at_off), V as the transposed slot-permuted image of
// vit_attn.h.  Scores are formed transposed (S^T = K Q^T): a lane owns ONE query (column l & 15) and 16 keys per tile, so the running
// maximum, the rescale of the accumulators and the row sum are lane-local (+ 2 shuffles over the four lane groups), and the exponentiated
// scores are already the B fragment of O^T += V^T P^T over the slot-permuted key index.  fp32 statistics, P rounded to f16 once, one f16
// rounding of O / l.  Keys >= T of the last tile: score -1e30 (p = 0) against zero K / V rows.  Queries >= T are computed on the clamped last
// row and not stored.
constexpr int kAttQT = 64, kAttKT = 64;
inline __global__ __launch_bounds__(256) void attn_long_fwd_kernel(const half_t* __restrict__ qkv, half_t* __restrict__ att, int T, int heads) {
  __shared__ __attribute__((aligned(16))) half_t lds[2 * 64 * 64];
  half_t* Ks = lds;
  half_t* Vt = lds + 64 * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6), c16 = lane & 15, g = lane >> 4;
  const int D = heads * 64, ld = 3 * D;
  const half_t* base = qkv + (size_t)blockIdx.z * T * ld + blockIdx.y * 64;
  const int q = blockIdx.x * kAttQT + wave * 16 + c16, qc = q < T ? q : T - 1;
  half8 qf[2];
#pragma unroll
  for (int kd = 0; kd < 2; ++kd) qf[kd] = *reinterpret_cast<const half8*>(base + (size_t)qc * ld + (kd * 4 + g) * 8);
  float m = -1e30f, l = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nkt = (T + kAttKT - 1) / kAttKT;
  for (int kt = 0; kt < nkt; ++kt) {
    const int k0 = kt * kAttKT, rows = T - k0 < kAttKT ? T - k0 : kAttKT;
    __syncthreads();                                   // the previous tile's fragment reads are done
    if (wave == 0) {
      at_stage_item(base + 2 * D + (size_t)k0 * ld, ld, rows, lane, nullptr, Vt, 64, false);
    } else {
      for (int i = tid - 64; i < 512; i += 192) {
        const int row = i >> 3, c = i & 7;
        half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (row < rows) v = *reinterpret_cast<const half8*>(base + D + (size_t)(k0 + row) * ld + c * 8);
        *reinterpret_cast<half8*>(Ks + at_off(row, c)) = v;
      }
    }
    __syncthreads();
    f32x4 st[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) st[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kd = 0; kd < 2; ++kd)
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) st[jt] = mfma_16x16x32_f16(at_frag(Ks, jt * 16 + c16, kd * 4 + g), qf[kd], st[jt]);
    // lane: query q, keys k0 + jt * 16 + g * 4 + r
    float mx = m;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) at_mask_max(st[jt], k0 + jt * 16, g * 4, T, mx);
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mxs = mx * kSL, sc = fast_exp2((m - mx) * kSL);      // the first tile: 2^-huge = 0 on accumulators that are zero anyway
    m = mx;
    float ls = 0.f;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = fast_exp2(fmaf(st[jt][r], kSL, -mxs));
        st[jt][r] = p;
        ls += p;
      }
    l = l * sc + ls;
    const half8 p0 = pack8(st[0], st[1]), p1 = pack8(st[2], st[3]);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      o[dt] *= sc;
      o[dt] = mfma_16x16x32_f16(at_frag(Vt, dt * 16 + c16, g), p0, o[dt]);
      o[dt] = mfma_16x16x32_f16(at_frag(Vt, dt * 16 + c16, 4 + g), p1, o[dt]);
    }
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  const float inv = 1.0f / l;
  // lane (c16, g), tile dt, reg r: O[q][dt * 16 + g * 4 + r]
  if (q < T) {
    half_t* orow = att + ((size_t)blockIdx.z * T + q) * D + blockIdx.y * 64 + g * 4;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) store_h4(orow + dt * 16, o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv);
  }
}
inline void launch_attn_long_fwd(const half_t* qkv, half_t* att, int B, int T, int heads, hipStream_t st) {
  APH_LAUNCH(attn_long_fwd_kernel, dim3((unsigned)((T + kAttQT - 1) / kAttQT), (unsigned)heads, (unsigned)B), dim3(256), 0, st, qkv, att, T, heads);
}

// ---- the neck's GEMM ---------------------------------------------------------------------------------------------------------------------
// C[m][n] = sum_k A[m][k] Bt[n][k]: A [M][lda] f16 (pixels x channels in), Bt [N][K] f16, N % 16 == 0, K % 8 == 0, any M.  The tile walk of
// lpips_conv.h with one tap: 64 rows (16 per wave, the MFMA's n index) x 64 output channels (the row index, so a lane ends up with four
// consecutive channels of one pixel), K in chunks of 32 staged in LDS at the 80-byte pitch.  apply4(m, n, v): channels n .. n + 3 of row m.
struct EpiDnBias {       // out [M][ldo] f16 = acc (+ bias)
  half_t* out; int ldo; const float* bias;
  __device__ __forceinline__ void apply4(int m, int n, f32x4 v) const {
    if (bias) v += ld4(bias + n);
    store_h4(out + (size_t)m * ldo + n, v[0], v[1], v[2], v[3]);
  }
};
// transpose convolution with kernel = stride = k as a GEMM over N = k k Cout columns ordered (ky, kx, co): row m = (image, y, x) of a gh x gw
// grid scatters its k x k block of output pixels, out [B][gh k][gw k][Cout] (Cout % 4 == 0: a lane's four columns are one pixel's)
struct EpiDnShuffle {
  half_t* out; const float* bias; int gh, gw, k, Cout;
  __device__ __forceinline__ void apply4(int m, int n, f32x4 v) const {
    const int P = gh * gw, b = m / P, p = m - b * P, y = p / gw, x = p - y * gw;
    const int tap = n / Cout, co = n - tap * Cout, ky = tap / k, kx = tap - ky * k;
    v += ld4(bias + co);
    store_h4(out + (((size_t)b * gh * k + (size_t)y * k + ky) * ((size_t)gw * k) + (size_t)x * k + kx) * Cout + co, v[0], v[1], v[2], v[3]);
  }
};
constexpr int kDnPS = 40;      // LDS row pitch in f16: 32 + 8 pad
template <class Epi>
__global__ __launch_bounds__(256) void dn_gemm_kernel(const half_t* __restrict__ A, int lda, const half_t* __restrict__ Bt, int M, int N, int K, Epi epi) {
  __shared__ __attribute__((aligned(16))) half_t sA[64 * kDnPS];
  __shared__ __attribute__((aligned(16))) half_t sB[64 * kDnPS];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6), li = lane & 15, lg = lane >> 4;
  const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
  const int nfrag = (N - n0) >= 64 ? 4 : (N - n0) / 16;
  f32x4 acc[4];
#pragma unroll
  for (int cf = 0; cf < 4; ++cf) acc[cf] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int srow = tid >> 2, sv = tid & 3;
  for (int k0 = 0; k0 < K; k0 += 32) {
    __syncthreads();
    {
      const int k = k0 + sv * 8, m = m0 + srow, n = n0 + srow;
      uint4 va = make_uint4(0u, 0u, 0u, 0u), vb = make_uint4(0u, 0u, 0u, 0u);
      if (m < M && k < K) va = *reinterpret_cast<const uint4*>(A + (size_t)m * lda + k);
      if (n < N && k < K) vb = *reinterpret_cast<const uint4*>(Bt + (size_t)n * K + k);
      *reinterpret_cast<uint4*>(sA + srow * kDnPS + sv * 8) = va;
      *reinterpret_cast<uint4*>(sB + srow * kDnPS + sv * 8) = vb;
    }
    __syncthreads();
    const half8 xf = *reinterpret_cast<const half8*>(sA + (wave * 16 + li) * kDnPS + lg * 8);
#pragma unroll
    for (int cf = 0; cf < 4; ++cf)
      if (cf < nfrag) acc[cf] = mfma_16x16x32_f16(*reinterpret_cast<const half8*>(sB + (cf * 16 + li) * kDnPS + lg * 8), xf, acc[cf]);
  }
  const int m = m0 + wave * 16 + li;
  if (m >= M) return;
#pragma unroll
  for (int cf = 0; cf < 4; ++cf)
    if (cf < nfrag) epi.apply4(m, n0 + cf * 16 + lg * 4, acc[cf]);
}
template <class Epi>
inline void launch_dn_gemm(const half_t* A, int lda, const half_t* Bt, int M, int N, int K, Epi epi, hipStream_t st) {
  APH_LAUNCH((dn_gemm_kernel<Epi>), dim3((unsigned)((M + 63) / 64), (unsigned)((N + 63) / 64)), dim3(256), 0, st, A, lda, Bt, M, N, K, epi);
}
// torch ConvTranspose2d weight [cin][cout][k][k] (fp32, host) -> Bt [(ky k + kx) cout + co][cin] f16
inline std::vector<half_t> pack_convt(const float* w, int cin, int cout, int k) {
  std::vector<half_t> p((size_t)k * k * cout * cin);
  for (int ci = 0; ci < cin; ++ci)
    for (int co = 0; co < cout; ++co)
      for (int t = 0; t < k * k; ++t) p[((size_t)t * cout + co) * cin + ci] = (half_t)w[((size_t)ci * cout + co) * k * k + t];
  return p;
}

// ---- small kernels ------------------------------------------------------------------------------------------------------------------------
// img f32 [B][3][h][w] in (0, 1) -> patch rows f16 [B gh gw][640]: element k = c 196 + py 14 + px of the normalised image (x - mean_c) / std_c,
// zeros from 588 on.  A thread per 8 elements.
inline __global__ __launch_bounds__(256) void dn_patch_kernel(const float* __restrict__ img, half_t* __restrict__ rows, int B, int h, int w) {
  const int gh = h / kPatch, gw = w / kPatch;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)B * gh * gw * (kPatchKP / 8)) return;
  const int k8 = (int)(idx % (kPatchKP / 8));
  const size_t mrow = idx / (kPatchKP / 8);
  const int b = (int)(mrow / ((size_t)gh * gw)), p = (int)(mrow - (size_t)b * gh * gw), gy = p / gw, gx = p - gy * gw;
  const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
  half8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = k8 * 8 + e;
    float v = 0.f;
    if (k < kPatchK) {
      const int c = k / (kPatch * kPatch), r = k - c * kPatch * kPatch, py = r / kPatch, px = r - py * kPatch;
      v = (img[(((size_t)b * 3 + c) * h + gy * kPatch + py) * w + gx * kPatch + px] - mean[c]) / sd[c];
    }
    o[e] = (half_t)v;
  }
  *reinterpret_cast<half8*>(rows + mrow * kPatchKP + k8 * 8) = o;
}
// the class rows: x[b T][:] = cls + pos[0]
inline __global__ __launch_bounds__(256) void dn_cls_kernel(const float* __restrict__ cls, const float* __restrict__ pos, float* __restrict__ x, int B, int T, int D) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * D) return;
  const int b = idx / D, d = idx - b * D;
  x[(size_t)b * T * D + d] = cls[d] + pos[d];
}
// LayerNorm, one wave per row of D <= 1024 floats (D % 4 == 0) held in registers -> f16.  DROP: row b T + t goes to row b (T - 1) + t - 1
// and the class rows (t == 0) are not written.
template <bool DROP>
__global__ __launch_bounds__(256) void dn_ln_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    half_t* __restrict__ out, int M, int T, int D, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  size_t orow = row;
  if (DROP) {
    const int s = row / T, t = row - s * T;
    if (t == 0) return;
    orow = (size_t)s * (T - 1) + t - 1;
  }
  f32x4 v[4];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = i * 256 + lane * 4;
    v[i] = d < D ? ld4(x + (size_t)row * D + d) : f32x4{0.f, 0.f, 0.f, 0.f};
    s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
  }
  const float mean = wave_sum(s) / D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i * 256 + lane * 4 < D) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { const float c = v[i][j] - mean; q += c * c; }
    }
  const float rstd = rsqrtf(wave_sum(q) / D + eps);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = i * 256 + lane * 4;
    if (d >= D) continue;
    const f32x4 gm = ld4(gamma + d), bt = ld4(beta + d);
    store_h4(out + orow * D + d, (v[i][0] - mean) * rstd * gm[0] + bt[0], (v[i][1] - mean) * rstd * gm[1] + bt[1],
             (v[i][2] - mean) * rstd * gm[2] + bt[2], (v[i][3] - mean) * rstd * gm[3] + bt[3]);
  }
}
template <bool DROP>
inline void launch_dn_ln(const float* x, const float* g, const float* b, half_t* out, int M, int T, int D, float eps, hipStream_t st) {
  APH_LAUNCH((dn_ln_kernel<DROP>), dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, x, g, b, out, M, T, D, eps);
}

// bilinear resize with align_corners = True, f16 [B][h][w][C] -> [B][H][W][C] (C % 8 == 0), a thread per 8 channels of an output pixel.
// The source coordinate Y (h - 1) / (H - 1) is split into its integer part and fraction in integer arithmetic: the weights carry one fp32
// rounding (the division), whatever the size.  fp32 blend in torch's order, one rounding to f16.
inline __global__ __launch_bounds__(256) void dn_resize_kernel(const half_t* __restrict__ in, int h, int w, half_t* __restrict__ out, int H, int W, int C, int B) {
  const int c8n = C >> 3;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)B * H * W * c8n) return;
  const int c8 = (int)(idx % c8n);
  size_t r = idx / c8n;
  const int X = (int)(r % W); r /= W;
  const int Y = (int)(r % H);
  const int b = (int)(r / H);
  int y0 = 0, x0 = 0;
  float fy = 0.f, fx = 0.f;
  if (H > 1) { const int ny = Y * (h - 1); y0 = ny / (H - 1); fy = (float)(ny - y0 * (H - 1)) / (float)(H - 1); }
  if (W > 1) { const int nx = X * (w - 1); x0 = nx / (W - 1); fx = (float)(nx - x0 * (W - 1)) / (float)(W - 1); }
  const int y1 = y0 + 1 < h ? y0 + 1 : h - 1, x1 = x0 + 1 < w ? x0 + 1 : w - 1;
  const half_t* base = in + (size_t)b * h * w * C + c8 * 8;
  const half8 a = *reinterpret_cast<const half8*>(base + ((size_t)y0 * w + x0) * C), bq = *reinterpret_cast<const half8*>(base + ((size_t)y0 * w + x1) * C);
  const half8 c = *reinterpret_cast<const half8*>(base + ((size_t)y1 * w + x0) * C), d = *reinterpret_cast<const half8*>(base + ((size_t)y1 * w + x1) * C);
  const float gy = 1.f - fy, gx = 1.f - fx;
  half8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (half_t)(gy * (gx * (float)a[e] + fx * (float)bq[e]) + fy * (gx * (float)c[e] + fx * (float)d[e]));
  *reinterpret_cast<half8*>(out + (((size_t)b * H + Y) * W + X) * C + c8 * 8) = o;
}
inline void launch_dn_resize(const half_t* in, int h, int w, half_t* out, int H, int W, int C, int B, hipStream_t st) {
  const size_t n = (size_t)B * H * W * (C / 8);
  APH_LAUNCH(dn_resize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, h, w, out, H, W, C, B);
}
// out [B][Ho][Wo][C] = in [B][H][W][C] at (2 y, 2 x), Ho = (H + 1) / 2, Wo = (W + 1) / 2: a stride-1 pad-1 3 x 3 convolution followed by this
// IS the stride-2 pad-1 one (the same taps at the same centres, the same sums)
inline __global__ __launch_bounds__(256) void dn_subsample_kernel(const half_t* __restrict__ in, int H, int W, half_t* __restrict__ out, int C, int B) {
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2, c8n = C >> 3;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)B * Ho * Wo * c8n) return;
  const int c8 = (int)(idx % c8n);
  size_t r = idx / c8n;
  const int x = (int)(r % Wo); r /= Wo;
  const int y = (int)(r % Ho);
  const int b = (int)(r / Ho);
  *reinterpret_cast<uint4*>(out + (((size_t)b * Ho + y) * Wo + x) * C + c8 * 8) =
      *reinterpret_cast<const uint4*>(in + (((size_t)b * H + 2 * y) * W + 2 * x) * C + c8 * 8);
}
inline void launch_dn_subsample(const half_t* in, int H, int W, half_t* out, int C, int B, hipStream_t st) {
  const size_t n = (size_t)B * ((H + 1) / 2) * ((W + 1) / 2) * (C / 8);
  APH_LAUNCH(dn_subsample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, H, W, out, C, B);
}
// the head's last 1 x 1 convolution to one channel and its ReLU: depth[i] = max(0, bias + sum_c w[c] in[i][c]), in f16 [n][C] (C % 8 == 0), a
// thread per pixel, the sum in channel order in fp32
inline __global__ __launch_bounds__(256) void dn_head_out_kernel(const half_t* __restrict__ in, const float* __restrict__ w, float bias, float* __restrict__ depth,
                                                                  size_t n, int C) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float acc = bias;
  for (int c = 0; c < C; c += 8) {
    const half8 v = *reinterpret_cast<const half8*>(in + i * C + c);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = fmaf((float)v[e], w[c + e], acc);
  }
  depth[i] = acc > 0.f ? acc : 0.f;
}
// per-image (d - min) / (max - min), in place on depth [B][n]: kMmBlocks partial (min, max) pairs per image, then every block of the second
// kernel reduces its image's pairs again (256 loads) and scales its share.  Deterministic.
constexpr int kMmBlocks = 256;
__device__ __forceinline__ void dn_block_minmax(float& lo, float& hi, float* red) {
#pragma unroll
  for (int msk = 32; msk >= 1; msk >>= 1) { lo = fminf(lo, __shfl_xor(lo, msk)); hi = fmaxf(hi, __shfl_xor(hi, msk)); }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { red[wv] = lo; red[4 + wv] = hi; }
  __syncthreads();
  lo = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
  hi = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
}
inline __global__ __launch_bounds__(256) void dn_minmax_partial_kernel(const float* __restrict__ depth, size_t n, float* __restrict__ part) {
  __shared__ float red[8];
  const float* d = depth + (size_t)blockIdx.y * n;
  float lo = 3.0e38f, hi = -3.0e38f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)kMmBlocks * 256) { const float v = d[i]; lo = fminf(lo, v); hi = fmaxf(hi, v); }
  dn_block_minmax(lo, hi, red);
  if (threadIdx.x == 0) { part[((size_t)blockIdx.y * kMmBlocks + blockIdx.x) * 2] = lo; part[((size_t)blockIdx.y * kMmBlocks + blockIdx.x) * 2 + 1] = hi; }
}
inline __global__ __launch_bounds__(256) void dn_minmax_scale_kernel(float* __restrict__ depth, size_t n, const float* __restrict__ part) {
  __shared__ float red[8];
  float lo = part[((size_t)blockIdx.y * kMmBlocks + threadIdx.x) * 2], hi = part[((size_t)blockIdx.y * kMmBlocks + threadIdx.x) * 2 + 1];
  dn_block_minmax(lo, hi, red);
  float* d = depth + (size_t)blockIdx.y * n;
  const float range = hi - lo;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) d[i] = (d[i] - lo) / range;
}
inline void launch_dn_minmax(float* depth, size_t n, int B, float* part, hipStream_t st) {
  APH_LAUNCH(dn_minmax_partial_kernel, dim3(kMmBlocks, (unsigned)B), dim3(256), 0, st, (const float*)depth, n, part);
  unsigned blocks = (unsigned)((n + 1023) / 1024);
  blocks = blocks > 1024u ? 1024u : blocks;
  APH_LAUNCH(dn_minmax_scale_kernel, dim3(blocks, (unsigned)B), dim3(256), 0, st, depth, n, (const float*)part);
}

}  // namespace depth
}  // namespace aph
