// The LPIPS term's 3x3 convolution (pad 1, stride 1) as an implicit GEMM on v_mfma_f32_16x16x32_f16: ONE kernel for every layer of the
// VGG-16 stack, forward and input gradient.
//   activations  f16, channel-innermost [H][W][C] (C a multiple of 8): the Cin run of one pixel is contiguous, 16 bytes per MFMA k-group
//   weights      f16 [tap][N][C]: the forward copy is [tap][Cout][Cin]; the input gradient is the same convolution over the flipped taps of
//                the transposed weights, a second packed copy [tap'][Cin][Cout] (pack_weights below), so dgrad is this kernel again
//   GEMM view    M = N = the output channels (A operand, 64 per workgroup), the MFMA's n index = 16 output pixels of one image row (B operand),
//                K = 9 * C walked as C / 32 chunks x 9 taps.  With the channels on the MFMA's row index a lane ends up holding four consecutive
//                channels of one pixel: the epilogue stores 8 bytes per lane.
//   workgroup    256 threads, a 16 x 16 pixel tile x 16 NF output channels; wave w owns pixel rows 4 w .. 4 w + 3 (4 NF accumulators of 16 x 16).
//                NF = 4 (64 channels) wherever that fills the chip; the deep stages have few pixel tiles (80 x 45 is 15), so their layers take
//                NF = 2 or 1 and spread over more workgroups instead (launch_conv: halve NF while the grid is under one workgroup per CU).
//                Every output is the same chunk-by-chunk, tap-by-tap sum for any NF: the choice never changes a bit.
//                Per chunk the 18 x 18 pixel input halo (zeros outside the image: the padding) and the 9 x 64 weight rows are staged in LDS, rows
//                of 32 f16 padded to 80 bytes so that the 16 lanes of one ds_read_b128 group fall on 16 distinct 16-byte slots.
//   epilogue     fp32: + bias, ReLU, x (mask > 0) (the ReLU derivative from the stored output of the layer below, dgrad), one rounding to f16;
//                or the first n32 channels as planar fp32 (the last dgrad, into the adjoint of the input scaling).
// A layer whose C is below 32 (the first: 3 channels stored as 8; narrow test networks) takes one zero-padded chunk.
#pragma once
#include <vector>

#include "aph_device.h"
#include "aph_host.h"

namespace aph {
namespace lpips {

constexpr int kTH = 16, kTW = 16;            // output pixel tile
constexpr int kCUs = 256;                    // compute units of the MI355X (the NF rule below)
constexpr int kKC = 32;                      // channels per chunk (one MFMA k-step per tap)
constexpr int kPS = 40;                      // LDS row pitch in f16: 32 + 8 pad (80 bytes)
constexpr int kHaloH = kTH + 2, kHaloW = kTW + 2;
constexpr int kLdsA = kHaloH * kHaloW * kPS;
template <int NF> constexpr size_t conv_smem() { return (size_t)(kLdsA + 9 * NF * 16 * kPS) * sizeof(half_t); }      // NF = 4: 72 000 bytes

struct ConvArgs {
  const half_t* in; int H, W, C;       // input [H][W][C]
  const half_t* wt; int N;             // packed weights [9][N][C], N a multiple of 16
  const float* bias;                   // [N] or null
  int relu;
  const half_t* mask;                  // [H][W][N] or null: the output is zeroed where mask <= 0
  half_t* out;                         // [H][W][N] or null
  float* out32; int n32;               // planar [n32][H][W] (channels < n32) or null
  // read by the X instantiation alone (conv3x3_kernel<NF, true>, the depth estimator's convolutions): blockIdx.z = the image of a batch
  int relu_in = 0;                     // ReLU on the input as it is staged (the pre-activation of a residual unit)
  const half_t* res = nullptr;         // [H][W][N] or null: added in fp32 after bias / ReLU, before the one rounding
  const half_t* res2 = nullptr;        // a second such term
  int batch = 1;                       // images; in, res, res2, out advance by H W C / H W N per image (mask, out32: not with a batch)
};

// X = false: the LPIPS term's kernel, exactly as it was.  X = true adds what the fields after n32 say, and nothing to the sums: the same
// chunk-by-chunk, tap-by-tap accumulation.
template <int NF, bool X = false>
static __global__ __launch_bounds__(256, 2) void conv3x3_kernel(ConvArgs a) {
  constexpr int kNT = NF * 16;                                     // output channels per workgroup
  if constexpr (X) {
    const size_t bi = (size_t)blockIdx.z * a.H * a.W * a.C, bo = (size_t)blockIdx.z * a.H * a.W * a.N;
    a.in += bi;
    if (a.out) a.out += bo;
    if (a.res) a.res += bo;
    if (a.res2) a.res2 += bo;
  }
  APH_DYN_SMEM(smem);
  half_t* sA = reinterpret_cast<half_t*>(smem);
  half_t* sB = sA + kLdsA;
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int tiles_x = (a.W + kTW - 1) / kTW;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x0 = tx * kTW, y0 = ty * kTH, n0 = blockIdx.y * kNT;
  const int nfrag = (a.N - n0) >= kNT ? NF : (a.N - n0) / 16;      // 16-channel fragments of this workgroup that exist

  f32x4 acc[NF][4];
#pragma unroll
  for (int cf = 0; cf < NF; ++cf)
#pragma unroll
    for (int pr = 0; pr < 4; ++pr) acc[cf][pr] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int c0 = 0; c0 < a.C; c0 += kKC) {
    __syncthreads();                                                // the previous chunk's fragment reads are done
    for (int i = tid; i < kHaloH * kHaloW * 4; i += 256) {
      const int v = i & 3, p = i >> 2, hy = p / kHaloW, hx = p - hy * kHaloW;
      const int y = y0 + hy - 1, x = x0 + hx - 1, c = c0 + v * 8;
      uint4 val = make_uint4(0u, 0u, 0u, 0u);
      if (y >= 0 && y < a.H && x >= 0 && x < a.W && c < a.C) val = *reinterpret_cast<const uint4*>(a.in + ((size_t)y * a.W + x) * a.C + c);
      if constexpr (X) {
        if (a.relu_in) {
          half8 h = *reinterpret_cast<const half8*>(&val);
#pragma unroll
          for (int e = 0; e < 8; ++e) h[e] = h[e] > (half_t)0.f ? h[e] : (half_t)0.f;
          val = *reinterpret_cast<const uint4*>(&h);
        }
      }
      *reinterpret_cast<uint4*>(sA + p * kPS + v * 8) = val;
    }
    for (int i = tid; i < 9 * kNT * 4; i += 256) {
      const int v = i & 3, r = i >> 2, t = r / kNT, n = n0 + r - t * kNT, c = c0 + v * 8;
      uint4 val = make_uint4(0u, 0u, 0u, 0u);
      if (n < a.N && c < a.C) val = *reinterpret_cast<const uint4*>(a.wt + ((size_t)t * a.N + n) * a.C + c);
      *reinterpret_cast<uint4*>(sB + r * kPS + v * 8) = val;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int dy = t / 3, dx = t - dy * 3;
      half8 wf[NF];
#pragma unroll
      for (int cf = 0; cf < NF; ++cf) wf[cf] = *reinterpret_cast<const half8*>(sB + (t * kNT + cf * 16 + li) * kPS + lg * 8);
#pragma unroll
      for (int pr = 0; pr < 4; ++pr) {
        const half8 xf = *reinterpret_cast<const half8*>(sA + ((wave * 4 + pr + dy) * kHaloW + li + dx) * kPS + lg * 8);
#pragma unroll
        for (int cf = 0; cf < NF; ++cf)
          if (cf < nfrag) acc[cf][pr] = mfma_16x16x32_f16(wf[cf], xf, acc[cf][pr]);
      }
    }
  }

  // lane (li, lg), fragment cf, row pr: channels n0 + 16 cf + 4 lg + (0 .. 3) of pixel (y0 + 4 wave + pr, x0 + li)
  const int x = x0 + li;
#pragma unroll
  for (int pr = 0; pr < 4; ++pr) {
    const int y = y0 + wave * 4 + pr;
    if (y >= a.H || x >= a.W) continue;
    const size_t pix = (size_t)y * a.W + x;
#pragma unroll
    for (int cf = 0; cf < NF; ++cf) {
      if (cf >= nfrag) continue;
      const int n = n0 + cf * 16 + lg * 4;
      f32x4 v = acc[cf][pr];
      if (a.bias) { v[0] += a.bias[n]; v[1] += a.bias[n + 1]; v[2] += a.bias[n + 2]; v[3] += a.bias[n + 3]; }
      if (a.relu) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = v[r] > 0.f ? v[r] : 0.f;
      }
      if (a.mask) {
        const half4 m = *reinterpret_cast<const half4*>(a.mask + pix * a.N + n);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = (float)m[r] > 0.f ? v[r] : 0.f;
      }
      if constexpr (X) {
        if (a.res) {
          const half4 q = *reinterpret_cast<const half4*>(a.res + pix * a.N + n);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += (float)q[r];
        }
        if (a.res2) {
          const half4 q = *reinterpret_cast<const half4*>(a.res2 + pix * a.N + n);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += (float)q[r];
        }
      }
      if (a.out) {
        half4 h;
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = (half_t)v[r];
        *reinterpret_cast<half4*>(a.out + pix * a.N + n) = h;
      }
      if (a.out32) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n + r < a.n32) a.out32[(size_t)(n + r) * a.H * a.W + pix] = v[r];
      }
    }
  }
}

template <int NF, bool X = false>
static inline void launch_conv_nf(const ConvArgs& a, unsigned tiles, hipStream_t st) {
  APH_ALLOW_SMEM((conv3x3_kernel<NF, X>), conv_smem<NF>());
  APH_LAUNCH((conv3x3_kernel<NF, X>), dim3(tiles, (unsigned)((a.N + NF * 16 - 1) / (NF * 16)), X ? (unsigned)a.batch : 1u), dim3(256), conv_smem<NF>(), st, a);
}
// nf: 16-channel fragments per workgroup, 4 / 2 / 1; 0 = the rule: 4, halved while the channels fit in half of it or the grid has fewer
// workgroups than the chip has CUs
template <bool X = false>
static inline void launch_conv(const ConvArgs& a, hipStream_t st, int nf = 0) {
  const unsigned tiles = (unsigned)(((a.W + kTW - 1) / kTW) * ((a.H + kTH - 1) / kTH));
  if (nf == 0) {
    const unsigned images = X ? (unsigned)a.batch : 1u;
    nf = 4;
    while (nf > 1 && (16 * (nf / 2) >= a.N || images * tiles * (unsigned)((a.N + 16 * nf - 1) / (16 * nf)) < (unsigned)kCUs)) nf >>= 1;
  }
  if (nf >= 4) launch_conv_nf<4, X>(a, tiles, st);
  else if (nf == 2) launch_conv_nf<2, X>(a, tiles, st);
  else launch_conv_nf<1, X>(a, tiles, st);
}

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// torch weight [cout][cin][3][3] (fp32, host) -> the packed f16 operand of conv3x3_kernel.
//   forward (dgrad == 0): [tap][cout][C],  C = cin rounded up to 8,  element (t, o, i) = w[o][i][t]
//   dgrad   (dgrad == 1): [tap][N][cout],  N = cin rounded up to 16, element (t, i, o) = w[o][i][8 - t]   (both taps flipped)
// pad rows / columns are zero.
static inline std::vector<half_t> pack_weights(const float* w, int cout, int cin, int dgrad) {
  const int N = dgrad ? round_up(cin, 16) : cout, C = dgrad ? cout : round_up(cin, 8);
  std::vector<half_t> p((size_t)9 * N * C, (half_t)0.f);
  for (int t = 0; t < 9; ++t)
    for (int o = 0; o < cout; ++o)
      for (int i = 0; i < cin; ++i) {
        const float v = w[((size_t)o * cin + i) * 9 + (dgrad ? 8 - t : t)];
        if (dgrad) p[((size_t)t * N + i) * C + o] = (half_t)v;
        else p[((size_t)t * N + o) * C + i] = (half_t)v;
      }
  return p;
}

}  // namespace lpips
}  // namespace aph
