// Inverse 2-D discrete wavelet transform and its adjoint.
//
// Replaces: pytorch_wavelets DWTInverse(wave, mode='symmetric') as called by aphantasia/image.py:36-38,67
// (dwt_image.inner), i.e. per level  lowlevel.SFB2D:
//     lo = sfb1d(ll, LH, dim H);  hi = sfb1d(HL, HH, dim H);  out = sfb1d(lo, hi, dim W)
//     sfb1d(a, b)[m] = full[m + L - 2],  full[2 i + k] += a[i] rec_lo[k] + b[i] rec_hi[k]     (length 2 n - L + 2)
// The per-level detail gain of dwt_scale (image.py:73-80) is folded in as `hscale`.
// HBM-bound (the finest level of a 4K image moves ~200 MB); each workgroup stages the input patch of its
// output tile in LDS once and every coefficient / pixel is read from HBM exactly once.  One launch per level for the
// levels that fill the chip; the coarse tail (every level whose output is a single tile) runs in ONE launch, a
// workgroup per channel walking the levels (aph_idwt_fwd / aph_idwt_bwd).
//
// Each filter sum is written once and called by the per-level tile and by the coarse-tail kernel: idwt_hpass / idwt_vpass
// (forward), idwt_adjoint_hpass / idwt_adjoint_vpass (adjoint); the callers differ in addressing and in where the gain is
// applied only.  Every kernel and tile takes the filter length LT as its template argument (0: run-time length);
// idwt_for_length is the one place that maps a run-time L to an instantiation, idwt_geom the one that does a level's sizes.
#include "aph_device.h"
#include "aph_host.h"

#include <cstdlib>
#include <type_traits>

namespace aph {

constexpr int DW_TY = 32, DW_TX = 128, DW_NT = 256;    // forward: output tile (rows x cols) per workgroup of the per-level kernel
constexpr int DW_IY = 16, DW_IX = 64;                  // adjoint: coefficient tile per workgroup
constexpr int DC_TY = 80, DC_TX = 128, DC_NT = 1024;   // coarse-tail kernels: one tile holds a whole level (out <= 80 x 128)
constexpr int DC_IY = 40, DC_IX = 64;                  //   adjoint: coefficient tile <= 40 x 64
constexpr int DC_MAX_LEVELS = 12;
constexpr int DC_HS_MAX = 12 * DC_NT;                  // detail-band values of all coarse levels together (one prefetch batch: 12 per thread)

// output length of one sfb1d: n coefficients, filter length L
__host__ __device__ constexpr int idwt_out(int n, int L) { return 2 * n - L + 2; }

// ---- the filter sums (LT = filter length at compile time, 0: the run-time L) ----------------------------------------------------
// rec_lo / rec_hi into LDS
template <int NT>
__device__ __forceinline__ void idwt_stage_taps(float* f0, float* f1, const float* g0, const float* g1, int L) {
  for (int k = threadIdx.x; k < L; k += NT) { f0[k] = g0[k]; f1[k] = g1[k]; }
}

// forward, horizontal: outputs 2j and 2j+1 read the same L/2 inputs i = j + L/2 - 1 - t with the even / odd filter taps:
// lo = g0 * ll + g1 * HL, hi = g0 * LH + g1 * HH.  in(t) returns that input's (ll, LH, HL, HH), detail bands with their gain.
template <int LT, class In>
__device__ __forceinline__ void idwt_hpass(const float* f0, const float* f1, int L, In in, float* lo, float* hi) {
  float lo_e = 0.f, lo_o = 0.f, hi_e = 0.f, hi_o = 0.f;
#pragma unroll
  for (int t = 0; t < (LT ? LT : L) / 2; ++t) {
    const float a_e = f0[2 * t], a_o = f0[2 * t + 1], b_e = f1[2 * t], b_o = f1[2 * t + 1];
    const float4 v = in(t);
    const float vll = v.x, vlh = v.y, vhl = v.z, vhh = v.w;
    lo_e += a_e * vll + b_e * vhl; lo_o += a_o * vll + b_o * vhl;
    hi_e += a_e * vlh + b_e * vhh; hi_o += a_o * vlh + b_o * vhh;
  }
  *reinterpret_cast<float2*>(lo) = make_float2(lo_e, lo_o);      // (8-byte aligned at every caller)
  *reinterpret_cast<float2*>(hi) = make_float2(hi_e, hi_o);
}

// forward, vertical: out = g0 * rlo + g1 * rhi for the output row pair (even, odd); rlo / rhi point at input row (rl + L/2 - 1),
// rows `pitch` apart.  V = float: one column; V = float4: four columns (16-byte LDS reads), the same sum in each component.
// (The float4 operands go by value and the sums live in locals: through references the L = 6 kernel took 98 VGPRs instead of 60.)
__device__ __forceinline__ void idwt_mac2(float& o, float a, float lo, float b, float hi) { o += a * lo + b * hi; }
__device__ __forceinline__ void idwt_mac2(float4& o, float a, float4 lo, float b, float4 hi) {
  o.x += a * lo.x + b * hi.x; o.y += a * lo.y + b * hi.y; o.z += a * lo.z + b * hi.z; o.w += a * lo.w + b * hi.w;
}
template <int LT, class V>
__device__ __forceinline__ void idwt_vpass(const float* f0, const float* f1, int L, const float* rlo, const float* rhi, int pitch, V& r_e, V& r_o) {
  V o_e = V(), o_o = o_e;
#pragma unroll
  for (int t = 0; t < (LT ? LT : L) / 2; ++t) {
    const V lo = *reinterpret_cast<const V*>(rlo - t * pitch), hi = *reinterpret_cast<const V*>(rhi - t * pitch);
    const float a_e = f0[2 * t], a_o = f0[2 * t + 1], b_e = f1[2 * t], b_o = f1[2 * t + 1];
    idwt_mac2(o_e, a_e, lo, b_e, hi);
    idwt_mac2(o_o, a_o, lo, b_o, hi);
  }
  r_e = o_e; r_o = o_o;
}

// adjoint, horizontal: slo = sum_k g0[k] d[2 ix + k], shi with g1.  in(t) returns (d[2 ix + 2 t], d[2 ix + 2 t + 1]), 0 outside.
template <int LT, class In>
__device__ __forceinline__ void idwt_adjoint_hpass(const float* f0, const float* f1, int L, In in, float* slo, float* shi) {
  float a = 0.f, b = 0.f;
#pragma unroll
  for (int t = 0; t < (LT ? LT : L) / 2; ++t) {
    const float2 v = in(t);
    a += f0[2 * t] * v.x; a += f0[2 * t + 1] * v.y;
    b += f1[2 * t] * v.x; b += f1[2 * t + 1] * v.y;
  }
  *slo = a;
  *shi = b;
}

// adjoint, vertical: (dll, dLH, dHL, dHH) = (sum g0 slo, sum g1 slo, sum g0 shi, sum g1 shi) over rows 2 iyl + k of column ixl
template <int LT>
__device__ __forceinline__ float4 idwt_adjoint_vpass(const float* f0, const float* f1, int L, const float* slo, const float* shi, int iyl, int ixl, int pitch) {
  float all = 0.f, alh = 0.f, ahl = 0.f, ahh = 0.f;
#pragma unroll
  for (int k = 0; k < (LT ? LT : L); ++k) {
    const int e = (2 * iyl + k) * pitch + ixl;
    const float lo = slo[e], hi = shi[e];
    all += f0[k] * lo; alh += f1[k] * lo;
    ahl += f0[k] * hi; ahh += f1[k] * hi;
  }
  return make_float4(all, alh, ahl, ahh);
}
// the detail-band gradients of idwt_adjoint_vpass, with the level's gain, into [3][h][w] at oh
__device__ __forceinline__ void idwt_store_highs(float* oh, int h, int w, const float4& a, float hscale) {
  oh[0] = a.y * hscale;
  oh[(size_t)h * w] = a.z * hscale;
  oh[2 * (size_t)h * w] = a.w * hscale;
}

// Forward tile, separable in LDS: a TY x TX output tile of one channel by NT threads.
//   1. the four band patches [PY][PX] (PY = TY/2 + L/2 input rows, PX likewise; zero beyond h / w) are loaded once --
//      with a compile-time filter length EVERY load of the patch is issued before the first LDS write (one memory round
//      trip per tile; the row loop this replaces waited for memory once per 64 columns of a row, ten times per wave, and
//      a workgroup's lifetime was those waits: 3.3 TB/s on the finest 4K level);
//   2. horizontal pass (idwt_hpass), one thread per (patch row, output column PAIR);
//   3. vertical pass (idwt_vpass): four columns of a row pair per thread (16-byte LDS reads and stores) when the output rows
//      are 16-byte aligned, else one column per thread.
// bll: [llh][llw] (only rows < h / cols < w are used -- the "unpad" of DWTInverse.forward), bh: [3][h][w] (LH, HL, HH),
// bout: [Ho][Wo], Ho = idwt_out(h), Wo = idwt_out(w) -- all of ONE channel.
// No __restrict__: the coarse-tail kernel reads what its previous level wrote.
template <int LT, int TY, int TX, int NT>
__device__ __forceinline__ void idwt_tile(char* smem, const float* bll, int llw, const float* bh, int h, int w, const float* g0,
                                          const float* g1, int L, float hscale, float* bout, int Ho, int Wo, int my0, int mx0) {
  const int H2 = LT ? LT / 2 : (L >> 1);
  const int PY = TY / 2 + H2, PX = TX / 2 + H2;
  float* f0 = reinterpret_cast<float*>(smem);  // rec_lo
  float* f1 = f0 + 2 * H2;                     // rec_hi
  float* pll = f1 + 2 * H2;                    // 4 band patches [PY][PX]
  float* plh = pll + PY * PX;
  float* phl = plh + PY * PX;
  float* phh = phl + PY * PX;
  float* rlo = phh + PY * PX;                  // [PY][TX]
  float* rhi = rlo + PY * TX;
  const int tid = threadIdx.x;
  // output m = 2 j + p (p = 0, 1) reads inputs i = j + H2 - 1 - t with tap k = p + 2 t;  the tile's first input is m0 / 2
  const int iy0 = my0 / 2, ix0 = mx0 / 2;
  if constexpr (LT > 0) {
    constexpr int PYc = TY / 2 + LT / 2, PXc = TX / 2 + LT / 2, NQ = PYc * PXc, NIT = (NQ + NT - 1) / NT;
    float v[NIT][4];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int q = it * NT + tid;
      const int py = q / PXc, px = q - py * PXc;
      const int iy = iy0 + py, ix = ix0 + px;
      const bool ok = q < NQ && iy < h && ix < w;
      const size_t o = ok ? (size_t)iy * w + ix : 0, oll = ok ? (size_t)iy * llw + ix : 0;      // (element 0 always exists)
      v[it][0] = bll[oll];
      v[it][1] = bh[o];
      v[it][2] = bh[(size_t)h * w + o];
      v[it][3] = bh[2 * (size_t)h * w + o];
    }
    idwt_stage_taps<NT>(f0, f1, g0, g1, 2 * H2);      // (behind the patch loads: same round trip)
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int q = it * NT + tid;
      const int py = q / PXc, px = q - py * PXc;
      const bool ok = iy0 + py < h && ix0 + px < w;
      if (q < NQ) {
        pll[q] = ok ? v[it][0] : 0.f;
        plh[q] = ok ? v[it][1] * hscale : 0.f;
        phl[q] = ok ? v[it][2] * hscale : 0.f;
        phh[q] = ok ? v[it][3] * hscale : 0.f;
      }
    }
  } else {
    const int lane = tid & 63, wave = tid >> 6;
    idwt_stage_taps<NT>(f0, f1, g0, g1, 2 * H2);
    for (int py = wave; py < PY; py += NT / 64) {
      const int iy = iy0 + py;
      for (int px = lane; px < PX; px += 64) {
        const int ix = ix0 + px;
        const bool ok = iy < h && ix < w;
        const size_t o = (size_t)iy * w + ix;
        const int q = py * PX + px;
        pll[q] = ok ? bll[(size_t)iy * llw + ix] : 0.f;
        plh[q] = ok ? bh[o] * hscale : 0.f;
        phl[q] = ok ? bh[(size_t)h * w + o] * hscale : 0.f;
        phh[q] = ok ? bh[2 * (size_t)h * w + o] * hscale : 0.f;
      }
    }
  }
  __syncthreads();
  for (int q = tid; q < PY * (TX / 2); q += NT) {
    const int py = q / (TX / 2), jl = q - py * (TX / 2);
    const int e0 = py * PX + jl + H2 - 1;
    idwt_hpass<LT>(f0, f1, L, [&](int t) { return make_float4(pll[e0 - t], plh[e0 - t], phl[e0 - t], phh[e0 - t]); },
                   rlo + py * TX + 2 * jl, rhi + py * TX + 2 * jl);
  }
  __syncthreads();
  if (((Wo & 3) | (int)(reinterpret_cast<size_t>(bout) & 15)) == 0) {
    // (the finest level of a 4K image, Wo = 3840, is three quarters of the transform's bytes)
    for (int q = tid; q < (TY / 2) * (TX / 4); q += NT) {
      const int rl = q / (TX / 4), c4 = q - rl * (TX / 4), my = my0 + 2 * rl, mx = mx0 + 4 * c4;
      const int e0 = (rl + H2 - 1) * TX + 4 * c4;
      float4 o_e, o_o;
      idwt_vpass<LT>(f0, f1, L, rlo + e0, rhi + e0, TX, o_e, o_o);
      if (mx < Wo) {
        if (my < Ho) *reinterpret_cast<float4*>(bout + (size_t)my * Wo + mx) = o_e;
        if (my + 1 < Ho) *reinterpret_cast<float4*>(bout + (size_t)(my + 1) * Wo + mx) = o_o;
      }
    }
  } else {
    for (int q = tid; q < (TY / 2) * TX; q += NT) {
      const int rl = q / TX, tx_ = q - rl * TX, my = my0 + 2 * rl, mx = mx0 + tx_;
      const int e0 = (rl + H2 - 1) * TX + tx_;
      float o_e, o_o;
      idwt_vpass<LT>(f0, f1, L, rlo + e0, rhi + e0, TX, o_e, o_o);
      if (mx < Wo) {
        if (my < Ho) bout[(size_t)my * Wo + mx] = o_e;
        if (my + 1 < Ho) bout[(size_t)(my + 1) * Wo + mx] = o_o;
      }
    }
  }
}
template <int TY, int TX>
constexpr size_t idwt_tile_smem(int L) { return sizeof(float) * (2 * L + 4 * (TY / 2 + L / 2) * (TX / 2 + L / 2) + 2 * (TY / 2 + L / 2) * TX); }

// ll: [C][llh][llw], highs: [C][3][h][w], out: [C][Ho][Wo]; one DW_TY x DW_TX output tile of one channel per workgroup
template <int LT>
__global__ __launch_bounds__(DW_NT) void idwt_level_kernel(const float* __restrict__ ll, int llh, int llw,
                                                           const float* __restrict__ highs, int h, int w, const float* __restrict__ g0,
                                                           const float* __restrict__ g1, int L, float hscale, float* __restrict__ out,
                                                           int Ho, int Wo) {
  APH_DYN_SMEM(smem);
  const int c = blockIdx.z;
  idwt_tile<LT, DW_TY, DW_TX, DW_NT>(smem, ll + (size_t)c * llh * llw, llw, highs + (size_t)c * 3 * h * w, h, w, g0, g1, L, hscale,
                                     out + (size_t)c * Ho * Wo, Ho, Wo, blockIdx.y * DW_TY, blockIdx.x * DW_TX);
}

// Adjoint tile, separable in LDS: bdout [Ho][Wo] -> bdll [llh][llw] (extra unpadded row/col = 0) and bdh [3][h][w]
// (x hscale), one channel.  Coefficient i touches outputs m = 2 i + k - (L - 2), k in [0, L).  Per IY x IX tile:
//   1. dout patch [PY][PX], PY = 2 IY + L - 2 (all loads in flight together, as in idwt_tile);
//   2. horizontal (idwt_adjoint_hpass): slo[y][ix], shi[y][ix] -> LDS [2][PY][IX];
//   3. vertical (idwt_adjoint_vpass): dll, dLH, dHL, dHH.
template <int LT, int IY, int IX, int NT>
__device__ __forceinline__ void idwt_adjoint_tile(char* smem, const float* bd, int Ho, int Wo, int h, int w, const float* g0,
                                                  const float* g1, int L_, float hscale, float* bdll, int llh, int llw, float* bdh,
                                                  int iy0, int ix0) {
  const int L = LT ? LT : L_;
  const int PY = 2 * IY + L - 2, PX = 2 * IX + L - 2;
  float* f0 = reinterpret_cast<float*>(smem);
  float* f1 = f0 + L;
  float* pd = f1 + L;                          // [PY][PX]
  float* slo = pd + PY * PX;                   // [PY][IX]
  float* shi = slo + PY * IX;
  const int tid = threadIdx.x;
  const int my0 = 2 * iy0 - (L - 2), mx0 = 2 * ix0 - (L - 2);
  if constexpr (LT > 0) {
    constexpr int PYc = 2 * IY + LT - 2, PXc = 2 * IX + LT - 2, NQ = PYc * PXc, NIT = (NQ + NT - 1) / NT;
    float v[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int q = it * NT + tid;
      const int py = q / PXc, px = q - py * PXc;
      const int my = my0 + py, mx = mx0 + px;
      const bool ok = q < NQ && my >= 0 && my < Ho && mx >= 0 && mx < Wo;
      v[it] = bd[ok ? (size_t)my * Wo + mx : 0];
    }
    idwt_stage_taps<NT>(f0, f1, g0, g1, L);
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int q = it * NT + tid;
      const int py = q / PXc, px = q - py * PXc;
      const int my = my0 + py, mx = mx0 + px;
      if (q < NQ) pd[q] = (my >= 0 && my < Ho && mx >= 0 && mx < Wo) ? v[it] : 0.f;
    }
  } else {
    const int lane = tid & 63, wave = tid >> 6;
    idwt_stage_taps<NT>(f0, f1, g0, g1, L);
    for (int py = wave; py < PY; py += NT / 64) {
      const int my = my0 + py;
      const bool rowok = my >= 0 && my < Ho;
      for (int px = lane; px < PX; px += 64) {
        const int mx = mx0 + px;
        pd[py * PX + px] = (rowok && mx >= 0 && mx < Wo) ? bd[(size_t)my * Wo + mx] : 0.f;
      }
    }
  }
  __syncthreads();
  for (int q = tid; q < PY * IX; q += NT) {
    const int py = q / IX, ixl = q - py * IX;
    const float2* row = reinterpret_cast<const float2*>(pd + py * PX + 2 * ixl);      // 8-byte aligned: PX and 2 L are even
    idwt_adjoint_hpass<LT>(f0, f1, L, [&](int t) { return row[t]; }, slo + q, shi + q);
  }
  __syncthreads();
  for (int q = tid; q < IY * IX; q += NT) {
    const int iyl = q / IX, ixl = q - iyl * IX, iy = iy0 + iyl, ix = ix0 + ixl;
    if (iy >= llh || ix >= llw) continue;
    float* ol = bdll + (size_t)iy * llw + ix;
    if (iy >= h || ix >= w) { *ol = 0.f; continue; }      // the row / column DWTInverse drops
    const float4 a = idwt_adjoint_vpass<LT>(f0, f1, L, slo, shi, iyl, ixl, IX);
    *ol = a.x;
    idwt_store_highs(bdh + (size_t)iy * w + ix, h, w, a, hscale);
  }
}
template <int IY, int IX>
constexpr size_t idwt_adjoint_tile_smem(int L) { return sizeof(float) * (2 * L + (2 * IY + L - 2) * (2 * IX + L - 2) + 2 * (2 * IY + L - 2) * IX); }

template <int LT>
__global__ __launch_bounds__(DW_NT) void idwt_level_adjoint_kernel(const float* __restrict__ dout, int Ho, int Wo, int h, int w,
                                                                   const float* __restrict__ g0, const float* __restrict__ g1, int L_,
                                                                   float hscale, float* __restrict__ dll, int llh, int llw,
                                                                   float* __restrict__ dhighs) {
  APH_DYN_SMEM(smem);
  const int c = blockIdx.z;
  idwt_adjoint_tile<LT, DW_IY, DW_IX, DW_NT>(smem, dout + (size_t)c * Ho * Wo, Ho, Wo, h, w, g0, g1, L_, hscale, dll + (size_t)c * llh * llw,
                                             llh, llw, dhighs + (size_t)c * 3 * h * w, blockIdx.y * DW_IY, blockIdx.x * DW_IX);
}

// ---- coarse tail: the levels whose bands fit the LDS, one workgroup per channel walking them -----------------------------------
// (eight such levels under a 4K db3 image were eight launches of 3 workgroups each, 6 us apiece of pure latency; a first fused
// version that still went through global memory between levels -- load, fence, barrier -- cost 4.7 us per level, hardly less.)
// Here nothing but the first level's low band, every level's detail bands (all requested up front: one memory round trip for the
// whole tail) and the last level's output touches global memory: the running low band stays in LDS between levels.  Whole levels
// need no zero padding: output pair jl reads inputs jl .. jl + L/2 - 1 <= w - 1, rows likewise.
struct IdwtLevel {                // forward: ll, highs -> out.  adjoint: out = incoming gradient, ll / highs = gradients written
  float* ll; float* highs; float* out;
  int llh, llw, h, w;
  float hscale;
  int hoff;                       // forward: offset (floats) of this level's detail bands in the LDS prefetch area
  int hdelta;                     // forward: highs - (the first level's highs), in floats (the host checks that it fits)
};
struct IdwtLevels { int n; IdwtLevel lv[DC_MAX_LEVELS]; };      // in execution order

constexpr int DC_LL = DC_TY * DC_TX;                  // running low band / incoming gradient, floats
constexpr int DC_R = DC_IY * DC_TX;                   // forward: one horizontal-pass plane [h <= DC_IY][Wo <= DC_TX]
inline size_t idwt_coarse_smem(int L, int hsum) { return sizeof(float) * (2 * L + DC_LL + 2 * DC_R + hsum); }
inline size_t idwt_coarse_adjoint_smem(int L) { return sizeof(float) * (2 * L + DC_LL + DC_IY * DC_IX + 2 * (2 * DC_IY + L - 2) * DC_IX); }

template <int LT>
__global__ __launch_bounds__(DC_NT) void idwt_coarse_kernel(IdwtLevels lv, const float* __restrict__ g0, const float* __restrict__ g1, int L) {
  APH_DYN_SMEM(smem);
  constexpr int H2 = LT / 2;
  float* f0 = reinterpret_cast<float*>(smem);
  float* f1 = f0 + 2 * H2;
  float* LL = f1 + 2 * H2;             // running low band, row pitch `pitch`
  float* rlo = LL + DC_LL;             // [h][Wo]
  float* rhi = rlo + DC_R;
  float* HS = rhi + DC_R;              // every level's (LH, HL, HH)
  const int c = blockIdx.x, tid = threadIdx.x;
  // everything the tail reads from global memory, requested before the first LDS write: the coarsest low band (<= DC_IY x DC_IX:
  // three values per thread) and the detail bands of all levels as ONE flat index space (HS is laid out in level order, so the
  // level of element q is the last one whose hoff <= q: a chain of selects over the level table, which sits in scalar registers)
  constexpr int NLL = (DC_IY * DC_IX + DC_NT - 1) / DC_NT, NB = DC_HS_MAX / DC_NT;
  float wll[NLL];
  {
    const IdwtLevel& l0 = lv.lv[0];
    const int n0 = l0.llh * l0.llw;
    const float* src = l0.ll + (size_t)c * n0;
#pragma unroll
    for (int u = 0; u < NLL; ++u) { const int q = u * DC_NT + tid; wll[u] = src[q < n0 ? q : 0]; }
  }
  const int hsum = lv.lv[lv.n - 1].hoff + 3 * lv.lv[lv.n - 1].h * lv.lv[lv.n - 1].w;      // <= DC_HS_MAX (idwt_coarse_count)
  {
    // element q of HS belongs to the last level whose hoff <= q; its address is (first level's highs) + q + d_k with
    // d_k = hdelta_k + c * 3 h_k w_k - hoff_k.  The level table is read at compile-time indices (scalar registers, loaded once):
    // per element one compare + select per level.  (A run-time loop over the table cost a dependent scalar load per level and
    // element: 10 us of the kernel's 22.)
    const float* h0 = lv.lv[0].highs;
    int dk[DC_MAX_LEVELS], ho[DC_MAX_LEVELS];       // (wave-uniform: scalar registers; an unused slot never matches)
#pragma unroll
    for (int k = 0; k < DC_MAX_LEVELS; ++k) {
      const bool on = k < lv.n;
      ho[k] = on ? lv.lv[k].hoff : 0x7fffffff;
      dk[k] = on ? lv.lv[k].hdelta + c * 3 * lv.lv[k].h * lv.lv[k].w - lv.lv[k].hoff : 0;
    }
    float v[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int q = u * DC_NT + tid, qc = q < hsum ? q : 0;
      int d = dk[0];
#pragma unroll
      for (int k = 1; k < DC_MAX_LEVELS; ++k) d = qc >= ho[k] ? dk[k] : d;
      v[u] = h0[(ptrdiff_t)d + qc];
    }
    idwt_stage_taps<DC_NT>(f0, f1, g0, g1, 2 * H2);
    const int n0 = lv.lv[0].llh * lv.lv[0].llw;
#pragma unroll
    for (int u = 0; u < NLL; ++u) { const int q = u * DC_NT + tid; if (q < n0) LL[q] = wll[u]; }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int q = u * DC_NT + tid;
      if (q < hsum) HS[q] = v[u];       // (unscaled: the level's gain is applied where the value is used)
    }
  }
  __syncthreads();
  int pitch = lv.lv[0].llw;
  for (int i = 0; i < lv.n; ++i) {
    const IdwtLevel& l = lv.lv[i];
    const int h = l.h, w = l.w, Ho = idwt_out(h, L), Wo = idwt_out(w, L), W2 = Wo >> 1;
    const float hsc = l.hscale;
    const float* Hlh = HS + l.hoff;
    const float* Hhl = Hlh + h * w;
    const float* Hhh = Hhl + h * w;
    for (int q = tid; q < h * W2; q += DC_NT) {
      const int py = q / W2, jl = q - py * W2;
      const int e0 = jl + H2 - 1;
      const float* rll = LL + py * pitch;
      const float* rlh = Hlh + py * w;
      const float* rhl = Hhl + py * w;
      const float* rhh = Hhh + py * w;
      idwt_hpass<LT>(f0, f1, L, [&](int t) { return make_float4(rll[e0 - t], rlh[e0 - t] * hsc, rhl[e0 - t] * hsc, rhh[e0 - t] * hsc); },
                     rlo + py * Wo + 2 * jl, rhi + py * Wo + 2 * jl);      // (8-byte aligned: Wo is even)
    }
    __syncthreads();
    // vertical pass: the level's output is the next level's low band (row pitch Wo); only the last one leaves the CU
    const bool last = i + 1 == lv.n;
    float* gout = l.out + (size_t)c * Ho * Wo;
    for (int q = tid; q < (Ho >> 1) * Wo; q += DC_NT) {
      const int rl = q / Wo, x = q - rl * Wo;
      const int e0 = (rl + H2 - 1) * Wo + x;
      float o_e, o_o;
      idwt_vpass<LT>(f0, f1, L, rlo + e0, rhi + e0, Wo, o_e, o_o);
      LL[2 * rl * Wo + x] = o_e;
      LL[(2 * rl + 1) * Wo + x] = o_o;
      if (last) { gout[(size_t)2 * rl * Wo + x] = o_e; gout[(size_t)(2 * rl + 1) * Wo + x] = o_o; }
    }
    __syncthreads();
    pitch = Wo;
  }
}

// adjoint of the coarse tail, finest of its levels first: the incoming gradient is read from global memory once, each level's
// low-band gradient stays in LDS as the next level's input, the detail-band gradients (and the coarsest low band's) are stored.
template <int LT>
__global__ __launch_bounds__(DC_NT) void idwt_coarse_adjoint_kernel(IdwtLevels lv, const float* __restrict__ g0, const float* __restrict__ g1, int L_) {
  APH_DYN_SMEM(smem);
  constexpr int L = LT;
  float* f0 = reinterpret_cast<float*>(smem);
  float* f1 = f0 + L;
  float* DA = f1 + L;                  // the level's incoming gradient [Ho][Wo]
  float* DB = DA + DC_LL;              // its low-band gradient [llh][llw] = the next level's incoming gradient (the two swap)
  float* slo = DB + DC_IY * DC_IX;     // [PY = 2 llh + L - 2][llw]
  float* shi = slo + (2 * DC_IY + L - 2) * DC_IX;
  const int c = blockIdx.x, tid = threadIdx.x;
  {
    // the tail's only read from global memory: the first level's incoming gradient (<= DC_TY x DC_TX), all loads in flight together
    constexpr int NA = (DC_LL + DC_NT - 1) / DC_NT;
    const IdwtLevel& l0 = lv.lv[0];
    const int n0 = idwt_out(l0.h, L) * idwt_out(l0.w, L);
    const float* src = l0.out + (size_t)c * n0;
    float v[NA];
#pragma unroll
    for (int u = 0; u < NA; ++u) { const int q = u * DC_NT + tid; v[u] = src[q < n0 ? q : 0]; }
    idwt_stage_taps<DC_NT>(f0, f1, g0, g1, L);
#pragma unroll
    for (int u = 0; u < NA; ++u) { const int q = u * DC_NT + tid; if (q < n0) DA[q] = v[u]; }
  }
  __syncthreads();
  for (int i = 0; i < lv.n; ++i) {
    const IdwtLevel& l = lv.lv[i];
    const int h = l.h, w = l.w, llh = l.llh, llw = l.llw, Ho = idwt_out(h, L), Wo = idwt_out(w, L);
    const int PY = 2 * llh + L - 2;
    for (int q = tid; q < PY * llw; q += DC_NT) {
      const int py = q / llw, ixl = q - py * llw;
      const int my = py - (L - 2), mxb = 2 * ixl - (L - 2);
      const bool rowok = my >= 0 && my < Ho;
      const float* row = DA + (rowok ? my : 0) * Wo;
      idwt_adjoint_hpass<LT>(f0, f1, L, [&](int t) {
        const int mx = mxb + 2 * t;
        const float vx = (rowok && mx >= 0 && mx < Wo) ? row[mx] : 0.f;
        const float vy = (rowok && mx + 1 >= 0 && mx + 1 < Wo) ? row[mx + 1] : 0.f;
        return make_float2(vx, vy);
      }, slo + q, shi + q);
    }
    __syncthreads();
    const bool last = i + 1 == lv.n;
    float* gll = l.ll + (size_t)c * llh * llw;
    float* gh = l.highs + (size_t)c * 3 * h * w;
    for (int q = tid; q < llh * llw; q += DC_NT) {
      const int iyl = q / llw, ixl = q - iyl * llw;
      if (iyl >= h || ixl >= w) {       // the row / column DWTInverse drops
        DB[q] = 0.f;
        if (last) gll[q] = 0.f;
        continue;
      }
      const float4 a = idwt_adjoint_vpass<LT>(f0, f1, L, slo, shi, iyl, ixl, llw);
      DB[q] = a.x;
      if (last) gll[q] = a.x;
      idwt_store_highs(gh + (size_t)iyl * w + ixl, h, w, a, l.hscale);
    }
    __syncthreads();
    float* t_ = DA; DA = DB; DB = t_;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// The filter lengths with an instantiation of their own (fully unrolled filter loops): the common orthogonal wavelets for the
// per-level kernels, which take every other length at run time (LT = 0); the coarse-tail kernels exist for their list only.
template <int... Ls> struct IdwtLengths {};
using IdwtLevelLengths = IdwtLengths<2, 4, 6, 8, 12>;
using IdwtCoarseLengths = IdwtLengths<2, 4, 6, 8>;
constexpr size_t kIdwtSmemMax = 150 * 1024;

// calls f(std::integral_constant<int, LT>) for the LT of the list that equals L; for no such length f(0) if RunTime, else nothing
template <bool RunTime, int... Ls, class F>
bool idwt_for_length(int L, IdwtLengths<Ls...>, F f) {
  const bool hit = ((L == Ls ? (f(std::integral_constant<int, Ls>{}), true) : false) || ...);
  if constexpr (RunTime) {
    if (!hit) f(std::integral_constant<int, 0>{});
  }
  return hit || RunTime;
}
inline bool idwt_coarse_length(int L) { return idwt_for_length<false>(L, IdwtCoarseLengths{}, [](auto) {}); }

// One level j of J (0 = finest): detail bands h x w, incoming low band llh x llw, output Ho x Wo
struct IdwtGeom { int h, w, llh, llw, Ho, Wo; };
inline IdwtGeom idwt_geom(int h, int w, int llh, int llw, int L) { return IdwtGeom{h, w, llh, llw, idwt_out(h, L), idwt_out(w, L)}; }
// the running low band that enters level j is the coarsest band itself, else the output of level j + 1
inline IdwtGeom idwt_geom(const int* hs, const int* ws, int J, int L, int j) {
  const bool top = j + 1 == J;
  return idwt_geom(hs[j], ws[j], top ? hs[j] : idwt_out(hs[j + 1], L), top ? ws[j] : idwt_out(ws[j + 1], L), L);
}
// ... and it lives in the buffer of level j + 1 (the same choice for its gradient, which level j's adjoint writes)
template <class T>
inline T* idwt_ll_of(T* coarsest, float* const* bufs, int J, int j) { return j + 1 < J ? bufs[j + 1] : coarsest; }
// the gradient that enters level j's adjoint
inline const float* idwt_grad_in(const float* img_grad, float* const* gbufs, int j) { return j ? gbufs[j] : img_grad; }

void idwt_level_fwd(const float* d_ll, const float* d_highs, const IdwtGeom& g, int C, const float* d_g0, const float* d_g1, int L,
                    float hscale, float* d_out, hipStream_t st) {
  const size_t smem = idwt_tile_smem<DW_TY, DW_TX>(L);
  const dim3 grid((g.Wo + DW_TX - 1) / DW_TX, (g.Ho + DW_TY - 1) / DW_TY, C);
  idwt_for_length<true>(L, IdwtLevelLengths{}, [&](auto lt) {
    APH_ALLOW_SMEM(idwt_level_kernel<decltype(lt)::value>, kIdwtSmemMax);
    APH_LAUNCH(idwt_level_kernel<decltype(lt)::value>, grid, dim3(DW_NT), smem, st, d_ll, g.llh, g.llw, d_highs, g.h, g.w, d_g0, d_g1, L, hscale,
               d_out, g.Ho, g.Wo);
  });
}
void idwt_level_bwd(const float* d_out_grad, const IdwtGeom& g, int C, const float* d_g0, const float* d_g1, int L, float hscale,
                    float* d_ll_grad, float* d_highs_grad, hipStream_t st) {
  const size_t smem = idwt_adjoint_tile_smem<DW_IY, DW_IX>(L);
  const dim3 grid((g.llw + DW_IX - 1) / DW_IX, (g.llh + DW_IY - 1) / DW_IY, C);
  idwt_for_length<true>(L, IdwtLevelLengths{}, [&](auto lt) {
    APH_ALLOW_SMEM(idwt_level_adjoint_kernel<decltype(lt)::value>, kIdwtSmemMax);
    APH_LAUNCH(idwt_level_adjoint_kernel<decltype(lt)::value>, grid, dim3(DW_NT), smem, st, d_out_grad, g.Ho, g.Wo, g.h, g.w, d_g0, d_g1, L, hscale,
               d_ll_grad, g.llh, g.llw, d_highs_grad);
  });
}
void idwt_coarse_fwd(const IdwtLevels& lv, int C, const float* d_g0, const float* d_g1, int L, hipStream_t st) {
  const IdwtLevel& lastl = lv.lv[lv.n - 1];
  const size_t smem = idwt_coarse_smem(L, lastl.hoff + 3 * lastl.h * lastl.w);
  idwt_for_length<false>(L, IdwtCoarseLengths{}, [&](auto lt) {
    APH_ALLOW_SMEM(idwt_coarse_kernel<decltype(lt)::value>, kIdwtSmemMax);
    APH_LAUNCH(idwt_coarse_kernel<decltype(lt)::value>, dim3(C), dim3(DC_NT), smem, st, lv, d_g0, d_g1, L);
  });
}
void idwt_coarse_bwd(const IdwtLevels& lv, int C, const float* d_g0, const float* d_g1, int L, hipStream_t st) {
  const size_t smem = idwt_coarse_adjoint_smem(L);
  idwt_for_length<false>(L, IdwtCoarseLengths{}, [&](auto lt) {
    APH_ALLOW_SMEM(idwt_coarse_adjoint_kernel<decltype(lt)::value>, kIdwtSmemMax);
    APH_LAUNCH(idwt_coarse_adjoint_kernel<decltype(lt)::value>, dim3(C), dim3(DC_NT), smem, st, lv, d_g0, d_g1, L);
  });
}

int idwt_check_levels(const char* who, const int* hs, const int* ws, int J, int C, int L) {
  if (!hs || !ws || J < 1 || C < 1 || L < 2 || L > 64 || (L & 1)) return aph_fail(APH_ERR_ARG, "%s: bad argument (J=%d C=%d L=%d)", who, J, C, L);
  for (int j = 0; j < J; ++j) {
    const IdwtGeom g = idwt_geom(hs, ws, J, L, j);
    if (g.h < 1 || g.w < 1 || g.Ho < 1 || g.Wo < 1 || g.llh < g.h || g.llw < g.w || g.llh > g.h + 1 || g.llw > g.w + 1)
      return aph_fail(APH_ERR_ARG, "%s: level %d is %dx%d but its low band would be %dx%d (filter length %d)", who, j, g.h, g.w, g.llh, g.llw, L);
  }
  return APH_OK;
}
// number of levels, counted from the coarsest, that the coarse-tail kernel takes (0: none -- it needs at least two to pay)
inline int idwt_coarse_count(const int* hs, const int* ws, int J, int L) {
  if (!idwt_coarse_length(L)) return 0;
  int n = 0, hsum = 0;
  for (int j = J - 1; j >= 0 && n < DC_MAX_LEVELS; --j, ++n) {
    const IdwtGeom g = idwt_geom(hs, ws, J, L, j);
    if (g.Ho > DC_TY || g.Wo > DC_TX || g.llh > DC_IY || g.llw > DC_IX) break;
    hsum += 3 * g.h * g.w;
    if (hsum > DC_HS_MAX || idwt_coarse_smem(L, hsum) > kIdwtSmemMax) break;      // (the detail bands of all its levels: one prefetch batch, and they must fit the LDS)
  }
  return n >= 2 ? n : 0;
}
// what both per-level entry points ask of their arguments (ptrs: every pointer is set)
inline bool idwt_level_args_ok(bool ptrs, int h, int w, int C, int L, int ll_h, int ll_w) {
  return ptrs && h >= 1 && w >= 1 && C >= 1 && L >= 2 && L <= 64 && !(L & 1) && ll_h >= h && ll_w >= w;
}

}  // namespace aph

using namespace aph;

extern "C" {

// one SFB2D level.  d_ll [C, ll_h, ll_w] (ll_h in {h, h+1}, ll_w in {w, w+1}), d_highs [C,3,h,w] (LH,HL,HH),
// d_g0/d_g1 = rec_lo / rec_hi taps on the device (L even, <= 64), hscale = dwt_scale gain of this level
// -> d_out [C, 2h-L+2, 2w-L+2]
int aph_idwt_level_fwd(const float* d_ll, int ll_h, int ll_w, const float* d_highs, int h, int w, int C, const float* d_g0,
                       const float* d_g1, int L, float hscale, float* d_out, void* stream_) {
  APH_TRY
  if (!idwt_level_args_ok(d_ll && d_highs && d_g0 && d_g1 && d_out, h, w, C, L, ll_h, ll_w))
    return aph_fail(APH_ERR_ARG, "aph_idwt_level_fwd: bad argument (h=%d w=%d L=%d ll=%dx%d)", h, w, L, ll_h, ll_w);
  const IdwtGeom g = idwt_geom(h, w, ll_h, ll_w, L);
  if (g.Ho < 1 || g.Wo < 1) return aph_fail(APH_ERR_ARG, "aph_idwt_level_fwd: level %dx%d too small for filter length %d", h, w, L);
  idwt_level_fwd(d_ll, d_highs, g, C, d_g0, d_g1, L, hscale, d_out, (hipStream_t)stream_);
  return aph_check_launch("aph_idwt_level_fwd");
  APH_CATCH
}

int aph_idwt_level_bwd(const float* d_out_grad, int h, int w, int C, const float* d_g0, const float* d_g1, int L, float hscale,
                       float* d_ll_grad, int ll_h, int ll_w, float* d_highs_grad, void* stream_) {
  APH_TRY
  if (!idwt_level_args_ok(d_out_grad && d_g0 && d_g1 && d_ll_grad && d_highs_grad, h, w, C, L, ll_h, ll_w))
    return aph_fail(APH_ERR_ARG, "aph_idwt_level_bwd: bad argument");
  idwt_level_bwd(d_out_grad, idwt_geom(h, w, ll_h, ll_w, L), C, d_g0, d_g1, L, hscale, d_ll_grad, d_highs_grad, (hipStream_t)stream_);
  return aph_check_launch("aph_idwt_level_bwd");
  APH_CATCH
}

// Every level of DWTInverse in one call (image.py:36-38,67).  Host arrays of J entries, level 0 = finest: hs / ws = size of
// the level's detail bands, hscales = dwt_scale gains, d_highs[j] [C,3,hs[j],ws[j]] (device), d_bufs[j] [C, 2 hs[j]-L+2,
// 2 ws[j]-L+2] = scratch for the running low band after level j (caller-owned; d_bufs[0] receives the image, the others are
// only written where a level's output has to travel through global memory).  d_yl [C, hs[J-1], ws[J-1]].
int aph_idwt_fwd(const float* d_yl, const float* const* d_highs, const int* hs, const int* ws, const float* hscales, int J, int C,
                 const float* d_g0, const float* d_g1, int L, float* const* d_bufs, void* stream_) {
  APH_TRY
  if (!d_yl || !d_highs || !hscales || !d_g0 || !d_g1 || !d_bufs) return aph_fail(APH_ERR_ARG, "aph_idwt_fwd: null argument");
  if (const int rc = idwt_check_levels("aph_idwt_fwd", hs, ws, J, C, L)) return rc;
  for (int j = 0; j < J; ++j)
    if (!d_highs[j] || !d_bufs[j]) return aph_fail(APH_ERR_ARG, "aph_idwt_fwd: null buffer at level %d", j);
  hipStream_t st = (hipStream_t)stream_;
  const int nc = idwt_coarse_count(hs, ws, J, L);
  int j = J - 1;
  if (nc) {
    IdwtLevels lv;
    lv.n = nc;
    int hoff = 0;
    bool fits = true;
    for (int i = 0; i < nc; ++i, --j) {
      const IdwtGeom g = idwt_geom(hs, ws, J, L, j);
      const ptrdiff_t delta = d_highs[j] - d_highs[J - 1];      // (in floats; the kernel addresses every level's bands from the first one's pointer)
      if (delta > (ptrdiff_t)0x3fffffff || delta < -(ptrdiff_t)0x3fffffff) { fits = false; break; }
      lv.lv[i] = IdwtLevel{const_cast<float*>(idwt_ll_of(d_yl, d_bufs, J, j)), const_cast<float*>(d_highs[j]), d_bufs[j], g.llh, g.llw, g.h, g.w, hscales[j], hoff,
                           (int)delta};
      hoff += 3 * g.h * g.w;
    }
    if (fits) idwt_coarse_fwd(lv, C, d_g0, d_g1, L, st);
    else j = J - 1;                      // (detail bands in allocations too far apart for 32-bit offsets: one launch per level)
  }
  for (; j >= 0; --j)
    idwt_level_fwd(idwt_ll_of(d_yl, d_bufs, J, j), d_highs[j], idwt_geom(hs, ws, J, L, j), C, d_g0, d_g1, L, hscales[j], d_bufs[j], st);
  return aph_check_launch("aph_idwt_fwd");
  APH_CATCH
}

// adjoint of aph_idwt_fwd: d_img_grad [C, 2 hs[0]-L+2, 2 ws[0]-L+2] -> d_highs_grad[j] [C,3,hs[j],ws[j]] and d_yl_grad
// [C, hs[J-1], ws[J-1]].  d_gbufs[j], j >= 1: scratch of d_bufs[j]'s size (gradient of the running low band; d_gbufs[0] unused).
int aph_idwt_bwd(const float* d_img_grad, const int* hs, const int* ws, const float* hscales, int J, int C, const float* d_g0,
                 const float* d_g1, int L, float* const* d_gbufs, float* d_yl_grad, float* const* d_highs_grad, void* stream_) {
  APH_TRY
  if (!d_img_grad || !hscales || !d_g0 || !d_g1 || !d_gbufs || !d_yl_grad || !d_highs_grad) return aph_fail(APH_ERR_ARG, "aph_idwt_bwd: null argument");
  if (const int rc = idwt_check_levels("aph_idwt_bwd", hs, ws, J, C, L)) return rc;
  for (int j = 0; j < J; ++j)
    if (!d_highs_grad[j] || (j && !d_gbufs[j])) return aph_fail(APH_ERR_ARG, "aph_idwt_bwd: null buffer at level %d", j);
  hipStream_t st = (hipStream_t)stream_;
  const int nc = idwt_coarse_count(hs, ws, J, L);
  int j = 0;
  for (; j < J - nc; ++j)
    idwt_level_bwd(idwt_grad_in(d_img_grad, d_gbufs, j), idwt_geom(hs, ws, J, L, j), C, d_g0, d_g1, L, hscales[j], idwt_ll_of(d_yl_grad, d_gbufs, J, j),
                   d_highs_grad[j], st);
  if (nc) {
    IdwtLevels lv;
    lv.n = nc;
    for (int i = 0; i < nc; ++i, ++j) {
      const IdwtGeom g = idwt_geom(hs, ws, J, L, j);
      lv.lv[i] = IdwtLevel{idwt_ll_of(d_yl_grad, d_gbufs, J, j), d_highs_grad[j], const_cast<float*>(idwt_grad_in(d_img_grad, d_gbufs, j)), g.llh, g.llw, g.h, g.w,
                           hscales[j], 0, 0};
    }
    idwt_coarse_bwd(lv, C, d_g0, d_g1, L, st);
  }
  return aph_check_launch("aph_idwt_bwd");
  APH_CATCH
}

// test hook (aphantasia_hip_test.h): how many levels, counted from the coarsest, aph_idwt_fwd / aph_idwt_bwd hand to the coarse-tail kernels
int aph_idwt_coarse_levels(const int* hs, const int* ws, int J, int L) {
  APH_TRY
  if (const int rc = idwt_check_levels("aph_idwt_coarse_levels", hs, ws, J, 1, L)) return rc;
  return idwt_coarse_count(hs, ws, J, L);
  APH_CATCH
}

}  // extern "C"
