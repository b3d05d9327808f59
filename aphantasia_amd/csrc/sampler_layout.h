// Sampler, shared by every stage: geometry, cut boxes, cubic weights, wrap addressing, the output / gradient layouts.  Included by sampler.hip.
#pragma once
#include "aph_device.h"
#include "aph_host.h"

namespace aph {

__device__ __constant__ const float kClipMean[3] = {0.48145466f, 0.4578275f, 0.40821073f};
__device__ __constant__ const float kClipStd[3] = {0.26862954f, 0.26130258f, 0.27577711f};

struct Geom { int H, W, Hp, Wp, py0, px0, S, size, patch; };

// cubic convolution weights, A = -0.75 (ATen UpSampleBicubic get_cubic_upsample_coefficients)
__device__ __forceinline__ void cubic_w(float t, float w[4]) {
  const float A = -0.75f;
  const float x1 = t, x2 = 1.0f - t;
  w[0] = ((A * (x1 + 1.0f) - 5.0f * A) * (x1 + 1.0f) + 8.0f * A) * (x1 + 1.0f) - 4.0f * A;
  w[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
  w[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
  w[3] = ((A * (x2 + 1.0f) - 5.0f * A) * (x2 + 1.0f) + 8.0f * A) * (x2 + 1.0f) - 4.0f * A;
}

// four consecutive floats at 4-byte alignment: the compiler emits one global_load_dwordx4 (gfx950 handles the misalignment)
struct __attribute__((packed, aligned(4))) F4u { float v[4]; };
// the three channels of one pixel of a patch-major gradient (contiguous: one 12-byte load for f32)
struct __attribute__((packed, aligned(4))) F3u { float v[3]; };

// "every ACTIVE lane of the wave satisfies p" (a speed choice only: the test interpreter decides per lane)
__device__ __forceinline__ bool wave_all(bool p) {
#ifdef APH_EMU
  return p;
#else
  return __builtin_amdgcn_ballot_w64(!p) == 0;
#endif
}

// v mod n for the wrap-tiled overscan frame (utils.py:165-167).  The padded frame is at most 2x the image (overmax), so
// v lies in [-n, 2n): one conditional correction instead of an integer division (there are eight of these per output
// pixel of the bicubic resize -- with `%` they were most of that kernel's instructions); the generic path is kept for safety.
__device__ __forceinline__ int wrap(int v, int n) {
  if (v < 0) v += n;
  else if (v >= n) v -= n;
  if (v < 0 || v >= n) { v %= n; if (v < 0) v += n; }
  return v;
}

// area_pixel_compute_scale(align_corners=True): (in-1)/(out-1), source index = scale*dst, all fp32
__device__ __forceinline__ float cut_scale(int cs, int size) { return size > 1 ? (float)(cs - 1) / (float)(size - 1) : 0.f; }

// source index of output index i: the float32 product, ROUNDED before anything is subtracted from it (ATen: real = scale * dst, floor, t = real - floor).
// Contracted into the subtraction -- fma(scale, i, -floor) -- t comes from the unrounded product and moves by up to half an ulp of the index (8e-6 at
// index 200): the crop adjoint then missed the coordinate-exact fp64 reference by 5.7 to 26 times the float32 oracle's own error (tests/sampler_checks.py)
__device__ __forceinline__ float src_index(float scale, int i) {
#pragma clang fp contract(off)
  return scale * (float)i;
}

struct CutBox { int cs, ox, oy; float scale; };
__device__ __forceinline__ CutBox load_cut(const int* __restrict__ table, int s, int size) {
  CutBox b;
  b.cs = table[3 * s]; b.ox = table[3 * s + 1]; b.oy = table[3 * s + 2];
  b.scale = cut_scale(b.cs, size);
  return b;
}

// ---------------------------------------------------------------------------------
// Element offsets of pixel (c, i, j) of cut s in the layouts that cross the C ABI, split into the separable parts the
// adjoints need:   index = s * cut_stride + rowpart(i) + colpart(j) + c * chan_stride.
//   planar (APH_OUT_NCHW_RAW / _NORM): [S][3][size][size]
//   patch-major (APH_OUT_PATCH_F16 / _F32 / _F16_HILO, APH_GRAD_PATCH_F16): [S * (size/p)^2][3 p^2] rows of the patch-embed GEMM.
// [r4] Inside a patch row the order is PIXEL-major, channel fastest:
//     k = ((i mod p) * p + (j mod p)) * 3 + c          (openai/CLIP's conv1.weight flattens as (c, i, j): aph_vit_set_weight permutes its
// columns once at load time -- the GEMM does not care in which order K is summed).  The three channels of a pixel are then 6 (f16) / 12 (f32)
// contiguous bytes: one access per bilinear tap / candidate in the warp adjoints instead of three 4-byte gathers at a 4 KiB stride (the kernels
// are bound by the L1's access rate), and one contiguous run per lane pair in the emit.  The patch side p is a power of two (checked on the
// host): shifts and masks instead of integer divisions in the per-pixel index arithmetic.
// APH_GRAD_PATCH_F16 is a backward-only layout: patch-major like APH_OUT_PATCH_F16 but the gradient elements are f16 (the ViT
// input-gradient written by aph_vit_backward_h, still carrying the loss scale).
// ---------------------------------------------------------------------------------
template <int OUT>
struct is_patch { static constexpr bool v = OUT == APH_OUT_PATCH_F16 || OUT == APH_GRAD_PATCH_F16; };

template <int OUT>
struct Layout {
  int size, p, lp;
  __device__ __forceinline__ Layout(int size_, int patch) : size(size_), p(patch), lp(is_patch<OUT>::v ? __ffs(patch) - 1 : 0) {}
  __device__ __forceinline__ int patch_elems() const { return 3 << (2 * lp); }              // elements of one patch row: 3 p^2
  __device__ __forceinline__ int cut_stride() const { return 3 * size * size; }             // (patch-major: (size/p)^2 rows of 3 p^2; size % p == 0 is checked on the host)
  __device__ __forceinline__ int chan_stride() const { return is_patch<OUT>::v ? 1 : size * size; }      // (patch-major: channel fastest)
  __device__ __forceinline__ int rowpart(int i) const { return is_patch<OUT>::v ? (i >> lp) * (size >> lp) * patch_elems() + ((i & (p - 1)) << lp) * 3 : i * size; }
  __device__ __forceinline__ int colpart(int j) const { return is_patch<OUT>::v ? (j >> lp) * patch_elems() + (j & (p - 1)) * 3 : j; }
  // inverses of rowpart / colpart
  __device__ __forceinline__ int row_of(int off) const {
    if (is_patch<OUT>::v) {
      const int rs = (size >> lp) * patch_elems();
      const int ip = off / rs;
      return (ip << lp) + (off - ip * rs) / (3 << lp);
    }
    return off / size;
  }
  __device__ __forceinline__ int col_of(int off) const {
    if (is_patch<OUT>::v) {
      const int jp = ((off >> (2 * lp)) * 43) >> 7;      // / 3 for values < 128 (at most size / patch = 7 .. 14 patch columns)
      return (jp << lp) + (((off - jp * patch_elems()) * 43) >> 7);      // 3 (j mod p) < 128 as well (p <= 32)
    }
    return off;
  }
  __device__ __forceinline__ size_t index(int s, int c, int i, int j) const {
    return (size_t)s * cut_stride() + (size_t)(rowpart(i) + colpart(j) + c * chan_stride());
  }
  // patch-major offset o -> its place in the split-precision rows [hi (3 p^2) | lo (3 p^2)] (the lo half is patch_elems() further on)
  __device__ __forceinline__ size_t hilo_index(size_t o) const { return o + (o / (size_t)patch_elems()) * (size_t)patch_elems(); }
  // one gradient element / the three channels of the pixel whose channel-0 element is at o
  __device__ __forceinline__ static float load(const void* __restrict__ g, size_t o) {
    return OUT == APH_GRAD_PATCH_F16 ? (float)reinterpret_cast<const half_t*>(g)[o] : reinterpret_cast<const float*>(g)[o];
  }
  __device__ __forceinline__ void load3(const void* __restrict__ g, size_t o, float q[3]) const {
    if (OUT == APH_GRAD_PATCH_F16) {
      const half_t* h = reinterpret_cast<const half_t*>(g) + o;
      q[0] = (float)h[0]; q[1] = (float)h[1]; q[2] = (float)h[2];
    } else if (is_patch<OUT>::v) {
      const F3u t = *reinterpret_cast<const F3u*>(reinterpret_cast<const float*>(g) + o);
      q[0] = t.v[0]; q[1] = t.v[1]; q[2] = t.v[2];
    } else {
      const size_t nn = (size_t)chan_stride();
      q[0] = load(g, o); q[1] = load(g, o + nn); q[2] = load(g, o + 2 * nn);
    }
  }
};

// patch-major element offset of pixel (c,i,j) of cut s (the forward's patch-major outputs and the patchify kernels)
__device__ __forceinline__ size_t patch_index(int s, int c, int i, int j, int size, int p) {
  return Layout<APH_OUT_PATCH_F16>(size, p).index(s, c, i, j);
}

// internal layout of the per-cut scratch of the FORWARD augment chain (never crosses the C ABI): f32 [S][size][size][4] = (r, g, b, pad).
// Every bilinear tap of the perspective / rotation warps is then ONE 16-byte access for the three channels instead of three 4-byte
// ones in three planes (the warps are bound by L1 line accesses: crop + persp + rotate 311 -> 280 us at C2).  The ADJOINT chain keeps
// planar [S][3][size][size] scratch: its gathers are bound by L2 / fabric bytes, and the pad lane made it slower (566 -> 594 us).
constexpr int APH_SCRATCH_HWC4 = 8;
__device__ __forceinline__ size_t hwc4_index(int s, int i, int j, int size) { return (((size_t)s * size + i) * size + j) * 4; }

// gradient w.r.t. the un-normalised cut pixel (i, j) of cut s, all three channels, read from `gout` in layout OUT: one index computation
template <int OUT>
__device__ __forceinline__ void fetch_grad3(const void* __restrict__ gout, int s, int i, int j, int size, int patch, float g[3]) {
  const Layout<OUT> L(size, patch);
  L.load3(gout, L.index(s, 0, i, j), g);
  if (OUT != APH_OUT_NCHW_RAW) { g[0] /= kClipStd[0]; g[1] /= kClipStd[1]; g[2] /= kClipStd[2]; }
}

// the three channels of cut pixel (i, j) into `out` in layout OUT (normalised, except APH_OUT_NCHW_RAW and the scratch)
template <int OUT>
__device__ __forceinline__ void emit3(void* out, int s, int i, int j, int size, int patch, float v0, float v1, float v2) {
  if (OUT == APH_SCRATCH_HWC4) {
    *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(out) + hwc4_index(s, i, j, size)) = f32x4{v0, v1, v2, 0.f};
    return;
  }
  constexpr bool raw = OUT == APH_OUT_NCHW_RAW;
  const float n0 = raw ? v0 : (v0 - kClipMean[0]) / kClipStd[0], n1 = raw ? v1 : (v1 - kClipMean[1]) / kClipStd[1], n2 = raw ? v2 : (v2 - kClipMean[2]) / kClipStd[2];
  if (OUT == APH_OUT_NCHW_RAW || OUT == APH_OUT_NCHW_NORM) {
    const Layout<OUT> L(size, patch);
    float* q = reinterpret_cast<float*>(out) + L.index(s, 0, i, j);
    q[0] = n0; q[L.chan_stride()] = n1; q[2 * (size_t)L.chan_stride()] = n2;
    return;
  }
  const Layout<APH_OUT_PATCH_F16> L(size, patch);
  const size_t o = L.index(s, 0, i, j);
  if (OUT == APH_OUT_PATCH_F32) {
    float* q = reinterpret_cast<float*>(out) + o;
    q[0] = n0; q[1] = n1; q[2] = n2;
    return;
  }
  const half_t h0 = (half_t)n0, h1 = (half_t)n1, h2 = (half_t)n2;
  if (OUT == APH_OUT_PATCH_F16_HILO) {
    // rows [hi (Kp) | lo (Kp)]: hi = f16(x), lo = f16(x - hi) -- the A operand of the split-precision patch embedding (aph_vit_forward_hilo)
    const int kp = L.patch_elems();
    half_t* q = reinterpret_cast<half_t*>(out) + L.hilo_index(o);
    q[0] = h0; q[1] = h1; q[2] = h2;
    q[kp] = (half_t)(n0 - (float)h0); q[kp + 1] = (half_t)(n1 - (float)h1); q[kp + 2] = (half_t)(n2 - (float)h2);
  } else {
    half_t* q = reinterpret_cast<half_t*>(out) + o;
    q[0] = h0; q[1] = h1; q[2] = h2;
  }
}

}  // namespace aph
