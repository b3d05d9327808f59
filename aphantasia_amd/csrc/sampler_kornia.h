// Sampler, kornia-style augment chains (transforms.py:147-163, `-tf custom` / `-tf elastic`) with their adjoints.  Included by sampler.hip.
//
//   custom  = pad(4, constant 0.5) -> random_rotate -> jitter(8) -> normalize
//   elastic = pad(4, constant 0.5) -> RandomErasing -> random_rotate -> random_elastic -> jitter(8) -> normalize
//
// All of it in PIXEL space on the P x P canvas, P = size + 8 (what kornia's normalised-grid call chains reduce to):
//   X0[y,x]  = cut[y-4, x-4] inside the cut, 0.5 on the ring, 0 inside the erase rectangle (drawn on the P canvas)
//   R[y,x]   = bilinear0(X0; cs (x-c) - sn (y-c) + c, sn (x-c) + cs (y-c) + c),  c = (P-1)/2       (warp_affine, align_corners=True,
//              zeros padding: taps outside [0,P) contribute 0, no ones-mask); has_rotation = 0: R = X0
//   E[v,u]   = bilinear0(R; u P/(P-1) - 0.5, v P/(P-1) - 0.5)                                      (elastic only: upstream passes zero
//              noise, what is left of elastic_transform2d is its align_corners=False resample of the linspace(-1,1) meshgrid)
//   J[y,x]   = prev[y-dy, x-dx], 0 where y < dy or x < dx                                          (K.translate by whole pixels)
// The pad ring, the canvas edge and the erase rectangle are read-side predicates on the tap coordinate, the jitter is an index offset:
// `custom` and `elastic` are each ONE forward gather from the crop scratch to the output (4 and 16 taps); only elastic's adjoint goes through
// a P x P scratch canvas (the gradient of R).
// The planar outputs are the full P x P canvas; the patch-major ones are its top-left size x size window -- all that a stride = kernel =
// patch convolution reads of it ((P - patch) / patch + 1 == size / patch for patch > 8), so canvas rows / columns >= size get no gradient.
#pragma once
#include "sampler_layout.h"
#include "sampler_warp.h"

namespace aph {

constexpr int kTfPad = 4;             // pad(4, ...)
constexpr float kTfRing = 0.5f;       // its constant
constexpr int kTfJitter = 8;          // jitter(8): dx, dy in 0 .. 7

template <int OUT>
struct is_window { static constexpr bool v = OUT == APH_OUT_PATCH_F16 || OUT == APH_GRAD_PATCH_F16 || OUT == APH_OUT_PATCH_F32 || OUT == APH_OUT_PATCH_F16_HILO; };
// side of what layout OUT holds of the canvas
template <int OUT>
__device__ __forceinline__ int tf_side(int n) { return is_window<OUT>::v ? n : n + 2 * kTfPad; }

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// pixel coordinate -> bilinear footprint
__device__ __forceinline__ Tap pix_tap(float fx, float fy) {
  Tap t;
  const float x0 = floorf(fx), y0 = floorf(fy);
  t.x0 = (int)x0; t.y0 = (int)y0;
  t.wx1 = fx - x0; t.wx0 = (x0 + 1.f) - fx;
  t.wy1 = fy - y0; t.wy0 = (y0 + 1.f) - fy;
  return t;
}
// source coordinate of canvas pixel (y, x) under the rotation (the inverse of get_rotation_matrix2d about the canvas centre)
__device__ __forceinline__ void rot_src(float cs, float sn, int y, int x, int P, float& fx, float& fy) {
  const float c = 0.5f * (float)(P - 1), ux = (float)x - c, uy = (float)y - c;      // (exact: half-integers)
  fx = fmaf(cs, ux, fmaf(-sn, uy, c));
  fy = fmaf(sn, ux, fmaf(cs, uy, c));
}
// source coordinate of the elastic resample along one axis
__device__ __forceinline__ float elastic_src(int u, int P) { return fmaf((float)u, (float)P / (float)(P - 1), -0.5f); }
__device__ __forceinline__ float tent(float d) { return fmaxf(0.f, 1.f - fabsf(d)); }

// v += w * X0[yy, xx], X0 read through the cut scratch (HWC4, n x n): branch-free, a tap off the canvas or inside the erase rectangle has
// weight 0, one on the ring the value 0.5, and the (clamped) 16-byte load is issued either way.  ERASE: the chain has a RandomErasing stage
// (elastic); custom has none and never reads a[9..12]
template <bool ERASE>
__device__ __forceinline__ void canvas_tap(const float* __restrict__ cut, const float* __restrict__ a, int yy, int xx, int n, float w, float v[3]) {
  const int P = n + 2 * kTfPad, cy = yy - kTfPad, cx = xx - kTfPad;
  const bool on = yy >= 0 && yy < P && xx >= 0 && xx < P && !(ERASE && in_rect(a, yy, xx));
  const bool inside = cy >= 0 && cy < n && cx >= 0 && cx < n;
  const f32x4 sv = *reinterpret_cast<const f32x4*>(cut + ((size_t)clampi(cy, n - 1) * n + clampi(cx, n - 1)) * 4);
  const float we = on ? w : 0.f;
  v[0] += we * (inside ? sv[0] : kTfRing); v[1] += we * (inside ? sv[1] : kTfRing); v[2] += we * (inside ? sv[2] : kTfRing);
}

// R[y, x] for a pixel of the canvas (pad + erase + rotation; the zero-angle cuts copy)
template <bool ERASE>
__device__ __forceinline__ void rotated3(const float* __restrict__ cut, const float* __restrict__ a, int y, int x, int n, float v[3]) {
  v[0] = v[1] = v[2] = 0.f;
  if (a[15] != 0.f) {
    float fx, fy;
    rot_src(a[13], a[14], y, x, n + 2 * kTfPad, fx, fy);
    const Tap t = pix_tap(fx, fy);
    canvas_tap<ERASE>(cut, a, t.y0, t.x0, n, t.wx0 * t.wy0, v);
    canvas_tap<ERASE>(cut, a, t.y0, t.x0 + 1, n, t.wx1 * t.wy0, v);
    canvas_tap<ERASE>(cut, a, t.y0 + 1, t.x0, n, t.wx0 * t.wy1, v);
    canvas_tap<ERASE>(cut, a, t.y0 + 1, t.x0 + 1, n, t.wx1 * t.wy1, v);
  } else {
    canvas_tap<ERASE>(cut, a, y, x, n, 1.f, v);
  }
}

// custom, the whole chain: crop scratch A -> out (thread = output pixel, 32 x 8 per workgroup: warp_block_note)
template <int OUT>
__global__ void custom_emit_kernel(const float* __restrict__ A, const float* __restrict__ aug, void* __restrict__ out, int n, int patch) {
  const int s = blockIdx.z, side = tf_side<OUT>(n), P = n + 2 * kTfPad;
  const float* a = aug + (size_t)s * APH_AUG_STRIDE;
  const int j = blockIdx.x * 32 + (threadIdx.x & 31), i = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (i >= side || j >= side) return;
  const int y = i - (int)a[1], x = j - (int)a[0];
  float v[3] = {0.f, 0.f, 0.f};
  if (y >= 0 && x >= 0 && y < P && x < P) rotated3<false>(A + hwc4_index(s, 0, 0, n), a, y, x, n, v);
  emit3<OUT>(out, s, i, j, side, patch, v[0], v[1], v[2]);
}

// elastic, the whole forward chain in ONE pass, crop scratch A -> out: each of the four taps of the fixed resample evaluates R through its
// own four canvas taps (16 scratch taps per output pixel, read-side pad and erase on each), then jitter + normalise + emit; no canvas
// scratch.  Measured against rotate-into-a-canvas + resample-from-it (two kernels, bit-identical output): DESIGN.md section 4
template <int OUT>
__global__ void elastic_emit_kernel(const float* __restrict__ A, const float* __restrict__ aug, void* __restrict__ out, int n, int patch) {
  const int s = blockIdx.z, side = tf_side<OUT>(n), P = n + 2 * kTfPad;
  const float* a = aug + (size_t)s * APH_AUG_STRIDE;
  const int j = blockIdx.x * 32 + (threadIdx.x & 31), i = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (i >= side || j >= side) return;
  const int y = i - (int)a[1], x = j - (int)a[0];
  float v[3] = {0.f, 0.f, 0.f};
  if (y >= 0 && x >= 0 && y < P && x < P) {
    const Tap t = pix_tap(elastic_src(x, P), elastic_src(y, P));
    const float* cut = A + hwc4_index(s, 0, 0, n);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int yy = t.y0 + (k >> 1), xx = t.x0 + (k & 1);
      const bool on = yy >= 0 && yy < P && xx >= 0 && xx < P;
      const float w = on ? ((k & 1) ? t.wx1 : t.wx0) * ((k >> 1) ? t.wy1 : t.wy0) : 0.f;
      float r[3];
      rotated3<true>(cut, a, clampi(yy, P - 1), clampi(xx, P - 1), n, r);
      v[0] += w * r[0]; v[1] += w * r[1]; v[2] += w * r[2];
    }
  }
  emit3<OUT>(out, s, i, j, side, patch, v[0], v[1], v[2]);
}

// ---- adjoints: gathers through the inverse maps (deterministic, no atomics), like rotate_emit_adjoint_kernel ----

// w * (gradient of the jittered output at pre-jitter canvas pixel (y, x)) added to g: the output pixel is (y + dy, x + dx), and one
// past the side of layout OUT (the canvas edge; for the patch-major layouts the window edge) has no gradient.  Clamped address, weight 0.
template <int OUT>
__device__ __forceinline__ void jitter_grad3(const void* __restrict__ gout, const Layout<OUT>& L, size_t base, int side, int dy, int dx,
                                             int y, int x, float w, float g[3]) {
  const int i = y + dy, j = x + dx;
  const bool on = i >= 0 && i < side && j >= 0 && j < side;
  float q[3];
  L.load3(gout, base + (size_t)L.rowpart(clampi(i, side - 1)) + (size_t)L.colpart(clampi(j, side - 1)), q);
  const float we = on ? w : 0.f;
  g[0] += we * q[0]; g[1] += we * q[1]; g[2] += we * q[2];
}

// Gradient of X0[cy, cx] through the rotation, given dR(y, x, w, g) which adds w * dR[y, x] to g.  The canvas pixels whose footprint
// holds (cy, cx) lie within |cs| + |sn| <= sqrt 2 of the inverse-rotated point: a 3 x 3 box of candidates, each weighted by the tent form
// of the forward's own footprint arithmetic (rot_src), a miss by 0.  ERASE (elastic): nothing flows into the erase rectangle.
template <bool ERASE, class DR>
__device__ __forceinline__ void rotation_adjoint3(const float* __restrict__ a, int cy, int cx, int P, DR&& dR, float g[3]) {
  g[0] = g[1] = g[2] = 0.f;
  if (ERASE && in_rect(a, cy, cx)) return;
  if (a[15] == 0.f) { dR(cy, cx, 1.f, g); return; }
  const float cs = a[13], sn = a[14], c = 0.5f * (float)(P - 1), ux = (float)cx - c, uy = (float)cy - c;
  const float qx = cs * ux + sn * uy + c, qy = cs * uy - sn * ux + c, rad = fabsf(cs) + fabsf(sn) + 0.02f;
  const int j0 = (int)ceilf(qx - rad), i0 = (int)ceilf(qy - rad);
#pragma unroll
  for (int d = 0; d < 9; ++d) {
    const int y = i0 + d / 3, x = j0 + d % 3;
    const bool on = y >= 0 && y < P && x >= 0 && x < P;
    const int yc = clampi(y, P - 1), xc = clampi(x, P - 1);
    float fx, fy;
    rot_src(cs, sn, yc, xc, P, fx, fy);
    dR(yc, xc, on ? tent(fx - (float)cx) * tent(fy - (float)cy) : 0.f, g);
  }
}

__device__ __forceinline__ void store_planar3(float* __restrict__ dst, int s, int y, int x, int side, const float g[3]) {
  const size_t nn = (size_t)side * side, o = (size_t)s * 3 * nn + (size_t)y * side + x;
  dst[o] = g[0]; dst[o + nn] = g[1]; dst[o + 2 * nn] = g[2];
}

// custom: gout -> dA, planar [S][3][n][n] (what the crop adjoint consumes).  thread = cut pixel
template <int OUT>
__global__ void custom_adjoint_kernel(const void* __restrict__ gout, const float* __restrict__ aug, float* __restrict__ dA, int n, int patch) {
  const int s = blockIdx.z, side = tf_side<OUT>(n), P = n + 2 * kTfPad;
  const float* a = aug + (size_t)s * APH_AUG_STRIDE;
  const int px = blockIdx.x * 32 + (threadIdx.x & 31), py = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (py >= n || px >= n) return;
  const Layout<OUT> L(side, patch);
  const size_t base = (size_t)s * L.cut_stride();
  const int dx = (int)a[0], dy = (int)a[1];
  float g[3];
  rotation_adjoint3<false>(a, py + kTfPad, px + kTfPad, P,
                    [&](int y, int x, float w, float acc[3]) { jitter_grad3<OUT>(gout, L, base, side, dy, dx, y, x, w, acc); }, g);
  if (OUT != APH_OUT_NCHW_RAW) { g[0] /= kClipStd[0]; g[1] /= kClipStd[1]; g[2] /= kClipStd[2]; }
  store_planar3(dA, s, py, px, n, g);
}

// elastic, adjoint of the resample: gout -> dB, planar [S][3][P][P].  thread = canvas pixel (y, x); the resample is a separable monotone
// scale, elastic_src(u) lies in [u - 0.5, u + 0.5]: only u = x - 1, x, x + 1 can hold x in their footprint
template <int OUT>
__global__ void resample_adjoint_kernel(const void* __restrict__ gout, const float* __restrict__ aug, float* __restrict__ dB, int n, int patch) {
  const int s = blockIdx.z, side = tf_side<OUT>(n), P = n + 2 * kTfPad;
  const float* a = aug + (size_t)s * APH_AUG_STRIDE;
  const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (y >= P || x >= P) return;
  const Layout<OUT> L(side, patch);
  const size_t base = (size_t)s * L.cut_stride();
  const int dx = (int)a[0], dy = (int)a[1];
  float wu[3], wv[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int u = x - 1 + t, v = y - 1 + t;
    wu[t] = (u >= 0 && u < P) ? tent(elastic_src(clampi(u, P - 1), P) - (float)x) : 0.f;
    wv[t] = (v >= 0 && v < P) ? tent(elastic_src(clampi(v, P - 1), P) - (float)y) : 0.f;
  }
  float g[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int d = 0; d < 9; ++d)
    jitter_grad3<OUT>(gout, L, base, side, dy, dx, clampi(y - 1 + d / 3, P - 1), clampi(x - 1 + d % 3, P - 1), wv[d / 3] * wu[d % 3], g);
  if (OUT != APH_OUT_NCHW_RAW) { g[0] /= kClipStd[0]; g[1] /= kClipStd[1]; g[2] /= kClipStd[2]; }
  store_planar3(dB, s, y, x, P, g);
}

// elastic, adjoint of pad + erase + rotation: dB (planar, P x P) -> dA (planar, n x n).  thread = cut pixel
__global__ void rotate_canvas_adjoint_kernel(const float* __restrict__ dB, const float* __restrict__ aug, float* __restrict__ dA, int n) {
  const int s = blockIdx.z, P = n + 2 * kTfPad;
  const float* a = aug + (size_t)s * APH_AUG_STRIDE;
  const int px = blockIdx.x * 32 + (threadIdx.x & 31), py = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (py >= n || px >= n) return;
  const size_t nn = (size_t)P * P;
  const float* src = dB + (size_t)s * 3 * nn;
  float g[3];
  rotation_adjoint3<true>(a, py + kTfPad, px + kTfPad, P,
                    [&](int y, int x, float w, float acc[3]) {
                      const size_t o = (size_t)y * P + x;
                      acc[0] += w * src[o]; acc[1] += w * src[o + nn]; acc[2] += w * src[o + 2 * nn];
                    }, g);
  store_planar3(dA, s, py, px, n, g);
}

}  // namespace aph
