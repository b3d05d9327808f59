// Sampler, torchvision-style warps (grid_sample bilinear, zeros padding, align_corners=False, ones-mask fill 0): the per-cut
// augment chain with its adjoints, and the whole-frame affine warp.  Included by sampler.hip.
#pragma once
#include "sampler_layout.h"

namespace aph {

struct Tap { int x0, y0; float wx0, wx1, wy0, wy1; };   // weights of x0, x0+1, y0, y0+1

// The grids below are torchvision's float32 operations in their order, every product and sum ROUNDED (fp contract off): fused, a source coordinate
// moves by a few n 2^-24 pixels, which the coordinate-exact fp64 reference sees as 4 to 11 times the float32 oracle's own error, and the tent form of
// rotate_emit_adjoint_kernel (separate products) would no longer re-derive the forward's footprint bit for bit (tests/sampler_checks.py)
// normalised grid coordinate -> bilinear footprint in a w x h image (at::native grid_sampler_unnormalize, align_corners=False)
__device__ __forceinline__ Tap make_tap(float gx, float gy, int w, int h) {
#pragma clang fp contract(off)
  const float ix = ((gx + 1.f) * (float)w - 1.f) * 0.5f;
  const float iy = ((gy + 1.f) * (float)h - 1.f) * 0.5f;
  Tap t;
  const float fx = floorf(ix), fy = floorf(iy);
  t.x0 = (int)fx; t.y0 = (int)fy;
  t.wx1 = ix - fx; t.wx0 = (fx + 1.f) - ix;
  t.wy1 = iy - fy; t.wy0 = (fy + 1.f) - iy;
  return t;
}
__device__ __forceinline__ Tap make_tap(float gx, float gy, int n) { return make_tap(gx, gy, n, n); }

// torchvision _perspective_grid: base grid linspace(0.5, n-0.5), theta1 / (0.5 n), theta2, g1/g2 - 1
__device__ __forceinline__ Tap persp_tap(const float* __restrict__ a, int i, int j, int n) {
#pragma clang fp contract(off)
  const float x = (float)j + 0.5f, y = (float)i + 0.5f, hn = 0.5f * (float)n;
  const float g1x = x * (a[0] / hn) + y * (a[1] / hn) + (a[2] / hn);
  const float g1y = x * (a[3] / hn) + y * (a[4] / hn) + (a[5] / hn);
  const float g2 = x * a[6] + y * a[7] + 1.0f;
  return make_tap(g1x / g2 - 1.0f, g1y / g2 - 1.0f, n);
}

// torchvision _gen_affine_grid with the inverse rotation matrix [cos, sin, 0; -sin, cos, 0]
__device__ __forceinline__ Tap rot_tap(float cs, float sn, int i, int j, int n) {
#pragma clang fp contract(off)
  const float x = -(float)n * 0.5f + 0.5f + (float)j, y = -(float)n * 0.5f + 0.5f + (float)i, hn = 0.5f * (float)n;
  const float gx = x * (cs / hn) + y * (sn / hn) + (0.0f / hn);
  const float gy = x * (-sn / hn) + y * (cs / hn) + (0.0f / hn);
  return make_tap(gx, gy, n);
}

__device__ __forceinline__ bool in_rect(const float* __restrict__ a, int y, int x) {
  const int eh = (int)a[11];
  if (eh <= 0) return false;
  const int ei = (int)a[9], ej = (int)a[10], ew = (int)a[12];
  return y >= ei && y < ei + eh && x >= ej && x < ej + ew;
}

// sampled value (three channels of one HWC4 cut image) times sampled ones-mask (fill = 0); ERASE: source pixels inside the
// erase rectangle read as 0
// warp_block_note [r3]: a workgroup of the four warp kernels covers 32 x 8 pixels (it was 64 x 4).  Under a rotation the taps of a
// 64 x 4 strip cross ~32 gradient rows and use a few pixels of every 128-byte line they touch, and the neighbouring strips that use
// the rest run on other XCDs: rotate_emit_adjoint measured 353 MB of L2 misses per launch for a 114 MB gradient.  A squarer tile
// shares fewer lines with its neighbours: augment adjoints 178-188 -> 154-162 us, forward chain 225 -> 217 us (16 x 16 measured the same).
template <bool ERASE>
__device__ __forceinline__ void warp_gather3(const float* __restrict__ src, const Tap& t, int n, const float* __restrict__ a, float v[3]) {
  // branch-free: out-of-range taps read a clamped address with weight 0, so the four 16-byte loads issue together
  float m = 0.f;
  v[0] = v[1] = v[2] = 0.f;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int yy = t.y0 + dy, xx = t.x0 + dx;
      const bool in = yy >= 0 && yy < n && xx >= 0 && xx < n;
      const float w = in ? (dx ? t.wx1 : t.wx0) * (dy ? t.wy1 : t.wy0) : 0.f;
      const int yc = yy < 0 ? 0 : (yy > n - 1 ? n - 1 : yy), xc = xx < 0 ? 0 : (xx > n - 1 ? n - 1 : xx);
      const f32x4 sv = *reinterpret_cast<const f32x4*>(src + ((size_t)yc * n + xc) * 4);
      m += w;
      const float we = (ERASE && in_rect(a, yc, xc)) ? 0.f : w;
      v[0] += we * sv[0]; v[1] += we * sv[1]; v[2] += we * sv[2];
    }
  v[0] *= m; v[1] *= m; v[2] *= m;
}

// stage 1: RandomPerspective for the cuts that drew it (A -> B, both HWC4); other cuts are skipped
__global__ void persp_kernel(const float* __restrict__ A, const float* __restrict__ aug, float* __restrict__ Bo, int n) {
  const int s = blockIdx.z;
  const float* a = aug + (size_t)s * APH_AUG_STRIDE;
  if (a[8] == 0.f) return;
  const int j = blockIdx.x * 32 + (threadIdx.x & 31), i = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (i >= n || j >= n) return;
  const Tap t = persp_tap(a, i, j, n);
  float v[3];
  warp_gather3<false>(A + hwc4_index(s, 0, 0, n), t, n, a, v);
  *reinterpret_cast<f32x4*>(Bo + hwc4_index(s, i, j, n)) = f32x4{v[0], v[1], v[2], 0.f};
}

// stage 2: RandomErasing (read-side) + rotation + normalise + emit
template <int OUT>
__global__ void rotate_emit_kernel(const float* __restrict__ A, const float* __restrict__ Bi, const float* __restrict__ aug,
                                   void* __restrict__ out, int n, int patch) {
  const int s = blockIdx.z;
  const float* a = aug + (size_t)s * APH_AUG_STRIDE;
  const int j = blockIdx.x * 32 + (threadIdx.x & 31), i = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (i >= n || j >= n) return;
  const float* src = (a[8] != 0.f ? Bi : A) + hwc4_index(s, 0, 0, n);
  float v[3];
  if (a[15] != 0.f) {
    const Tap t = rot_tap(a[13], a[14], i, j, n);
    warp_gather3<true>(src, t, n, a, v);
  } else {
    const f32x4 q = *reinterpret_cast<const f32x4*>(src + ((size_t)i * n + j) * 4);
    const bool er = in_rect(a, i, j);
    v[0] = er ? 0.f : q[0]; v[1] = er ? 0.f : q[1]; v[2] = er ? 0.f : q[2];
  }
  emit3<OUT>(out, s, i, j, n, patch, v[0], v[1], v[2]);
}

// sum of the in-bounds bilinear weights (= the sampled ones-mask of torchvision's fill handling)
__device__ __forceinline__ float tap_mask(const Tap& t, int n) {
  float m = 0.f;
  if (t.y0 >= 0 && t.y0 < n) { if (t.x0 >= 0 && t.x0 < n) m += t.wx0 * t.wy0; if (t.x0 + 1 >= 0 && t.x0 + 1 < n) m += t.wx1 * t.wy0; }
  if (t.y0 + 1 >= 0 && t.y0 + 1 < n) { if (t.x0 >= 0 && t.x0 < n) m += t.wx0 * t.wy1; if (t.x0 + 1 >= 0 && t.x0 + 1 < n) m += t.wx1 * t.wy1; }
  return m;
}
// weight with which output pixel's footprint `t` reads source pixel (py, px); 0 if it does not
__device__ __forceinline__ float tap_hits(const Tap& t, int py, int px) {
  const int dy = py - t.y0, dx = px - t.x0;
  if (dy < 0 || dy > 1 || dx < 0 || dx > 1) return 0.f;
  return (dx ? t.wx1 : t.wx0) * (dy ? t.wy1 : t.wy0);
}

// Adjoint of stage 2 as a GATHER (deterministic, no atomics): thread = source pixel p of the pre-rotation
// cut; the output pixels whose bilinear footprint contains p lie in the inverse-rotated 2x2 square around p.
// Each candidate's footprint is re-derived with the forward's own arithmetic.
template <int OUT>
__global__ void rotate_emit_adjoint_kernel(const void* __restrict__ gout, const float* __restrict__ aug,
                                           float* __restrict__ dA, float* __restrict__ dB, int n, int patch) {
  const int s = blockIdx.z;
  const float* a = aug + (size_t)s * APH_AUG_STRIDE;
  const int px = blockIdx.x * 32 + (threadIdx.x & 31), py = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (py >= n || px >= n) return;
  float* dst = a[8] != 0.f ? dB : dA;
  float g0 = 0.f, g1 = 0.f, g2 = 0.f;
  if (!in_rect(a, py, px)) {
    if (a[15] != 0.f) {
      const float cs = a[13], sn = a[14], c = 0.5f * (float)(n - 1);
      // forward: (ix, iy) = Rot (q - c) + c with Rot = [[cs, sn], [-sn, cs]]  ->  q = Rot^T (p - c) + c
      const float ux = (float)px - c, uy = (float)py - c;
      const float qx = cs * ux - sn * uy + c, qy = sn * ux + cs * uy + c;
      const float rad = fabsf(cs) + fabsf(sn) + 0.02f;
      int j0 = (int)ceilf(qx - rad), j1 = (int)floorf(qx + rad), i0 = (int)ceilf(qy - rad), i1 = (int)floorf(qy + rad);
      if (rad <= 1.45f) {
        // a rotation: the candidates fit a 3 x 3 box.  Branch-free: a miss gets weight 0 and a clamped address, the 27 gathers issue
        // together (one memory round trip instead of one per candidate).  [r3] The weight of candidate (i, j) is the TENT form of the
        // forward's bilinear footprint -- max(0, 1 - |ix - px|) * max(0, 1 - |iy - py|), with (ix, iy) from the forward's own grid
        // arithmetic (rot_tap / make_tap), its row and column terms computed once per box row / column -- times the sampled ones-mask
        // clamp(min(ix + 1, n - ix), 0, 1) * (same in y): identical to tap_hits * tap_mask up to one rounding of (1 - frac), at a third
        // of the instructions.  (Time unchanged: the kernel is bound by the L1's access rate -- 27 scalar gathers per pixel, about 46
        // cache accesses per gather instruction whatever the wave's pixel footprint, 64 x 1 and 16 x 4 measured alike; only a
        // channel-interleaved gradient layout would cut that.)
        const float fn = (float)n, hn = 0.5f * fn, ka = cs / hn, kb = sn / hn;
        const Layout<OUT> L(n, patch);
        float gxj[3], gyj[3], gxi[3], gyi[3];
        size_t rowo[3], colo[3];
        bool iok[3], jok[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
#pragma clang fp contract(off)
          const int i = i0 + t, j = j0 + t;
          iok[t] = i >= 0 && i <= n - 1 && i <= i1;
          jok[t] = j >= 0 && j <= n - 1 && j <= j1;
          const int ic = i < 0 ? 0 : (i > n - 1 ? n - 1 : i), jc = j < 0 ? 0 : (j > n - 1 ? n - 1 : j);
          const float x = -fn * 0.5f + 0.5f + (float)jc, y = -fn * 0.5f + 0.5f + (float)ic;
          gxj[t] = x * ka; gyj[t] = x * -kb;
          gxi[t] = y * kb; gyi[t] = y * ka;
          colo[t] = (size_t)L.colpart(jc);
          rowo[t] = (size_t)L.rowpart(ic);
        }
        const size_t base = (size_t)s * L.cut_stride();
        const float fpx = (float)px, fpy = (float)py;
        float wm[9];
        size_t off[9];
#pragma unroll
        for (int d = 0; d < 9; ++d) {
#pragma clang fp contract(off)
          const int a3 = d / 3, b3 = d % 3;
          const float gx = gxj[b3] + gxi[a3], gy = gyj[b3] + gyi[a3];
          const float ix = ((gx + 1.f) * fn - 1.f) * 0.5f, iy = ((gy + 1.f) * fn - 1.f) * 0.5f;
          const float wx = fmaxf(0.f, 1.f - fabsf(ix - fpx)), wy = fmaxf(0.f, 1.f - fabsf(iy - fpy));
          const float mx = fminf(fmaxf(fminf(ix + 1.f, fn - ix), 0.f), 1.f), my = fminf(fmaxf(fminf(iy + 1.f, fn - iy), 0.f), 1.f);
          wm[d] = (iok[a3] && jok[b3]) ? (wx * wy) * (mx * my) : 0.f;
          off[d] = base + rowo[a3] + colo[b3];
        }
        float gv[9][3];
#pragma unroll
        for (int d = 0; d < 9; ++d) L.load3(gout, off[d], gv[d]);
#pragma unroll
        for (int d = 0; d < 9; ++d) { g0 += wm[d] * gv[d][0]; g1 += wm[d] * gv[d][1]; g2 += wm[d] * gv[d][2]; }
        if (OUT != APH_OUT_NCHW_RAW) { g0 /= kClipStd[0]; g1 /= kClipStd[1]; g2 /= kClipStd[2]; }
      } else {
        j0 = j0 < 0 ? 0 : j0; i0 = i0 < 0 ? 0 : i0; j1 = j1 > n - 1 ? n - 1 : j1; i1 = i1 > n - 1 ? n - 1 : i1;
        for (int i = i0; i <= i1; ++i)
          for (int j = j0; j <= j1; ++j) {
            const Tap t = rot_tap(cs, sn, i, j, n);
            const float w = tap_hits(t, py, px);
            if (w == 0.f) continue;
            const float wmm = w * tap_mask(t, n);
            float gq[3];
            fetch_grad3<OUT>(gout, s, i, j, n, patch, gq);
            g0 += wmm * gq[0]; g1 += wmm * gq[1]; g2 += wmm * gq[2];
          }
      }
    } else {
      float gq[3];
      fetch_grad3<OUT>(gout, s, py, px, n, patch, gq);
      g0 = gq[0]; g1 = gq[1]; g2 = gq[2];
    }
  }
  const size_t pl = (size_t)s * 3 * n * n, pix = (size_t)py * n + px;
  dst[pl + pix] = g0;
  dst[pl + (size_t)n * n + pix] = g1;
  dst[pl + 2 * (size_t)n * n + pix] = g2;
}

// Adjoint of stage 1 (perspective) as a gather: dB -> dA (in place of the cut's slot in dA).  Candidates =
// bounding box of the inverse homography applied to the 2x2 square around p.
__global__ void persp_adjoint_kernel(const float* __restrict__ dB, const float* __restrict__ aug, float* __restrict__ dA, int n) {
  const int s = blockIdx.z;
  const float* a = aug + (size_t)s * APH_AUG_STRIDE;
  if (a[8] == 0.f) return;
  const int px = blockIdx.x * 32 + (threadIdx.x & 31), py = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (py >= n || px >= n) return;
    // forward: (u, v) = H (x, y), x = j + .5, y = i + .5, source index = (u - .5, v - .5);  adj(H) maps back
  const float m00 = a[4] - a[5] * a[7], m01 = a[2] * a[7] - a[1], m02 = a[1] * a[5] - a[2] * a[4];
  const float m10 = a[5] * a[6] - a[3], m11 = a[0] - a[2] * a[6], m12 = a[2] * a[3] - a[0] * a[5];
  const float m20 = a[3] * a[7] - a[4] * a[6], m21 = a[1] * a[6] - a[0] * a[7], m22 = a[0] * a[4] - a[1] * a[3];
  float xmin = 1e30f, xmax = -1e30f, ymin = 1e30f, ymax = -1e30f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float u = (float)px + 0.5f + ((k & 1) ? 1.01f : -1.01f), v = (float)py + 0.5f + ((k & 2) ? 1.01f : -1.01f);
    const float d = m20 * u + m21 * v + m22;
    const float xx = (m00 * u + m01 * v + m02) / d - 0.5f, yy = (m10 * u + m11 * v + m12) / d - 0.5f;
    xmin = fminf(xmin, xx); xmax = fmaxf(xmax, xx); ymin = fminf(ymin, yy); ymax = fmaxf(ymax, yy);
  }
  int j0 = (int)ceilf(xmin - 0.05f), j1 = (int)floorf(xmax + 0.05f), i0 = (int)ceilf(ymin - 0.05f), i1 = (int)floorf(ymax + 0.05f);
  j0 = j0 < 0 ? 0 : j0; i0 = i0 < 0 ? 0 : i0; j1 = j1 > n - 1 ? n - 1 : j1; i1 = i1 > n - 1 ? n - 1 : i1;
  if (!(xmax - xmin < 64.f && ymax - ymin < 64.f)) { j0 = 0; i0 = 0; j1 = n - 1; i1 = n - 1; }   // degenerate map: exhaustive
  float g0 = 0.f, g1 = 0.f, g2 = 0.f;
  const size_t pl = (size_t)s * 3 * n * n, nn = (size_t)n * n;
  for (int i = i0; i <= i1; ++i)
    for (int j = j0; j <= j1; ++j) {
      const Tap t = persp_tap(a, i, j, n);
      const float w = tap_hits(t, py, px);
      if (w == 0.f) continue;
      const float wm = w * tap_mask(t, n);
      const size_t o = pl + (size_t)i * n + j;
      g0 += wm * dB[o];
      g1 += wm * dB[o + nn];
      g2 += wm * dB[o + 2 * nn];
    }
  const size_t pix = (size_t)py * n + px;
  dA[pl + pix] = g0;
  dA[pl + nn + pix] = g1;
  dA[pl + 2 * nn + pix] = g2;
}

// ---------------------------------------------------------------------------------
// illustrip's frame_transform (illustrip.py:130-138): T.functional.affine(img, angle, shift, scale, shear, fill=0,
// BILINEAR) of a whole [C,H,W] image, once per frame.  m = the 2x3 INVERSE affine matrix (host, torchvision's
// _get_inverse_affine_matrix); grid = [x, y, 1] . (m^T / (0.5 W, 0.5 H)) over the centred base grid, bilinear, zeros
// padding, ones-mask fill -- the same sampler arithmetic as the per-cut rotation above.
// ---------------------------------------------------------------------------------
struct Affine6 { float m[6]; };

__global__ void frame_affine_kernel(const float* __restrict__ src, float* __restrict__ dst, int C, int H, int W, Affine6 a) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  const float bx = -(float)W * 0.5f + 0.5f + (float)x, by = -(float)H * 0.5f + 0.5f + (float)y;
  const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
  const float gx = bx * (a.m[0] / hw) + by * (a.m[1] / hw) + (a.m[2] / hw);
  const float gy = bx * (a.m[3] / hh) + by * (a.m[4] / hh) + (a.m[5] / hh);
  const Tap t = make_tap(gx, gy, W, H);
  float w[4];
  int off[4];
  float mask = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int xx = t.x0 + (k & 1), yy = t.y0 + (k >> 1);
    const bool in = xx >= 0 && xx < W && yy >= 0 && yy < H;
    w[k] = in ? ((k & 1) ? t.wx1 : t.wx0) * ((k >> 1) ? t.wy1 : t.wy0) : 0.f;
    off[k] = in ? yy * W + xx : 0;
    mask += w[k];
  }
  for (int c = 0; c < C; ++c) {
    const float* pl = src + (size_t)c * H * W;
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) v += w[k] * pl[off[k]];
    dst[((size_t)c * H + y) * W + x] = v * mask;
  }
}

}  // namespace aph
