// Sampler, forward: crop + bicubic resize of all cuts in one launch (utils.py:248-249).  Included by sampler.hip.
#pragma once
#include "sampler_layout.h"

namespace aph {

// bicubic value (all three channels) of resized-cut pixel (i, j): utils.py:248-249
__device__ __forceinline__ void bicubic3(const float* __restrict__ rgb, const Geom& g, const CutBox& b, int i, int j, float v[3]) {
  const float sy = src_index(b.scale, i), sx = src_index(b.scale, j);
  const int y0 = (int)floorf(sy), x0 = (int)floorf(sx);
  float wy[4], wx[4];
  cubic_w(sy - (float)y0, wy);
  cubic_w(sx - (float)x0, wx);
  int ry[4], rx[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int yy = y0 - 1 + k; yy = yy < 0 ? 0 : (yy > b.cs - 1 ? b.cs - 1 : yy);   // clamp inside the cut
    int xx = x0 - 1 + k; xx = xx < 0 ? 0 : (xx > b.cs - 1 ? b.cs - 1 : xx);
    ry[k] = wrap(b.oy + yy - g.py0, g.H);                                       // tile_pad wrap (utils.py:165-167)
    rx[k] = wrap(b.ox + xx - g.px0, g.W);
  }
  // the four column taps are consecutive source pixels unless the clamp at the cut's edge or the wrap at the image's
  // edge intervenes: one 16-byte load per tap row (4-byte aligned) instead of four scalar gathers.  [r3] The choice is made per
  // WAVE: with a per-lane branch the compiler shared the first and last tap between the two paths and emitted dword + dwordx2 + dword
  // per tap row, each behind its own divergent branch (46 vector-memory instructions per wave and pixel; the kernel is bound by the
  // L1's access rate: TCP_TOTAL_CACHE_ACCESSES 150 M per launch at C2).
  if (wave_all(rx[3] == rx[0] + 3)) {
    F4u t[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int a = 0; a < 4; ++a) t[c][a] = *reinterpret_cast<const F4u*>(rgb + ((size_t)c * g.H + ry[a]) * g.W + rx[0]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float acc = 0.f;
#pragma unroll
      for (int a = 0; a < 4; ++a) acc += (t[c][a].v[0] * wx[0] + t[c][a].v[1] * wx[1] + t[c][a].v[2] * wx[2] + t[c][a].v[3] * wx[3]) * wy[a];
      v[c] = acc;
    }
    return;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* pl = rgb + (size_t)c * g.H * g.W;
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const float* row = pl + (size_t)ry[a] * g.W;
      acc += (row[rx[0]] * wx[0] + row[rx[1]] * wx[1] + row[rx[2]] * wx[2] + row[rx[3]] * wx[3]) * wy[a];
    }
    v[c] = acc;
  }
}

// XCD-aware forward (speed only; any assignment is correct).  The image (11 MB at 720p) does not fit one XCD's 4 MB L2, and with
// the plain (x, y, cut) grid every XCD gathers from all of it: 487 MB of fabric fetch per launch for 11 MB of source.  Here the
// unit of work is (cut, group of 4 output rows); strip_list_kernel assigns every unit to the XCD that owns the 16-pixel image
// strip its source rows fall into (strips interleaved over the XCDs: strip t -> XCD t % 8, so every XCD sees centre and edge
// strips alike), and crop_resize_strips_kernel's workgroup b, which runs on XCD b % 8 (observed dispatch order), walks that
// XCD's list.  An XCD then touches ~1.4 / 8 of the image.
constexpr int kStripPx = 16;          // [r3] 32 -> 16: the 22.5 strips of a 720-row image left one XCD a third short of work (148 -> 145 us; 8: 143.5, 64: 170)
constexpr int kUnitRows = 4;              // output rows of one unit of work (8: 153 us against 145; 128-thread workgroups: 150)
constexpr int kStripSlots = 768;          // workgroups per XCD in crop_resize_strips_kernel

// lists: [8][cap] unit ids (cut * groups + row group), counts: [8]; one workgroup of 1024 threads
__global__ __launch_bounds__(1024) void strip_list_kernel(const int* __restrict__ table, int* __restrict__ lists, int* __restrict__ counts, int cap, Geom g, int strip_px) {
  __shared__ int cnt[8];
  if (threadIdx.x < 8) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int groups = (g.size + kUnitRows - 1) / kUnitRows, units = g.S * groups;
  for (int u = threadIdx.x; u < units; u += blockDim.x) {
    const int s = u / groups, rg = u - s * groups;
    const CutBox b = load_cut(table, s, g.size);
    int i = rg * kUnitRows + kUnitRows / 2; i = i > g.size - 1 ? g.size - 1 : i;
    int yy = (int)floorf(src_index(b.scale, i)); yy = yy > b.cs - 1 ? b.cs - 1 : yy;
    const int yc = wrap(b.oy + yy - g.py0, g.H);
    const int xcd = (yc / strip_px) & 7;
    const int pos = atomicAdd(&cnt[xcd], 1);            // (order inside a list is irrelevant: units are independent)
    lists[xcd * cap + pos] = u;
  }
  __syncthreads();
  if (threadIdx.x < 8) counts[threadIdx.x] = cnt[threadIdx.x];
}

template <int OUT>
__global__ __launch_bounds__(256) void crop_resize_strips_kernel(const float* __restrict__ rgb, const int* __restrict__ table, void* __restrict__ out, Geom g,
                                                                 const int* __restrict__ lists, const int* __restrict__ counts, int cap) {
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, nslot = gridDim.x >> 3;
  const int count = counts[xcd], groups = (g.size + kUnitRows - 1) / kUnitRows, n = g.size;
  for (int it = slot; it < count; it += nslot) {
    const int u = lists[xcd * cap + it];
    const int s = u / groups, rg = u - s * groups;
    const CutBox b = load_cut(table, s, n);
    for (int p = threadIdx.x; p < kUnitRows * n; p += blockDim.x) {
      const int di = p / n, j = p - di * n, i = rg * kUnitRows + di;
      if (i >= n) continue;
      float v[3];
      bicubic3(rgb, g, b, i, j, v);
      emit3<OUT>(out, s, i, j, n, g.patch, v[0], v[1], v[2]);
    }
  }
}

// per-XCD unit lists of the forward, in the caller's workspace: lists [8][cap] + counts [8] ints
inline int strip_cap(const Geom& g) { return g.S * ((g.size + kUnitRows - 1) / kUnitRows); }

template <int OUT>
void launch_crop_resize(const float* rgb, const int* table, void* out, const Geom& g, int* lists, hipStream_t st) {
  int* counts = lists + 8 * (size_t)strip_cap(g);
  APH_LAUNCH(strip_list_kernel, dim3(1), dim3(1024), 0, st, table, lists, counts, strip_cap(g), g, kStripPx);
  APH_LAUNCH(crop_resize_strips_kernel<OUT>, dim3(8 * kStripSlots), dim3(256), 0, st, rgb, table, out, g, (const int*)lists, (const int*)counts, strip_cap(g));
}

}  // namespace aph
