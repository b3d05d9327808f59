// Sampler, adjoint of the crop + bicubic resize: tap tables, gather kernel, separable row-block kernel, their launcher.  Included by sampler.hip.
#pragma once
#include <type_traits>
#include "sampler_layout.h"

namespace aph {

// Adjoint of crop_resize over all cuts -- deterministic gather, one 16x16 pixel tile per workgroup.
//   d rgb[y][x] = sum_s sum_{i,j} Wy_s[i][y - oy_s] Wx_s[j][x - ox_s] G_s[i][j]       (fixed order s = 0..S-1)
// 1. wave 0 culls the S cuts (x wrap-padding aliases) against the tile into an ordered LDS list;
// 2. per batch of 8 listed cuts, 256 threads build the 1-D tables: for each of the tile's 16 rows and 16
//    columns the (<= 4, for down-sampling cuts) output indices whose clamped cubic taps land on it, with the
//    forward's own fp32 weights and the separable gradient-layout offsets;
// 3. every pixel accumulates its <= 4x4 products per cut.  Work ~ the forward's 16 taps per output pixel.
// Up-sampling cuts (csize < size, only possible for images smaller than `size`) take the per-pixel generic path.
struct AdjEntry { int off[4]; float w[4]; };

// weight of output index i on crop-local source position q (sum over clamped taps; forward arithmetic)
__device__ __forceinline__ float tap_weight(float scale, int i, int cs, int q) {
  const float sy = src_index(scale, i);
  const int y0 = (int)floorf(sy);
  float wv[4];
  cubic_w(sy - (float)y0, wv);
  float w = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int yy = y0 - 1 + k; yy = yy < 0 ? 0 : (yy > cs - 1 ? cs - 1 : yy);
    if (yy == q) w += wv[k];
  }
  return w;
}

// Ordered compaction by wave 0 (called by threads 0..63 of the workgroup, all of them): of the candidates k = 0..n-1, those with
// hit(k) are handed to put(position, k) in increasing k, positions 0, 1, ...; *count = how many.  hit() and put() of a candidate run
// on the same lane, so hit() may leave what put() stores in the caller's locals.
template <class Hit, class Put>
__device__ __forceinline__ void wave0_compact(int n, int* count, Hit hit, Put put) {
  int c = 0;
  for (int k0 = 0; k0 < n; k0 += 64) {
    const int k = k0 + (int)threadIdx.x;
    const bool h = k < n && hit(k);
    const unsigned long long m = __ballot(h);
    if (h) put(c + __popcll(m & ((1ull << threadIdx.x) - 1ull)), k);
    c += __popcll(m);
  }
  if (threadIdx.x == 0) *count = c;
}

// Generic per-pixel path of an up-sampling cut (cs < size: its source positions have more than four outputs each, so the tap
// tables do not hold them): acc[ch] += wy * wx * G[i][j][ch] over every output (i, j) whose taps land on crop-local (yc, xc), for the
// NC channels from gb on (gb = the cut's base, plus the channel's for NC = 1).
template <int OUT, int NC>
__device__ __forceinline__ void upsample_cut_sum(const void* __restrict__ gout, size_t gb, const Layout<OUT>& L, float scale, int cs, int yc, int xc, float (&acc)[NC]) {
  for (int i = 0; i < L.size; ++i) {
    const float wy = tap_weight(scale, i, cs, yc);
    if (wy == 0.f) continue;
    for (int j = 0; j < L.size; ++j) {
      const float wx = tap_weight(scale, j, cs, xc);
      if (wx == 0.f) continue;
      const int o = L.rowpart(i) + L.colpart(j);
#pragma unroll
      for (int ch = 0; ch < NC; ++ch) acc[ch] += wy * wx * L.load(gout, gb + o + ch * L.chan_stride());
    }
  }
}

// Per-cut 1-D tap tables, once per step: for every crop-local source position q of cut s and each axis, the (<= 4)
// output indices whose clamped cubic taps land on q, with the forward's own fp32 weights and the gradient-layout
// offsets.  tab[(s * 2 + axis) * maxcs + q]; entries of up-sampling cuts stay unused (generic path).
template <int OUT>
__global__ void tap_table_kernel(const int* __restrict__ table, AdjEntry* __restrict__ tab, int maxcs, Geom g) {
  const int s = blockIdx.z, isrow = blockIdx.y == 0;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  const int cs = table[3 * s];
  if (q >= cs || q >= maxcs) return;
  const Layout<OUT> L(g.size, g.patch);
  AdjEntry e;
#pragma unroll
  for (int a = 0; a < 4; ++a) { e.off[a] = 0; e.w[a] = 0.f; }
  const float scale = cut_scale(cs, g.size);
  if (scale >= 1.0f) {
    const float inv = 1.0f / scale;
    int lo = (int)floorf((float)(q - 2) * inv) - 1, hi = (int)floorf((float)(q + 2) * inv) + 1;
    lo = lo < 0 ? 0 : lo; hi = hi > g.size - 1 ? g.size - 1 : hi;
    int n = 0;
    for (int i = lo; i <= hi && n < 4; ++i) {
      const float w = tap_weight(scale, i, cs, q);
      if (w != 0.f || n > 0) {             // contiguous run starting at the first non-zero
        e.w[n] = w;
        e.off[n] = isrow ? L.rowpart(i) : L.colpart(i);
        ++n;
      }
    }
  }
  tab[((size_t)s * 2 + (isrow ? 0 : 1)) * maxcs + q] = e;
}

template <int OUT>
__global__ __launch_bounds__(256) void crop_resize_adjoint_kernel(const void* __restrict__ gout, float gscale,
                                                                  const int* __restrict__ table, float* __restrict__ grgb, Geom g,
                                                                  const AdjEntry* __restrict__ tab, int maxcs) {
  constexpr int MAXV = 1024, NB = 8;
  __shared__ int vlist[MAXV];
  __shared__ int vcount;
  __shared__ AdjEntry ent[NB][32];
  __shared__ int vinfo[NB][3];     // cut index, generic-path flag, longest run of outputs per source position
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  // XCD-aware tile order (speed only; any order is correct).  Workgroup b runs on XCD b % 8 (observed dispatch order).  XCD k takes
  // the tile rows k, k + 8, k + 16, ...: a gradient row of a cut lands on 1-3 image rows, so almost every gradient line is then
  // gathered by ONE XCD's L2 instead of all eight (the plain 2-D grid measured 816 MB of fabric fetch per launch for a 114 MB
  // gradient, L2 hit rate 0.29), while every XCD still sees the same mix of centre and edge rows (contiguous bands were slower:
  // edge bands are covered by half as many cuts).  486 -> 375 us at the headline size.  Workgroups beyond an XCD's share exit.
  const int ntx_ = (g.W + 15) / 16, nty_ = (g.H + 15) / 16;
  const int xcd_ = blockIdx.x & 7, idx_ = blockIdx.x >> 3;
  const int lrow_ = idx_ / ntx_, bx_ = idx_ - lrow_ * ntx_, by_ = lrow_ * 8 + xcd_;
  if (by_ >= nty_) return;
  const int x = bx_ * 16 + tx, y = by_ * 16 + ty;
  const bool live = x < g.W && y < g.H;
  const int nay = (g.Hp + g.H - 1) / g.H, nax = (g.Wp + g.W - 1) / g.W;     // aliases per axis (1 without overscan)
  const int nvirt = g.S * nay * nax;
  const int ty0 = by_ * 16, tx0 = bx_ * 16;
  const Layout<OUT> L(g.size, g.patch);
  const int cchan = L.chan_stride(), ccut = L.cut_stride();
  float acc[3] = {0.f, 0.f, 0.f};
  for (int vbase = 0; vbase < nvirt; vbase += MAXV) {
    // ---- 1. ordered compaction by wave 0
    __syncthreads();
    if (threadIdx.x < 64) {
      wave0_compact(nvirt - vbase < MAXV ? nvirt - vbase : MAXV, &vcount, [&](int k) {
        const int v = vbase + k;
        const int s = v / (nay * nax), al = v - s * (nay * nax), ay = al / nax, ax = al - ay * nax;
        const int cs = table[3 * s], ox = table[3 * s + 1], oy = table[3 * s + 2];
        // alias coordinates of the tile's first/last row and column (a wrapping tile is not culled on that axis)
        // (the LAST LIVE row / column: a tile taller or wider than the whole image must not wrap its end into the middle of it --
        // images under 16 pixels on a side lost every cut that misses their first rows)
        const int ylast = ty0 + 15 < g.H - 1 ? ty0 + 15 : g.H - 1, xlast = tx0 + 15 < g.W - 1 ? tx0 + 15 : g.W - 1;
        const int Ya = wrap(ty0 + g.py0, g.H) + ay * g.H, Yb = wrap(ylast + g.py0, g.H) + ay * g.H;
        const int Xa = wrap(tx0 + g.px0, g.W) + ax * g.W, Xb = wrap(xlast + g.px0, g.W) + ax * g.W;
        const bool yhit = Yb < Ya ? true : (Yb >= oy && Ya < oy + cs);
        const bool xhit = Xb < Xa ? true : (Xb >= ox && Xa < ox + cs);
        return yhit && xhit;
      }, [&](int pos, int k) { vlist[pos] = vbase + k; });
    }
    __syncthreads();
    const int nlist = vcount;
    for (int b0 = 0; b0 < nlist; b0 += NB) {
      // ---- 2. tables for up to NB cuts: thread -> (cut vb, row/col idx)
      {
        const int vb = threadIdx.x >> 5, idx = threadIdx.x & 31;
        AdjEntry e;
#pragma unroll
        for (int a = 0; a < 4; ++a) { e.off[a] = 0; e.w[a] = 0.f; }
        if (b0 + vb < nlist) {
          const int v = vlist[b0 + vb];
          const int s = v / (nay * nax), al = v - s * (nay * nax), ay = al / nax, ax = al - ay * nax;
          const int cs = table[3 * s], ox = table[3 * s + 1], oy = table[3 * s + 2];
          const float scale = cut_scale(cs, g.size);
          const bool generic = !(scale >= 1.0f);
          // a source position lies inside the 4-tap windows of at most floor(4 / scale) + 1 outputs per axis (<= 4 entries):
          // wave-uniform loop bounds instead of 4 x 4 mostly-zero products for the (common) strongly down-sampling cuts
          int run = (int)floorf(4.0f / (scale > 1.0f ? scale : 1.0f)) + 1;
          run = run > 4 ? 4 : run;
          if (idx == 0) { vinfo[vb][0] = v; vinfo[vb][1] = generic ? 1 : 0; vinfo[vb][2] = run; }
          if (!generic) {
            const bool isrow = idx < 16;
            const int q = isrow ? wrap(ty0 + idx + g.py0, g.H) + ay * g.H - oy : wrap(tx0 + (idx - 16) + g.px0, g.W) + ax * g.W - ox;
            const int lim = isrow ? g.Hp : g.Wp;
            const int absq = q + (isrow ? oy : ox);
            if (q >= 0 && q < cs && q < maxcs && absq < lim) e = tab[((size_t)s * 2 + (isrow ? 0 : 1)) * maxcs + q];
          }
        } else if (idx == 0) { vinfo[vb][0] = -1; vinfo[vb][1] = 0; vinfo[vb][2] = 0; }
        ent[vb][idx] = e;
      }
      __syncthreads();
      // ---- 3. accumulate
      for (int vb = 0; vb < NB; ++vb) {
        const int v = vinfo[vb][0];
        if (v < 0) break;
        const int s = v / (nay * nax);
        if (vinfo[vb][1]) {
          // generic per-pixel path (up-sampling cut)
          const int al = v - s * (nay * nax), ay = al / nax, ax = al - ay * nax;
          const int cs = table[3 * s], ox = table[3 * s + 1], oy = table[3 * s + 2];
          const int Y = wrap(y + g.py0, g.H) + ay * g.H, X = wrap(x + g.px0, g.W) + ax * g.W;
          const int yc = Y - oy, xc = X - ox;
          if (live && Y < g.Hp && X < g.Wp && yc >= 0 && yc < cs && xc >= 0 && xc < cs)
            upsample_cut_sum<OUT, 3>(gout, (size_t)s * ccut, L, cut_scale(cs, g.size), cs, yc, xc, acc);
          continue;
        }
        const AdjEntry re = ent[vb][ty], ce = ent[vb][16 + tx];
        if (re.w[0] == 0.f && re.w[1] == 0.f) continue;     // (a run starts with its first non-zero weight)
        const size_t gb = (size_t)s * ccut;
        const int run = vinfo[vb][2];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          if (a >= run) break;
          if (re.w[a] == 0.f) continue;
#pragma unroll
          for (int bq = 0; bq < 4; ++bq) {
            if (bq >= run) break;
            if (ce.w[bq] == 0.f) continue;
            const float w = re.w[a] * ce.w[bq];
            const int o = re.off[a] + ce.off[bq];
            acc[0] += w * L.load(gout, gb + o);
            acc[1] += w * L.load(gout, gb + o + cchan);
            acc[2] += w * L.load(gout, gb + o + 2 * cchan);
          }
        }
      }
      __syncthreads();
    }
  }
  if (live) {
    const size_t HW = (size_t)g.H * g.W, o = (size_t)y * g.W + x;
    const float k0 = OUT == APH_OUT_NCHW_RAW ? gscale : gscale / kClipStd[0];
    const float k1 = OUT == APH_OUT_NCHW_RAW ? gscale : gscale / kClipStd[1];
    const float k2 = OUT == APH_OUT_NCHW_RAW ? gscale : gscale / kClipStd[2];
    grgb[o] = acc[0] * k0;
    grgb[HW + o] = acc[1] * k1;
    grgb[2 * HW + o] = acc[2] * k2;
  }
}

// ---------------------------------------------------------------------------------
// [r3] Crop / resize adjoint, SEPARABLE and row-block stationary (frames without wrap padding: --align uniform / central).
//
//   d img[oy + q][ox + p] += sum_i Wy[i -> q] * ( sum_j Wx[j -> p] * G[i][j] )        per cut, Wy / Wx = the per-cut 1-D tap tables
//
// The gather kernel above visits every (pixel, covering cut) pair with up to 16 gathers x 3 channels and is bound by that per-pair
// skeleton (332 us at C2).  Here a workgroup owns RB image rows of ONE channel across the whole width, every thread owns CPT columns and
// keeps their RB accumulators in registers.  The covering cuts are walked in index order (deterministic, no atomics) in batches of NBC:
//   phase 0  the batch's cut boxes -> LDS; per (cut, four image rows) the union of the <= 8 gradient rows their taps come from, with
//            one weight per image row (QuadRow)
//   phase 1  column pass: U[b][j][4 qq .. 4 qq + 3] = sum_r W[r][.] * G_b[i_lo + r][j] for all `size` columns of each cut (coalesced
//            along j; a gradient row is read once per four image rows it feeds, the four results leave as one 16-byte LDS write)
//   phase 2  row pass: acc[q][x] += sum_b wx[b] * U[b][j_b][q], the RB rows of a column tap fetched as 16-byte LDS reads
// Up-sampling cuts (cs < size: never at 1280x720) take the per-pixel generic path of the gather kernel.
// ---------------------------------------------------------------------------------
struct __attribute__((aligned(16))) QuadRow {      // one gradient row of the union behind four consecutive image rows of a cut
  float w[4];        // its weight on each of the four image rows
  int off;           // gradient-layout row offset, -1 = unused
  int pad[3];
};
constexpr int ADJ_NBC = 12;         // cuts per batch (the launcher lowers it when LDS is short)

template <int OUT, int RBQ, int CPT>
__global__ __launch_bounds__(768) void crop_adjoint_rows_kernel(const void* __restrict__ gout, float gscale, const int* __restrict__ table,
                                                                 float* __restrict__ grgb, Geom g, const AdjEntry* __restrict__ tab, int maxcs,
                                                                 int RB, int NBC, int XW, int center_out) {
  // [r4] XW: columns per workgroup; blockIdx.z selects the column segment [x0, x0 + XW) (frames wider than 768 threads x 3 columns: the
  // 3840-wide C4 frame is two segments; a segment culls the cuts that do not reach it)
  constexpr int RBP = RBQ * 4, MAXV = 512;
  APH_DYN_SMEM(smem);
  float* U = reinterpret_cast<float*>(smem);                                   // [NBC][size][RBP]
  QuadRow* qtab2 = reinterpret_cast<QuadRow*>(U + (size_t)NBC * g.size * RBP); // [2][NBC][RBQ][8]: the <= 8 gradient rows behind four image rows
  int* binfo2 = reinterpret_cast<int*>(qtab2 + 2 * NBC * RBQ * 8);             // [2][NBC][4] = s (-1: none), cs, ox, oy (cs < 0: generic cut)
  int* vlist = binfo2 + 2 * NBC * 4;                                           // [MAXV]
  int* vbox = vlist + MAXV;                                                    // [MAXV][3] = cs, ox, oy of the listed cuts
  int* vcount = vbox + 3 * MAXV;
  const int tid = threadIdx.x, nthr = blockDim.x;
  // [r6] center_out: workgroup i of a (channel, segment) takes row block centre + i / 2 (i even) or centre - (i + 1) / 2 (i odd): with random crops the
  // middle rows of the frame are covered by the most cuts (1.2x the mean, 3.6x the edge blocks), and a grid with more workgroups than CUs
  // should start its longest items first
  const int nrb = gridDim.x, bi = blockIdx.x, rbi = center_out ? ((bi & 1) ? nrb / 2 - (bi + 1) / 2 : nrb / 2 + bi / 2) : bi;
  const int c = blockIdx.y, y0 = rbi * RB;
  const int x0 = blockIdx.z * XW, x1 = (x0 + XW < g.W ? x0 + XW : g.W);
  const int rows = g.H - y0 < RB ? g.H - y0 : RB;
  const Layout<OUT> L(g.size, g.patch);
  const int cchan = L.chan_stride(), ccut = L.cut_stride();
  f32x4 acc[CPT][RBQ];
#pragma unroll
  for (int i = 0; i < CPT; ++i)
#pragma unroll
    for (int k = 0; k < RBQ; ++k) acc[i][k] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < NBC * g.size * RBP; i += nthr) U[i] = 0.f;              // (the padding rows q >= RB stay zero for good)
  for (int vbase = 0; vbase < g.S; vbase += MAXV) {
    // ---- ordered list of the cuts that touch this row block (wave 0, ballot compaction)
    __syncthreads();
    if (tid < 64) {
      int cs = 0, ox = 0, oy = 0;
      wave0_compact(g.S - vbase < MAXV ? g.S - vbase : MAXV, vcount, [&](int k) {
        const int s = vbase + k;
        cs = table[3 * s]; ox = table[3 * s + 1]; oy = table[3 * s + 2];
        return oy < y0 + rows && oy + cs > y0 && ox < x1 && ox + cs > x0;
      }, [&](int pos, int k) { vlist[pos] = vbase + k; vbox[3 * pos] = cs; vbox[3 * pos + 1] = ox; vbox[3 * pos + 2] = oy; });
    }
    __syncthreads();
    const int nlist = *vcount;
    // ---- phase 0 (of batch b0, into table buffer `buf`): boxes of the batch, and per (cut, four image rows) the union of the gradient
    // rows their taps come from.  Image row y of a down-sampling cut (scale >= 1) is touched by output rows i with floor(i scale) in
    // [y - 2, y + 1] (clamped taps land on rows that are in that set anyway), so four consecutive image rows draw on i in
    // [(y - 2) / scale, (y + 5) / scale): at most 8 rows.  Thread (b, qq, r) merges the four per-row tap entries into row r of that
    // union: gradient offset + 4 weights.
    // It runs one batch AHEAD, on the last 256 threads during the row pass of the batch before: those threads own the fewest columns
    // (W = 1280 on 768 threads x 2 columns: the last four waves have one), so the two dependent table loads cost the batch nothing.
    constexpr int P0_THREADS = 256;
    const int p0_first = nthr - P0_THREADS;
    auto phase0 = [&](int b0, int buf) {
      if (tid < p0_first) return;
      QuadRow* qt = qtab2 + buf * NBC * RBQ * 8;
      int* bi = binfo2 + buf * NBC * 4;
      for (int pt = tid - p0_first; pt < NBC * RBQ * 8; pt += P0_THREADS) {
        const int b = pt / (RBQ * 8), qq = (pt >> 3) % RBQ, r = pt & 7;
        QuadRow qr;
        qr.off = -1; qr.w[0] = qr.w[1] = qr.w[2] = qr.w[3] = 0.f;
        if (b0 + b < nlist) {
          const int s = vlist[b0 + b];
          const int cs = vbox[3 * (b0 + b)], ox = vbox[3 * (b0 + b) + 1], oy = vbox[3 * (b0 + b) + 2];      // (kept by the list build: one dependent load less)
          const bool generic = !(cut_scale(cs, g.size) >= 1.0f);
          if (qq == 0 && r == 0) { bi[4 * b] = s; bi[4 * b + 1] = generic ? -cs : cs; bi[4 * b + 2] = ox; bi[4 * b + 3] = oy; }
          if (!generic) {
            AdjEntry e[4];
            int i0[4], ilo = 1 << 30;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int q = 4 * qq + k, yc = y0 + q - oy;
              const bool live = q < rows && yc >= 0 && yc < cs && yc < maxcs;
              if (live) e[k] = tab[((size_t)s * 2) * maxcs + yc];
              i0[k] = 1 << 30;
              if (live && (e[k].w[0] != 0.f || e[k].w[1] != 0.f || e[k].w[2] != 0.f || e[k].w[3] != 0.f)) i0[k] = L.row_of(e[k].off[0]);
              else { e[k].w[0] = e[k].w[1] = e[k].w[2] = e[k].w[3] = 0.f; }
              ilo = i0[k] < ilo ? i0[k] : ilo;
            }
            if (ilo < (1 << 30)) {
              const int i = ilo + r;
              bool any = false;
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                float w = 0.f;
#pragma unroll
                for (int a = 0; a < 4; ++a) w += (i0[k] + a == i) ? e[k].w[a] : 0.f;
                qr.w[k] = w;
                any = any || w != 0.f;
              }
              if (any && i < g.size) qr.off = L.rowpart(i);
            }
          }
        } else if (qq == 0 && r == 0) bi[4 * b] = -1;
        qt[pt] = qr;
      }
    };
    phase0(0, 0);
    __syncthreads();
    for (int b0 = 0, cur = 0; b0 < nlist; b0 += NBC, cur ^= 1) {
      const QuadRow* qtab = qtab2 + cur * NBC * RBQ * 8;
      const int* binfo = binfo2 + cur * NBC * 4;
      // ---- phase 1: column pass into U[b][j][4 qq .. 4 qq + 3]: one wave per (cut, four rows), lanes across the cut's columns; the
      // gradient rows of the union are read once for the four image rows they feed, and the four results leave as one 16-byte LDS write
      // (the scalar writes of a per-row pass are 8-way bank conflicted under the 16-byte-aligned column pitch the row pass needs)
      const int nb = nlist - b0 < NBC ? nlist - b0 : NBC;
      {
        // one quad per wave and trip, its 32 gathers issued before the first is used: the pass is bound by memory latency
        const int lane = tid & 63, wv = tid >> 6, nwv = nthr >> 6, nquad = nb * RBQ;
        constexpr int JT = 4;                                      // column trips of 64 lanes: size <= 256 (checked by the launcher)
        unsigned colj[JT];                                         // 32-bit lane offsets against a scalar row base: one address register per column trip
#pragma unroll
        for (int m = 0; m < JT; ++m) { const int j = lane + 64 * m; colj[m] = (unsigned)L.colpart(j < g.size ? j : 0); }
        for (int pq = wv; pq < nquad; pq += nwv) {
          float v[JT][8];
          const int b = pq / RBQ, qq = pq - b * RBQ;
          const size_t gb = (size_t)wave_uniform(binfo[4 * b]) * ccut + (size_t)c * cchan;
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            const int off = wave_uniform(qtab[pq * 8 + r].off);
            const size_t rowbase = gb + (size_t)(off >= 0 ? off : 0);
#pragma unroll
            for (int m = 0; m < JT; ++m) {
              float x = 0.f;
              if (off >= 0 && lane + 64 * m < g.size) {
                if (OUT == APH_GRAD_PATCH_F16) x = (float)(reinterpret_cast<const half_t*>(gout) + rowbase)[colj[m]];
                else x = (reinterpret_cast<const float*>(gout) + rowbase)[colj[m]];
              }
              v[m][r] = x;
            }
          }
          f32x4 u[JT];
#pragma unroll
          for (int m = 0; m < JT; ++m) u[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            const f32x4 w = *reinterpret_cast<const f32x4*>(qtab[pq * 8 + r].w);
#pragma unroll
            for (int m = 0; m < JT; ++m) u[m] += w * v[m][r];
          }
#pragma unroll
          for (int m = 0; m < JT; ++m) {
            const int j = lane + 64 * m;
            if (j < g.size) *reinterpret_cast<f32x4*>(U + ((size_t)b * g.size + j) * RBP + 4 * qq) = u[m];
          }
        }
      }
      __syncthreads();
      if (b0 + NBC < nlist) phase0(b0 + NBC, cur ^ 1);
      // ---- phase 2: row pass, cuts in list order
      // ([r5] measured and not adopted, profiles/r05_sampler_pipelined_ab.txt: the entries of groups of two cuts loaded two groups ahead into a
      // register ring -- unconditional clamped loads, partial vmcnt waits in the ISA -- 293.6 -> 301.5 us: this pass does not wait for L2; and the
      // taps of a (column, cut) read back to back without the per-tap zero-weight skips: 296.6 -> 310.4 us -- every skipped tap is three LDS reads)
      {
        // four cuts x CPT columns at a time: the first offset and the four weights of every column-tap entry (20 of its 32 bytes) are
        // loaded together, then accumulated per column in list order
#pragma unroll
        for (int bh = 0; bh < ADJ_NBC; bh += 4) {
          if (bh >= nb) break;
          f32x4 cw[CPT][4];
          int coff[CPT][4];
#pragma unroll
          for (int i = 0; i < CPT; ++i) {
            const int x = x0 + i * nthr + tid;
#pragma unroll
            for (int bb = 0; bb < 4; ++bb) {
              const int b = bh + bb;
              coff[i][bb] = -1;
              cw[i][bb] = f32x4{0.f, 0.f, 0.f, 0.f};
              if (b < nb && x < x1) {
                const int s = binfo[4 * b], csx = binfo[4 * b + 1], p = x - binfo[4 * b + 2];
                if (csx > 0 && p >= 0 && p < csx && p < maxcs) {
                  const AdjEntry* ep = tab + ((size_t)s * 2 + 1) * maxcs + p;
                  coff[i][bb] = ep->off[0];
                  cw[i][bb] = *reinterpret_cast<const f32x4*>(ep->w);
                }
              }
            }
          }
#pragma unroll
          for (int i = 0; i < CPT; ++i)
#pragma unroll
            for (int bb = 0; bb < 4; ++bb) {
              if (coff[i][bb] < 0) continue;
              // the taps of an entry are CONSECUTIVE output columns (tap_table_kernel: a contiguous run from the first non-zero weight)
              const float* u0 = U + ((size_t)(bh + bb) * g.size + L.col_of(coff[i][bb])) * RBP;
#pragma unroll
              for (int t = 0; t < 4; ++t) {
                if (cw[i][bb][t] == 0.f) continue;
                const float* up = u0 + t * RBP;
#pragma unroll
                for (int k = 0; k < RBQ; ++k) acc[i][k] += cw[i][bb][t] * *reinterpret_cast<const f32x4*>(up + 4 * k);
              }
            }
        }
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
          const int x = x0 + i * nthr + tid;
          if (x >= x1) continue;
          // up-sampling cuts (cs < size; none at 1280x720): the per-pixel generic path of crop_resize_adjoint_kernel.  Kept out of the
          // unrolled loop above (a loop the compiler does not unroll would index ce[] at run time and move it to scratch memory); the
          // sum of such a cut is added after the batch's table-driven cuts -- a fixed order all the same.
          for (int b = 0; b < nb; ++b) {
            const int csx = binfo[4 * b + 1];
            if (csx >= 0) continue;
            const int s = binfo[4 * b], oy = binfo[4 * b + 3], cs = -csx, p = x - binfo[4 * b + 2];
            if (p < 0 || p >= cs) continue;
            const float scale = cut_scale(cs, g.size);
            const size_t gb = (size_t)s * ccut + (size_t)c * cchan;
#pragma unroll
            for (int q = 0; q < RBP; ++q) {            // (fully unrolled: a run-time index into acc would move it to scratch memory)
              const int yc = y0 + q - oy;
              if (q >= rows || yc < 0 || yc >= cs) continue;
              float sum[1] = {0.f};
              upsample_cut_sum<OUT, 1>(gout, gb, L, scale, cs, yc, p, sum);
              acc[i][q >> 2][q & 3] += sum[0];
            }
          }
        }
      }
      __syncthreads();
    }
  }
  const float kc = OUT == APH_OUT_NCHW_RAW ? gscale : gscale / kClipStd[c];
  const size_t HW = (size_t)g.H * g.W;
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int x = x0 + i * nthr + tid;
    if (x >= x1) continue;
#pragma unroll
    for (int k = 0; k < RBQ; ++k)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = 4 * k + r;
        if (q < rows) grgb[(size_t)c * HW + (size_t)(y0 + q) * g.W + x] = acc[i][k][r] * kc;
      }
  }
}

// 1: always the round-2 gather kernel (aph_crop_adjoint_set_gather: A/B runs and the equivalence tests)
inline int& crop_adjoint_gather() {
  static int v = 0;
  return v;
}

// launch shape of the separable crop adjoint: 0 / -1 = automatic (aph_crop_adjoint_set_shape: the sweep of tools/exp/crop_adjoint_sweep.py)
struct CropAdjointShape { int rb = 0, cpt = 0, nbc = 0, nseg = 0, order = -1; };
inline CropAdjointShape& crop_adjoint_shape() {
  static CropAdjointShape v;
  return v;
}
inline int device_cu_count() {          // CUs of the current device (256 on MI355X); the interpreter build says 3 so that the centre-out order is exercised
#ifdef APH_EMU
  return 3;
#else
  static const int n = [] { int dev = 0, cu = 256; if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev); return cu > 0 ? cu : 256; }();
  return n;
#endif
}

template <int OUT>
int launch_crop_adjoint(const void* gout, float gscale, const int* table, float* grgb, const Geom& g, AdjEntry* tab, hipStream_t st) {
  const int maxcs = g.Hp < g.Wp ? g.Hp : g.Wp;
  APH_LAUNCH(tap_table_kernel<OUT>, dim3((maxcs + 127) / 128, 2, g.S), dim3(128), 0, st, table, tab, maxcs, g);
  // [r3] frames without wrap padding: the separable row-block kernel (APH_CROP_ADJOINT=gather keeps the round-2 gather kernel for A/B runs)
  if (!crop_adjoint_gather() && g.Hp == g.H && g.Wp == g.W && g.py0 == 0 && g.px0 == 0 && g.W <= 4 * 2304 && g.size <= 256) {
    // column segments of at most 2304 (768 threads x 3 columns); [r4] wider frames (C4: 3840) take several segments per row block
    int nseg = (g.W + 2303) / 2304;
    const CropAdjointShape& ov = crop_adjoint_shape();
    if (ov.nseg > 0) nseg = ov.nseg;
    const int xw = ((g.W + nseg - 1) / nseg + 3) & ~3;
    int cpt = xw <= 1536 ? 2 : 3;                             // columns per thread, at most 768 threads (three waves per SIMD: 168 VGPRs)
    if (ov.cpt > 0) cpt = ov.cpt;
    int nthr = (((xw + cpt - 1) / cpt) + 63) / 64 * 64;
    nthr = nthr < 256 ? 256 : nthr;
    if (nthr > 768) return aph_fail(APH_ERR_ARG, "crop adjoint: %d columns per segment need more than 768 threads x %d columns", xw, cpt);
    // rows per workgroup: about one workgroup per CU over rows x 3 channels (85 row blocks), 12 or 16 accumulator rows per column.
    // [r6] launch-shape sweep (tools/exp/crop_adjoint_sweep.py, profiles/r06_crop_adjoint_sweep.txt): at 1280x720 / 190 cuts the automatic
    // 9 rows x 2 columns x 1 segment (240 workgroups) is the fastest of 180 shapes (293 us with the tap tables; every finer split of rows or
    // columns loses: the pass pays per (column, cut) entry, and more rows per workgroup amortise it); at 3840x2160 / 95 cuts 16 rows x
    // 3 columns x 2 segments takes 495 us against 581 for the 12 rows segmented frames used to be held at (the 168-VGPR concern of round 4
    // did not materialise: no scratch in the ISA)
    int rb = (g.H + 84) / 85;
    rb = rb < 4 ? 4 : (rb > 16 ? 16 : rb);
    if (ov.rb > 0) rb = ov.rb;
    int rbq = rb <= 12 ? 3 : 4;
    const int rbp = rbq * 4;
    int nbc = ov.nbc > 0 && ov.nbc <= ADJ_NBC ? ov.nbc : ADJ_NBC;
    auto lds = [&](int n) { return (size_t)n * g.size * rbp * 4 + 2 * (size_t)n * rbq * 8 * sizeof(QuadRow) + 2 * (size_t)n * 16 + 512 * 16 + 16; };
    while (nbc > 1 && lds(nbc) > 150 * 1024) --nbc;
    if (lds(nbc) <= 150 * 1024) {
      const dim3 rgrid((g.H + rb - 1) / rb, 3, nseg);
      const size_t smem = lds(nbc);
      const int center_out = ov.order >= 0 ? ov.order : ((int)(rgrid.x * 3 * nseg) > device_cu_count() ? 1 : 0);
      auto rows = [&](auto rbq_, auto cpt_) {
        constexpr int RBQ = decltype(rbq_)::value, CPT = decltype(cpt_)::value;
        APH_ALLOW_SMEM((crop_adjoint_rows_kernel<OUT, RBQ, CPT>), 150 * 1024);
        APH_LAUNCH((crop_adjoint_rows_kernel<OUT, RBQ, CPT>), rgrid, dim3(nthr), smem, st, gout, gscale, table, grgb, g, (const AdjEntry*)tab, maxcs, rb, nbc, xw, center_out);
      };
      using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>; using I4 = std::integral_constant<int, 4>;
      if (rbq == 3 && cpt == 2) rows(I3{}, I2{});
      else if (rbq == 3) rows(I3{}, I3{});
      else if (cpt == 2) rows(I4{}, I2{});
      else rows(I4{}, I3{});
      return APH_OK;
    }
  }
  const dim3 agrid(8 * (((g.H + 15) / 16 + 7) / 8) * ((g.W + 15) / 16));        // 8 XCD shares of ceil(tile rows / 8) rows each (see the kernel's tile order)
  APH_LAUNCH(crop_resize_adjoint_kernel<OUT>, agrid, dim3(256), 0, st, gout, gscale, table, grgb, g, (const AdjEntry*)tab, maxcs);
  return APH_OK;
}

}  // namespace aph
