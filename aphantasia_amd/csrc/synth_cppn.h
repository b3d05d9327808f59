// CPPN generator (the reference's cppn.py:71-116): a coordinate network of 1x1 convolutions, image = sigmoid(net(x, y)), whose weights are
// the optimised parameters.  Forward and backward are one launch each, every layer fused per pixel tile; a third launch sums the
// per-workgroup gradient partials in a fixed order.  Included by synth.hip.
//
//   conv 0: 2 -> nf | conv 1 .. layers-1: nhi -> nf | conv `layers`: nhi -> 3, sigmoid          nhi = 2 nf (unbias, comp) or nf (relu)
//   unbias: t = atan(z), cat[t / 0.67, (t^2 - 0.45) / 0.396]   comp: cat[t / 0.67, t^2 / 0.6]   relu: (relu(z) - 0.40) / 0.58
//   flat parameters: per conv in network order weight[out][in] row-major, then bias[out]
//
// Arithmetic: f32 end to end on v_mfma_f32_32x32x2_f32 (an exact k-ordered fmaf chain).  The WEIGHTS are the A operand (rows = output
// channels, padded to 32 with zeros), the PIXELS the N dimension: a wave owns 32 pixels per MFMA tile, lane l holds pixel l & 31, and the
// D layout leaves channel ch(r, h) = (r & 3) + 8 (r >> 2) + 4 h of that pixel in register r of half h = l >> 5.  The activation is then
// lane-local, and register r feeds the next layer's B operand at k-step r directly, because the weight columns are permuted on their way
// into LDS: the A fragment of k-step r holds column ch(r, h) in half h (the trick of gemm_ws_brow).  Only the weight gradient, which
// contracts over pixels, needs a transpose: dz and the layer's input go through a per-wave LDS tile and come back as A / B fragments.
//
// Tiling: a workgroup of 4 waves takes 512 pixels per pass, each wave 4 sub-tiles of 32; workgroups stride over the passes.  In the
// backward a wave keeps dz of its 4 sub-tiles in registers (64) and walks the layers from the output down, so that one layer's weight
// gradient accumulates in registers (32) over the 4 sub-tiles before the 4 waves' sums are added, in wave order, into the workgroup's own
// row of partials.  No atomics: the same shapes give the same bits.
//
// The forward stashes each hidden conv's pre-activation z (f32, [layer][channel][pixel]) when given a workspace; the backward reads it and
// recomputes t = atan(z), so that the activation's derivative is 1 / (1 + z^2) as in the reference's autograd (layers nf 4 B per pixel).
#pragma once
#include "aph_device.h"
#include "aph_host.h"

namespace aph {

constexpr int kCppnMaxLayers = 12, kCppnMaxNf = 32;
constexpr int kCppnSub = 4, kCppnWaves = 4;                 // 32-pixel sub-tiles per wave; waves per workgroup
constexpr int kCppnTile = 32 * kCppnSub * kCppnWaves;       // pixels per workgroup pass
constexpr int kCppnFwdBlocks = 512, kCppnBwdBlocks = 256;   // grid caps (256 CUs; the forward's LDS lets two workgroups share one)
constexpr int kCppnTrow = 33;                               // padded row of the transpose tiles (floats)
constexpr int kCppnScratch = 3 * 32 * kCppnTrow;            // per wave: dz^T [32][33], input^T [2][32][33]

struct CppnNet {
  int layers, nf, act, nq, nhi, ks;       // nq = activation parts (2, relu 1); nhi = nq nf; ks = k-steps that cover nf channels (4 per 8)
  __host__ __device__ int nin(int l) const { return l == 0 ? 2 : nhi; }
  __host__ __device__ int nout(int l) const { return l == layers ? 3 : nf; }
  __host__ __device__ int off(int l) const { return l == 0 ? 0 : 3 * nf + (l - 1) * (nf * nhi + nf); }
  __host__ __device__ int count() const { return off(layers) + 3 * nhi + 3; }
  // LDS floats of the forward: conv 0 [64], biases [layers + 1][32], then conv l >= 1 as [nq][ks][64]
  __host__ __device__ int fwd_lds() const { return 64 + (layers + 1) * 32 + layers * nq * ks * 64; }
  // LDS floats of the backward's transposed weights: conv 1 .. layers-1 as [nq][ks][64], the output conv as [nq][4][64]
  __host__ __device__ int bwd_w(int l) const { return (l - 1) * nq * ks * 64; }
  __host__ __device__ int bwd_lds() const { return bwd_w(layers) + nq * 4 * 64 + kCppnWaves * kCppnScratch; }
};

static inline CppnNet cppn_net(int layers, int nf, int act) {
  CppnNet n;
  n.layers = layers; n.nf = nf; n.act = act;
  n.nq = act == 2 ? 1 : 2;
  n.nhi = n.nq * nf;
  n.ks = 4 * ((nf + 7) / 8);
  return n;
}

__device__ __forceinline__ int cppn_ch(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

template <int ACT>
__device__ __forceinline__ void cppn_act(float z, float& t, float& a0, float& a1) {
  if (ACT == 2) {
    t = z;
    a0 = (fmaxf(z, 0.f) - 0.40f) * (float)(1.0 / 0.58);
    a1 = 0.f;
  } else {
    t = atanf(z);
    a0 = t * (float)(1.0 / 0.67);
    a1 = ACT == 0 ? (t * t - 0.45f) * (float)(1.0 / 0.396) : t * t * (float)(1.0 / 0.6);
  }
}

// d loss / d z from the gradients of the two activation parts
template <int ACT>
__device__ __forceinline__ float cppn_act_bwd(float d0, float d1, float z, float t) {
  if (ACT == 2) return z > 0.f ? d0 * (float)(1.0 / 0.58) : 0.f;
  const float k1 = ACT == 0 ? (float)(2.0 / 0.396) : (float)(2.0 / 0.6);
  return (d0 * (float)(1.0 / 0.67) + d1 * (t * k1)) / (1.0f + z * z);
}

// params -> rgb [3][HW]; stash (nullable) [layers][nf][HW] <- z of conv 0 .. layers-1
template <int ACT>
__global__ __launch_bounds__(256) void cppn_fwd_kernel(const float* __restrict__ params, CppnNet net, const float* __restrict__ xs,
                                                       const float* __restrict__ ys, int W, size_t HW, float* __restrict__ stash,
                                                       float* __restrict__ rgb, int ntiles) {
  APH_DYN_SMEM(smem);
  float* w0 = reinterpret_cast<float*>(smem);
  float* bias = w0 + 64;
  float* wf = bias + (net.layers + 1) * 32;
  const int L = net.layers, nf = net.nf, nq = net.nq, ks = net.ks, nhi = net.nhi;
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int e = tid; e < 64; e += nt) {
    const int i = e & 31, h = e >> 5;
    w0[e] = i < nf ? params[i * 2 + h] : 0.f;
  }
  for (int e = tid; e < (L + 1) * 32; e += nt) {
    const int l = e >> 5, c = e & 31;
    bias[e] = c < net.nout(l) ? params[net.off(l) + net.nout(l) * net.nin(l) + c] : 0.f;
  }
  for (int e = tid; e < L * nq * ks * 64; e += nt) {
    const int i = e & 31, h = (e >> 5) & 1, rest = e >> 6;
    const int r = rest % ks, q = (rest / ks) % nq, l = 1 + rest / (ks * nq), c = cppn_ch(r, h);
    wf[e] = (i < net.nout(l) && c < nf) ? params[net.off(l) + i * nhi + q * nf + c] : 0.f;
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6, n = lane & 31, h = lane >> 5;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    for (int s = 0; s < kCppnSub; ++s) {
      const size_t base = (size_t)tile * kCppnTile + (size_t)(wave * kCppnSub + s) * 32;
      if (base >= HW) continue;                     // (the whole wave)
      const size_t p = base + n;
      const bool valid = p < HW;
      const size_t pc = valid ? p : HW - 1;
      const float in = h ? ys[pc / W] : xs[pc % W];
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = bias[cppn_ch(r, h)];
      acc = mfma_32x32x2_f32(w0[lane], in, acc);
      for (int l = 1; l <= L; ++l) {
        f32x16 a0, a1;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float t, u0, u1;
          cppn_act<ACT>(acc[r], t, u0, u1);
          a0[r] = u0; a1[r] = u1;
          const int c = cppn_ch(r, h);
          if (stash && valid && c < nf) stash[((size_t)(l - 1) * nf + c) * HW + p] = acc[r];
        }
        const float* bl = bias + l * 32;
        const float* wl = wf + (size_t)(l - 1) * nq * ks * 64;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = bl[cppn_ch(r, h)];
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (r < ks) acc = mfma_32x32x2_f32(wl[r * 64 + lane], a0[r], acc);
        if (nq == 2) {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (r < ks) acc = mfma_32x32x2_f32(wl[(ks + r) * 64 + lane], a1[r], acc);
        }
      }
      if (valid && h == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[(size_t)c * HW + p] = 1.0f / (1.0f + expf(-acc[c]));
      }
    }
  }
}

// d rgb (x gscale) -> this workgroup's row of `partials` [gridDim.x][P]: the parameter gradient summed over the workgroup's pixels
template <int ACT>
__global__ __launch_bounds__(256) void cppn_bwd_kernel(const float* __restrict__ params, CppnNet net, const float* __restrict__ xs,
                                                       const float* __restrict__ ys, int W, size_t HW, const float* __restrict__ drgb,
                                                       float gscale, const float* __restrict__ rgb, const float* __restrict__ stash,
                                                       float* __restrict__ partials, int P, int ntiles) {
  APH_DYN_SMEM(smem);
  float* wb = reinterpret_cast<float*>(smem);
  const int L = net.layers, nf = net.nf, nq = net.nq, ks = net.ks, nhi = net.nhi;
  float* scratch = wb + net.bwd_w(L) + nq * 4 * 64;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int nhid = net.bwd_w(L);
  for (int e = tid; e < nhid + nq * 4 * 64; e += nt) {
    const bool out = e >= nhid;
    const int f = out ? e - nhid : e, kso = out ? 4 : ks;
    const int i = f & 31, h = (f >> 5) & 1, rest = f >> 6;
    const int r = rest % kso, q = (rest / kso) % nq, l = out ? L : 1 + rest / (kso * nq), c = cppn_ch(r, h);
    wb[e] = (c < net.nout(l) && i < nf) ? params[net.off(l) + c * nhi + q * nf + i] : 0.f;
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6, n = lane & 31, h = lane >> 5;
  float* dzT = scratch + wave * kCppnScratch;
  float* aT = dzT + 32 * kCppnTrow;
  float* mine = partials + (size_t)blockIdx.x * P;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const bool first = tile == (int)blockIdx.x;
    const size_t pbase = (size_t)tile * kCppnTile + (size_t)wave * (32 * kCppnSub);
    f32x16 dz[kCppnSub];
#pragma unroll
    for (int s = 0; s < kCppnSub; ++s) {
      const size_t p = pbase + s * 32 + n;
#pragma unroll
      for (int r = 0; r < 16; ++r) dz[s][r] = 0.f;
      if (p < HW && h == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float v = rgb[(size_t)c * HW + p];
          dz[s][c] = drgb[(size_t)c * HW + p] * gscale * (v * (1.0f - v));
        }
      }
    }
    for (int l = L; l >= 0; --l) {
      f32x16 acc0, acc1;
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
      float db = 0.f;
      const bool two = nq == 2 && l > 0;
#pragma unroll
      for (int s = 0; s < kCppnSub; ++s) {
        const size_t base = pbase + s * 32;
        if (base < HW) {                            // (the whole wave)
          const size_t p = base + n;
          const bool valid = p < HW;
          f32x16 z, t, a0, a1;
          if (l > 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int c = cppn_ch(r, h);
              z[r] = (valid && c < nf) ? stash[((size_t)(l - 1) * nf + c) * HW + p] : 0.f;
              float tt, u0, u1;
              cppn_act<ACT>(z[r], tt, u0, u1);
              t[r] = tt; a0[r] = u0; a1[r] = u1;
            }
          } else {
            const size_t pc = valid ? p : HW - 1;
#pragma unroll
            for (int r = 0; r < 16; ++r) { z[r] = 0.f; t[r] = 0.f; a0[r] = 0.f; a1[r] = 0.f; }
            if (h == 0) { a0[0] = xs[pc % W]; a0[1] = ys[pc / W]; }
          }
          // the weight gradient contracts over pixels: dz and the layer's input, transposed through LDS, as A and B fragments
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int c = cppn_ch(r, h);
            dzT[c * kCppnTrow + n] = dz[s][r];
            aT[c * kCppnTrow + n] = a0[r];
            if (two) aT[(32 + c) * kCppnTrow + n] = a1[r];
          }
          wave_lds_fence();
#pragma unroll
          for (int st = 0; st < 16; ++st) {
            const float a = dzT[n * kCppnTrow + 2 * st + h];
            acc0 = mfma_32x32x2_f32(a, aT[n * kCppnTrow + 2 * st + h], acc0);
            if (two) acc1 = mfma_32x32x2_f32(a, aT[(32 + n) * kCppnTrow + 2 * st + h], acc1);
          }
          if (lane < 32)
            for (int px = 0; px < 32; ++px) db += dzT[lane * kCppnTrow + px];
          wave_lds_fence();
          if (l > 0) {                              // dz of the conv below: W^T dz, then the activation's derivative
            f32x16 d0, d1;
#pragma unroll
            for (int r = 0; r < 16; ++r) { d0[r] = 0.f; d1[r] = 0.f; }
            const int kso = l == L ? 4 : ks;
            const float* wl = wb + net.bwd_w(l);
#pragma unroll
            for (int r = 0; r < 16; ++r)
              if (r < kso) {
                d0 = mfma_32x32x2_f32(wl[r * 64 + lane], dz[s][r], d0);
                if (nq == 2) d1 = mfma_32x32x2_f32(wl[(kso + r) * 64 + lane], dz[s][r], d1);
              }
#pragma unroll
            for (int r = 0; r < 16; ++r) dz[s][r] = cppn_act_bwd<ACT>(d0[r], d1[r], z[r], t[r]);
          }
        }
      }
      // the four waves' sums of this conv, added in wave order into the workgroup's partial row
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = cppn_ch(r, h);
        aT[c * 32 + n] = acc0[r];
        aT[1024 + c * 32 + n] = acc1[r];
      }
      if (lane < 32) dzT[lane] = db;
      __syncthreads();
      const int nout = net.nout(l), nin = net.nin(l), nw = nout * nin;
      for (int e = tid; e < nw + nout; e += nt) {
        int idx = e - nw;                           // bias: dzT[out]
        if (e < nw) {
          const int o = e / nin, i = e - o * nin, q = l > 0 ? i / nf : 0;
          idx = 32 * kCppnTrow + q * 1024 + o * 32 + (i - q * nf);
        }
        float v = 0.f;
        for (int w = 0; w < kCppnWaves; ++w) v += scratch[w * kCppnScratch + idx];
        float* dst = mine + net.off(l) + e;
        *dst = first ? v : *dst + v;
      }
      __syncthreads();
    }
  }
}

// partials [nrows][P] -> grad [P]: 32 parameters x 8 row slices per workgroup, each slice in row order, the slices in slice order (fp64)
__global__ __launch_bounds__(256) void cppn_reduce_kernel(const float* __restrict__ partials, int nrows, int P, float* __restrict__ grad) {
  __shared__ double red[8][32];
  const int j = threadIdx.x & 31, sl = threadIdx.x >> 5, idx = blockIdx.x * 32 + j;
  double s = 0.0;
  if (idx < P)
    for (int g = sl; g < nrows; g += 8) s += (double)partials[(size_t)g * P + idx];
  red[sl][j] = s;
  __syncthreads();
  if (sl == 0 && idx < P) {
    double total = 0.0;
    for (int k = 0; k < 8; ++k) total += red[k][j];
    grad[idx] = (float)total;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
// -> APH_OK, or the error of a (layers, nf, act, H, W) outside the supported range, naming `call`
static inline int cppn_check_shape(const char* call, int layers, int nf, int act, int H, int W) {
  if (H < 1 || W < 1) return aph_fail(APH_ERR_ARG, "%s: bad shape H=%d W=%d", call, H, W);
  if (layers < 1 || layers > kCppnMaxLayers)
    return aph_fail(APH_ERR_UNSUPPORTED, "%s: layers = %d, supported 1 .. %d", call, layers, kCppnMaxLayers);
  if (nf < 1 || nf > kCppnMaxNf) return aph_fail(APH_ERR_UNSUPPORTED, "%s: nf = %d, supported 1 .. %d", call, nf, kCppnMaxNf);
  if (act < 0 || act > 2) return aph_fail(APH_ERR_UNSUPPORTED, "%s: act = %d, supported 0 (unbias), 1 (comp), 2 (relu)", call, act);
  return APH_OK;
}

struct CppnLayout {           // the caller-owned workspace: [stash | partials]
  int ntiles, bwd_blocks;
  size_t stash_floats, partial_floats;
};

static inline CppnLayout cppn_layout(const CppnNet& net, int H, int W) {
  CppnLayout g;
  const size_t HW = (size_t)H * W;
  g.ntiles = (int)((HW + kCppnTile - 1) / kCppnTile);
  g.bwd_blocks = g.ntiles < kCppnBwdBlocks ? g.ntiles : kCppnBwdBlocks;
  g.stash_floats = ((size_t)net.layers * net.nf * HW + 63) / 64 * 64;
  g.partial_floats = (size_t)g.bwd_blocks * net.count();
  return g;
}

}  // namespace aph
