// Image parameteriser, FFT stage: the LDS-resident Stockham transform and the column / row kernels of the synthesis and its adjoint.
// Included by synth.hip.
//
// Stockham autosort, mixed radix (2/3/4/5 specialised, any other prime <= 31 generic in registers, larger primes by direct sums),
// one workgroup per column tile / per row PAIR, whole sequence resident in LDS (ping-pong).
// The C2R / R2C row transforms process two real rows as one complex sequence
// (z = a + i b), which halves the work and keeps odd W legal.
// HBM-bound: 11 MB in, 11 MB intermediate (write + read), 11 MB out at 1280x720.
#pragma once
#include "synth_rgb.h"

namespace aph {

struct Fft1D {
  int n, npass;
  int radix[14];
};

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
// multiply by SIGN * i
template <int SIGN>
__device__ __forceinline__ float2 cmuli(float2 a) {
  return SIGN > 0 ? make_float2(-a.y, a.x) : make_float2(a.y, -a.x);
}
template <int SIGN>
__device__ __forceinline__ float2 twiddle(const float2* __restrict__ tw, int t) {
  float2 w = tw[t];  // exp(+2 pi i t / N)
  if (SIGN < 0) w.y = -w.y;
  return w;
}

// Butterfly j (of nb = N / R) of sequence q in a Stockham pass of radix R over sequences of length N held in LDS: it reads x[r nb], r < R,
// term r twiddled by w^(k r tscale), tscale = N / (Ns R), and writes y[qq Ns], qq < R.
struct Butterfly {
  const float2* x;
  float2* y;
  int k;
  __device__ __forceinline__ Butterfly(const float2* src, float2* dst, int N, int R, int Ns, int q, int j)
      : x(src + q * N + j), y(dst + q * N + (j / Ns) * Ns * R + j % Ns), k(j % Ns) {}
};

// One pass over nseq sequences (src -> dst), a work item is one butterfly with its R values in registers.  RT = the radix at compile
// time: 2 / 3 / 4 have their butterflies, 5 an unrolled direct DFT; RT = 0: a run-time prime radix R <= 31, direct DFT.
template <int SIGN, int RT>
__device__ __forceinline__ void fft_pass(const float2* src, float2* dst, int N, int R_, int Ns, int nseq,
                                         const float2* __restrict__ tw) {
  const int R = RT ? RT : R_;
  const int nb = N / R, tscale = N / (Ns * R);
  for (int idx = threadIdx.x; idx < nb * nseq; idx += blockDim.x) {
    const int q = idx / nb;
    const Butterfly bf(src, dst, N, R, Ns, q, idx - q * nb);
    float2 v[RT ? RT : 32];
    for (int r = 0; r < R; ++r) {
      v[r] = bf.x[r * nb];
      if (r > 0) v[r] = cmul(v[r], twiddle<SIGN>(tw, bf.k * r * tscale));
    }
    if (RT == 2) {
      bf.y[0] = cadd(v[0], v[1]);
      bf.y[Ns] = csub(v[0], v[1]);
    } else if (RT == 3) {
      const float2 s = cadd(v[1], v[2]);
      const float2 t = make_float2(v[0].x - 0.5f * s.x, v[0].y - 0.5f * s.y);
      float2 u = csub(v[1], v[2]);
      u = cmuli<SIGN>(make_float2(u.x * 0.86602540378443865f, u.y * 0.86602540378443865f));
      bf.y[0] = cadd(v[0], s);
      bf.y[Ns] = cadd(t, u);
      bf.y[2 * Ns] = csub(t, u);
    } else if (RT == 4) {
      const float2 a0 = cadd(v[0], v[2]), a1 = csub(v[0], v[2]);
      const float2 a2 = cadd(v[1], v[3]), a3 = cmuli<SIGN>(csub(v[1], v[3]));
      bf.y[0] = cadd(a0, a2);
      bf.y[Ns] = cadd(a1, a3);
      bf.y[2 * Ns] = csub(a0, a2);
      bf.y[3 * Ns] = csub(a1, a3);
    } else {  // odd radix: direct DFT with table roots of unity
      for (int qq = 0; qq < R; ++qq) {
        float2 acc = v[0];
        for (int r = 1; r < R; ++r) acc = cadd(acc, cmul(v[r], twiddle<SIGN>(tw, ((qq * r) % R) * nb)));
        bf.y[qq * Ns] = acc;
      }
    }
  }
}

// any larger prime radix (37, 41, ... up to N itself): the R inputs of a butterfly do not fit registers, so a work item is ONE
// output: y[qq] = sum_r x[j + r nb] w^(k r tscale + (qq r mod R) nb), the two twiddles folded into one table index.  O(N R) per pass
// instead of O(N log N): sizes with a big prime factor (1366 = 2 x 683) are transformed correctly, just not fast -- torch.fft takes
// any size, and a --size the reference accepts must not be refused here.
template <int SIGN>
__device__ void fft_pass_large(const float2* src, float2* dst, int N, int R, int Ns, int nseq, const float2* __restrict__ tw) {
  const int nb = N / R, tscale = N / (Ns * R);
  for (int idx = threadIdx.x; idx < N * nseq; idx += blockDim.x) {
    const int q = idx / N, o = idx - q * N;
    const int qq = o / nb;
    const Butterfly bf(src, dst, N, R, Ns, q, o - qq * nb);
    const float2* x = bf.x;
    // (the R-term sum is kept in fp64: in fp32 its rounding grows with sqrt(R) -- 6e-6 on the image at R = 1307, found by tools/gpu_fuzz.py)
    double ar = x[0].x, ai = x[0].y;
    // twiddle index of term r: r (k tscale + qq nb) mod N  (N = R nb, so (qq r mod R) nb == qq r nb mod N): one modular add per term
    const int step = (int)(((long long)bf.k * tscale + (long long)qq * nb) % N);
    int t = 0;
    for (int r = 1; r < R; ++r) {
      t += step; if (t >= N) t -= N;
      const float2 pr = cmul(x[r * nb], twiddle<SIGN>(tw, t));
      ar += pr.x; ai += pr.y;
    }
    bf.y[qq * Ns] = make_float2((float)ar, (float)ai);
  }
}

// Full transform of nseq LDS-resident sequences; returns the buffer holding the result.
template <int SIGN>
__device__ float2* fft_lds(float2* a, float2* b, const Fft1D& plan, int nseq, const float2* __restrict__ tw) {
  int Ns = 1;
  const int N = plan.n;
  for (int p = 0; p < plan.npass; ++p) {
    const int R = plan.radix[p];
    switch (R) {
      case 2: fft_pass<SIGN, 2>(a, b, N, R, Ns, nseq, tw); break;
      case 3: fft_pass<SIGN, 3>(a, b, N, R, Ns, nseq, tw); break;
      case 4: fft_pass<SIGN, 4>(a, b, N, R, Ns, nseq, tw); break;
      case 5: fft_pass<SIGN, 5>(a, b, N, R, Ns, nseq, tw); break;
      default:
        if (R <= 31) fft_pass<SIGN, 0>(a, b, N, R, Ns, nseq, tw);
        else fft_pass_large<SIGN>(a, b, N, R, Ns, nseq, tw);
        break;
    }
    __syncthreads();
    float2* t = a; a = b; b = t;
    Ns *= R;
  }
  return a;
}

constexpr int kLoadBatch = 8;      // items per thread whose global loads are in flight together in the passes' load phases

// Element idx of a column kernel's tile: TC of the C * Wc columns (plane c, column kx; the last tile may be ragged), each H long,
// column fastest.  `valid`: idx is in the tile and its column exists; the offsets of an invalid element are those of element
// (c, y, kx) = (0, 0, 0), so a load may be issued before the value is masked.
struct ColElem {
  bool in_tile, valid;
  int lds;          // [TC][H]: where the element sits in the transform's buffer (for every element in the tile)
  int plane;        // [H][Wc]: its offset in scale / shift
  size_t global;    // [C][H][Wc]: its offset in params / tmp / grad
  __device__ __forceinline__ ColElem(int idx, int C, int H, int Wc, int TC) {
    const int t = idx % TC, y = idx / TC, g = blockIdx.x * TC + t;
    in_tile = idx < TC * H;
    valid = in_tile && g < C * Wc;
    const int c = valid ? g / Wc : 0, kx = valid ? g - c * Wc : 0;
    lds = t * H + y;
    plane = (valid ? y : 0) * Wc + kx;
    global = (size_t)c * H * Wc + plane;
  }
};

// Block of a row kernel: rows (2p, 2p + 1) of plane c as one complex sequence; the last pair of an odd H has no second row.
struct RowPair {
  size_t row0, row1, row1_or_0;      // row numbers in a [C * H][.] array; row1_or_0: a legal row to load from where the value is masked afterwards
  bool has1;
  __device__ __forceinline__ explicit RowPair(int H) {
    const int pairs = (H + 1) / 2, c = blockIdx.x / pairs, y0 = 2 * (blockIdx.x - c * pairs);
    has1 = y0 + 1 < H;
    row0 = (size_t)c * H + y0;
    row1 = row0 + 1;
    row1_or_0 = has1 ? row1 : row0;
  }
};

// ---------------------------------------------------------------------------------
// column pass, forward synthesis: tmp[c][y][kx] = sum_ky scale*params[c][ky][kx] e^{+2 pi i ky y/H}
// ---------------------------------------------------------------------------------
__global__ void fft_col_synth_kernel(const float2* __restrict__ params, const float* __restrict__ scale,
                                     const float* __restrict__ shift, float2* __restrict__ tmp, Fft1D plan,
                                     const float2* __restrict__ tw, int C, int H, int Wc, int TC) {
  APH_DYN_SMEM(smem);
  float2* a = reinterpret_cast<float2*>(smem);
  float2* b = a + TC * H;
  // kLoadBatch items per thread with all their loads issued before the first LDS write (clamped addresses, the value masked
  // afterwards): one memory round trip per batch instead of one per item
  for (int base = 0; base < TC * H; base += kLoadBatch * blockDim.x) {
    float2 v[kLoadBatch];
    float sc[kLoadBatch], sf[kLoadBatch];
#pragma unroll
    for (int u = 0; u < kLoadBatch; ++u) {
      const ColElem e(base + u * blockDim.x + threadIdx.x, C, H, Wc, TC);
      v[u] = params[e.global];
      sc[u] = scale ? scale[e.plane] : 1.0f;
      sf[u] = shift ? shift[e.plane] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kLoadBatch; ++u) {
      const ColElem e(base + u * blockDim.x + threadIdx.x, C, H, Wc, TC);
      if (e.in_tile) {
        float2 w = make_float2(0.f, 0.f);
        if (e.valid) {
          const float s = sc[u];
          w = v[u];
          w.x *= s; w.y *= s;
          if (shift) { const float sh = s * sf[u]; w.x += sh; w.y += sh; }
        }
        a[e.lds] = w;
      }
    }
  }
  __syncthreads();
  const float2* r = fft_lds<+1>(a, b, plan, TC, tw);
  for (int idx = threadIdx.x; idx < TC * H; idx += blockDim.x) {
    const ColElem e(idx, C, H, Wc, TC);
    if (e.valid) tmp[e.global] = r[e.lds];
  }
}

// column pass, adjoint: grad[c][ky][kx] = scale * sum_y tmp[c][y][kx] e^{-2 pi i ky y/H}
__global__ void fft_col_adjoint_kernel(const float2* __restrict__ tmp, const float* __restrict__ scale,
                                       float2* __restrict__ grad, Fft1D plan, const float2* __restrict__ tw,
                                       int C, int H, int Wc, int TC) {
  APH_DYN_SMEM(smem);
  float2* a = reinterpret_cast<float2*>(smem);
  float2* b = a + TC * H;
  for (int base = 0; base < TC * H; base += kLoadBatch * blockDim.x) {      // (batched loads: see fft_col_synth_kernel)
    float2 v[kLoadBatch];
#pragma unroll
    for (int u = 0; u < kLoadBatch; ++u) v[u] = tmp[ColElem(base + u * blockDim.x + threadIdx.x, C, H, Wc, TC).global];
#pragma unroll
    for (int u = 0; u < kLoadBatch; ++u) {
      const ColElem e(base + u * blockDim.x + threadIdx.x, C, H, Wc, TC);
      if (e.in_tile) a[e.lds] = e.valid ? v[u] : make_float2(0.f, 0.f);
    }
  }
  __syncthreads();
  const float2* r = fft_lds<-1>(a, b, plan, TC, tw);
  for (int idx = threadIdx.x; idx < TC * H; idx += blockDim.x) {
    const ColElem e(idx, C, H, Wc, TC);
    if (e.valid) {
      const float s = scale ? scale[e.plane] : 1.0f;
      const float2 v = r[e.lds];
      grad[e.global] = make_float2(v.x * s, v.y * s);
    }
  }
}

// ---------------------------------------------------------------------------------
// row pass, forward synthesis (C2R): rows (2p, 2p+1) of plane c as one complex transform.
// Emits raw[c][y][x] and per-block fp64 partial (sum, sum of squares) for the global std.
// ---------------------------------------------------------------------------------
__global__ void fft_row_synth_kernel(const float2* __restrict__ tmp, float* __restrict__ raw,
                                     double* __restrict__ partials, Fft1D plan, const float2* __restrict__ tw,
                                     int H, int W, int Wc, float norm) {
  APH_DYN_SMEM(smem);
  float2* a = reinterpret_cast<float2*>(smem);
  float2* b = a + W;
  __shared__ double red[16];
  const RowPair rp(H);
  const float2* ra = tmp + rp.row0 * Wc;
  const float2* rb = tmp + rp.row1_or_0 * Wc;
  for (int base = 0; base < Wc; base += kLoadBatch * blockDim.x) {      // (batched loads: see fft_col_synth_kernel)
    float2 Av[kLoadBatch], Bw[kLoadBatch];
#pragma unroll
    for (int u = 0; u < kLoadBatch; ++u) {
      const int k = base + u * blockDim.x + threadIdx.x, kc = k < Wc ? k : 0;
      Av[u] = ra[kc];
      Bw[u] = rb[kc];
    }
#pragma unroll
    for (int u = 0; u < kLoadBatch; ++u) {
      const int k = base + u * blockDim.x + threadIdx.x;
      if (k < Wc) {
        const float2 A = Av[u];
        const float2 Bv = rp.has1 ? Bw[u] : make_float2(0.f, 0.f);
        const bool edge = (k == 0) || (2 * k == W);   // DC / Nyquist: imaginary part ignored (C2R)
        if (edge) {
          a[k] = make_float2(A.x, Bv.x);
        } else {
          a[k] = make_float2(A.x - Bv.y, A.y + Bv.x);
          a[W - k] = make_float2(A.x + Bv.y, Bv.x - A.y);
        }
      }
    }
  }
  __syncthreads();
  const float2* r = fft_lds<+1>(a, b, plan, 1, tw);
  SumSq s;
  float* o0 = raw + rp.row0 * W;
  float* o1 = raw + rp.row1 * W;
  for (int x = threadIdx.x; x < W; x += blockDim.x) {
    const float2 z = r[x];
    const float v0 = z.x * norm, v1 = z.y * norm;
    o0[x] = v0;
    s.add(v0);
    if (rp.has1) { o1[x] = v1; s.add(v1); }
  }
  s.store_block_total(red, partials + 2 * blockIdx.x);
}

// row pass, adjoint (R2C with interior columns doubled).  The std-normalisation adjoint is
// fused into the load:  d raw = A * dn + B * (raw - mean)   (bstats = {A, B, mean}).
__global__ void fft_row_adjoint_kernel(const float* __restrict__ dn, const float* __restrict__ raw,
                                       const float* __restrict__ bstats, float2* __restrict__ tmp, Fft1D plan,
                                       const float2* __restrict__ tw, int H, int W, int Wc, float norm, int plain) {
  APH_DYN_SMEM(smem);
  float2* a = reinterpret_cast<float2*>(smem);
  float2* b = a + W;
  const RowPair rp(H);
  // plain: the forward transform rfft2 itself (aph_rfft2) -- no normalisation adjoint, no doubling of interior columns
  const float A = plain ? 1.0f : bstats[0], Bc = plain ? 0.0f : bstats[1], mu = plain ? 0.0f : bstats[2];
  const size_t o0 = rp.row0 * W, o1c = rp.row1_or_0 * W;
  for (int base = 0; base < W; base += kLoadBatch * blockDim.x) {      // (batched loads: see fft_col_synth_kernel)
    float d0[kLoadBatch], r0[kLoadBatch], d1[kLoadBatch], r1[kLoadBatch];
#pragma unroll
    for (int u = 0; u < kLoadBatch; ++u) {
      const int x = base + u * blockDim.x + threadIdx.x, xc = x < W ? x : 0;
      d0[u] = dn[o0 + xc]; r0[u] = raw[o0 + xc];
      d1[u] = dn[o1c + xc]; r1[u] = raw[o1c + xc];
    }
#pragma unroll
    for (int u = 0; u < kLoadBatch; ++u) {
      const int x = base + u * blockDim.x + threadIdx.x;
      if (x < W) {
        const float g0 = A * d0[u] + Bc * (r0[u] - mu);
        const float g1 = rp.has1 ? A * d1[u] + Bc * (r1[u] - mu) : 0.f;
        a[x] = make_float2(g0, g1);
      }
    }
  }
  __syncthreads();
  const float2* r = fft_lds<-1>(a, b, plan, 1, tw);
  float2* t0 = tmp + rp.row0 * Wc;
  float2* t1 = tmp + rp.row1 * Wc;
  for (int k = threadIdx.x; k < Wc; k += blockDim.x) {
    const float2 z = r[k];
    const float2 zc = r[k == 0 ? 0 : W - k];
    // Ga = (Z[k] + conj(Z[-k])) / 2 ; Gb = (Z[k] - conj(Z[-k])) / (2i)
    const float f = ((!plain && k >= 1 && k <= W - Wc) ? 1.0f : 0.5f) * norm;
    t0[k] = make_float2((z.x + zc.x) * f, (z.y - zc.y) * f);
    if (rp.has1) t1[k] = make_float2((z.y + zc.y) * f, (zc.x - z.x) * f);
  }
}

}  // namespace aph
