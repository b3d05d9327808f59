// fp32-in / fp32-accumulate GEMM of the EXACT ViT path (aph_vit_forward_f32 / aph_vit_backward_f32), gfx950.
//
//   C[m][n] = sum_k A[m][k] * Bt[n][k]        A: [M,K] f32 (row pitch lda), Bt: [N,K] f32 (row pitch ldb)
//
// Main loop on v_mfma_f32_32x32x2_f32: every product is one fmaf of the exact f32 operands, the sums are f32 -- the
// result differs from an fp32 CPU GEMM only in summation order.  128x128x32 tile, 4 waves (2x2 of 64x64, 2x2 MFMA tiles of
// 32x32 each), operands streamed into a 2-stage LDS ring by global_load_lds_dwordx4 (64 KiB: two workgroups per CU).
// The LDS image is the f16 kernels' (vit_gemm.h): rows of 128 bytes = 8 chunks of 16 bytes, chunk c of row r at physical
// chunk c ^ ((r >> 1) & 7), the swizzle applied to the DMA's per-lane source address.  One k-step of the MFMA sums over
// two k values, taken from the two lane halves: lane half h of a fragment reads chunk 2p + h of its row (k = 8p + 4h + j)
// as one 16-byte read, and element j of it feeds MFMA j -- the same k permutation on both operands, so the sum is over
// the right pairs (order of the sum: fixed, bitwise repeatable).
// Operands are swapped at the MFMA (weights as the A fragment): lane l then holds output row m = l & 31 of its 32x32
// tile and columns n = (r & 3) + 8 (r >> 2) + 4 (l >> 5); one exchange with the other lane half (__shfl_xor 32) gives
// every lane two runs of 8 consecutive columns, handed to the epilogue's apply8 (EpiResidual, EpiF32, EpiPatchEmbed and
// the fp32 epilogues below).
// Small M (the class-row GEMMs of the last block, M = cuts): split-K over the k-tiles, fp32 partials to a workspace and
// splitk_reduce_kernel (vit_gemm.h) summing them in split order -- no atomics, deterministic.
// Constraints: N % 128 == 0, K % 32 == 0, lda / ldb % 4 == 0 and 16-byte aligned operands; M arbitrary (row loads clamp,
// stores are predicated).  a_rowP > 0: A row m is read from physical row m + m / a_rowP + 1 (the patch rows of a
// token-major [S*T, D] buffer: the patch-embedding dgrad).
#pragma once
#include "aph_device.h"
#include "vit_gemm.h"

namespace aph {

struct GemmF32 {
  static constexpr int BM = 128, BN = 128, BK = 32, NTHREAD = 256;
  static constexpr int STAGE = (BM + BN) * BK;             // floats per stage
  static constexpr int SMEM = 2 * STAGE * 4;               // bytes (64 KiB)
  static constexpr int GA = BM / 8 / 4, GB = BN / 8 / 4;   // DMA instructions (8 rows each) per wave per tile
};

__device__ __forceinline__ int lds_off_f32(int row, int chunk) { return row * GemmF32::BK + ((chunk ^ ((row >> 1) & 7)) << 2); }

// SPLIT: blockIdx.y = split index; the k-tiles [kbeg, kend) of this split, partial tile to ws[split][M][N]
template <class Epi, bool SPLIT>
__global__ __launch_bounds__(256) void gemm_f32_kernel(const float* __restrict__ A, int lda, int a_rowP, const float* __restrict__ Bt, int ldb,
                                                       int M, int N, int K, Epi epi, float* __restrict__ ws) {
  using C = GemmF32;
  APH_DYN_SMEM(smem);
  float* lds = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int ntn = N / C::BN;
  const int tm = blockIdx.x / ntn;
  const int n0 = (blockIdx.x - tm * ntn) * C::BN, m0 = tm * C::BM;
  int nk = K / C::BK, kbeg = 0;
  if (SPLIT) {
    const int sp = blockIdx.y, ns = gridDim.y;
    kbeg = (int)((long long)nk * sp / ns);
    nk = (int)((long long)nk * (sp + 1) / ns) - kbeg;
  }
  const float* ga[C::GA];
  const float* gb[C::GB];
  const int lrow = lane >> 3, pc = lane & 7;
#pragma unroll
  for (int k = 0; k < C::GA; ++k) {
    const int row = (wave * C::GA + k) * 8 + lrow;
    int am = m0 + row; am = am < M ? am : M - 1;
    const size_t pr = a_rowP > 0 ? (size_t)am + am / a_rowP + 1 : (size_t)am;
    ga[k] = A + pr * lda + (size_t)kbeg * C::BK + ((pc ^ ((row >> 1) & 7)) << 2);
  }
#pragma unroll
  for (int k = 0; k < C::GB; ++k) {
    const int row = (wave * C::GB + k) * 8 + lrow;
    gb[k] = Bt + (size_t)(n0 + row) * ldb + (size_t)kbeg * C::BK + ((pc ^ ((row >> 1) & 7)) << 2);
  }
  auto issue = [&](int kt, int stage) {
    float* As = lds + stage * C::STAGE;
    float* Bs = As + C::BM * C::BK;
    const int ko = kt * C::BK;
#pragma unroll
    for (int k = 0; k < C::GA; ++k) glds16(ga[k] + ko, As + (wave * C::GA + k) * 8 * C::BK);
#pragma unroll
    for (int k = 0; k < C::GB; ++k) glds16(gb[k] + ko, Bs + (wave * C::GB + k) * 8 * C::BK);
  };
  f32x16 acc[2][2];      // [weight (n) tile][activation (m) tile]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int frow = lane & 31, half = lane >> 5;
  const int arow = wm * 64 + frow, brow = wn * 64 + frow;
  if (nk > 0) issue(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    wait_lgkm0();                 // this wave's fragment reads of tile kt-1 have returned
    wait_vm_barrier<0>();         // tile kt has landed for everyone; everyone is done reading stage (kt+1) & 1
    if (kt + 1 < nk) issue(kt + 1, (kt + 1) & 1);
    const float* As = lds + (kt & 1) * C::STAGE;
    const float* Bs = As + C::BM * C::BK;
#pragma unroll
    for (int p = 0; p < C::BK / 8; ++p) {
      f32x4 fa[2], fb[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        fa[t] = *reinterpret_cast<const f32x4*>(As + lds_off_f32(arow + t * 32, 2 * p + half));
        fb[t] = *reinterpret_cast<const f32x4*>(Bs + lds_off_f32(brow + t * 32, 2 * p + half));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) acc[nt][mt] = mfma_32x32x2_f32(fb[nt][j], fa[mt][j], acc[nt][mt]);
    }
  }
  // epilogue: lane half 0 takes column runs 0-7 and 16-23 of every 32-column tile, half 1 runs 8-15 and 24-31
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const f32x16& c = acc[nt][mt];
      f32x4 own[2], snd[2];
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        // registers 8g .. 8g+7 hold columns 16g + {0..3, 8..11} (+4 in half 1)
        const f32x4 lo = f32x4{c[8 * g], c[8 * g + 1], c[8 * g + 2], c[8 * g + 3]};
        const f32x4 hi = f32x4{c[8 * g + 4], c[8 * g + 5], c[8 * g + 6], c[8 * g + 7]};
        own[g] = half ? hi : lo;
        snd[g] = half ? lo : hi;
      }
      f32x4 rcv[2];
#pragma unroll
      for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) rcv[g][e] = __shfl_xor(snd[g][e], 32);
      const int m = m0 + wm * 64 + mt * 32 + frow;
      if (m < M) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          const int n = n0 + wn * 64 + nt * 32 + 16 * g + 8 * half;
          const f32x4 a = half ? rcv[g] : own[g], b = half ? own[g] : rcv[g];
          if (SPLIT) {
            float* o = ws + ((size_t)blockIdx.y * M + m) * N + n;
            st4(o, a);
            st4(o + 4, b);
          } else {
            epi.apply8(m, n, a, b);
          }
        }
      }
    }
}

// ---- epilogues of the fp32 path (fp32 outputs where the f16 path stores f16) ----
struct EpiBiasF32 {      // out = acc + bias   (QKV)
  float* out; int ldo; const float* bias;
  __device__ __forceinline__ void apply8(int m, int n, f32x4 a, f32x4 b) const {
    st4(out + (size_t)m * ldo + n, a + ld4(bias + n));
    st4(out + (size_t)m * ldo + n + 4, b + ld4(bias + n + 4));
  }
};
// QuickGELU g = u sigmoid(1.702 u), u = acc + bias, with IEEE division and the accurate expf (a few ulp): g and dg/du in fp32
__device__ __forceinline__ void quick_gelu4_f32(const f32x4& u, f32x4& g, f32x4& dg) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float s = 1.0f / (1.0f + expf(-1.702f * u[i]));
    g[i] = u[i] * s;
    dg[i] = s + 1.702f * (g[i] - g[i] * s);
  }
}
struct EpiGeluF32 {
  float* dg; float* g; int ldo; const float* bias;
  __device__ __forceinline__ void apply8(int m, int n, f32x4 a, f32x4 b) const {
    a += ld4(bias + n); b += ld4(bias + n + 4);
    f32x4 ga, da, gb, db;
    quick_gelu4_f32(a, ga, da);
    quick_gelu4_f32(b, gb, db);
    const size_t o = (size_t)m * ldo + n;
    st4(g + o, ga); st4(g + o + 4, gb);
    st4(dg + o, da); st4(dg + o + 4, db);
  }
};
struct EpiGeluBwdF32 {   // du = acc * dg/du (fp32, stored by the forward)
  float* out; const float* dg; int ldo;
  __device__ __forceinline__ void apply8(int m, int n, f32x4 a, f32x4 b) const {
    const size_t o = (size_t)m * ldo + n;
    st4(out + o, a * ld4(dg + o));
    st4(out + o + 4, b * ld4(dg + o + 4));
  }
};

// split-K workspace of the fp32 path (carved in the handle's fp32 arena)
struct F32Space {
  float* ws = nullptr;
  size_t ws_floats = 0;
};

inline bool gemm_f32_shape_ok(int M, int N, int K, int lda, int ldb) {
  return M >= 1 && N >= 128 && N % 128 == 0 && K >= 32 && K % 32 == 0 && lda % 4 == 0 && ldb % 4 == 0 && lda >= K && ldb >= K;
}

// split count of a shape: none while the tiles fill the chip; else enough splits for ~2 workgroups per CU, >= 4 k-tiles per split
inline int gemm_f32_splits(int M, int N, int K, const F32Space* sp) {
  const int tiles = (N / GemmF32::BN) * ((M + GemmF32::BM - 1) / GemmF32::BM), nk = K / GemmF32::BK;
  if (!sp || !sp->ws || tiles >= 128) return 1;
  int s = (512 + tiles - 1) / tiles;
  if (s > nk / 4) s = nk / 4;
  if (s > 16) s = 16;
  while (s > 1 && (size_t)s * M * N > sp->ws_floats) --s;
  return s < 1 ? 1 : s;
}

template <class Epi>
void launch_gemm_f32(const float* A, int lda, const float* Bt, int ldb, int M, int N, int K, Epi epi, hipStream_t st, const F32Space* sp,
                     int a_rowP = 0) {
  const int tiles = (N / GemmF32::BN) * ((M + GemmF32::BM - 1) / GemmF32::BM);
  const int splits = gemm_f32_splits(M, N, K, sp);
  if (splits > 1) {
    APH_ALLOW_SMEM((gemm_f32_kernel<Epi, true>), GemmF32::SMEM);
    APH_LAUNCH((gemm_f32_kernel<Epi, true>), dim3(tiles, splits), dim3(256), GemmF32::SMEM, st, A, lda, a_rowP, Bt, ldb, M, N, K, epi, sp->ws);
    const size_t n8 = (size_t)M * (N / 8);
    APH_LAUNCH(splitk_reduce_kernel<Epi>, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, st, (const float*)sp->ws, splits, M, N, epi);
    return;
  }
  APH_ALLOW_SMEM((gemm_f32_kernel<Epi, false>), GemmF32::SMEM);
  APH_LAUNCH((gemm_f32_kernel<Epi, false>), dim3(tiles), dim3(256), GemmF32::SMEM, st, A, lda, a_rowP, Bt, ldb, M, N, K, epi, (float*)nullptr);
}

}  // namespace aph
