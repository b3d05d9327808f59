// Small-M fp16 GEMM for the CLIP ViT linears (round 5), gfx950: operands staged through REGISTERS, no barrier in the main loop.
//
//   C[m][n] = sum_k A[m][k] * Bt[n][k]        same contract as vit_gemm.h
//
// What the ring kernels of vit_gemm.h do at M ~ 1200 rows (a 24-cut shard: one of eight ranks; also C1 / C3 / C5): 228 tiles of 64 x 64 on
// 256 CUs is ONE 4-wave workgroup per CU, and (profiles/r05_load_rate.txt, tools/exp/load_rate.hip) four waves cannot feed a CU through
// global_load_lds_dwordx4: 70 GB/s per CU from L2-resident data whatever the number in flight (8 waves: 126, the 64 B/clk limit is 134),
// and their k loop is a chain of counted wait -> s_barrier -> fragment reads -> MFMAs with nothing else resident to fill the waits:
// 50-60 GB/s per CU in the event, fc2 17.9 us / dqkv 14.4 us for 5.7 / 4.2 GFLOP.  The same four waves reach 110-125 GB/s with plain
// global_load_dwordx4 into registers -- provided every QUAD of lanes reads 64 contiguous bytes (the MFMA fragment pattern straight from a
// row-major matrix, 16 rows x 16 bytes per quarter wave, is stuck at 37 GB/s at any occupancy).  So here:
//   * loads are global_load_dwordx4 of [16 rows][64 bytes] blocks (lane >> 2 = row, lane & 3 = 16-byte chunk), PD k-steps of 32 in flight
//     per wave in registers (the register file is the prefetch buffer: one wave per SIMD owns 512 VGPRs);
//   * a wave writes a landed k-step into its PRIVATE LDS image (ds_write_b128, chunk p of row r at piece p ^ ((-(r >> 2)) & 3): the four
//     lane groups of a ds_read_b128 fragment fetch then hit 16 different 16-byte bank groups) and reads its MFMA fragments back: LDS is
//     the transposer, and since only the owning wave touches an image, program order is all the synchronisation there is -- NO s_barrier,
//     NO hand-counted vmcnt (the compiler's own counted waits cover the register loads); the four waves drift freely;
//   * operands are swapped at the MFMA (weights as A fragment) and the weight rows of a 16-row tile are permuted through the load address so
//     that lane l ends up with 4 NT CONSECUTIVE columns of token row l & 15: the epilogues are vit_gemm.h's apply8.
// The kernel:
//   gemm_sk_kernel  64 x 64 tile per workgroup, the four waves SPLIT K (wave w owns the k-tiles w, w + 4, ...: whole 128-byte lines of every
//                   operand row) and each accumulates the full tile; the four fp32 partials meet in LDS at the end and are summed in the
//                   fixed order 0, 1, 2, 3 (bitwise reproducible).  Every operand byte is fetched once per workgroup.  For the long-K,
//                   narrow-N shapes (out-proj, fc2, dfc1, dqkv, patch embedding).
// (An A-resident 64 x 256 variant for the wide-N shapes was measured slower than the ring kernels inside the step at every shard size --
// profiles/r05_gemm_rs_shapes.txt, r05_fused_v4_steps.txt -- and is not in the tree: DESIGN.md section 4.)
#pragma once
#include "vit_gemm.h"

namespace aph {

// k-step image: [rows][64 bytes]; 16-byte piece p of row r holds chunk p ^ rs_swz(r)
__device__ __forceinline__ int rs_swz(int row) { return (0 - (row >> 2)) & 3; }

struct RSLane {
  int lrow, lpc;      // load role: row within a 16-row block, 16-byte chunk of the 64-byte k-step row (a quad of lanes = 64 contiguous bytes)
  int wpos;           // byte position of that piece within a 16-row (1 KiB) block of a k-step image
  int fpos;           // fragment read role: row lane & 15, chunk lane >> 4 -> byte position within a 16-row block
  __device__ __forceinline__ explicit RSLane(int lane) {
    lrow = lane >> 2; lpc = lane & 3;
    wpos = lrow * 64 + ((lpc ^ rs_swz(lrow)) << 4);
    const int frow = lane & 15;
    fpos = frow * 64 + (((lane >> 4) ^ rs_swz(frow)) << 4);
  }
};

__device__ __forceinline__ half8 ldg8(const char* p) { return *reinterpret_cast<const half8*>(p); }
__device__ __forceinline__ void sts8(char* p, const half8& v) { *reinterpret_cast<half8*>(p) = v; }
__device__ __forceinline__ half8 lds8(const char* p) { return *reinterpret_cast<const half8*>(p); }

// XCD-aware tile run (as gemm_f16_kernel): workgroup b runs on XCD b % 8 (observed dispatch, speed only); every XCD gets one contiguous
// run of tile indices.  Bijective for any grid size.
__device__ __forceinline__ int rs_tile_index() {
  const int nwg = gridDim.x, b = blockIdx.x;
  const int q = nwg >> 3, r = nwg & 7, xcd = b & 7, idx = b >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// measurement hook (aph_gemm_rs_probe): chip-wide 100 MHz clock stamps of wave 0 of every workgroup, slot k of trace[wg][8]
__device__ __forceinline__ void rs_stamp(unsigned long long* trace, int k) {
#ifndef APH_EMU
  if (trace && threadIdx.x == 0) trace[(size_t)blockIdx.x * 8 + k] = __builtin_amdgcn_s_memrealtime();
#endif
}

// ---- split-K kernel -----------------------------------------------------------------------------------------------------------------
struct GemmSK {
  static constexpr int BM = 64, BN = 64, NTHREAD = 256;
  static constexpr int IMG = (BM + BN) * 64;                 // bytes of one k-step image (both operands)
  static constexpr int SMEM = 4 * BM * BN * 4;               // four fp32 partial tiles (>= 4 waves x 2 images)
};

// NS = k-steps per wave = K / 128 (K % 256 == 0): a COMPILE-TIME count -- the loop is straight-line code, so every register load is
// unconditional and the compiler's in-order vmcnt bookkeeping is exact (with the loads behind run-time conditions it has to assume they
// were not issued, and every wait drains the whole prefetch queue: found in the ISA of the first version).
template <int NS, int PD, class Epi>
__global__ __launch_bounds__(256) void gemm_sk_kernel(const half_t* __restrict__ A, int lda, const half_t* __restrict__ Bt, int ldb, int M, int N,
                                                      Epi epi, unsigned long long* __restrict__ trace) {
  using C = GemmSK;
  APH_DYN_SMEM(smem);
  rs_stamp(trace, 0);
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6);
  int m0, n0;
  {
    const int tile = rs_tile_index(), ntn = N / C::BN, tm = tile / ntn;      // n-tiles fastest: the workgroups of an XCD share A panels
    n0 = (tile - tm * ntn) * C::BN;
    m0 = tm * C::BM;
  }
  char* ring = smem + wave * (2 * C::IMG);
  const RSLane L(lane);
  unsigned offT[4], offW[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    int am = m0 + 16 * q + L.lrow;
    am = am < M ? am : M - 1;
    offT[q] = ((unsigned)am * (unsigned)lda + L.lpc * 8) * 2u;
    // tile q, tile row i = lrow is weight row 16 (i >> 2) + 4 q + (i & 3) of the workgroup's 64
    offW[q] = ((unsigned)(n0 + 16 * (L.lrow >> 2) + 4 * q + (L.lrow & 3)) * (unsigned)ldb + L.lpc * 8) * 2u;
  }
  const char* Ab = reinterpret_cast<const char*>(A);
  const char* Bb = reinterpret_cast<const char*>(Bt);
  auto load = [&](int s, half8 (&r)[8]) {                           // k-step s of this wave: half s & 1 of its k-tile wave + 4 (s >> 1)
    const size_t kb = (size_t)(wave + 4 * (s >> 1)) * 128 + (s & 1) * 64;
#pragma unroll
    for (int q = 0; q < 4; ++q) { r[q] = ldg8(Ab + offT[q] + kb); r[4 + q] = ldg8(Bb + offW[q] + kb); }
  };
  auto stage = [&](char* img, const half8 (&r)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) sts8(img + q * 1024 + L.wpos, r[q]);
  };
  struct Frags { half8 t[4], w[4]; };
  auto frags = [&](Frags& f, const char* img) {
#pragma unroll
    for (int q = 0; q < 4; ++q) { f.t[q] = lds8(img + q * 1024 + L.fpos); f.w[q] = lds8(img + 4096 + q * 1024 + L.fpos); }
  };
  f32x4 acc[4][4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto mma = [&](const Frags& f) {
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = mfma_16x16x32_f16(f.w[nt], f.t[mt], acc[mt][nt]);
  };
  {
    half8 R[PD][8];
    Frags f[2];
#pragma unroll
    for (int d = 0; d < PD; ++d)
      if (d < NS) load(d, R[d]);
    stage(ring, R[0]);
    if (PD < NS) load(PD, R[0]);
    wave_lds_fence();
    frags(f[0], ring);
    rs_stamp(trace, 1);
    // Steady state as a ROLLED loop of U k-steps per trip (every step of it requests a k-step: no load behind a condition, exact vmcnt
    // bookkeeping), the last steps unrolled with compile-time conditions.  Fully unrolled, a loop of this length is kilobytes of straight-line
    // code that a wave runs through once: in the step, where three dozen kernels take turns, that is an instruction-cache miss stream per
    // launch (measured on the A-resident variant: 18-21 us in the step against 13 us back to back, profiles/r05_gemm_rs_shapes.txt).
    constexpr int U = (PD % 2) ? 2 * PD : PD;
    constexpr int NMAIN = NS > PD + 1 ? ((NS - PD - 1) / U) * U : 0;
    auto step = [&](int s, int u, bool more, bool req) {
      if (more) {
        char* img = ring + ((u + 1) & 1) * C::IMG;
        wave_lds_fence();                                     // (the fragment reads of k-step s - 1 from this image are behind every lane)
        stage(img, R[(u + 1) % PD]);
        if (req) load(s + 1 + PD, R[(u + 1) % PD]);
        wave_lds_fence();
        frags(f[(u + 1) & 1], img);
      }
      mma(f[u & 1]);
    };
#pragma unroll 1
    for (int s0 = 0; s0 < NMAIN; s0 += U) {
#pragma unroll
      for (int u = 0; u < U; ++u) step(s0 + u, u, true, true);
    }
#pragma unroll
    for (int s = NMAIN; s < NS; ++s) step(s, s % U, s + 1 < NS, s + 1 + PD < NS);
  }
  // the four partial tiles meet in LDS: [source wave][row tile][column tile][lane] as f32x4
  rs_stamp(trace, 2);
  __syncthreads();                                                   // every wave is done with its images
  rs_stamp(trace, 3);
  f32x4* part = reinterpret_cast<f32x4*>(smem);
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) part[((wave * 4 + mt) * 4 + nt) * 64 + lane] = acc[mt][nt];
  __syncthreads();
  f32x4 sum[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    sum[nt] = part[((0 * 4 + wave) * 4 + nt) * 64 + lane];
#pragma unroll
    for (int src = 1; src < 4; ++src) sum[nt] += part[((src * 4 + wave) * 4 + nt) * 64 + lane];
  }
  // lane: token row m0 + 16 wave + (lane & 15), columns n0 + 16 (lane >> 4) + 4 nt + r
  const int m = m0 + 16 * wave + (lane & 15);
  if (m < M) {
    epi.apply8(m, n0 + 16 * (lane >> 4), sum[0], sum[1]);
    epi.apply8(m, n0 + 16 * (lane >> 4) + 8, sum[2], sum[3]);
  }
  rs_stamp(trace, 4);
}

template <int NS, int PD, class Epi>
inline void launch_gemm_sk_n(const half_t* A, int lda, const half_t* Bt, int ldb, int M, int N, Epi epi, hipStream_t st, unsigned long long* trace) {
  const dim3 grid((N / GemmSK::BN) * ((M + GemmSK::BM - 1) / GemmSK::BM));
  APH_ALLOW_SMEM((gemm_sk_kernel<NS, PD, Epi>), GemmSK::SMEM);
  APH_LAUNCH((gemm_sk_kernel<NS, PD, Epi>), grid, dim3(GemmSK::NTHREAD), GemmSK::SMEM, st, A, lda, Bt, ldb, M, N, epi, trace);
}
// the K values the kernel is instantiated for (k-steps per wave = K / 128): the linears of a ViT of width 768 (B/32, B/16) and of the
// width-256 test models; other shapes stay on the ring kernels
inline bool gemm_sk_fits(int N, int K) { return N % 64 == 0 && (K == 256 || K == 768 || K == 1024 || K == 2304 || K == 3072); }
template <int PD, class Epi>
inline void launch_gemm_sk(const half_t* A, int lda, const half_t* Bt, int ldb, int M, int N, int K, Epi epi, hipStream_t st,
                           unsigned long long* trace = nullptr) {
  switch (K) {
    case 256: launch_gemm_sk_n<2, PD>(A, lda, Bt, ldb, M, N, epi, st, trace); break;
    case 768: launch_gemm_sk_n<6, PD>(A, lda, Bt, ldb, M, N, epi, st, trace); break;
    case 1024: launch_gemm_sk_n<8, PD>(A, lda, Bt, ldb, M, N, epi, st, trace); break;
    case 2304: launch_gemm_sk_n<18, PD>(A, lda, Bt, ldb, M, N, epi, st, trace); break;
    default: launch_gemm_sk_n<24, PD>(A, lda, Bt, ldb, M, N, epi, st, trace); break;       // 3072
  }
}

// the split-K kernel if it is instantiated for this shape (false: the caller falls back to the ring kernels of vit_gemm.h)
template <class Epi>
inline bool launch_gemm_rs_auto(const half_t* A, int lda, const half_t* Bt, int ldb, int M, int N, int K, Epi epi, hipStream_t st) {
  if (!gemm_sk_fits(N, K)) return false;
  launch_gemm_sk<4>(A, lda, Bt, ldb, M, N, K, epi, st);
  return true;
}

}  // namespace aph
