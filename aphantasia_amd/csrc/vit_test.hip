// Test and measurement entries of include/aphantasia_hip_test.h for the ViT's kernels: the GEMM families, the LayerNorm and attention launches
// alone, the probes and the process-wide switches.  Nothing here is on the product path: aph_vit_* (vit.hip) needs none of it, and the
// launchers and kernels it calls live in the headers both units include.
#include <utility>

#include "aph_device.h"
#include "aph_host.h"
#include "vit_gemm.h"
#include "vit_gemm_ws.h"
#include "vit_gemm_rs.h"
#include "vit_ops.h"
#include "vit_attn.h"
#include "vit_attn_f32.h"
#include "vit_gemm_f32.h"

using namespace aph;

// the split-K workspace of the test entries' tile_cfg 8 / 9 / 22 / 24 (one per process, allocated on first use)
static int gemm_test_splitk_space(SplitKSpace** out) {
  static SplitKSpace sp;
  if (!sp.ws) {
    if (hipMalloc((void**)&sp.ws, ((size_t)4 << 24) * sizeof(float)) != hipSuccess) return aph_fail(APH_ERR_HIP, "GEMM test entry: split-K workspace");
    sp.ws_floats = (size_t)4 << 24;
  }
  *out = &sp;
  return 0;
}

// tile_cfg -> kernel family for the product's families (0, 1, 2, 5, 8, 9, 10, 14, 15), shared by aph_gemm_f16_ld and aph_gemm_f16_epi_test;
// the shape limits of each family are the callers' to check.  0 = launch_gemm with `sp` (its split-K workspace and small_batch flag, or null).
template <class Epi>
static int gemm_f16_launch_cfg(const half_t* A, int lda, const half_t* B, int ldb, int M, int N, int K, Epi epi, int tile_cfg, const SplitKSpace* sp,
                               hipStream_t st) {
  switch (tile_cfg) {
    case 0: launch_gemm(A, lda, B, ldb, M, N, K, epi, st, sp); break;
    case 1: launch_gemm_cfg<GemmSmall>(A, lda, B, ldb, M, N, K, epi, st); break;
    case 2: launch_gemm_cfg<GemmBig>(A, lda, B, ldb, M, N, K, epi, st); break;
    case 5: launch_gemm_ws_cfg<GemmWS>(A, lda, B, ldb, M, N, K, epi, st, nullptr); break;
    case 8:
    case 9: {                // split-K (2 / 4 ways) of the 64x64 configuration, private workspace
      SplitKSpace* ws = nullptr;
      if (const int rc = gemm_test_splitk_space(&ws)) return rc;
      launch_gemm_splitk<GemmSmall>(A, lda, B, ldb, M, N, K, epi, tile_cfg == 8 ? 2 : 4, *ws, st);
      break;
    }
    case 10: launch_gemm_cfg<GemmMidDeep8>(A, lda, B, ldb, M, N, K, epi, st); break;
    case 14: launch_gemm_sk<4>(A, lda, B, ldb, M, N, K, epi, st); break;
    case 15: launch_gemm_sk<3>(A, lda, B, ldb, M, N, K, epi, st); break;
    default: return aph_fail(APH_ERR_ARG, "GEMM test entry: tile_cfg %d is not a product kernel family", tile_cfg);
  }
  return 0;
}
// the shape limits of tile_cfg 5, 8 / 9 / 22 / 24 and 14 / 15 (false: refuse)
static bool gemm_test_cfg_fits(int tile_cfg, int M, int lda, int N, int ldb, int K) {
  if (tile_cfg == 5) return gemm_addressable32(M, lda, N, ldb) && N <= GemmWS::BIAS_MAX;
  if (tile_cfg == 14 || tile_cfg == 15) return gemm_addressable32(M, lda, N, ldb) && gemm_sk_fits(N, K);
  if (tile_cfg == 8 || tile_cfg == 9 || tile_cfg == 22 || tile_cfg == 24)
    return K / GEMM_BK >= ((tile_cfg == 8 || tile_cfg == 22) ? 2 : 4) && (size_t)M * N <= ((size_t)1 << 24);
  return true;
}

extern "C" {

// the process-wide switches (each documented at its prototype): set, return the previous value
int aph_vit_set_fuse_ln(int on) { return std::exchange(vit_fuse_ln(), on ? 1 : 0); }
int aph_vit_set_grad_stream_f16(int on) { return std::exchange(vit_grad_stream_f16(), on ? 1 : 0); }
int aph_gemm_set_mfma32(int on) { return std::exchange(gemm_mfma32(), on ? 1 : 0); }
int aph_gemm_set_ws_min_tiles(int tiles) { return std::exchange(gemm_ws_min_tiles(), tiles < 0 ? 0 : tiles); }
int aph_gemm_set_rs(int mode) { return std::exchange(gemm_rs_mode(), mode < 0 ? 0 : (mode > 2 ? 2 : mode)); }
int aph_gemm_set_ws_pgroup(int g) { return std::exchange(gemm_ws_pgroup_override(), g < 0 ? 0 : g); }

// aph_mfma_rate: a pure v_mfma_f32_16x16x32_f16 loop, 128 accumulator registers per wave, 8 waves per workgroup, no memory traffic inside the loop
namespace {
__global__ __launch_bounds__(512) void mfma_rate_kernel(const half8* __restrict__ src, float* out, int iters) {
  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  half8 a[8], b[4];
#pragma unroll
  for (int i = 0; i < 8; ++i) a[i] = src[(threadIdx.x * 16 + i) & 8191];
#pragma unroll
  for (int i = 0; i < 4; ++i) b[i] = src[(threadIdx.x * 16 + 8 + i) & 8191];
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = mfma_16x16x32_f16(b[j], a[i], acc[i][j]);
  }
  f32x4 s = acc[0][0];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) s += acc[i][j];
  if (s[0] == 12345.678f) out[threadIdx.x] = s[1] + s[2] + s[3];
}
}  // namespace
int aph_mfma_rate(int blocks, int iters, const void* d_src, float* d_out, void* stream_) {
  APH_TRY
  if (blocks < 1 || iters < 1 || !d_src || !d_out) return aph_fail(APH_ERR_ARG, "aph_mfma_rate: bad argument");
  APH_LAUNCH(mfma_rate_kernel, dim3(blocks), dim3(512), 0, (hipStream_t)stream_, (const half8*)d_src, d_out, iters);
  return aph_check_launch("aph_mfma_rate");
  APH_CATCH
}

// d_trace: gridDim x 16 tiles x 4 uint64 {first k-tile done, main loop done, epilogue issued, -} of consumer wave 0, or null
int aph_gemm_ws_probe(const void* d_A, const void* d_Bt, int M, int N, int K, void* d_out, void* d_out2, const float* d_bias, int epi_kind,
                      unsigned long long* d_trace, void* stream_) {
  APH_TRY
  if (!d_A || !d_Bt || !d_out || M < 1 || N % 128 || K % GEMM_BK || N > 4096 || !gemm_addressable32(M, K, N, K))
    return aph_fail(APH_ERR_ARG, "aph_gemm_ws_probe: bad shape");
  const half_t* A = (const half_t*)d_A;
  const half_t* B = (const half_t*)d_Bt;
  hipStream_t st = (hipStream_t)stream_;
  if (epi_kind == 0) launch_gemm_ws(A, K, B, K, M, N, K, EpiF16{(half_t*)d_out, N, d_bias}, st, d_trace);
  else if (epi_kind == 1 && d_out2 && d_bias) launch_gemm_ws(A, K, B, K, M, N, K, EpiGelu{(half_t*)d_out2, (half_t*)d_out, N, d_bias}, st, d_trace);
  else if (epi_kind == 2 && d_bias) launch_gemm_ws(A, K, B, K, M, N, K, EpiResidual{(float*)d_out, (const float*)d_out, N, d_bias}, st, d_trace);
  else if (epi_kind == 3) launch_gemm_ws(A, K, B, K, M, N, K, EpiNoStore{(float*)d_out, N}, st, d_trace);
  else return aph_fail(APH_ERR_ARG, "aph_gemm_ws_probe: bad epilogue kind / missing buffer");
  return aph_check_launch("aph_gemm_ws_probe");
  APH_CATCH
}

// d_trace: per workgroup 8 uint64 stamps of the chip-wide 100 MHz clock (entry, first fragments read, main loop done, past the barrier, end), or null
int aph_gemm_rs_probe(const void* d_A, const void* d_Bt, int M, int N, int K, void* d_out, int kind, unsigned long long* d_trace, void* stream_) {
  APH_TRY
  if (kind != 0) return aph_fail(APH_ERR_ARG, "aph_gemm_rs_probe: kind %d is not a kernel of this library (0 = split-K register-staged)", kind);
  if (!d_A || !d_Bt || !d_out || M < 1 || !gemm_addressable32(M, K, N, K) || !gemm_sk_fits(N, K)) return aph_fail(APH_ERR_ARG, "aph_gemm_rs_probe: bad shape");
  const EpiF16 epi{(half_t*)d_out, N, nullptr};
  launch_gemm_sk<4>((const half_t*)d_A, K, (const half_t*)d_Bt, K, M, N, K, epi, (hipStream_t)stream_, d_trace);
  return aph_check_launch("aph_gemm_rs_probe");
  APH_CATCH
}

// the attention launches of vit_attn.h alone; d_delta: unused (no kernel takes row-dot scratch)
int aph_attn_test(const void* d_qkv, void* d_att, float* d_lse, const void* d_datt, float* /*d_delta*/, void* d_dqkv, int S, int T, int heads,
                  int mode, void* stream_) {
  APH_TRY
  if (!d_qkv || !d_att || !d_lse || S < 1 || T < 1 || T > AT_TMAX || heads < 1 || (mode != 0 && mode != 1) ||
      (mode == 1 && (!d_datt || !d_dqkv)))
    return aph_fail(APH_ERR_ARG, "aph_attn_test: bad argument");
  const AttnArgs a{(const half_t*)d_qkv, (half_t*)d_att, d_lse, (const half_t*)d_datt, (half_t*)d_dqkv, S, T, heads};
  if (mode == 0) launch_attn_fwd(a, (hipStream_t)stream_);
  else launch_attn_bwd(a, (hipStream_t)stream_);
  return aph_check_launch("aph_attn_test");
  APH_CATCH
}

// the exact path's fp32 attention launches (vit_attn_f32.h) alone; the backward takes no att
int aph_attn_f32_test(const float* d_qkv, float* d_att, float* d_lse, const float* d_datt, float* d_delta, float* d_dqkv, int S, int T, int heads,
                      int mode, void* stream_) {
  APH_TRY
  if (!d_qkv || !d_att || !d_lse || S < 1 || T < 1 || T > 256 || heads < 1 || (mode != 0 && mode != 1) ||
      (mode == 1 && (!d_datt || !d_delta || !d_dqkv)))
    return aph_fail(APH_ERR_ARG, "aph_attn_f32_test: bad argument");
  if (mode == 0) launch_attn_fwd_f32(d_qkv, d_att, d_lse, S, T, heads, (hipStream_t)stream_);
  else launch_attn_bwd_f32(d_qkv, d_datt, d_lse, d_delta, d_dqkv, S, T, heads, (hipStream_t)stream_);
  return aph_check_launch("aph_attn_f32_test");
  APH_CATCH
}

// the text tower's causal instantiation of the fp32 attention forward alone
int aph_attn_causal_f32_test(const float* d_qkv, float* d_att, float* d_lse, int S, int T, int heads, void* stream_) {
  APH_TRY
  if (!d_qkv || !d_att || !d_lse || S < 1 || T < 1 || T > 256 || heads < 1) return aph_fail(APH_ERR_ARG, "aph_attn_causal_f32_test: bad argument");
  launch_attn_fwd_f32<true>(d_qkv, d_att, d_lse, S, T, heads, (hipStream_t)stream_);
  return aph_check_launch("aph_attn_causal_f32_test");
  APH_CATCH
}

// the exact path's GEMM (vit_gemm_f32.h) alone, one launch per epi_kind
int aph_gemm_f32_test(const float* d_A, int lda, int a_rowP, const float* d_Bt, int ldb, int M, int N, int K, float* d_C, int ldc, const float* d_bias,
                      float* d_aux, int epi_kind, float* d_ws, size_t ws_floats, void* stream_) {
  APH_TRY
  if (!d_A || !d_Bt || !d_C || !gemm_f32_shape_ok(M, N, K, lda, ldb) || ldc < N || ldc % 4 || a_rowP < 0 || epi_kind < 0 || epi_kind > 4 ||
      ((epi_kind == 1 || epi_kind == 2 || epi_kind == 4) && !d_bias) || (epi_kind >= 2 && !d_aux))
    return aph_fail(APH_ERR_ARG, "aph_gemm_f32_test: bad argument (need N %% 128 == 0, K %% 32 == 0, pitches %% 4 == 0; M=%d N=%d K=%d)", M, N, K);
  F32Space sp;
  sp.ws = d_ws; sp.ws_floats = d_ws ? ws_floats : 0;
  hipStream_t st = (hipStream_t)stream_;
  if (epi_kind == 0) launch_gemm_f32(d_A, lda, d_Bt, ldb, M, N, K, EpiF32{d_C, ldc, 1.0f}, st, &sp, a_rowP);
  else if (epi_kind == 1) launch_gemm_f32(d_A, lda, d_Bt, ldb, M, N, K, EpiBiasF32{d_C, ldc, d_bias}, st, &sp, a_rowP);
  else if (epi_kind == 2) launch_gemm_f32(d_A, lda, d_Bt, ldb, M, N, K, EpiGeluF32{d_aux, d_C, ldc, d_bias}, st, &sp, a_rowP);
  else if (epi_kind == 3) launch_gemm_f32(d_A, lda, d_Bt, ldb, M, N, K, EpiGeluBwdF32{d_C, d_aux, ldc}, st, &sp, a_rowP);
  else launch_gemm_f32(d_A, lda, d_Bt, ldb, M, N, K, EpiResidual{d_C, d_aux, ldc, d_bias}, st, &sp, a_rowP);
  return aph_check_launch("aph_gemm_f32_test");
  APH_CATCH
}

// plain C = A * Bt^T (f16 in, f32 out) -- exported for the GEMM unit tests and micro-benchmarks
int aph_gemm_f16(const void* d_A, const void* d_Bt, int M, int N, int K, float* d_C, void* stream_) {
  APH_TRY
  if (!d_A || !d_Bt || !d_C || M < 1 || N % 128 || K % GEMM_BK || N < 1 || K < 1)
    return aph_fail(APH_ERR_ARG, "aph_gemm_f16: need N %% 128 == 0 and K %% 64 == 0 (M=%d N=%d K=%d)", M, N, K);
  launch_gemm((const half_t*)d_A, K, (const half_t*)d_Bt, K, M, N, K, EpiF32{d_C, N, 1.0f}, (hipStream_t)stream_);
  return aph_check_launch("aph_gemm_f16");
  APH_CATCH
}

// same with explicit row pitches and tile configuration (the table of tile_cfg values is at the prototype); any other tile_cfg is refused
int aph_gemm_f16_ld(const void* d_A, int lda, const void* d_Bt, int ldb, int M, int N, int K, float* d_C, int tile_cfg, void* stream_) {
  APH_TRY
  const bool nostore = (tile_cfg & 0x100) != 0;
  tile_cfg &= 0xff;
  if (!(tile_cfg == 0 || tile_cfg == 1 || tile_cfg == 2 || tile_cfg == 5 || (tile_cfg >= 8 && tile_cfg <= 12) || tile_cfg == 14 || tile_cfg == 15 || tile_cfg == 22 || tile_cfg == 24))
    return aph_fail(APH_ERR_ARG, "aph_gemm_f16_ld: tile_cfg %d is not a configuration of this library (0, 1, 2, 5, 8 ... 12, 14, 15, 22, 24)", tile_cfg);
  if (!d_A || !d_Bt || !d_C || M < 1 || N % 128 || K % GEMM_BK || N < 1 || K < 1 || lda < K || ldb < K || (lda & 7) || (ldb & 7) ||
      !gemm_test_cfg_fits(tile_cfg, M, lda, N, ldb, K))
    return aph_fail(APH_ERR_ARG, "aph_gemm_f16_ld: bad shape");
  const half_t* A = (const half_t*)d_A;
  const half_t* B = (const half_t*)d_Bt;
  const EpiF32 epi{d_C, N, 1.0f};
  hipStream_t st = (hipStream_t)stream_;
  if (nostore) {          // measurement only: the same main loops with the output stores compiled out of the taken path
    const EpiNoStore en{d_C, N};
    if (tile_cfg == 2) launch_gemm_cfg<GemmBig>(A, lda, B, ldb, M, N, K, en, st);
    else if (tile_cfg == 5) launch_gemm_ws_cfg<GemmWS>(A, lda, B, ldb, M, N, K, en, st, nullptr);
    else return aph_fail(APH_ERR_ARG, "aph_gemm_f16_ld: the no-store variant exists for tile_cfg 2 and 5");
    return aph_check_launch("aph_gemm_f16_ld");
  }
  // the measurement-only families; everything else goes through gemm_f16_launch_cfg
  if (tile_cfg == 22 || tile_cfg == 24) {                // split-K (2 / 4 ways) of the 128x128 configuration, private workspace
    SplitKSpace* ws = nullptr;
    if (const int rc = gemm_test_splitk_space(&ws)) return rc;
    launch_gemm_splitk<GemmMidDeep8>(A, lda, B, ldb, M, N, K, epi, tile_cfg == 22 ? 2 : 4, *ws, st);
  }
  else if (tile_cfg == 11) launch_gemm_cfg<GemmPair>(A, lda, B, ldb, M, N, K, epi, st);
  else if (tile_cfg == 12) launch_gemm_cfg<GemmFat>(A, lda, B, ldb, M, N, K, epi, st);
  else if (const int rc = gemm_f16_launch_cfg(A, lda, B, ldb, M, N, K, epi, tile_cfg, nullptr, st)) return rc;
  return aph_check_launch("aph_gemm_f16_ld");
  APH_CATCH
}

// One f16 GEMM with one of the ViT's epilogues (include/aphantasia_hip_test.h); tile_cfg: the product's families only
int aph_gemm_f16_epi_test(const void* d_A, int lda, const void* d_Bt, int ldb, int M, int N, int K, void* d_out, int ldo, void* d_aux, const float* d_bias,
                          const float* d_res, float scale, int epi_kind, int P, int T, int tile_cfg, float* d_ws, size_t ws_floats, int small_batch,
                          void* stream_) {
  APH_TRY
  const bool cfg_ok = tile_cfg == 0 || tile_cfg == 1 || tile_cfg == 2 || tile_cfg == 5 || tile_cfg == 8 || tile_cfg == 9 || tile_cfg == 10 ||
                      tile_cfg == 14 || tile_cfg == 15;
  const bool need_ok = !((epi_kind == APH_EPI_RESIDUAL && (!d_bias || !d_res)) || (epi_kind == APH_EPI_GELU && (!d_aux || !d_bias)) ||
                         (epi_kind == APH_EPI_GELU_BWD && !d_aux) || (epi_kind == APH_EPI_PATCH_EMBED && (!d_bias || P < 1 || T < P + 1 || M % P)));
  if (!d_A || !d_Bt || !d_out || M < 1 || N < 128 || N % 128 || K < GEMM_BK || K % GEMM_BK || lda < K || ldb < K || (lda & 7) || (ldb & 7) ||
      (epi_kind != APH_EPI_PATCH_EMBED && (ldo < N || (ldo & 7))) || epi_kind < APH_EPI_F32 || epi_kind > APH_EPI_PATCH_EMBED || !need_ok || !cfg_ok ||
      !gemm_test_cfg_fits(tile_cfg, M, lda, N, ldb, K) || (d_ws && !ws_floats))
    return aph_fail(APH_ERR_ARG, "aph_gemm_f16_epi_test: bad argument (epi_kind %d, tile_cfg %d, M=%d N=%d K=%d lda=%d ldb=%d ldo=%d)", epi_kind, tile_cfg,
                    M, N, K, lda, ldb, ldo);
  const half_t* A = (const half_t*)d_A;
  const half_t* B = (const half_t*)d_Bt;
  hipStream_t st = (hipStream_t)stream_;
  SplitKSpace sp;
  sp.ws = d_ws;
  sp.ws_floats = d_ws ? ws_floats : 0;
  sp.small_batch = small_batch != 0;
  int rc = 0;
  auto run = [&](auto epi) { rc = gemm_f16_launch_cfg(A, lda, B, ldb, M, N, K, epi, tile_cfg, &sp, st); };
  switch (epi_kind) {
    case APH_EPI_F32: run(EpiF32{(float*)d_out, ldo, scale}); break;
    case APH_EPI_F16: run(EpiF16{(half_t*)d_out, ldo, d_bias}); break;
    case APH_EPI_F16_SCALE: run(EpiF16Scale{(half_t*)d_out, ldo, scale}); break;
    case APH_EPI_RESIDUAL: run(EpiResidual{(float*)d_out, d_res, ldo, d_bias}); break;
    case APH_EPI_GELU: run(EpiGelu{(half_t*)d_aux, (half_t*)d_out, ldo, d_bias}); break;
    case APH_EPI_GELU_BWD: run(EpiGeluBwd{(half_t*)d_out, (const half_t*)d_aux, ldo}); break;
    default: run(EpiPatchEmbed{(float*)d_out, d_bias, N, P, T}); break;
  }
  if (rc) return rc;
  return aph_check_launch("aph_gemm_f16_epi_test");
  APH_CATCH
}

// The f16 path's LayerNorm launches alone, with the argument sets of vit.hip (include/aphantasia_hip_test.h)
int aph_ln_test(int mode, int D, int M, int T, int xs, int res_T, int flags, const float* d_x, const float* d_g, const float* d_b, const void* d_dy,
                const void* d_res, void* d_out, void* d_out2, const float* d_cls, const float* d_pos, float* d_x_fill, const float* d_x2,
                const float* d_g2, const float* d_b2, void* stream_) {
  APH_TRY
  const int nv = D / 256, hilo = flags & 1, res_f16 = (flags >> 1) & 1;
  bool ok = D % 256 == 0 && nv >= 1 && nv <= 4 && M >= 1 && T >= 1 && xs >= 1 && res_T >= 0 && d_x && d_g && (flags & ~3) == 0;
  if (mode == 0) ok = ok && d_b && d_out && d_cls && d_pos && d_x_fill && xs == 1 && (!d_g2 == !d_b2) && (!d_g2 == !d_out2) && (!hilo || d_g2);
  else if (mode == 1) ok = ok && d_b && d_out;
  else if (mode == 2) ok = ok && d_dy && (d_out || d_out2) && (!d_x2 == !d_g2) && (!d_x2 || (d_out2 && !d_out && xs == 1)) && (!res_f16 || d_res);
  else if (mode == 3) ok = ok && d_dy && d_out2 && xs == 1;
  else ok = false;
  if (!ok) return aph_fail(APH_ERR_ARG, "aph_ln_test: bad argument (mode %d, D=%d M=%d T=%d xs=%d flags=%d)", mode, D, M, T, xs, flags);
  hipStream_t st = (hipStream_t)stream_;
  if (mode == 0)
    launch_ln_fwd<false, true>(nv, {.x = d_x, .g = d_g, .b = d_b, .out = d_out, .M = M, .T = T, .cls = d_cls, .pos = d_pos, .x_fill = d_x_fill,
                                    .g2 = d_g2, .b2 = d_b2, .out2 = (half_t*)d_out2, .hilo = hilo}, st);
  else if (mode == 1)
    launch_ln_fwd<true, false>(nv, {.x = d_x, .g = d_g, .b = d_b, .out = d_out, .M = M, .T = T, .xs = xs, .hilo = hilo}, st);
  else if (mode == 2)
    launch_ln_bwd<true, false>(nv, {.dy = d_dy, .x = d_x, .g = d_g, .res = d_res, .out32 = (float*)d_out, .out16 = (half_t*)d_out2, .M = M, .T = T,
                                    .xs = xs, .res_T = res_T, .x_b = d_x2, .g_b = d_g2, .res_f16 = res_f16}, st);
  else
    launch_ln_bwd<false, true>(nv, {.dy = d_dy, .x = d_x, .g = d_g, .out16 = (half_t*)d_out2, .M = M, .T = T}, st);
  return aph_check_launch("aph_ln_test");
  APH_CATCH
}

}  // extern "C"
