/* libaphantasia_hip.so -- test and measurement hooks.  NOT part of the drop-in boundary (include/aphantasia_hip.h):
 * nothing a reference-side binding needs is declared here.  Used by tests/ (GEMM core alone, every tile
 * configuration) and by bench.py's roofline leg (per-launch GEMM timing on the launch stream).
 */
#ifndef APHANTASIA_HIP_TEST_H
#define APHANTASIA_HIP_TEST_H

#include "aphantasia_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-launch HIP-event timing of the ViT's GEMM launches (bench.py roofline): on/off, then read the sums */
int aph_vit_profile(aph_vit* vit, int on);
int aph_vit_profile_read(aph_vit* vit, double* ms_total, long long* launches, double* flops);
/* The ViT's attention kernels alone (head dim 64, T <= 256): mode 0 = forward (qkv -> att, lse), mode 1 = backward
 * ((qkv, att, lse, datt) -> dqkv).  qkv / dqkv [S*T, 3*heads*64] f16 (q | k | v column blocks), att / datt [S*T, heads*64] f16,
 * lse [S*heads*T] f32 (log-sum-exp of the scores / 8); d_delta: unused and may be NULL (no kernel takes row-dot scratch; the argument stays
 * so that the prototype does not change).  Of the backward kernels only the blocked one (T > 64) reads d_att (D_i = dO_i . att_i); the
 * one-tile backward (T <= 64) forms D_i from the probabilities and never touches it -- the pointer must still not be NULL. */
int aph_attn_test(const void* d_qkv, void* d_att, float* d_lse, const void* d_datt, float* d_delta, void* d_dqkv, int S, int T, int heads,
                  int mode, void* stream);
/* The exact path's fp32 attention kernels alone (vit_attn_f32.h; head dim 64, T <= 256), every buffer f32 in the layouts above: mode 0 = forward
 * (qkv -> att, lse), mode 1 = backward ((qkv, lse, datt) -> dqkv, and d_delta [S*heads*T] = sum_j P_ij dP_ij, which the dK / dV kernel reads
 * back).  The backward does not read d_att.  Refused (APH_ERR_ARG) like aph_attn_test: NULL qkv / att / lse, S, T, heads < 1, T > 256, another
 * mode, and in mode 1 a NULL d_datt, d_delta or d_dqkv. */
int aph_attn_f32_test(const float* d_qkv, float* d_att, float* d_lse, const float* d_datt, float* d_delta, float* d_dqkv, int S, int T, int heads,
                      int mode, void* stream);
/* The text tower's causal instantiation of the fp32 attention forward alone: as aph_attn_f32_test mode 0, but query row i sees the keys j <= i
 * only (the later keys are not read into a score at all).  Refused (APH_ERR_ARG): a NULL buffer, S, T, heads < 1, T > 256. */
int aph_attn_causal_f32_test(const float* d_qkv, float* d_att, float* d_lse, int S, int T, int heads, void* stream);
/* the exact path's f32-input MFMA GEMM alone: C = epilogue(A * Bt^T), f32 in / out.  epi_kind 0 = plain (pitch ldc), 1 = + bias, 2 = QuickGELU
 * (C = g, d_aux = dg/du), 3 = GELU backward (C = acc * d_aux), 4 = residual (C = d_aux + acc + bias).  d_ws (ws_floats): split-K workspace or
 * NULL (never split).  a_rowP > 0: A row m is read from row m + m / a_rowP + 1 (the patch rows of a token-major buffer). */
int aph_gemm_f32_test(const float* d_A, int lda, int a_rowP, const float* d_Bt, int ldb, int M, int N, int K, float* d_C, int ldc,
                      const float* d_bias, float* d_aux, int epi_kind, float* d_ws, size_t ws_floats, void* stream);
/* C[M,N] f32 = A[M,K] f16 * Bt[N,K]^T f16 (N % 128 == 0, K % 64 == 0): the ViT GEMM core with the automatic tile choice */
int aph_gemm_f16(const void* d_A, const void* d_Bt, int M, int N, int K, float* d_C, void* stream);
/* same with explicit row pitches (elements, multiples of 8) and an explicit tile configuration:
 *    0  automatic (the shape heuristic of launch_gemm)
 *    1  64x64, 4 waves            2  256x128, 8 waves, 3-stage ring
 *    5  256x128 wave-specialised persistent (2 DMA producer waves + 8 MFMA consumer waves, register epilogue: vit_gemm_ws.h)
 *    8 / 9   64x64 split-K x2 / x4                10  128x128, 8 waves, 4-stage ring
 *   11  128x128, 4 waves, 2-stage ring, two workgroups per CU (measured slower than 2 on every ViT shape: profiles/r02_gemm_shapes.txt)
 *   12  256x128 on four waves of 128x64, one per SIMD (measured slower than 2: same file)
 *   14 / 15  64x64 register-staged split-K: each of the four waves streams its own k-tiles (global_load_dwordx4 -> private LDS image ->
 *            fragments; 4 / 3 k-steps of 32 in flight), no barrier in the main loop, ordered 4-way sum at the end (vit_gemm_rs.h: the small-M
 *            default for narrow outputs)
 *   22 / 24  128x128 split-K x2 / x4
 * | 0x100 (with 2 or 5 only): measurement variant whose epilogue keeps the accumulators live but never stores (upper bound of
 *   what overlapping the store phase could gain: tools/exp/gemm_nostore.py).
 * any other value is rejected (APH_ERR_ARG, the message names tile_cfg) before anything is launched -- 4 (the phased 256x256 kernel) and
 * 16 / 17 (the A-resident 64x256 kernel) among them: those families lost their measurements and are no longer in the library. */
int aph_gemm_f16_ld(const void* d_A, int lda, const void* d_Bt, int ldb, int M, int N, int K, float* d_C, int tile_cfg,
                    void* stream);

/* One f16 GEMM with one of the ViT's epilogues (vit_gemm.h), an explicit tile configuration and explicit pitches (elements, multiples of 8):
 * out = epilogue(A[M,K] * Bt[N,K]^T), N % 128 == 0, K % 64 == 0.  epi_kind (bias: N floats):
 *    APH_EPI_F32          d_out f32 [M, ldo] = acc * scale                                   (patch-embedding dgrad, f32 gradient)
 *    APH_EPI_F16          d_out f16 [M, ldo] = acc (+ d_bias if not NULL)                    (QKV; the dgrads without bias)
 *    APH_EPI_F16_SCALE    d_out f16 [M, ldo] = acc * scale                                   (patch-embedding dgrad, f16 gradient)
 *    APH_EPI_RESIDUAL     d_out f32 [M, ldo] = d_res [M, ldo] + acc + d_bias                  (out-proj, fc2)
 *    APH_EPI_GELU         u = acc + d_bias: d_out f16 [M, ldo] = QuickGELU(u), d_aux f16 [M, ldo] = its derivative   (fc1)
 *    APH_EPI_GELU_BWD     d_out f16 [M, ldo] = acc * d_aux (f16 [M, ldo])                    (fc2 dgrad)
 *    APH_EPI_PATCH_EMBED  patch row m = s P + p -> d_out f32 row s T + 1 + p (pitch N) = acc + d_bias[(1 + p) N ...] (d_bias = pos [T, N];
 *                         M % P == 0, T > P, ldo ignored; class rows s T are not written)
 * tile_cfg: the product's families only -- 0 (automatic: launch_gemm with d_ws / ws_floats as the split-K workspace, or NULL, and small_batch as
 * SplitKSpace::small_batch), 1, 2, 5, 8, 9, 10, 14, 15 as for aph_gemm_f16_ld; any other value, or a shape outside the family's limits, is
 * rejected (APH_ERR_ARG). */
#define APH_EPI_F32 0
#define APH_EPI_F16 1
#define APH_EPI_F16_SCALE 2
#define APH_EPI_RESIDUAL 3
#define APH_EPI_GELU 4
#define APH_EPI_GELU_BWD 5
#define APH_EPI_PATCH_EMBED 6
int aph_gemm_f16_epi_test(const void* d_A, int lda, const void* d_Bt, int ldb, int M, int N, int K, void* d_out, int ldo, void* d_aux,
                          const float* d_bias, const float* d_res, float scale, int epi_kind, int P, int T, int tile_cfg, float* d_ws,
                          size_t ws_floats, int small_batch, void* stream);
/* The f16 path's LayerNorm kernels (vit_ops.h) alone, D = 256 ... 1024 (a multiple of 256), rows of D floats unless said otherwise.
 *   mode 0  ln_pre: d_out f32 [M, D] = LN(x; g, b); row t == 0 of every image (row % T == 0) is read as d_cls + d_pos[0 .. D) and also written
 *           to d_x_fill.  d_g2 / d_b2 / d_out2 (all or none): the next LayerNorm fused behind it, d_out2 f16 = LN(out; g2, b2).  xs must be 1.
 *   mode 1  d_out f16 [M, D] = LN(x; g, b), x row m at row m * xs (xs = T: class rows only)
 *   mode 2  LayerNorm backward from f16 dy [M, D] (compact): x, res and the outputs at row m * xs; d_out f32 (or NULL), d_out2 f16 (or NULL);
 *           d_res (or NULL) added on the rows m % res_T == 0 only when res_T > 0; flags & 2: d_res is f16 (it may alias d_out2).
 *           d_x2 / d_g2: the previous LayerNorm's backward fused behind (input d_x2, gain d_g2): d_out2 then receives ITS input gradient in the
 *           patch-row layout below and nothing else is written (d_out NULL, xs 1)
 *   mode 3  LayerNorm backward from f32 dy [M, D] into d_out2 f16 in the patch-row layout: row s T + t -> s (T - 1) + t - 1, class rows dropped
 * flags & 1 (modes 0, 1): hilo -- the f16 rows are [hi (D) | lo (D)] (the fused output of mode 0 only). */
int aph_ln_test(int mode, int D, int M, int T, int xs, int res_T, int flags, const float* d_x, const float* d_g, const float* d_b, const void* d_dy,
                const void* d_res, void* d_out, void* d_out2, const float* d_cls, const float* d_pos, float* d_x_fill, const float* d_x2,
                const float* d_g2, const float* d_b2, void* stream);

/* Read-only descriptions of the path a parameteriser call takes (tests/param_checks.py asserts them per case, so that a retuned tile
 * constant cannot silently move a case onto another kernel).
 *   aph_idwt_coarse_levels: the number of levels, counted from the coarsest, that aph_idwt_fwd / aph_idwt_bwd run in the single coarse-tail
 *     launch (0: one launch per level).  hs / ws / J / L as for aph_idwt_fwd (host arrays, level 0 = finest).
 *   aph_synth_plan_describe: out31[0] = columns per workgroup of the column pass (TC); out31[1] = number of passes over H and
 *     out31[2 .. 15] their radices in order (0 beyond the last pass); out31[16], out31[17 .. 30] the same for W. */
int aph_idwt_coarse_levels(const int* hs, const int* ws, int J, int L);
int aph_synth_plan_describe(const aph_synth_plan* plan, int* out31);

/* Crop / resize adjoint of aph_sample_bwd: 1 = always the per-pixel gather kernel (round 2), 0 = automatic (the separable row-block kernel
 * on frames without wrap padding).  Process-wide, returns the previous value.  (No environment variable changes which kernels the library
 * runs: every switch here is an explicit call.) */
int aph_crop_adjoint_set_gather(int on);
/* Launch shape of the separable crop adjoint: rows per workgroup (rb), columns per thread (cpt), cuts per batch (nbc), column segments (nseg),
 * row-block order (0 = top-down, 1 = centre-out); 0 (order: -1) = automatic.  The kernel is instantiated for 12 or 16
 * accumulator rows (rb <= 12 / rb <= 16) x 2 or 3 columns per thread (tools/exp/crop_adjoint_sweep.py sweeps exactly those). */
int aph_crop_adjoint_set_shape(int rb, int cpt, int nbc, int nseg, int order);

/* MFMA shape of the main loops of the GEMM TEST ENTRIES (aph_gemm_f16, aph_gemm_f16_ld; the ViT's own GEMMs are compiled for the default
 * only) launched from now on: 0 = v_mfma_f32_16x16x32_f16 (default: measured
 * faster on MI355X with real operands -- the chip is power-limited there and the 32x32x16 form sustains less),
 * 1 = v_mfma_f32_32x32x16_f16.  Returns the previous setting.  For within-process A/B measurements and the unit tests. */
int aph_gemm_set_mfma32(int on);
/* the first block's LayerNorm pairs (ln_pre + ln_1 forward, ln_1 + ln_pre backward) as one kernel each and no zero fill of the
 * fp32 gradient stream: on (1, default) / off (0).  Bit-identical either way.
 * Returns the previous value.  Captured graphs keep the setting they were recorded with. */
int aph_vit_set_fuse_ln(int on);
/* [r6] 1 = the ViT backward keeps its residual-stream gradient in f16 only (every LayerNorm backward reads the f16 copy its predecessor wrote
 * for the dgrad GEMM and writes no fp32 stream: 73 instead of 117 MB per launch at 190 cuts); 0 (default) = fp32 stream.  Measurement switch for
 * the loss-curve ensemble (tools/loss_ensemble.py); returns the previous value.  Captured graphs keep the setting they were recorded with. */
int aph_vit_set_grad_stream_f16(int on);
/* Number of 256x128 output tiles from which the shape heuristic picks the wave-specialised persistent kernel (tile_cfg 5)
 * for the ViT's own GEMMs; 0 = never.  Process-wide, returns the previous value (A/B measurements, unit tests at small sizes). */
int aph_gemm_set_ws_min_tiles(int tiles);
/* Register-staged GEMMs (tile_cfg 14 / 15) inside the ViT: 1 (default) = the split-K kernel for GEMMs of at most 128 rows over K <= 1024
 * when the WHOLE batch of the ViT call is that small (cuts x tokens <= 128: one or two cuts) -- the class-row GEMMs of a larger batch's
 * last block stay on the two-pass split-K kernels; 2 = every shape below the wave-specialised kernel's threshold (A/B measurements),
 * 0 = never (the shared-ring tile configurations 1 / 2 / 10 and their two-pass split-K).  The stand-alone entries (aph_gemm_f16 with
 * tile_cfg 0) count as small batches.  Returns the previous value. */
int aph_gemm_set_rs(int mode);
/* Tile order of the wave-specialised GEMM inside an XCD's run: groups of g row panels, column tile by column tile inside a group
 * (0 = automatic: 4 for outputs of >= 12 column tiles, else 1 = n-fastest).  Returns the previous value. */
int aph_gemm_set_ws_pgroup(int g);
/* Pure-MFMA rate probe (bench.py `roofline.peak_measured`): `blocks` workgroups of 8 waves run `iters` x 32 v_mfma_f32_16x16x32_f16 on
 * operands read once from d_src (>= 128 KiB of f16; random data sustains less than zeros: the part is power limited), nothing stored unless a
 * never-true condition holds (d_out: 512 floats).  FLOPs per launch = blocks * 8 * iters * 32 * 16384. */
int aph_mfma_rate(int blocks, int iters, const void* d_src, float* d_out, void* stream);
/* The wave-specialised GEMM (tile_cfg 5) with one of the ViT's real epilogues and optional per-tile shader-clock stamps
 * (tools/exp/gemm_ws_trace.py).  A [M,K], Bt [N,K] f16 dense; epi_kind 0: d_out f16 [M,N] = acc + bias; 1: QuickGELU, d_out = g,
 * d_out2 = dg/du (both f16); 2: d_out f32 [M,N] += acc + bias (residual in place); 3: nothing stored.
 * d_trace: (workgroups x 16 x 4) uint64 or NULL. */
int aph_gemm_ws_probe(const void* d_A, const void* d_Bt, int M, int N, int K, void* d_out, void* d_out2, const float* d_bias, int epi_kind,
                      unsigned long long* d_trace, void* stream);

/* The register-staged split-K small-M GEMM (tile_cfg 14) with an f16 output and per-phase stamps of the chip-wide 100 MHz clock
 * (tools/exp/gemm_rs_trace.py): kind must be 0 (any other kind is rejected with APH_ERR_ARG before anything is launched);
 * d_trace: (workgroups x 8) uint64 or NULL. */
int aph_gemm_rs_probe(const void* d_A, const void* d_Bt, int M, int N, int K, void* d_out, int kind, unsigned long long* d_trace, void* stream);

/* ---- the LPIPS term's kernels alone (csrc/lpips_conv.h, lpips_ops.h).  Activations are f16 [H][W][C], channel-innermost. ----
 * aph_lpips_pack_test: the weight packing of aph_lpips_set_weight.  h_w fp32 HOST [cout][cin][3][3] -> d_out f16:
 *   dgrad 0: [9][cout][C], C = cin rounded up to 8;   dgrad 1: [9][N][cout], N = cin rounded up to 16, taps flipped.  out_elems = that size.
 * aph_lpips_conv_test: one launch of the convolution kernel: d_in [H][W][C] (C % 8 == 0), d_wt packed [9][N][C] (N % 16 == 0), d_bias [N] or
 *   NULL, relu 0 / 1, d_mask [H][W][N] or NULL (output zeroed where mask <= 0), d_out f16 [H][W][N] or NULL, d_out32 planar fp32 [n32][H][W]
 *   or NULL; nf = output channels per workgroup / 16: 4, 2, 1, or 0 for the library's own rule (bit-identical either way).  The forward is (packed forward weights, bias, relu 1); the input gradient is (gradient as d_in, packed dgrad weights, mask).
 * aph_lpips_pool_test: d_out (nullable) [H/2][W/2][C] = 2x2 floor max-pool of d_in; d_din (nullable) [H][W][C] = its backward of d_dpool,
 *   argmax recomputed from d_in (first maximum in row-major window order).
 * aph_lpips_head_test: features d_f against target features d_fy (f16 [P][C]): d_ny fp32 [P][C] = the normalised target, *d_value =
 *   mean_p sum_c lin_c (n_c - ny_c)^2, d_hg (nullable) fp32 [P][C] = gcoef * d(sum_p ...)/df; d_partial: 512 doubles of scratch.
 * aph_lpips_resize_test: adjoint 0: d_half [3][H/2][W/2] = bicubic resize (align_corners) of d_full [3][H][W]; adjoint 1: d_full += the
 *   transpose applied to d_half. */
int aph_lpips_pack_test(const float* h_w, int cout, int cin, int dgrad, void* d_out, size_t out_elems);
int aph_lpips_conv_test(const void* d_in, int H, int W, int C, const void* d_wt, int N, const float* d_bias, int relu, const void* d_mask, void* d_out,
                        float* d_out32, int n32, int nf, void* stream);
int aph_lpips_pool_test(const void* d_in, int H, int W, int C, void* d_out, const void* d_dpool, void* d_din, void* stream);
int aph_lpips_head_test(const void* d_f, const void* d_fy, const float* d_lin, int P, int C, float gcoef, float* d_ny, float* d_hg, double* d_partial,
                        float* d_value, void* stream);
int aph_lpips_resize_test(float* d_full, int H, int W, float* d_half, int adjoint, void* stream);

/* ---- the depth estimator's kernels alone (csrc/depth_kernels.h, the batched / residual instantiation of lpips_conv.h, depth_epi.h's erf-GELU
 * epilogue).  Activations are f16, channel-innermost.
 * aph_depth_attn_test: d_att [B T][64 heads] = softmax(Q K^T / 8) V per (image, head) from d_qkv [B T][3 x 64 heads] (Q | K | V), any T >= 1.
 * aph_depth_conv_test: 3 x 3 pad 1 convolution of `batch` maps d_in [batch][H][W][C] with d_wt packed [9][N][C] (aph_lpips_pack_test):
 *   out = f16(relu?(conv(relu_in ? max(in, 0) : in) + bias) + res + res2) (d_bias, d_res, d_res2 [batch][H][W][N] nullable); stride 2: the
 *   stride-1 result goes to d_tmp [batch][H][W][N] and its even rows / columns to d_out [batch][(H+1)/2][(W+1)/2][N].
 * aph_depth_gemm_test: d_out [M][N] = d_a [M][lda] x d_bt [N][K]^T + d_bias (nullable), N % 16 == 0, K % 8 == 0: the neck's 1 x 1 convolution.
 * aph_depth_convt_test: ConvTranspose2d with kernel = stride = k (1 .. 4): h_w fp32 HOST [cin][cout][k][k], d_wpack = k k cout cin f16 of
 *   scratch, d_in [B][gh][gw][cin] -> d_out [B][gh k][gw k][cout].
 * aph_depth_resize_test: bilinear, align_corners = True, d_in [B][h][w][C] -> d_out [B][H][W][C] (C % 8 == 0).
 * aph_depth_gelu_gemm_test: d_out [M][N] = gelu_erf(d_a [M][K] x d_bt [N][K]^T + d_bias) through launch_gemm (N % 128 == 0, K % 64 == 0). */
int aph_depth_attn_test(const void* d_qkv, void* d_att, int B, int T, int heads, void* stream);
int aph_depth_conv_test(const void* d_in, int H, int W, int C, const void* d_wt, int N, const float* d_bias, int relu, int relu_in, const void* d_res,
                        const void* d_res2, int batch, int stride, void* d_tmp, void* d_out, void* stream);
int aph_depth_gemm_test(const void* d_a, int lda, const void* d_bt, int M, int N, int K, const float* d_bias, void* d_out, void* stream);
int aph_depth_convt_test(const void* d_in, int B, int gh, int gw, int cin, const float* h_w, int cout, int k, const float* d_bias, void* d_wpack, void* d_out,
                         void* stream);
int aph_depth_resize_test(const void* d_in, int B, int h, int w, int C, void* d_out, int H, int W, void* stream);
int aph_depth_gelu_gemm_test(const void* d_a, const void* d_bt, int M, int N, int K, const float* d_bias, void* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
