// Image parameteriser (SURVEY.md K1-K4 and their adjoints): the plan, the launch of each stage, and the C ABI.
//
//   spectrum params --x scale--> column C2C (length H) --> row C2R (length W) --> raw image          synth_fft.h
//   raw --(global unbiased std, contrast)--> 3x3 colour mix --> sigmoid --> rgb in (0,1)              synth_rgb.h
//   the RGB priors and the --sharp term on rgb                                                       synth_terms.h
//   the CPPN generator (cppn.py): network weights --> rgb, and its adjoint                           synth_cppn.h
//
// Replaces: aphantasia/image.py:164-175 (fft_image.inner), :21-28 (to_valid_rgb.inner),
//           :114-118 (pixel_image.inner).  All arithmetic fp32, reductions in fp64.
#include "synth_fft.h"
#include "synth_rgb.h"
#include "synth_terms.h"
#include "synth_cppn.h"

#include <memory>

using namespace aph;

static const int kElemBlocks = 1024;      // grid of the element-wise kernels (256 threads each)

struct aph_synth_plan {
  int C, H, W, Wc, TC, col_threads = 1024;   // column pass: 8 columns x 1024 threads measured best at 720p (95 vs 122 us per synth fwd+bwd)
  Fft1D ph, pw;
  int col_blocks, nrow_blocks;               // column tiles; row pairs
  size_t col_lds, row_lds;                   // dynamic LDS of the column / row kernels: two buffers of TC x H / W complex values
  float norm;                                // 1 / sqrt(H W)   (norm='ortho')
  float2 *twH = nullptr, *twW = nullptr;   // exp(+2 pi i t / H), t < H; the same for W
  float2* tmp = nullptr;      // [C][H][Wc] complex intermediate
  float* dn = nullptr;        // [C][H][W]
  double* partials = nullptr; // max(nrow_blocks, kElemBlocks) * 2
  float* stats = nullptr;     // mean, std
  float* bstats = nullptr;    // A, B, mean
  size_t HW() const { return (size_t)H * W; }
  double n() const { return (double)C * H * W; }
  ~aph_synth_plan() {
    for (void* q : {(void*)twH, (void*)twW, (void*)tmp, (void*)dn, (void*)partials, (void*)stats, (void*)bstats}) (void)hipFree(q);
  }
};

static bool factorize(int n, Fft1D* p) {
  p->n = n; p->npass = 0;
  int m = n;
  auto push = [&](int r) { if (p->npass >= 14) return false; p->radix[p->npass++] = r; return true; };
  while (m % 4 == 0) { if (!push(4)) return false; m /= 4; }
  while (m % 2 == 0) { if (!push(2)) return false; m /= 2; }
  for (int r = 3; (long long)r * r <= m || r <= 31; r += 2)
    while (m % r == 0) { if (!push(r)) return false; m /= r; }
  if (m > 1 && !push(m)) return false;             // the remaining factor is a prime > 31 (fft_pass_large)
  return true;
}

template <typename T>
static bool dev_alloc(T** p, size_t n) { return hipMalloc((void**)p, sizeof(T) * n) == hipSuccess; }

static float2* make_twiddles(int n) {
  std::vector<float2> h(n);
  for (int t = 0; t < n; ++t) {
    const double ang = 2.0 * M_PI * (double)t / (double)n;
    h[t] = make_float2((float)cos(ang), (float)sin(ang));
  }
  float2* d = nullptr;
  if (!dev_alloc(&d, n)) return nullptr;
  if (hipMemcpy(d, h.data(), sizeof(float2) * n, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return nullptr; }
  return d;
}

// ---- one launch helper per stage: the plan and the pointers that differ between the entry points ---------------------------------
// spectrum [C][H][Wc] (x scale, + scale * shift; both nullable) -> plan.tmp
static void launch_col_synth(const aph_synth_plan* p, const float* spectrum, const float* scale, const float* shift, hipStream_t st) {
  APH_LAUNCH(fft_col_synth_kernel, dim3(p->col_blocks), dim3(p->col_threads), p->col_lds, st, (const float2*)spectrum, scale, shift, p->tmp,
             p->ph, (const float2*)p->twH, p->C, p->H, p->Wc, p->TC);
}
// plan.tmp -> image [C][H][W], and its (sum, sumsq) per row pair in plan.partials
static void launch_row_synth(const aph_synth_plan* p, float* image, hipStream_t st) {
  APH_LAUNCH(fft_row_synth_kernel, dim3(p->nrow_blocks), dim3(256), p->row_lds, st, (const float2*)p->tmp, image, p->partials, p->pw,
             (const float2*)p->twW, p->H, p->W, p->Wc, p->norm);
}
// plain: rfft2 of dn itself; else the adjoint row pass of plan.bstats[0] dn + plan.bstats[1] (raw - plan.bstats[2])  -> plan.tmp
static void launch_row_adjoint(const aph_synth_plan* p, const float* dn, const float* raw, int plain, hipStream_t st) {
  APH_LAUNCH(fft_row_adjoint_kernel, dim3(p->nrow_blocks), dim3(256), p->row_lds, st, dn, raw, plain ? (const float*)nullptr : (const float*)p->bstats,
             p->tmp, p->pw, (const float2*)p->twW, p->H, p->W, p->Wc, p->norm, plain);
}
// plan.tmp (x scale, nullable) -> spectrum [C][H][Wc]
static void launch_col_adjoint(const aph_synth_plan* p, const float* scale, float* spectrum, hipStream_t st) {
  APH_LAUNCH(fft_col_adjoint_kernel, dim3(p->col_blocks), dim3(p->col_threads), p->col_lds, st, (const float2*)p->tmp, scale, (float2*)spectrum,
             p->ph, (const float2*)p->twH, p->C, p->H, p->Wc, p->TC);
}
// plan.partials[nparts][2] -> plan.stats
static void launch_stats_finalize(const aph_synth_plan* p, int nparts, hipStream_t st) {
  APH_LAUNCH(stats_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)p->partials, nparts, p->n(), p->stats);
}

static ColorMat to_cm(const float* cc) { ColorMat m; for (int i = 0; i < 9; ++i) m.m[i] = cc ? cc[i] : (i % 4 == 0 ? 1.f : 0.f); return m; }

// raw, plan.stats -> rgb
static void launch_rgb_fwd(const aph_synth_plan* p, const float* raw, float contrast, float fixed_div, const float* colcorr_t9, int decorrelate,
                           float* rgb, hipStream_t st) {
  APH_LAUNCH(rgb_fwd_kernel, dim3(kElemBlocks), dim3(256), 0, st, raw, (const float*)p->stats, contrast, fixed_div, to_cm(colcorr_t9),
             decorrelate, rgb, p->HW());
}
// d_rgb -> plan.dn (the gradient before the std normalisation) and plan.bstats (the coefficients of that normalisation's adjoint)
static void launch_rgb_bwd(const aph_synth_plan* p, const float* d_rgb, float gscale, const float* rgb, const float* raw, float contrast,
                           float fixed_div, const float* colcorr_t9, int decorrelate, hipStream_t st) {
  APH_LAUNCH(rgb_bwd_kernel, dim3(kElemBlocks), dim3(256), 0, st, d_rgb, rgb, raw, to_cm(colcorr_t9), decorrelate, gscale, p->dn,
             p->partials, p->HW());
  APH_LAUNCH(bstats_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)p->partials, kElemBlocks, p->n(), (const float*)p->stats,
             contrast, fixed_div, p->bstats);
}

// ---- CPPN generator: what both launches share, and one launch helper per kernel (the activation is the kernels' template argument)
struct CppnArgs {
  const float *params, *xs, *ys;
  int W;
  size_t HW;
  CppnLayout g;
  hipStream_t st;
};
template <int ACT>
static void launch_cppn_fwd(const CppnNet& net, const CppnArgs& a, float* stash, float* rgb) {
  const size_t lds = sizeof(float) * net.fwd_lds();
  APH_ALLOW_SMEM(cppn_fwd_kernel<ACT>, lds);
  APH_LAUNCH(cppn_fwd_kernel<ACT>, dim3(a.g.ntiles < kCppnFwdBlocks ? a.g.ntiles : kCppnFwdBlocks), dim3(64 * kCppnWaves), lds, a.st, a.params, net,
             a.xs, a.ys, a.W, a.HW, stash, rgb, a.g.ntiles);
}
template <int ACT>
static void launch_cppn_bwd(const CppnNet& net, const CppnArgs& a, const float* d_rgb, float gscale, const float* rgb, const float* stash,
                            float* partials) {
  const size_t lds = sizeof(float) * net.bwd_lds();
  APH_ALLOW_SMEM(cppn_bwd_kernel<ACT>, lds);
  APH_LAUNCH(cppn_bwd_kernel<ACT>, dim3(a.g.bwd_blocks), dim3(64 * kCppnWaves), lds, a.st, a.params, net, a.xs, a.ys, a.W, a.HW, d_rgb, gscale,
             rgb, stash, partials, net.count(), a.g.ntiles);
}

extern "C" {

int aph_synth_plan_create(int C, int H, int W, aph_synth_plan** out) {
  APH_TRY
  if (!out || C < 1 || H < 2 || W < 2) return aph_fail(APH_ERR_ARG, "aph_synth_plan_create: bad shape C=%d H=%d W=%d", C, H, W);
  std::unique_ptr<aph_synth_plan> p(new aph_synth_plan());
  p->C = C; p->H = H; p->W = W; p->Wc = W / 2 + 1;
  if (!factorize(H, &p->ph) || !factorize(W, &p->pw))
    return aph_fail(APH_ERR_UNSUPPORTED, "FFT size %dx%d has more than 14 prime factors", W, H);
  if (W > 8192 || H > 8192) return aph_fail(APH_ERR_UNSUPPORTED, "FFT dimension > 8192 not supported (%dx%d)", W, H);
  int tc = (64 * 1024) / (H * 8);
  p->TC = tc < 1 ? 1 : (tc > 8 ? 8 : tc);
  p->col_blocks = (C * p->Wc + p->TC - 1) / p->TC;
  p->nrow_blocks = C * ((H + 1) / 2);
  p->col_lds = sizeof(float2) * 2 * p->TC * H;
  p->row_lds = sizeof(float2) * 2 * W;
  p->norm = (float)(1.0 / sqrt((double)H * (double)W));
  const int npart = p->nrow_blocks > kElemBlocks ? p->nrow_blocks : kElemBlocks;
  const bool ok = (p->twH = make_twiddles(H)) && (p->twW = make_twiddles(W)) && dev_alloc(&p->tmp, (size_t)C * H * p->Wc) &&
                  dev_alloc(&p->dn, (size_t)C * H * W) && dev_alloc(&p->partials, 2 * (size_t)npart) && dev_alloc(&p->stats, 2) &&
                  dev_alloc(&p->bstats, 4);
  if (!ok) return aph_fail(APH_ERR_HIP, "synth plan allocation failed");
  APH_ALLOW_SMEM(fft_col_synth_kernel, p->col_lds);
  APH_ALLOW_SMEM(fft_col_adjoint_kernel, p->col_lds);
  APH_ALLOW_SMEM(fft_row_synth_kernel, p->row_lds);
  APH_ALLOW_SMEM(fft_row_adjoint_kernel, p->row_lds);
  *out = p.release();
  return APH_OK;
  APH_CATCH
}

int aph_synth_plan_destroy(aph_synth_plan* p) {
  delete p;
  return APH_OK;
}

// test hook (aphantasia_hip_test.h): the plan's column tile and the radices of both transforms, in pass order
int aph_synth_plan_describe(const aph_synth_plan* p, int* out31) {
  APH_TRY
  if (!p || !out31) return aph_fail(APH_ERR_ARG, "aph_synth_plan_describe: null argument");
  out31[0] = p->TC;
  const Fft1D* plans[2] = {&p->ph, &p->pw};
  for (int a = 0; a < 2; ++a) {
    int* o = out31 + 1 + 15 * a;
    o[0] = plans[a]->npass;
    for (int i = 0; i < 14; ++i) o[1 + i] = i < plans[a]->npass ? plans[a]->radix[i] : 0;
  }
  return APH_OK;
  APH_CATCH
}

// params [C,H,Wc,2] f32, scale [H,Wc] f32, shift [H,Wc] f32 or NULL  ->  raw [C,H,W], rgb [C,H,W]
// (image.py:164-175 + :24-28).  stats (mean, std of raw at contrast 1) stay in the plan for the adjoint.
int aph_synth_fft_fwd(aph_synth_plan* p, const float* params, const float* scale, const float* shift, float contrast,
                      const float* colcorr_t9, int decorrelate, float* raw, float* rgb, void* stream_) {
  APH_TRY
  if (!p || !params || !scale || !raw || !rgb) return aph_fail(APH_ERR_ARG, "aph_synth_fft_fwd: null argument");
  hipStream_t st = (hipStream_t)stream_;
  launch_col_synth(p, params, scale, shift, st);
  launch_row_synth(p, raw, st);
  launch_stats_finalize(p, p->nrow_blocks, st);
  launch_rgb_fwd(p, raw, contrast, 0.f, colcorr_t9, decorrelate, rgb, st);
  return aph_check_launch("aph_synth_fft_fwd");
  APH_CATCH
}

// d_rgb [C,H,W] (times gscale) -> grad_params [C,H,Wc,2]   (adjoint of aph_synth_fft_fwd)
int aph_synth_fft_bwd(aph_synth_plan* p, const float* d_rgb, float gscale, const float* rgb, const float* raw,
                      const float* scale, float contrast, const float* colcorr_t9, int decorrelate, float* grad_params,
                      void* stream_) {
  APH_TRY
  if (!p || !d_rgb || !rgb || !raw || !scale || !grad_params) return aph_fail(APH_ERR_ARG, "aph_synth_fft_bwd: null argument");
  hipStream_t st = (hipStream_t)stream_;
  launch_rgb_bwd(p, d_rgb, gscale, rgb, raw, contrast, 0.f, colcorr_t9, decorrelate, st);
  launch_row_adjoint(p, p->dn, raw, 0, st);
  launch_col_adjoint(p, scale, grad_params, st);
  return aph_check_launch("aph_synth_fft_bwd");
  APH_CATCH
}

// Standalone transforms on the plan's geometry, torch.fft semantics with norm='ortho' (illustrip.py:401-409: the per-frame
// irfftn -> warp -> rfftn round trip of `--gen FFT`).
//   aph_irfft2: spectrum [C,H,Wc,2] -> image [C,H,W]   (= torch.fft.irfftn(view_as_complex(x), s=(H,W), norm='ortho'))
//   aph_rfft2:  image [C,H,W] -> spectrum [C,H,Wc,2]   (= view_as_real(torch.fft.rfftn(x, s=(H,W), dim=[-2,-1], norm='ortho')))
int aph_irfft2(aph_synth_plan* p, const float* spectrum, float* image, void* stream_) {
  APH_TRY
  if (!p || !spectrum || !image) return aph_fail(APH_ERR_ARG, "aph_irfft2: null argument");
  hipStream_t st = (hipStream_t)stream_;
  launch_col_synth(p, spectrum, nullptr, nullptr, st);
  launch_row_synth(p, image, st);
  return aph_check_launch("aph_irfft2");
  APH_CATCH
}

int aph_rfft2(aph_synth_plan* p, const float* image, float* spectrum, void* stream_) {
  APH_TRY
  if (!p || !image || !spectrum) return aph_fail(APH_ERR_ARG, "aph_rfft2: null argument");
  hipStream_t st = (hipStream_t)stream_;
  launch_row_adjoint(p, image, image, 1, st);
  launch_col_adjoint(p, nullptr, spectrum, st);
  return aph_check_launch("aph_rfft2");
  APH_CATCH
}

// Spatial-domain parameterisers (pixel_image image.py:114-118; the DWT path after its inverse transform):
// raw [C,H,W] -> rgb.  fixed_div > 0: image * contrast / fixed_div (fixcontrast), else / global std.
int aph_synth_spatial_fwd(aph_synth_plan* p, const float* raw, float contrast, float fixed_div, const float* colcorr_t9,
                          int decorrelate, float* rgb, void* stream_) {
  APH_TRY
  if (!p || !raw || !rgb) return aph_fail(APH_ERR_ARG, "aph_synth_spatial_fwd: null argument");
  hipStream_t st = (hipStream_t)stream_;
  APH_LAUNCH(stats_partial_kernel, dim3(kElemBlocks, 1), dim3(256), 0, st, raw, (size_t)p->C * p->HW(), p->partials);
  launch_stats_finalize(p, kElemBlocks, st);
  launch_rgb_fwd(p, raw, contrast, fixed_div, colcorr_t9, decorrelate, rgb, st);
  return aph_check_launch("aph_synth_spatial_fwd");
  APH_CATCH
}

int aph_synth_spatial_bwd(aph_synth_plan* p, const float* d_rgb, float gscale, const float* rgb, const float* raw,
                          float contrast, float fixed_div, const float* colcorr_t9, int decorrelate, float* d_raw,
                          void* stream_) {
  APH_TRY
  if (!p || !d_rgb || !rgb || !raw || !d_raw) return aph_fail(APH_ERR_ARG, "aph_synth_spatial_bwd: null argument");
  hipStream_t st = (hipStream_t)stream_;
  launch_rgb_bwd(p, d_rgb, gscale, rgb, raw, contrast, fixed_div, colcorr_t9, decorrelate, st);
  APH_LAUNCH(norm_bwd_kernel, dim3(kElemBlocks), dim3(256), 0, st, (const float*)p->dn, raw, (const float*)p->bstats, d_raw, (size_t)p->C * p->HW());
  return aph_check_launch("aph_synth_spatial_bwd");
  APH_CATCH
}

// copies {mean, std} of the last forward to host-visible device memory `out2` (2 floats, device pointer)
int aph_synth_stats(aph_synth_plan* p, float* out2, void* stream_) {
  APH_TRY
  if (!p || !out2) return aph_fail(APH_ERR_ARG, "aph_synth_stats: null argument");
  if (hipMemcpyAsync(out2, p->stats, 2 * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream_) != hipSuccess)
    return aph_fail(APH_ERR_HIP, "aph_synth_stats: copy failed");
  return APH_OK;
  APH_CATCH
}

// restores {mean, std} saved by aph_synth_stats (an autograd node whose forward was followed by other forwards)
int aph_synth_set_stats(aph_synth_plan* p, const float* in2, void* stream_) {
  APH_TRY
  if (!p || !in2) return aph_fail(APH_ERR_ARG, "aph_synth_set_stats: null argument");
  if (hipMemcpyAsync(p->stats, in2, 2 * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream_) != hipSuccess)
    return aph_fail(APH_ERR_HIP, "aph_synth_set_stats: copy failed");
  return APH_OK;
  APH_CATCH
}

// illustrip.py:438-440 RGB priors on rgb [3,H,W]: adds weight * value to *d_loss (nullable) and weight * gradient to
// d_rgb_grad (nullable, accumulated in place).  d_ws: >= aph_rgb_priors_ws_bytes() bytes of device scratch.
size_t aph_rgb_priors_ws_bytes(void) { return sizeof(double) * 3 * kPriorBlocks * 2; }

int aph_rgb_priors(const float* d_rgb, int H, int W, float t_mean, float t_std, float weight, void* d_ws, float* d_loss,
                   float* d_rgb_grad, void* stream_) {
  APH_TRY
  if (!d_rgb || !d_ws || H < 1 || W < 1 || (size_t)H * W < 2) return aph_fail(APH_ERR_ARG, "aph_rgb_priors: bad argument");
  hipStream_t st = (hipStream_t)stream_;
  const size_t HW = (size_t)H * W;
  APH_LAUNCH(stats_partial_kernel, dim3(kPriorBlocks, 3), dim3(256), 0, st, d_rgb, HW, (double*)d_ws);
  APH_LAUNCH(rgb_prior_apply_kernel, dim3(kPriorBlocks, 3), dim3(256), 0, st, d_rgb, HW, (const double*)d_ws, kPriorBlocks, t_mean, t_std,
             weight, d_loss, d_rgb_grad);
  return aph_check_launch("aph_rgb_priors");
  APH_CATCH
}

// clip_fft.py:269-270: adds weight * derivat(rgb, 'naiv') to *d_loss (nullable) and its gradient into d_rgb_grad (nullable,
// accumulated); pass weight = -a.sharp.  d_ws as for aph_rgb_priors.
int aph_rgb_sharp(const float* d_rgb, int H, int W, float weight, void* d_ws, float* d_loss, float* d_rgb_grad, void* stream_) {
  APH_TRY
  if (!d_rgb || !d_ws || H < 2 || W < 2) return aph_fail(APH_ERR_ARG, "aph_rgb_sharp: bad argument");
  hipStream_t st = (hipStream_t)stream_;
  APH_LAUNCH(rgb_sharp_partial_kernel, dim3(kPriorBlocks), dim3(256), 0, st, d_rgb, H, W, (double*)d_ws);
  APH_LAUNCH(rgb_sharp_apply_kernel, dim3(1024), dim3(256), 0, st, d_rgb, H, W, (const double*)d_ws, kPriorBlocks, weight, d_loss, d_rgb_grad);
  return aph_check_launch("aph_rgb_sharp");
  APH_CATCH
}

// ---- CPPN generator (cppn.py:71-116; csrc/synth_cppn.h).  act: 0 unbias, 1 comp, 2 relu.  The library allocates nothing.
size_t aph_cppn_param_count(int layers, int nf, int act) {
  if (layers < 1 || layers > kCppnMaxLayers || nf < 1 || nf > kCppnMaxNf || act < 0 || act > 2) return 0;
  return (size_t)cppn_net(layers, nf, act).count();
}

size_t aph_cppn_ws_bytes(int layers, int nf, int act, int H, int W) {
  if (aph_cppn_param_count(layers, nf, act) == 0 || H < 1 || W < 1) return 0;
  const CppnLayout g = cppn_layout(cppn_net(layers, nf, act), H, W);
  return sizeof(float) * (g.stash_floats + g.partial_floats);
}

// params -> d_rgb [3,H,W]; with d_ws also the stash of pre-activations that aph_cppn_bwd reads
int aph_cppn_fwd(const float* d_params, int layers, int nf, int act, const float* d_xs, const float* d_ys, int H, int W, void* d_ws,
                 float* d_rgb, void* stream_) {
  APH_TRY
  if (!d_params || !d_xs || !d_ys || !d_rgb) return aph_fail(APH_ERR_ARG, "aph_cppn_fwd: null argument");
  if (int rc = cppn_check_shape("aph_cppn_fwd", layers, nf, act, H, W)) return rc;
  const CppnNet net = cppn_net(layers, nf, act);
  const CppnArgs a{d_params, d_xs, d_ys, W, (size_t)H * W, cppn_layout(net, H, W), (hipStream_t)stream_};
  if (act == 0) launch_cppn_fwd<0>(net, a, (float*)d_ws, d_rgb);
  else if (act == 1) launch_cppn_fwd<1>(net, a, (float*)d_ws, d_rgb);
  else launch_cppn_fwd<2>(net, a, (float*)d_ws, d_rgb);
  return aph_check_launch("aph_cppn_fwd");
  APH_CATCH
}

// d_rgb_grad [3,H,W] (times gscale) -> d_grad (flat, the parameters' layout): adjoint of the aph_cppn_fwd that filled d_ws and d_rgb
int aph_cppn_bwd(const float* d_params, int layers, int nf, int act, const float* d_xs, const float* d_ys, int H, int W,
                 const float* d_rgb_grad, float gscale, const float* d_rgb, void* d_ws, float* d_grad, void* stream_) {
  APH_TRY
  if (!d_params || !d_xs || !d_ys || !d_rgb_grad || !d_rgb || !d_ws || !d_grad)
    return aph_fail(APH_ERR_ARG, "aph_cppn_bwd: null argument (the workspace of the forward is required)");
  if (int rc = cppn_check_shape("aph_cppn_bwd", layers, nf, act, H, W)) return rc;
  const CppnNet net = cppn_net(layers, nf, act);
  const CppnArgs a{d_params, d_xs, d_ys, W, (size_t)H * W, cppn_layout(net, H, W), (hipStream_t)stream_};
  float* stash = (float*)d_ws;
  float* partials = stash + a.g.stash_floats;
  if (act == 0) launch_cppn_bwd<0>(net, a, d_rgb_grad, gscale, d_rgb, stash, partials);
  else if (act == 1) launch_cppn_bwd<1>(net, a, d_rgb_grad, gscale, d_rgb, stash, partials);
  else launch_cppn_bwd<2>(net, a, d_rgb_grad, gscale, d_rgb, stash, partials);
  const int P = net.count();
  APH_LAUNCH(cppn_reduce_kernel, dim3((P + 31) / 32), dim3(256), 0, a.st, (const float*)partials, a.g.bwd_blocks, P, d_grad);
  return aph_check_launch("aph_cppn_bwd");
  APH_CATCH
}

}  // extern "C"
