/* libaphantasia_hip.so -- C ABI of the MI355X (gfx950) hot path of eps696/aphantasia.
 *
 * The reference has no FFI layer of its own: its per-step loop (clip_fft.py:235-306) calls
 * Python functions (aphantasia/image.py, aphantasia/utils.py, aphantasia/transforms.py,
 * openai/CLIP's model.encode_image, torch.optim.Adam).  Each entry point below replaces one of
 * those call sites; the ctypes stubs a maintainer would add are in INTEGRATION.md.
 *
 * Conventions: plain C types; every pointer named d_* / documented "device" is a HIP device
 * pointer (tensor.data_ptr()); `stream` is a hipStream_t passed as void* (0 = default stream);
 * all calls are asynchronous on that stream and never allocate per call; return value 0 = ok,
 * < 0 = error (message through aph_last_error(), thread-local).
 */
#ifndef APHANTASIA_HIP_H
#define APHANTASIA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APH_OK 0
#define APH_ERR_ARG (-1)
#define APH_ERR_HIP (-2)
#define APH_ERR_UNSUPPORTED (-3)
#define APH_ERR_INTERNAL (-4)
#define APH_ERR_COMM (-5)      /* RCCL error */

int aph_version(void);
const char* aph_last_error(void);

/* ---- image parameteriser: aphantasia/image.py ------------------------------------------- */
typedef struct aph_synth_plan aph_synth_plan;

/* twiddles + workspace for a C x H x W image (fft_image closure state, image.py:152-162) */
int aph_synth_plan_create(int C, int H, int W, aph_synth_plan** out);
int aph_synth_plan_destroy(aph_synth_plan* plan);

/* to_valid_rgb(fft_image(...))(shift, contrast): image.py:164-175 + :21-28.
 * params [C,H,W/2+1,2] f32, scale [H,W/2+1] f32, shift [H,W/2+1] f32 or NULL, colcorr_t9 = 3x3
 * row-major colcorr_t (image.py:19) host pointer or NULL (identity).  Writes raw [C,H,W] (the
 * irfft2 output before std-normalisation) and rgb [C,H,W] in (0,1). */
int aph_synth_fft_fwd(aph_synth_plan* plan, const float* d_params, const float* d_scale, const float* d_shift,
                      float contrast, const float* colcorr_t9, int decorrelate, float* d_raw, float* d_rgb, void* stream);
/* adjoint: d_rgb_grad [C,H,W] (multiplied by gscale) -> d_grad_params [C,H,W/2+1,2].  Must follow the
 * aph_synth_fft_fwd that produced rgb/raw (the plan keeps mean/std). */
int aph_synth_fft_bwd(aph_synth_plan* plan, const float* d_rgb_grad, float gscale, const float* d_rgb, const float* d_raw,
                      const float* d_scale, float contrast, const float* colcorr_t9, int decorrelate,
                      float* d_grad_params, void* stream);
/* The two transforms alone, torch.fft semantics with norm='ortho' on the plan's geometry -- illustrip.py:401-409, the
 * per-frame `irfftn -> frame_transform -> rfftn` round trip of `--gen FFT`:
 *   aph_irfft2: d_spectrum [C,H,W/2+1,2] -> d_image [C,H,W]   == torch.fft.irfftn(view_as_complex(x), s=(H,W), norm='ortho')
 *   aph_rfft2:  d_image [C,H,W] -> d_spectrum [C,H,W/2+1,2]   == view_as_real(torch.fft.rfftn(x, s=(H,W), dim=[2,3], norm='ortho')) */
int aph_irfft2(aph_synth_plan* plan, const float* d_spectrum, float* d_image, void* stream);
int aph_rfft2(aph_synth_plan* plan, const float* d_image, float* d_spectrum, void* stream);
/* to_valid_rgb(pixel_image(...)) (image.py:114-118) and the post-inverse-DWT part of dwt_image (image.py:68):
 * raw -> raw*contrast/std (or /fixed_div when fixed_div > 0) -> colour mix -> sigmoid */
int aph_synth_spatial_fwd(aph_synth_plan* plan, const float* d_raw, float contrast, float fixed_div,
                          const float* colcorr_t9, int decorrelate, float* d_rgb, void* stream);
int aph_synth_spatial_bwd(aph_synth_plan* plan, const float* d_rgb_grad, float gscale, const float* d_rgb,
                          const float* d_raw, float contrast, float fixed_div, const float* colcorr_t9, int decorrelate,
                          float* d_raw_grad, void* stream);
/* {mean, std} of raw from the last forward -> d_out2 (device, 2 floats) */
int aph_synth_stats(aph_synth_plan* plan, float* d_out2, void* stream);
/* restore them (d_in2 device, 2 floats) before an adjoint whose forward was followed by other forwards */
int aph_synth_set_stats(aph_synth_plan* plan, const float* d_in2, void* stream);

/* illustrip.py:438-440 (`--gen RGB` priors): mean_c |mean_hw(rgb_c) - t_mean| + mean_c |std_hw(rgb_c) - t_std| (unbiased
 * std) over d_rgb [3,H,W].  Adds weight * value to *d_loss (nullable) and weight * gradient into d_rgb_grad (nullable,
 * accumulated).  d_ws: device scratch of aph_rgb_priors_ws_bytes() bytes. */
size_t aph_rgb_priors_ws_bytes(void);
int aph_rgb_priors(const float* d_rgb, int H, int W, float t_mean, float t_std, float weight, void* d_ws, float* d_loss,
                   float* d_rgb_grad, void* stream);

/* clip_fft.py:269-270 (`--sharp`): weight * derivat(rgb, 'naiv') (utils.py:265-268), value into *d_loss and gradient into
 * d_rgb_grad (both nullable, accumulated); the reference subtracts, so pass weight = -sharp.  d_ws as for aph_rgb_priors. */
int aph_rgb_sharp(const float* d_rgb, int H, int W, float weight, void* d_ws, float* d_loss, float* d_rgb_grad, void* stream);

/* ---- CPPN generator: the reference's cppn.py:71-116, a coordinate network of 1x1 convolutions whose weights are the
 * optimised parameters.  Conv(2 -> nf), (layers - 1) x Conv(nhi -> nf), Conv(nhi -> 3) + sigmoid; act 0 `unbias`
 * (t = atan z; cat[t / 0.67, (t^2 - 0.45) / 0.396]), 1 `comp` (cat[t / 0.67, t^2 / 0.6]), 2 `relu` ((relu z - 0.40) / 0.58);
 * nhi = 2 nf, relu nf.  d_params: per conv in network order weight[out][in] row-major, then bias[out] (f32; 10 803 floats
 * for layers 10, nf 24, unbias).  d_xs [W], d_ys [H]: the input coordinates (channel 0 = x along W, channel 1 = y along H).
 * Supported: 1 <= layers <= 12, 1 <= nf <= 32, any H, W >= 1; else APH_ERR_UNSUPPORTED.  f32 arithmetic on the f32-input
 * MFMA; no atomics: the same shapes give the same bits.  The workspace is the caller's (aph_cppn_ws_bytes: the stash of
 * pre-activations, layers * nf * 4 bytes per pixel, plus one gradient partial per workgroup). */
size_t aph_cppn_param_count(int layers, int nf, int act);
size_t aph_cppn_ws_bytes(int layers, int nf, int act, int H, int W);
/* -> d_rgb [3,H,W] in (0,1).  d_ws NULL: no stash (a forward that no backward follows). */
int aph_cppn_fwd(const float* d_params, int layers, int nf, int act, const float* d_xs, const float* d_ys, int H, int W,
                 void* d_ws, float* d_rgb, void* stream);
/* adjoint of the aph_cppn_fwd that filled d_ws and d_rgb: d_rgb_grad [3,H,W] (times gscale) -> d_grad (layout of d_params) */
int aph_cppn_bwd(const float* d_params, int layers, int nf, int act, const float* d_xs, const float* d_ys, int H, int W,
                 const float* d_rgb_grad, float gscale, const float* d_rgb, void* d_ws, float* d_grad, void* stream);

/* ---- wavelet parameteriser: aphantasia/image.py:33-80 (dwt_image) over pytorch_wavelets.DWTInverse ------- */
/* One synthesis level (lowlevel.SFB2D, mode 'symmetric').  d_ll [C,ll_h,ll_w] running low band (ll_h in {h,h+1}:
 * the extra row/col DWTInverse.forward drops is ignored), d_highs [C,3,h,w] = (LH,HL,HH) of this level,
 * d_g0/d_g1 = rec_lo/rec_hi taps (device, L even <= 64), hscale = dwt_scale gain (image.py:73-80)
 * -> d_out [C, 2h-L+2, 2w-L+2]. */
int aph_idwt_level_fwd(const float* d_ll, int ll_h, int ll_w, const float* d_highs, int h, int w, int C,
                       const float* d_g0, const float* d_g1, int L, float hscale, float* d_out, void* stream);
/* adjoint: d_out_grad -> d_ll_grad [C,ll_h,ll_w] (dropped row/col = 0) and d_highs_grad [C,3,h,w] */
int aph_idwt_level_bwd(const float* d_out_grad, int h, int w, int C, const float* d_g0, const float* d_g1, int L,
                       float hscale, float* d_ll_grad, int ll_h, int ll_w, float* d_highs_grad, void* stream);

/* Every level of DWTInverse in one call (what dwt_image.inner runs per step, image.py:36-38,67).  Host arrays of J entries,
 * level 0 = finest: hs / ws = size of the level's detail bands, hscales = dwt_scale gains (image.py:73-80), d_highs[j]
 * [C,3,hs[j],ws[j]] (device pointers), d_bufs[j] [C, 2 hs[j]-L+2, 2 ws[j]-L+2] = caller-owned scratch for the running low band
 * after level j (d_bufs[0] receives the image; the others are written only where a level's output travels through global
 * memory).  d_yl [C, hs[J-1], ws[J-1]] = the coarsest low band.  The coarse levels -- output up to 80 x 128 -- run in one launch
 * with the running low band kept in LDS (filter lengths 2-8). */
int aph_idwt_fwd(const float* d_yl, const float* const* d_highs, const int* hs, const int* ws, const float* hscales, int J,
                 int C, const float* d_g0, const float* d_g1, int L, float* const* d_bufs, void* stream);
/* adjoint: d_img_grad [C, 2 hs[0]-L+2, 2 ws[0]-L+2] -> d_highs_grad[j] [C,3,hs[j],ws[j]] and d_yl_grad [C,hs[J-1],ws[J-1]];
 * d_gbufs[j] (j >= 1) = scratch of d_bufs[j]'s size (d_gbufs[0] is not used). */
int aph_idwt_bwd(const float* d_img_grad, const int* hs, const int* ws, const float* hscales, int J, int C,
                 const float* d_g0, const float* d_g1, int L, float* const* d_gbufs, float* d_yl_grad,
                 float* const* d_highs_grad, void* stream);

/* ---- sampler: aphantasia/utils.py:218-254 slice_imgs + transforms.py:102-109,165-170 ------- */
/* Geometry of one slice_imgs call.  (Hp,Wp,py0,px0) describe the wrap-tiled overscan frame of
 * pad_up_to/tile_pad (utils.py:152-187); Hp=H, Wp=W, py0=px0=0 when align has no 'over'. */
typedef struct aph_sample_geom {
  int H, W;          /* source image */
  int Hp, Wp;        /* padded frame the crop table refers to */
  int py0, px0;      /* top / left padding */
  int S;             /* number of cuts */
  int size;          /* output side (224) */
  int patch;         /* ViT patch size for the patch-major layouts (32 / 16) */
} aph_sample_geom;

#define APH_OUT_NCHW_RAW 0   /* f32 [S,3,size,size], no normalisation (transform=None) */
#define APH_OUT_NCHW_NORM 1  /* f32 [S,3,size,size], CLIP mean/std normalised (transforms.normalize) */
#define APH_OUT_PATCH_F16 2  /* f16 [S*(size/patch)^2, 3*patch*patch] normalised = patch-embed GEMM operand; row = patch (s, gy, gx), column
                              * k = (iy*patch + ix)*3 + c: pixel-major inside the patch, channel fastest (aph_vit_set_weight permutes conv1.weight to match) */
#define APH_OUT_PATCH_F16_HILO 4 /* aph_sample_fwd only: APH_OUT_PATCH_F16 rows written as [hi (3*patch^2) | lo (3*patch^2)], hi = f16(x), lo = f16(x - hi):
                              * the operand of the split-precision forward aph_vit_forward_hilo */
#define APH_OUT_PATCH_F32 5  /* the APH_OUT_PATCH_F16 row layout in f32 (the exact path, aph_vit_forward_f32); aph_sample_bwd: the gradient in the
                              * same f32 patch-major layout (aph_vit_backward_f32) */
#define APH_GRAD_PATCH_F16 3 /* aph_sample_bwd only: gradient in the patch-major layout stored as f16 (aph_vit_backward_h) */

#define APH_AUG_STRIDE 16
/* per-cut augment row (f32 x 16): [0..7] perspective coeffs, [8] has_perspective, [9..12] erase i,j,h,w
 * (h=0: none), [13] cos(angle), [14] sin(angle), [15] has_rotation (transforms_fast always 1).  The rows of the custom / elastic chains
 * (aph_sample_fwd_tf): [0] dx, [1] dy, [8] = 0, [9..12] the erase rectangle on the (size + 8)-sided canvas, [13..15] as here. */

/* bytes of the caller-owned device workspace d_ws of one forward/backward pair on geometry g (per-cut tap tables of the
 * crop adjoint, per-XCD work lists of the forward; with_aug != 0 adds the cut scratch of the geometric augmentations).  The library never allocates in a
 * launch path, so the calls can be captured into a hipGraph that stays valid as long as the caller's buffers do. */
size_t aph_sample_ws_bytes(const aph_sample_geom* g, int with_aug);
/* d_rgb [3,H,W] f32; d_table int32 [S,3] rows (csize, offx, offy) (utils.py:245-247);
 * d_aug f32 [S,16] or NULL (no geometric augmentation); d_ws: see aph_sample_ws_bytes (required).
 * out layout per out_mode. */
int aph_sample_fwd(const aph_sample_geom* g, const float* d_rgb, const int32_t* d_table, const float* d_aug,
                   void* d_ws, void* d_out, int out_mode, void* stream);
/* adjoint.  d_out_grad: f32 in the layout of out_mode (patch-major f32 for APH_OUT_PATCH_F16; patch-major f16 for
 * APH_GRAD_PATCH_F16), multiplied by gscale.  d_ws as above (required, overwritten).
 * Writes (does not accumulate) d_rgb_grad [3,H,W]. */
int aph_sample_bwd(const aph_sample_geom* g, const void* d_out_grad, float gscale, const int32_t* d_table,
                   const float* d_aug, void* d_ws, float* d_rgb_grad, int out_mode, void* stream);
/* The augment chain by kind (`-tf fast | custom | elastic`, transforms.py:147-170).  APH_TF_FAST is the chain above: the three _tf entry
 * points then forward to aph_sample_ws_bytes(g, 1) / aph_sample_fwd / aph_sample_bwd unchanged.  The two kornia-style chains work on the
 * P x P canvas of pad(4, constant 0.5), P = size + 8:
 *   APH_TF_CUSTOM:  pad -> random_rotate -> jitter(8) -> normalize                         (one gather from the crop scratch to the output)
 *   APH_TF_ELASTIC: pad -> RandomErasing -> random_rotate -> random_elastic -> jitter(8) -> normalize.  Upstream calls elastic_transform2d
 *                   with zero noise: what it computes is a fixed bilinear resample E[v,u] = R(u P/(P-1) - 0.5, v P/(P-1) - 0.5).
 *                   (one 16-tap gather forward; the adjoint goes through a P x P gradient canvas in the workspace)
 * Rotation: kornia warp_affine in pixel space (bilinear, zeros padding, align_corners=True, no ones-mask); jitter: a whole-pixel shift
 * right / down by (dx, dy), zeros shifted in.  Their augment row (APH_AUG_STRIDE floats, same table):
 *   [0] dx, [1] dy (integers 0 .. 7), [2..7] unused, [8] = 0, [9..12] erase i,j,h,w ON THE P x P CANVAS (h=0: none; custom has no erase stage and does not read them),
 *   [13] cos(angle), [14] sin(angle), [15] has_rotation (0: the cut is copied, not resampled).
 * Output: the planar modes hold the whole canvas, f32 [S,3,P,P]; the patch-major modes hold its top-left size x size window in their usual
 * shape -- exactly what a stride = kernel = patch convolution reads of a P-sided input ((P - patch) / patch + 1 == size / patch needs
 * patch > 8, else APH_ERR_ARG); the gradient of the planar modes is [S,3,P,P] likewise.
 * h_aug: HOST copy of the S rows or NULL; when given, dx / dy are range-checked before any launch (the device table cannot be read
 * without a synchronisation; the kernels themselves are memory-safe for any value).  The elastic workspace holds a P x P canvas per cut (its adjoint's). */
#define APH_TF_FAST 0
#define APH_TF_CUSTOM 1
#define APH_TF_ELASTIC 2
size_t aph_sample_ws_bytes_tf(const aph_sample_geom* g, int tf);
int aph_sample_fwd_tf(const aph_sample_geom* g, int tf, const float* d_rgb, const int32_t* d_table, const float* d_aug, const float* h_aug,
                      void* d_ws, void* d_out, int out_mode, void* stream);
int aph_sample_bwd_tf(const aph_sample_geom* g, int tf, const void* d_out_grad, float gscale, const int32_t* d_table, const float* d_aug,
                      const float* h_aug, void* d_ws, float* d_rgb_grad, int out_mode, void* stream);
/* illustrip.py:130-138 frame_transform = T.functional.affine(img, angle, shift, scale, shear, fill=0, BILINEAR) of a whole
 * [C,H,W] image (once per frame).  h_inv_matrix6: HOST pointer, row-major 2x3 inverse affine matrix (torchvision's
 * _get_inverse_affine_matrix with the image centre as origin).  d_dst must not alias d_src. */
int aph_frame_affine(const float* d_src, int C, int H, int W, const float* h_inv_matrix6, float* d_dst, void* stream);
/* ---- depth warp of the illustrip frame loop (/root/reference/depth/depth.py:41-84, illustrip.py:115-128) ----
 * Everything but the depth ESTIMATOR (Depth-Anything-V2, depth.py:20-32, a third-party network): the caller runs it (or
 * anything else) between aph_resize_bicubic and aph_flip_w and hands the depth map to aph_grid_warp.  All images f32,
 * [C,H,W] contiguous; destinations must not alias sources.
 *   aph_triangle_blur: d_dst = torch.lerp(src, triangle_blur(src, kernel_size, power), mix)   (utils.py:137-147; depth.py:75
 *                      uses kernel_size 5, power 2, mix 0.5; mix = 1 is the plain blur).  kernel_size odd, <= 9.
 *   aph_resize_bicubic: F.interpolate(src [C,h,w], (H,W), mode='bicubic', align_corners=True)          (depth.py:41-42)
 *   aph_flip_w: d_dst = flip(src, [-1]), times d_mul elementwise when d_mul != NULL                     (depth.py:77)
 *   aph_grid_warp: depth.py:44-66 -- two bilinear, reflection-padded, align_corners=True grid samples: the depth push
 *                  grid + (centre - grid) * (depth - max(depth) * midpoint) * strength, then the lens stretch
 *                  grid + (centre - grid) * |centre - grid| * strength * dlens.  d_depth [H,W]; centre in [-1,1] (x, y);
 *                  d_ws: C*H*W + 256 floats of scratch (intermediate image + the depth maximum and its partials). */
int aph_triangle_blur(const float* d_src, int C, int H, int W, int kernel_size, float power, float mix, float* d_dst, void* stream);
int aph_resize_bicubic(const float* d_src, int C, int h, int w, float* d_dst, int H, int W, void* stream);
int aph_flip_w(const float* d_src, const float* d_mul, int C, int H, int W, float* d_dst, void* stream);
int aph_grid_warp(const float* d_img, const float* d_depth, int C, int H, int W, float strength, float centre_x, float centre_y,
                  float midpoint, float dlens, float* d_ws, float* d_out, void* stream);
/* NCHW f32 [S,3,R,R] <-> patch-major (entry of model.encode_image for a caller-made batch) */
int aph_patchify_f16(const float* d_nchw, int S, int R, int patch, void* d_patches_f16, void* stream);
/* the same into the [hi | lo] rows of APH_OUT_PATCH_F16_HILO: d_patches_hilo f16 [S*(R/patch)^2, 2 * 3*patch^2] */
int aph_patchify_f16_hilo(const float* d_nchw, int S, int R, int patch, void* d_patches_hilo, void* stream);
/* the same in f32 (APH_OUT_PATCH_F32 layout, values unchanged): d_patches f32 [S*(R/patch)^2, 3*patch^2] */
int aph_patchify_f32(const float* d_nchw, int S, int R, int patch, float* d_patches, void* stream);
int aph_unpatchify_f32(const float* d_patch_grad, int S, int R, int patch, float gscale, float* d_nchw_grad, void* stream);
/* Elements of one row of the patch-major operand: round_up(3*patch^2, 128) -- 3072 for patch 32, 768 for patch 16 (3*patch^2 itself: a
 * multiple of 128 already), 640 for patch 14 (588 elements and 52 pad columns that are always zero: the patch-embedding GEMM needs
 * K % 64 == 0 and its dgrad N % 128 == 0).  Padded rows exist only for patch sides that are no power of two (made by aph_patchify_f16_win);
 * a power-of-two patch of 8 or less (3*patch^2 = 192 ...) has no padded form and aph_vit_create refuses it.  0 for patch < 1. */
int aph_patch_row_elems(int patch);
/* The same conversions for ANY patch side (the sampler's patch-major modes and the entries above need a power of two), with a window: reads the
 * top-left R x R window of d_nchw f32 [S,3,R_src,R_src] and writes d_patches f16 [S*(R/patch)^2, aph_patch_row_elems(patch)], order
 * k = (iy*patch + ix)*3 + c inside a row, the pad columns k >= 3*patch^2 written as zero on every call.  R_src >= R, R % patch == 0. */
int aph_patchify_f16_win(const float* d_nchw, int S, int R_src, int R, int patch, void* d_patches, void* stream);
/* its exact adjoint: d_patch_grad f32 [S*(R/patch)^2, aph_patch_row_elems(patch)] -> d_nchw_grad f32 [S,3,R_src,R_src] = gradient * gscale
 * inside the window, 0 outside; every element is written, nothing is accumulated; the pad columns are not read. */
int aph_unpatchify_f32_win(const float* d_patch_grad, int S, int R_src, int R, int patch, float gscale, float* d_nchw_grad, void* stream);

/* ---- CLIP ViT visual tower: model.encode_image (clip_fft.py:254) + its input-gradient ----- */
typedef struct aph_vit aph_vit;
/* mirrors clip.model.VisionTransformer(input_resolution, patch_size, width, layers, heads, output_dim);
 * max_batch = largest number of cuts per call (activation arena is sized once, never re-allocated) */
int aph_vit_create(int input_resolution, int patch_size, int width, int layers, int heads, int output_dim,
                   int max_batch, aph_vit** out);
int aph_vit_destroy(aph_vit* vit);
size_t aph_vit_workspace_bytes(const aph_vit* vit);
/* one tensor by its OpenAI checkpoint key without the "visual." prefix (fp32 HOST data) */
int aph_vit_set_weight(aph_vit* vit, const char* name, const float* h_data, size_t count);
/* Shapes below: P = (input_resolution / patch)^2 patches per cut, Kp = aph_patch_row_elems(patch) elements per patch row.  Kp = 3*patch^2 for
 * the power-of-two patches (ViT-B/32, ViT-B/16); for patch 14 (ViT-L/14) Kp = 640: rows of 588 elements and 52 zero pad columns, made by
 * aph_patchify_f16_win.  aph_vit_set_weight zero-fills the pad columns of conv1.weight in W and W^T, so the patch embedding (K = Kp) ignores
 * whatever the pad columns of its operand hold only if they are finite -- aph_patchify_f16_win writes zeros -- and the last dgrad GEMM
 * (N = Kp) writes exact zeros into the pad columns of the gradient.
 * Supported: width in {256, 512, 768, 1024} with head dim 64; a power-of-two patch with 3*patch^2 % 128 == 0 (16, 32, 64) and T = P + 1 <= 256
 * tokens, as before; any patch <= 64 that is no power of two, T <= 320 (ViT-L/14: patch 14, 257 tokens).  The split-precision and exact paths
 * (aph_vit_enable_hilo / aph_vit_enable_f32) are refused (APH_ERR_UNSUPPORTED) for T > 256 or a patch that is no power of two.
 * d_patches f16 [S*P, Kp] (APH_OUT_PATCH_F16 layout) -> d_enc f32 [S, output_dim] */
int aph_vit_forward(aph_vit* vit, const void* d_patches, int S, float* d_enc, void* stream);
/* SPLIT-PRECISION forward (opt-in: clip_fft.py --precise, bench.py --split; the default is aph_vit_forward -- f16 operands everywhere, the
 * reference's own GPU dtype -- since round 6): d_patches_hilo f16 [S*P, 2 * 3*patch^2] (APH_OUT_PATCH_F16_HILO rows [hi | lo]).  The
 * patch-embedding GEMM and every block's QKV GEMM take their activation operand as a hi + lo pair of f16 values (~22 bits; the GEMMs run over
 * twice the K against the weights repeated along K): the two f16 roundings that dominate the input-gradient error on weights with realistic
 * dynamic range (profiles/r04_precision_attribution.txt; single-step input-gradient error 7.7e-4 against 1.10e-3).  At full batch the lo half
 * feeds the Q and K columns of the QKV GEMM only -- the V column tiles run over the hi half, in the same launch (DESIGN.md section 4
 * *Precision* [r5]).  Same outputs / saved activations as aph_vit_forward; the backward (aph_vit_backward) is unchanged.  Costs ~5 % of a C2
 * step; over the 30-member stress-weight loss-curve ensemble its free-running curves are not significantly closer to the fp32 CPU reference
 * than the default's (profiles/r06_precision_ensemble.txt), which is why it is no longer the default.  Needs aph_vit_enable_hilo once. */
int aph_vit_forward_hilo(aph_vit* vit, const void* d_patches_hilo, int S, float* d_enc, void* stream);
/* [r6] Allocates and fills the K-repeated copies of the patch-embedding / QKV weights aph_vit_forward_hilo needs (85 MB at ViT-B/32; a handle
 * does not carry them by default).  Once per handle, after aph_vit_set_weight of every tensor, outside any stream capture; idempotent. */
int aph_vit_enable_hilo(aph_vit* vit);
/* EXACT path (opt-in: clip_fft.py --exact).  Allocates a separate arena with fp32 copies of the weight matrices (and their transposes), the
 * fp32 activation stash and fp32 gradient buffers, filled from host fp32 copies aph_vit_set_weight keeps -- exact for any weights; a later
 * aph_vit_set_weight refreshes them.  Once per handle, after aph_vit_set_weight of every tensor, outside any stream capture; idempotent. */
int aph_vit_enable_f32(aph_vit* vit);
/* fp32 forward: every GEMM on the f32-input MFMA (a k-ordered fmaf chain), fp32 attention / LayerNorm / GELU.  d_patches f32 [S*P, 3*patch^2]
 * (APH_OUT_PATCH_F32) -> d_enc f32 [S, output_dim].  Refused (APH_ERR_ARG) before aph_vit_enable_f32. */
int aph_vit_forward_f32(aph_vit* vit, const float* d_patches, int S, float* d_enc, void* stream);
/* input-gradient of the last aph_vit_forward_f32 (refused after any other forward; aph_vit_backward is refused after this forward):
 * d_genc f32 [S, output_dim] -> d_patch_grad f32 [S*P, 3*patch^2] x out_scale; fp32 gradient stream end to end */
int aph_vit_backward_f32(aph_vit* vit, const float* d_genc, int S, float* d_patch_grad, float out_scale, void* stream);
/* d_genc f32 [S, output_dim] (times the caller's loss scale) -> d_patch_grad f32 [S*P, Kp] times out_scale (pad columns: exact zeros) */
int aph_vit_backward(aph_vit* vit, const float* d_genc, int S, float* d_patch_grad, float out_scale, void* stream);
/* same with the patch gradient stored as f16 [S*P, Kp] (keep the loss scale in it: out_scale = 1, and undo it in aph_sample_bwd's
 * gscale with out_mode APH_GRAD_PATCH_F16): halves the bytes the sampler adjoint gathers */
int aph_vit_backward_h(aph_vit* vit, const float* d_genc, int S, void* d_patch_grad_f16, float out_scale, void* stream);
/* (test / measurement hooks -- GEMM core alone, per-launch GEMM timing -- are declared in aphantasia_hip_test.h) */

/* ---- CLIP text tower: clip_fft.py:119 `model.encode_text(clip.tokenize(text))`, forward only (a prompt is a constant) ----
 * mirrors the text half of clip.model.CLIP: context_length tokens, vocab_size embeddings, `layers` residual blocks of `width` (causal
 * attention, head dim 64), ln_final and text_projection [width, output_dim].  fp32 throughout -- the kernels of the exact ViT path
 * (f32-input MFMA GEMM, fp32 LayerNorm, fp32 attention in its causal form): the result differs from an fp32 CPU evaluation in summation
 * order only, and a prompt's embedding does not depend on the other prompts of its batch.  One arena holds the fp32 weights [N, K] and
 * the activations of max_batch prompts; it is sized at create and aph_text_forward allocates nothing.
 * Refused: width != 64 * heads, width no multiple of 256 or above 1024, context_length > 256 (APH_ERR_UNSUPPORTED); S outside 1 .. max_batch,
 * a forward before every tensor is loaded, an unknown key or a wrong element count (APH_ERR_ARG). */
typedef struct aph_text aph_text;
int aph_text_create(int context_length, int vocab_size, int width, int layers, int heads, int output_dim, int max_batch, aph_text** out);
int aph_text_destroy(aph_text* text);
size_t aph_text_workspace_bytes(const aph_text* text);
/* one tensor by its OpenAI checkpoint key (fp32 HOST data, the checkpoint's layout): token_embedding.weight, positional_embedding,
 * ln_final.{weight,bias}, text_projection, transformer.resblocks.N.{ln_1,ln_2}.{weight,bias},
 * transformer.resblocks.N.attn.{in_proj_weight,in_proj_bias,out_proj.weight,out_proj.bias}, transformer.resblocks.N.mlp.{c_fc,c_proj}.{weight,bias} */
int aph_text_set_weight(aph_text* text, const char* name, const float* h_data, size_t count);
/* d_tokens int32 [S, context_length] (device; clip.tokenize rows: SOT, ids, EOT, zero padding) -> d_enc f32 [S, output_dim]: row s is
 * ln_final of the token row at the first position of the largest id of sequence s (upstream's text.argmax(dim=-1)) times text_projection.
 * Ids are clamped into [0, vocab_size) on the device, so no id reads out of bounds; callers should refuse them earlier. */
int aph_text_forward(aph_text* text, const int32_t* d_tokens, int S, float* d_enc, void* stream);

/* ---- LPIPS image term: clip_fft.py:219-222,268-270 (`--sync`), lpips.LPIPS(net='vgg') v0.1 with normalize=True --------------
 * value = LPIPS(resize(rgb), resize(target)): both images [3,H,W] in [0,1] go through a bicubic resize (align_corners=True) to
 * [H/2, W/2], the input scaling (2 t - 1, then (t - shift_c) / scale_c) and the VGG-16 feature stack (13 convolutions 3x3 + bias + ReLU,
 * 2x2 max-pool before stages 2 .. 5); the five stage outputs are unit-normalised over channels, and the value is
 * sum_l mean_hw sum_c lin_l[c] (n_l(x) - n_l(y))^2.  Convolutions on the f16 MFMA (f16 NHWC activations, fp32 accumulation), head and
 * resize in fp32, spatial sums through fp64 partials; deterministic.  The network is frozen: the only gradient is the image's.
 * widths[5]: channels of the five stages (VGG-16: 64, 128, 256, 512, 512), each a multiple of 16 up to 1024; H/2 and W/2 at least 16:
 * else APH_ERR_UNSUPPORTED.  One arena holds weights, activations and the backward stream; it is sized at create and no later call
 * allocates or waits for the device, so aph_lpips_value_grad can be captured into a graph. */
typedef struct aph_lpips aph_lpips;
int aph_lpips_create(const int* widths, int H, int W, aph_lpips** out);
int aph_lpips_destroy(aph_lpips* lp);
size_t aph_lpips_workspace_bytes(const aph_lpips* lp);
/* one tensor (fp32 HOST data): features.N.weight [cout][cin][3][3] / features.N.bias [cout] with torchvision's vgg16 numbering
 * (N = 0 2 5 7 10 12 14 17 19 21 24 26 28), linL.weight [C_L] for L = 0 .. 4.  Unknown key or wrong count: APH_ERR_ARG. */
int aph_lpips_set_weight(aph_lpips* lp, const char* name, const float* h_data, size_t count);
/* the constant image y: d_img f32 [3,h,w] (device), (h, w) = the full frame (resized here) or its half size (taken as is); computes and
 * stores the normalised taps of y.  After every weight is set; again after a weight changes. */
int aph_lpips_set_target(aph_lpips* lp, const float* d_img, int h, int w, void* stream);
/* *d_loss (nullable) += *d_weight * value and d_rgb_grad [3,H,W] (nullable) += *d_weight * dvalue/drgb, d_rgb f32 [3,H,W].
 * d_weight: ONE DEVICE float, read by the kernels at run time (a captured graph replays with whatever it holds then). */
int aph_lpips_value_grad(aph_lpips* lp, const float* d_rgb, const float* d_weight, float* d_loss, float* d_rgb_grad, void* stream);
/* the same on an image that already has the network's size: d_x, d_x_grad f32 [3,H/2,W/2] (what the reference's own call hands to
 * lpips: its resize is done by the caller) */
int aph_lpips_value_grad_half(aph_lpips* lp, const float* d_x, const float* d_weight, float* d_loss, float* d_x_grad, void* stream);

/* ---- depth estimator: depth/depth.py:20-32, Depth-Anything-V2 (DINOv2 S / B / L + DPT neck and head) behind `illustrip.py -d` ----------
 * Inference of transformers' DepthAnythingForDepthEstimation (relative depth): f16 MFMA GEMMs, attention and convolutions with fp32
 * accumulation, an fp32 residual stream.  d_img f32 [B,3,h,w] in (0,1) (the ImageNet normalisation is part of the first kernel), h and w
 * multiples of 14 up to max_h / max_w, B up to max_batch -> d_depth f32 [B,1,h,w]; normalise != 0: (d - min) / (max - min) per image, as
 * InferDepthAny.__call__ does.  hidden = 64 * heads, a multiple of 128 up to 1024; out_indices[4]: the tapped layers (1-based, non-decreasing);
 * neck_sizes[4] multiples of 16, fusion a multiple of 32, head_hidden a multiple of 16; swiglu != 0 (the giant encoder): APH_ERR_UNSUPPORTED.
 * One arena holds weights and the activations of max_batch images of max_h x max_w; aph_depth_forward allocates nothing.
 * aph_depth_set_weight: one tensor (fp32 HOST data) under its name in the Hugging Face state dict (backbone.embeddings.cls_token, ...
 * head.conv3.bias); position_embeddings and mask_token are not taken.  Unknown name or wrong count: APH_ERR_ARG.
 * aph_depth_set_pos_embed: the position rows [1 + gh gw][hidden] (fp32 HOST) for images of (14 gh) x (14 gw): row 0 the class position, the
 * rest the checkpoint's 37 x 37 grid interpolated the way transformers does (bicubic, align_corners = False) -- set-up, done by the caller
 * once per size (aphantasia_amd/depthnet.py).  aph_depth_forward refuses an image whose grid is not the one last set, names the first weight
 * that was never set, and refuses h / w that are no multiple of 14 or exceed max_h / max_w and B above max_batch (APH_ERR_ARG). */
typedef struct aph_depth aph_depth;
int aph_depth_create(int hidden, int layers, int heads, int swiglu, const int* out_indices, const int* neck_sizes, int fusion, int head_hidden, int max_h,
                     int max_w, int max_batch, aph_depth** out);
int aph_depth_destroy(aph_depth* dn);
size_t aph_depth_workspace_bytes(const aph_depth* dn);
int aph_depth_set_weight(aph_depth* dn, const char* name, const float* h_data, size_t count);
int aph_depth_set_pos_embed(aph_depth* dn, int gh, int gw, const float* h_rows, size_t count);
int aph_depth_forward(aph_depth* dn, const float* d_img, int B, int h, int w, int normalise, float* d_depth, void* stream);

/* ---- loss: aphantasia/utils.py:270-295 sim_func, assembled as at clip_fft.py:257-267 -------- */
#define APH_SIM_COS 0   /* type None / 'cossim' */
#define APH_SIM_MIX 1   /* 'mix' (default) */
#define APH_SIM_ANG 2   /* 'ang' */
#define APH_SIM_DOT 3   /* 'dot' */
/* loss = sum_t coef_t * sim_func(target_t, enc, type), value -> d_loss (1 float) and
 * gscale * dloss/denc -> d_genc [S,D].  d_targets = n_broadcast rows [D] (one embedding vs every cut: text
 * prompts) followed by T-n_broadcast blocks [s_total,D] of per-cut targets (reference-image term,
 * clip_fft.py:216,267; s_offset = first global cut of this rank's shard), d_coef [T] (sign*weight), h_coef = host copy
 * (needed for 'ang'), denom = sample count of the global mean (S, or the all-rank total),
 * d_ws = f32 scratch of S*(T+2) elements. */
int aph_sim_loss(const float* d_enc, int S, int D, const float* d_targets, const float* d_coef, const float* h_coef,
                 int T, int n_broadcast, int s_total, int s_offset, int type, float denom, float gscale, float* d_ws,
                 float* d_loss, float* d_genc, void* stream);

/* the aesthetic predictor term, clip_fft.py:255-256 / utils.py:402-413 (`loss -= 0.001 * a.aest * aest(out_enc).mean()`,
 * aest = nn.Linear(D, 1)): adds coef * mean_s(w . enc_s + bias) to *d_loss and its gradient (times gscale) into d_genc
 * (nullable), both ACCUMULATED on top of what aph_sim_loss wrote; denom as there.  d_w [D] device, bias a host scalar;
 * pass coef = -0.001 * aest. */
int aph_linear_head(const float* d_enc, int S, int D, const float* d_w, float bias, float coef, float denom, float gscale,
                    float* d_loss, float* d_genc, void* stream);

/* d_y[i] += alpha * d_x[i] -- partial results summed inside a step (--enforce, clip_fft.py:271-275: two cut sets contribute to
 * one image gradient and one loss) */
int aph_axpy_f32(float* d_y, const float* d_x, float alpha, size_t n, void* stream);
/* the per-step frame (clip_fft.py:297-306 / utils.py:94-100 checkout): d_rgb f32 [3,H,W] in [0,1] -> d_out_u8 uint8 [H,W,3] =
 * clip(rgb ** gamma * 255, 0, 255) truncated; one launch on `stream`, the caller copies it to the host asynchronously */
int aph_rgb_to_u8(const float* d_rgb, int H, int W, float gamma, void* d_out_u8, void* stream);

/* ---- optimiser: torch.optim.Adam / AdamW as configured at clip_fft.py:108-115 --------------- */
/* d_hyper: 8 device floats {lr, beta1, beta2, eps, weight_decay, 1-beta1^t, sqrt(1-beta2^t), grad_scale};
 * d_m may be NULL when beta1 == 0, d_vmax NULL unless amsgrad; decoupled_wd = AdamW */
int aph_adam_step(float* d_p, const float* d_g, float* d_m, float* d_v, float* d_vmax, const float* d_hyper,
                  int decoupled_wd, size_t n, void* stream);
/* the same update behind an overflow guard: a gradient with a NaN / inf element (fp16 overflow in the loss-scaled backward)
 * skips the step and increments d_guard[0] (running count); d_guard[1] is scratch.  d_guard: 2 ints zeroed once by the
 * caller, who lowers its loss scale when the count moves. */
int aph_adam_step_guarded(float* d_params, const float* d_grad, float* d_m, float* d_v, float* d_vmax, const float* d_hyper8,
                          int decoupled_wd, size_t n, int* d_guard2, void* stream);

/* ---- multi-GPU: the one collective of the step (the reference is single-GPU) ------------
 * Samples are split over the ranks of one node (one process per GPU); every rank forms its partial spectrum gradient
 * and ONE all-reduce (sum, f32) per step makes it the global gradient before the (replicated) Adam update.  RCCL is
 * called directly and bound at run time; torch.distributed is not on the data path.
 *   rank 0: aph_comm_unique_id(h_uid128) -> ship the 128 bytes to the other ranks (file, env, socket: the caller's choice);
 *   every rank, with its GPU current: aph_comm_init(rank, nranks, h_uid128, &comm);
 *   per step: aph_allreduce_f32(comm, d_buf, n, stream) -- in place, asynchronous on `stream`, capturable into a hipGraph. */
typedef struct aph_comm aph_comm;
int aph_comm_unique_id(void* h_uid128);
int aph_comm_init(int rank, int nranks, const void* h_uid128, aph_comm** out);
int aph_allreduce_f32(aph_comm* comm, float* d_buf, size_t n, void* stream);
/* the number of ranks the communicator itself reports (ncclCommCount) */
int aph_comm_ranks(aph_comm* comm, int* nranks);
int aph_comm_destroy(aph_comm* comm);

#ifdef __cplusplus
}
#endif
#endif
