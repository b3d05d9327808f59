// Sampler kernels (SURVEY.md K5-K10 and adjoints): random square crops of the rgb image,
// bicubic resize to size x size, optional torchvision-style geometric augmentation, CLIP
// normalisation, and layout conversion to the patch-embed GEMM operand.
//
// Replaces: aphantasia/utils.py:243-253 (the per-cut Python loop: slice + F.interpolate bicubic
// align_corners=True), utils.py:152-187 (pad_up_to / tile_pad wrap padding, folded in as modular
// addressing), transforms.py:102-109 (normalize), transforms.py:165-170 (transforms_fast:
// RandomPerspective -> RandomErasing -> rotate, torchvision grid_sample semantics).
//
// All random parameters are drawn on the host exactly as the reference draws them; kernels are
// RNG-free.  One launch covers all S cuts (the reference issues S x ~10 tiny launches).
//
// Adjoint of the crop/resize: deterministic GATHER over crops per image pixel (fixed summation
// order s = 0..S-1, no atomics) so a given crop table gives bitwise-reproducible gradients.
// Adjoint of the bilinear warps: gathers through the inverse maps (deterministic as well).
// The kernels live in the sampler_*.h headers, one per stage; here: checks, workspace layout, patchify kernels, the C ABI.
#include <cstring>
#include <cstdlib>
#include <type_traits>

#include "sampler_layout.h"
#include "sampler_crop.h"
#include "sampler_crop_adjoint.h"
#include "sampler_warp.h"
#include "sampler_kornia.h"

namespace aph {

// ---------------------------------------------------------------------------------
// layout conversion for caller-made batches (model.encode_image(x) on an NCHW tensor)
// ---------------------------------------------------------------------------------
struct Nchw { int s, c, i, j; };
__device__ __forceinline__ Nchw nchw_of(size_t idx, int R) {      // element idx of a contiguous [S][3][R][R] tensor
  return Nchw{(int)(idx / ((size_t)3 * R * R)), (int)((idx / ((size_t)R * R)) % 3), (int)((idx / R) % R), (int)(idx % R)};
}

__global__ void patchify_kernel(const float* __restrict__ x, half_t* __restrict__ out, int S, int R, int p, int hilo) {
  const size_t n = (size_t)S * 3 * R * R;
  const Layout<APH_OUT_PATCH_F16> L(R, p);
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) {
    const Nchw e = nchw_of(idx, R);
    const size_t o = L.index(e.s, e.c, e.i, e.j);
    const half_t h = (half_t)x[idx];
    if (!hilo) { out[o] = h; continue; }
    const size_t q = L.hilo_index(o);                         // rows [hi | lo]
    out[q] = h;
    out[q + L.patch_elems()] = (half_t)(x[idx] - (float)h);
  }
}
__global__ void patchify_f32_kernel(const float* __restrict__ x, float* __restrict__ out, int S, int R, int p) {
  const size_t n = (size_t)S * 3 * R * R;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) {
    const Nchw e = nchw_of(idx, R);
    out[patch_index(e.s, e.c, e.i, e.j, R, p)] = x[idx];
  }
}
__global__ void unpatchify_kernel(const float* __restrict__ g, float* __restrict__ out, int S, int R, int p, float gscale) {
  const size_t n = (size_t)S * 3 * R * R;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) {
    const Nchw e = nchw_of(idx, R);
    out[idx] = g[patch_index(e.s, e.c, e.i, e.j, R, p)] * gscale;
  }
}


// Any patch side, with a window (aph_patchify_f16_win / aph_unpatchify_f32_win): the patch-major rows are `kp` >= 3 p^2 elements long, the
// pad columns written as zero; divisions instead of Layout's shifts -- one pass over 0.6 MB per cut next to a ViT step.
__global__ void patchify_win_kernel(const float* __restrict__ x, half_t* __restrict__ out, int S, int Rs, int R, int p, int kp) {
  const int gp = R / p, k3 = 3 * p * p;
  const size_t n = (size_t)S * gp * gp * kp;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t row = idx / kp;
    const int k = (int)(idx - row * kp);
    float v = 0.f;
    if (k < k3) {
      const int s = (int)(row / ((size_t)gp * gp)), pr = (int)(row - (size_t)s * gp * gp), py = pr / gp, px = pr - py * gp;
      const int pix = k / 3, c = k - pix * 3, iy = pix / p, ix = pix - iy * p;
      v = x[(((size_t)s * 3 + c) * Rs + (py * p + iy)) * Rs + (px * p + ix)];
    }
    out[idx] = (half_t)v;
  }
}
__global__ void unpatchify_win_kernel(const float* __restrict__ g, float* __restrict__ out, int S, int Rs, int R, int p, int kp, float gscale) {
  const int gp = R / p;
  const size_t n = (size_t)S * 3 * Rs * Rs;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) {
    const Nchw e = nchw_of(idx, Rs);
    float v = 0.f;
    if (e.i < R && e.j < R) {
      const int py = e.i / p, px = e.j / p, iy = e.i - py * p, ix = e.j - px * p;
      v = g[(((size_t)e.s * gp + py) * gp + px) * kp + (iy * p + ix) * 3 + e.c] * gscale;
    }
    out[idx] = v;
  }
}

}  // namespace aph

using namespace aph;

static Geom to_geom(const aph_sample_geom* g) { return Geom{g->H, g->W, g->Hp, g->Wp, g->py0, g->px0, g->S, g->size, g->patch}; }

static int check_geom(const aph_sample_geom* g, int out_mode, const char* who, int max_mode = 2) {
  if (!g) return aph_fail(APH_ERR_ARG, "%s: null geometry", who);
  if (out_mode == APH_OUT_PATCH_F16_HILO && max_mode == 2) max_mode = APH_OUT_PATCH_F16_HILO;      // forward only: the split-precision patch rows
  if (out_mode == APH_OUT_PATCH_F32) max_mode = APH_OUT_PATCH_F32;            // both ways: the exact path's fp32 patch rows / their gradient
  if (g->S < 1 || g->size < 1 || g->H < 1 || g->W < 1 || g->Hp < g->H || g->Wp < g->W)
    return aph_fail(APH_ERR_ARG, "%s: bad geometry S=%d size=%d H=%d W=%d Hp=%d Wp=%d", who, g->S, g->size, g->H, g->W, g->Hp, g->Wp);
  if (out_mode < 0 || out_mode > max_mode || (out_mode == APH_GRAD_PATCH_F16 && max_mode != APH_GRAD_PATCH_F16))
    return aph_fail(APH_ERR_ARG, "%s: bad out_mode %d", who, out_mode);
  if (out_mode >= APH_OUT_PATCH_F16 && (g->patch < 1 || g->size % g->patch || (g->patch & (g->patch - 1))))
    return aph_fail(APH_ERR_ARG, "%s: size %d not divisible by patch %d, or patch not a power of two", who, g->size, g->patch);
  return APH_OK;
}

namespace {
// run-time out_mode -> template argument: f(std::integral_constant<int, OUT>{}) for the one of MODES (the caller's legal set) that
// out_mode names; false if it names none
template <int... MODES> struct Modes {};
template <int... MODES, class F>
bool dispatch_out(Modes<MODES...>, int out_mode, F&& f) {
  return ((out_mode == MODES ? (f(std::integral_constant<int, MODES>{}), true) : false) || ...);
}
using FwdModes = Modes<APH_OUT_NCHW_RAW, APH_OUT_NCHW_NORM, APH_OUT_PATCH_F16, APH_OUT_PATCH_F32, APH_OUT_PATCH_F16_HILO>;
using GradModes = Modes<APH_OUT_NCHW_RAW, APH_OUT_NCHW_NORM, APH_OUT_PATCH_F16, APH_GRAD_PATCH_F16>;      // (APH_OUT_PATCH_F32 arrives as APH_OUT_PATCH_F16)

// Workspace of one sampler call (caller-owned, aph_sample_ws_bytes): [per-cut 1-D tap tables of the crop adjoint |
// per-XCD strip lists of the forward | cut scratch A | cut scratch B], the scratch planes only with geometric augmentation.
// Nothing is allocated or freed in a launch path, so a captured hipGraph never holds a pointer the library could invalidate.
size_t tab_bytes(const Geom& g) {
  const size_t maxcs = (size_t)(g.Hp < g.Wp ? g.Hp : g.Wp);    // a cut fits the (padded) image; csize <= min(H, W) upstream (utils.py:231,245)
  return ((size_t)g.S * 2 * maxcs * sizeof(AdjEntry) + 255) & ~(size_t)255;
}
size_t scratch_floats(const Geom& g) { return (size_t)g.S * 4 * g.size * g.size; }     // HWC4 in the forward; the adjoint uses 3/4 of it, planar
size_t strip_bytes(const Geom& g) { return ((size_t)(8 * (size_t)strip_cap(g) + 8) * sizeof(int) + 255) & ~(size_t)255; }
int* ws_strips(void* ws, const Geom& g) { return reinterpret_cast<int*>(static_cast<char*>(ws) + tab_bytes(g)); }
float* ws_scratch(void* ws, const Geom& g) { return reinterpret_cast<float*>(static_cast<char*>(ws) + tab_bytes(g) + strip_bytes(g)); }
// the kornia-style chains: scratch A as above (custom needs no more), then for elastic the P x P canvas B, P = size + 8 (the adjoint's planar gradient of the rotated canvas)
size_t canvas_floats(const Geom& g) { const size_t P = (size_t)g.size + 2 * kTfPad; return (size_t)g.S * 4 * P * P; }

// arguments of aph_sample_fwd_tf / aph_sample_bwd_tf beyond check_geom, for the two kornia-style chains
int check_tf(const aph_sample_geom* g, int tf, int out_mode, const float* aug, const float* h_aug, const char* who) {
  if (tf != APH_TF_CUSTOM && tf != APH_TF_ELASTIC) return aph_fail(APH_ERR_ARG, "%s: bad chain kind %d (APH_TF_FAST / _CUSTOM / _ELASTIC)", who, tf);
  if (!aug) return aph_fail(APH_ERR_ARG, "%s: null augment table (the custom / elastic chains draw a rotation and a jitter per cut)", who);
  if (out_mode >= APH_OUT_PATCH_F16 && g->patch <= 2 * kTfPad)
    return aph_fail(APH_ERR_ARG, "%s: patch %d <= 8: the %d x %d canvas holds more than %d patches a side, which the positional embedding of a %d-pixel tower does not cover",
                    who, g->patch, g->size + 2 * kTfPad, g->size + 2 * kTfPad, g->size / g->patch, g->size);
  for (int s = 0; h_aug && s < g->S; ++s) {
    const float dx = h_aug[(size_t)s * APH_AUG_STRIDE], dy = h_aug[(size_t)s * APH_AUG_STRIDE + 1];
    if (!(dx >= 0.f && dx < (float)kTfJitter && dy >= 0.f && dy < (float)kTfJitter && dx == (float)(int)dx && dy == (float)(int)dy))
      return aph_fail(APH_ERR_ARG, "%s: cut %d: jitter (dx, dy) = (%g, %g) outside 0 .. %d", who, s, dx, dy, kTfJitter - 1);
  }
  return APH_OK;
}
}  // namespace

extern "C" {

// test / measurement hook: launch shape of the separable crop adjoint (rows per workgroup, columns per thread, cuts per batch, column
// segments, row-block order 0 = top-down / 1 = centre-out); 0 (order: -1) = automatic.  The kernel is instantiated for 12 or 16 accumulator rows x 2 or 3 columns per thread.
int aph_crop_adjoint_set_shape(int rb, int cpt, int nbc, int nseg, int order) {
  CropAdjointShape& v = crop_adjoint_shape();
  v.rb = rb; v.cpt = cpt; v.nbc = nbc; v.nseg = nseg; v.order = order;
  return APH_OK;
}
// test / measurement hook: 1 = the crop adjoint always runs the gather kernel, 0 = automatic.  Returns the previous value.
int aph_crop_adjoint_set_gather(int on) {
  const int prev = crop_adjoint_gather();
  crop_adjoint_gather() = on ? 1 : 0;
  return prev;
}

size_t aph_sample_ws_bytes(const aph_sample_geom* gg, int with_aug) {
  if (!gg || gg->S < 1 || gg->size < 1 || gg->Hp < 1 || gg->Wp < 1) return 0;
  const Geom g = to_geom(gg);
  return tab_bytes(g) + strip_bytes(g) + (with_aug ? 2 * scratch_floats(g) * sizeof(float) : 0);
}

int aph_sample_fwd(const aph_sample_geom* gg, const float* rgb, const int32_t* table_, const float* aug, void* ws,
                   void* out, int out_mode, void* stream_) {
  APH_TRY
  if (int e = check_geom(gg, out_mode, "aph_sample_fwd")) return e;
  if (!rgb || !table_ || !out || !ws) return aph_fail(APH_ERR_ARG, "aph_sample_fwd: null argument (the workspace of aph_sample_ws_bytes is required)");
  hipStream_t st = (hipStream_t)stream_;
  const Geom g = to_geom(gg);
  const int n = g.size;
  const int* table = (const int*)table_;
  int* strips = ws_strips(ws, g);
  if (!aug) {
    if (!dispatch_out(FwdModes{}, out_mode, [&](auto m) { launch_crop_resize<decltype(m)::value>(rgb, table, out, g, strips, st); })) return aph_fail(APH_ERR_ARG, "aph_sample_fwd: no kernel for out_mode %d", out_mode);
    return aph_check_launch("aph_sample_fwd");
  }
  float* A = ws_scratch(ws, g);
  float* Bv = A + scratch_floats(g);
  const dim3 grid((n + 31) / 32, (n + 7) / 8, g.S), block(256);       // thread = (column, row) of a cut: 32 x 8 pixels per workgroup (warp_block_note)
  // resized cut -> A; RandomPerspective for the cuts that drew it A -> B; RandomErasing + rotation + normalise (A or B) -> out
  launch_crop_resize<APH_SCRATCH_HWC4>(rgb, table, (void*)A, g, strips, st);
  APH_LAUNCH(persp_kernel, grid, block, 0, st, (const float*)A, aug, Bv, n);
  if (!dispatch_out(FwdModes{}, out_mode, [&](auto m) { APH_LAUNCH(rotate_emit_kernel<decltype(m)::value>, grid, block, 0, st, (const float*)A, (const float*)Bv, aug, out, n, g.patch); })) return aph_fail(APH_ERR_ARG, "aph_sample_fwd: no kernel for out_mode %d", out_mode);
  return aph_check_launch("aph_sample_fwd");
  APH_CATCH
}

int aph_sample_bwd(const aph_sample_geom* gg, const void* gout, float gscale, const int32_t* table_, const float* aug,
                   void* ws, float* grgb, int out_mode, void* stream_) {
  APH_TRY
  if (int e = check_geom(gg, out_mode, "aph_sample_bwd", APH_GRAD_PATCH_F16)) return e;
  if (out_mode == APH_OUT_PATCH_F32) out_mode = APH_OUT_PATCH_F16;      // the same gradient layout: f32 patch-major
  if (!gout || !table_ || !grgb || !ws) return aph_fail(APH_ERR_ARG, "aph_sample_bwd: null argument (the workspace of aph_sample_ws_bytes is required)");
  hipStream_t st = (hipStream_t)stream_;
  const Geom g = to_geom(gg);
  const int n = g.size;
  const int* table = (const int*)table_;
  AdjEntry* tab = static_cast<AdjEntry*>(ws);
  int rc = APH_OK;
  if (!aug) {
    if (!dispatch_out(GradModes{}, out_mode, [&](auto m) { rc = launch_crop_adjoint<decltype(m)::value>(gout, gscale, table, grgb, g, tab, st); })) return aph_fail(APH_ERR_ARG, "aph_sample_bwd: no kernel for out_mode %d", out_mode);
    return rc ? rc : aph_check_launch("aph_sample_bwd");
  }
  float* dA = ws_scratch(ws, g);
  float* dB = dA + scratch_floats(g);
  const dim3 grid((n + 31) / 32, (n + 7) / 8, g.S), block(256);
  if (!dispatch_out(GradModes{}, out_mode, [&](auto m) { APH_LAUNCH(rotate_emit_adjoint_kernel<decltype(m)::value>, grid, block, 0, st, gout, aug, dA, dB, n, g.patch); })) return aph_fail(APH_ERR_ARG, "aph_sample_bwd: no kernel for out_mode %d", out_mode);
  APH_LAUNCH(persp_adjoint_kernel, grid, block, 0, st, (const float*)dB, aug, dA, n);
  rc = launch_crop_adjoint<APH_OUT_NCHW_RAW>((const void*)dA, gscale, table, grgb, g, tab, st);
  return rc ? rc : aph_check_launch("aph_sample_bwd");
  APH_CATCH
}

size_t aph_sample_ws_bytes_tf(const aph_sample_geom* gg, int tf) {
  if (tf == APH_TF_FAST) return aph_sample_ws_bytes(gg, 1);
  if (!gg || gg->S < 1 || gg->size < 1 || gg->Hp < 1 || gg->Wp < 1 || (tf != APH_TF_CUSTOM && tf != APH_TF_ELASTIC)) return 0;
  const Geom g = to_geom(gg);
  return tab_bytes(g) + strip_bytes(g) + (scratch_floats(g) + (tf == APH_TF_ELASTIC ? canvas_floats(g) : 0)) * sizeof(float);
}

int aph_sample_fwd_tf(const aph_sample_geom* gg, int tf, const float* rgb, const int32_t* table_, const float* aug, const float* h_aug,
                      void* ws, void* out, int out_mode, void* stream_) {
  if (tf == APH_TF_FAST) return aph_sample_fwd(gg, rgb, table_, aug, ws, out, out_mode, stream_);
  APH_TRY
  if (int e = check_geom(gg, out_mode, "aph_sample_fwd_tf")) return e;
  if (int e = check_tf(gg, tf, out_mode, aug, h_aug, "aph_sample_fwd_tf")) return e;
  if (!rgb || !table_ || !out || !ws) return aph_fail(APH_ERR_ARG, "aph_sample_fwd_tf: null argument (the workspace of aph_sample_ws_bytes_tf is required)");
  hipStream_t st = (hipStream_t)stream_;
  const Geom g = to_geom(gg);
  const int n = g.size, P = n + 2 * kTfPad, side = out_mode >= APH_OUT_PATCH_F16 ? n : P;      // patch-major: the top-left window
  float* A = ws_scratch(ws, g);
  const dim3 grid((side + 31) / 32, (side + 7) / 8, g.S), block(256);
  launch_crop_resize<APH_SCRATCH_HWC4>(rgb, (const int*)table_, (void*)A, g, ws_strips(ws, g), st);
  bool ok;
  if (tf == APH_TF_CUSTOM) {
    ok = dispatch_out(FwdModes{}, out_mode, [&](auto m) { APH_LAUNCH(custom_emit_kernel<decltype(m)::value>, grid, block, 0, st, (const float*)A, aug, out, n, g.patch); });
  } else {
    ok = dispatch_out(FwdModes{}, out_mode, [&](auto m) { APH_LAUNCH(elastic_emit_kernel<decltype(m)::value>, grid, block, 0, st, (const float*)A, aug, out, n, g.patch); });
  }
  if (!ok) return aph_fail(APH_ERR_ARG, "aph_sample_fwd_tf: no kernel for out_mode %d", out_mode);
  return aph_check_launch("aph_sample_fwd_tf");
  APH_CATCH
}

int aph_sample_bwd_tf(const aph_sample_geom* gg, int tf, const void* gout, float gscale, const int32_t* table_, const float* aug,
                      const float* h_aug, void* ws, float* grgb, int out_mode, void* stream_) {
  if (tf == APH_TF_FAST) return aph_sample_bwd(gg, gout, gscale, table_, aug, ws, grgb, out_mode, stream_);
  APH_TRY
  if (int e = check_geom(gg, out_mode, "aph_sample_bwd_tf", APH_GRAD_PATCH_F16)) return e;
  if (int e = check_tf(gg, tf, out_mode, aug, h_aug, "aph_sample_bwd_tf")) return e;
  if (out_mode == APH_OUT_PATCH_F32) out_mode = APH_OUT_PATCH_F16;      // the same gradient layout: f32 patch-major
  if (!gout || !table_ || !grgb || !ws) return aph_fail(APH_ERR_ARG, "aph_sample_bwd_tf: null argument (the workspace of aph_sample_ws_bytes_tf is required)");
  hipStream_t st = (hipStream_t)stream_;
  const Geom g = to_geom(gg);
  const int n = g.size, P = n + 2 * kTfPad;
  float* dA = ws_scratch(ws, g);
  float* dB = dA + scratch_floats(g);
  const dim3 grid((n + 31) / 32, (n + 7) / 8, g.S), canvas((P + 31) / 32, (P + 7) / 8, g.S), block(256);
  bool ok;
  if (tf == APH_TF_CUSTOM) {
    ok = dispatch_out(GradModes{}, out_mode, [&](auto m) { APH_LAUNCH(custom_adjoint_kernel<decltype(m)::value>, grid, block, 0, st, gout, aug, dA, n, g.patch); });
  } else {
    ok = dispatch_out(GradModes{}, out_mode, [&](auto m) { APH_LAUNCH(resample_adjoint_kernel<decltype(m)::value>, canvas, block, 0, st, gout, aug, dB, n, g.patch); });
    if (ok) APH_LAUNCH(rotate_canvas_adjoint_kernel, grid, block, 0, st, (const float*)dB, aug, dA, n);
  }
  if (!ok) return aph_fail(APH_ERR_ARG, "aph_sample_bwd_tf: no kernel for out_mode %d", out_mode);
  const int rc = launch_crop_adjoint<APH_OUT_NCHW_RAW>((const void*)dA, gscale, (const int*)table_, grgb, g, static_cast<AdjEntry*>(ws), st);
  return rc ? rc : aph_check_launch("aph_sample_bwd_tf");
  APH_CATCH
}

int aph_patchify_f16(const float* x, int S, int R, int patch, void* out, void* stream_) {
  APH_TRY
  if (!x || !out || S < 1 || R < 1 || patch < 1 || R % patch) return aph_fail(APH_ERR_ARG, "aph_patchify_f16: bad argument");
  APH_LAUNCH(patchify_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream_, x, (half_t*)out, S, R, patch, 0);
  return aph_check_launch("aph_patchify_f16");
  APH_CATCH
}

// the same into the split-precision rows [hi | lo] of aph_vit_forward_hilo: out f16 [S*(R/patch)^2, 2 * 3*patch*patch]
int aph_patchify_f16_hilo(const float* x, int S, int R, int patch, void* out, void* stream_) {
  APH_TRY
  if (!x || !out || S < 1 || R < 1 || patch < 1 || R % patch) return aph_fail(APH_ERR_ARG, "aph_patchify_f16_hilo: bad argument");
  APH_LAUNCH(patchify_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream_, x, (half_t*)out, S, R, patch, 1);
  return aph_check_launch("aph_patchify_f16_hilo");
  APH_CATCH
}

// the exact path's operand: out f32 [S*(R/patch)^2, 3*patch*patch] (APH_OUT_PATCH_F32 layout), values unchanged
int aph_patchify_f32(const float* x, int S, int R, int patch, float* out, void* stream_) {
  APH_TRY
  if (!x || !out || S < 1 || R < 1 || patch < 1 || R % patch) return aph_fail(APH_ERR_ARG, "aph_patchify_f32: bad argument");
  APH_LAUNCH(patchify_f32_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream_, x, out, S, R, patch);
  return aph_check_launch("aph_patchify_f32");
  APH_CATCH
}

int aph_unpatchify_f32(const float* g, int S, int R, int patch, float gscale, float* out, void* stream_) {
  APH_TRY
  if (!g || !out || S < 1 || R < 1 || patch < 1 || R % patch) return aph_fail(APH_ERR_ARG, "aph_unpatchify_f32: bad argument");
  APH_LAUNCH(unpatchify_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream_, g, out, S, R, patch, gscale);
  return aph_check_launch("aph_unpatchify_f32");
  APH_CATCH
}

int aph_patch_row_elems(int patch) { return patch < 1 || patch > 1024 ? 0 : (3 * patch * patch + 127) / 128 * 128; }

int aph_patchify_f16_win(const float* x, int S, int R_src, int R, int patch, void* out, void* stream_) {
  APH_TRY
  if (!x || !out || S < 1 || R < 1 || R_src < R || patch < 1 || patch > 1024 || R % patch)
    return aph_fail(APH_ERR_ARG, "aph_patchify_f16_win: bad argument (S=%d R_src=%d R=%d patch=%d)", S, R_src, R, patch);
  APH_LAUNCH(patchify_win_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream_, x, (half_t*)out, S, R_src, R, patch, aph_patch_row_elems(patch));
  return aph_check_launch("aph_patchify_f16_win");
  APH_CATCH
}

int aph_unpatchify_f32_win(const float* g, int S, int R_src, int R, int patch, float gscale, float* out, void* stream_) {
  APH_TRY
  if (!g || !out || S < 1 || R < 1 || R_src < R || patch < 1 || patch > 1024 || R % patch)
    return aph_fail(APH_ERR_ARG, "aph_unpatchify_f32_win: bad argument (S=%d R_src=%d R=%d patch=%d)", S, R_src, R, patch);
  APH_LAUNCH(unpatchify_win_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream_, g, out, S, R_src, R, patch, aph_patch_row_elems(patch), gscale);
  return aph_check_launch("aph_unpatchify_f32_win");
  APH_CATCH
}

// illustrip.py:130-138 frame_transform: d_dst [C,H,W] = affine warp of d_src [C,H,W] (d_dst != d_src).
// inv_matrix6: row-major 2x3 inverse affine matrix as torchvision's _get_inverse_affine_matrix returns it.
int aph_frame_affine(const float* d_src, int C, int H, int W, const float* inv_matrix6, float* d_dst, void* stream_) {
  APH_TRY
  if (!d_src || !d_dst || !inv_matrix6 || d_src == d_dst || C < 1 || H < 1 || W < 1) return aph_fail(APH_ERR_ARG, "aph_frame_affine: bad argument");
  Affine6 a;
  for (int i = 0; i < 6; ++i) a.m[i] = inv_matrix6[i];
  APH_LAUNCH(frame_affine_kernel, dim3((W + 255) / 256, H), dim3(256), 0, (hipStream_t)stream_, d_src, d_dst, C, H, W, a);
  return aph_check_launch("aph_frame_affine");
  APH_CATCH
}

}  // extern "C"
