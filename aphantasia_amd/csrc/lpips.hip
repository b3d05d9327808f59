// The LPIPS (VGG-16) image term of clip_fft.py --sync (reference clip_fft.py:219-222, 268-270): lpips.LPIPS(net='vgg') v0.1 with
// normalize=True between the half-size bicubic resize of the step's image and of the -i image, value and gradient with respect to the image.
//   forward   prep (resize + input scaling -> f16 NHWC) . 13 x conv3x3 + bias + ReLU (lpips_conv.h) with a 2x2 max-pool before stages 2 .. 5;
//             every layer's output stays stored (f16): the taps read them, the backward takes its ReLU masks and pool argmaxes from them
//   head      per tap, fp32: unit-normalise over channels, difference against the stored normalised taps of the target, lin weights, spatial mean
//             through fp64 partials (lpips_ops.h); value = the sum over the five taps
//   backward  per stage from the last: head gradient (fp32) + the pooled gradient from above -> merged, masked, f16; then the same conv kernel over
//             the flipped, transposed weights down the stage.  The network is frozen: no weight gradient exists.
//   gradient stream  f16 carrying gradient x a power of two (`gscale` = 16 x the half-size pixel count rounded up, fixed at create): the unweighted head
//             gradient is of order lin / (H W) and would sit under the f16 normal range.  The step's weight w is NOT in the stream: the last
//             kernel (adjoint of the input scaling and of the resize, fp32) multiplies by w / gscale, so the relative accuracy of the gradient
//             does not depend on w, and w = 0 adds exact zeros.
// Every launch is on the caller's stream; nothing is allocated and the host never waits after create / set_weight.
#include <algorithm>
#include <cmath>
#include <string>

#include "aph_device.h"
#include "aph_host.h"
#include "tower_store.h"
#include "lpips_conv.h"
#include "lpips_ops.h"

using namespace aph;
using namespace aph::lpips;

namespace {
constexpr int kConvsOfStage[5] = {2, 2, 3, 3, 3};
constexpr int kFeatureIdx[13] = {0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28};      // torchvision vgg16.features numbering

struct ConvLayer {
  int cin, cout, stage;
  half_t *wf = nullptr, *wd = nullptr;      // packed forward [9][cout][cin8] and dgrad [9][cin16][cout] copies
  float* bias = nullptr;
  half_t* act = nullptr;                    // stored output [Hs][Ws][cout]
  bool w_set = false, b_set = false;
};
}  // namespace

struct aph_lpips {
  int H, W;                 // full frame
  int hs[5], ws[5], C[5];   // stage sizes (hs[0] x ws[0] = the half-size frame) and widths
  int first[5], last[5];    // conv indices of each stage
  ConvLayer conv[13];
  float* lin[5] = {};
  bool lin_set[5] = {};
  half_t* x0 = nullptr;     // network input [hs0][ws0][8]
  half_t* pooled[4] = {};   // input of stages 2 .. 5
  float* ny[5] = {};        // normalised taps of the target
  float* hg = nullptr;      // head gradient of the tap in hand
  half_t* g[2] = {};        // backward stream, ping-pong
  float* g32 = nullptr;     // [3][hs0][ws0]: gradient at the network input
  double* partial = nullptr;
  float* value = nullptr;
  float gscale = 1.f;
  bool target_set = false;
  char* arena = nullptr;
  size_t arena_bytes = 0;
};

namespace {

size_t lpips_carve(aph_lpips* v, char* base) {
  Carver c{base};
  size_t gmax = 0, hmax = 0;
  v->x0 = c.take<half_t>((size_t)v->hs[0] * v->ws[0] * 8);
  for (int k = 0; k < 13; ++k) {
    ConvLayer& l = v->conv[k];
    const size_t P = (size_t)v->hs[l.stage] * v->ws[l.stage];
    l.wf = c.take<half_t>((size_t)9 * l.cout * round_up(l.cin, 8));
    l.wd = c.take<half_t>((size_t)9 * round_up(l.cin, 16) * l.cout);
    l.bias = c.take<float>(l.cout);
    l.act = c.take<half_t>(P * l.cout);
    gmax = std::max(gmax, P * (size_t)std::max(l.cout, round_up(l.cin, 16)));
  }
  for (int s = 0; s < 5; ++s) {
    const size_t P = (size_t)v->hs[s] * v->ws[s];
    v->lin[s] = c.take<float>(v->C[s]);
    v->ny[s] = c.take<float>(P * v->C[s]);
    hmax = std::max(hmax, P * v->C[s]);
    if (s) v->pooled[s - 1] = c.take<half_t>(P * v->C[s - 1]);
  }
  v->hg = c.take<float>(hmax);
  v->g[0] = c.take<half_t>(gmax); v->g[1] = c.take<half_t>(gmax);
  v->g32 = c.take<float>((size_t)3 * v->hs[0] * v->ws[0]);
  v->partial = c.take<double>(5 * kHeadBlocks);
  v->value = c.take<float>(64);
  return c.off;
}

int lpips_ready(const aph_lpips* v, const char* who) {
  int n = 0;
  for (int k = 0; k < 13; ++k) n += v->conv[k].w_set + v->conv[k].b_set;
  for (int s = 0; s < 5; ++s) n += v->lin_set[s];
  if (n != 31) return aph_fail(APH_ERR_ARG, "%s: weights not fully loaded (%d of 31 tensors)", who, n);
  return APH_OK;
}

// the image (d_img [3][ih][iw], the full frame or already half size) through the stack; every activation is left stored
void lpips_forward(aph_lpips* v, const float* d_img, int ih, int iw, hipStream_t st) {
  launch_prep(d_img, ih, iw, v->x0, v->hs[0], v->ws[0], st);
  const half_t* in = v->x0;
  int cin_stored = 8;
  for (int s = 0; s < 5; ++s) {
    if (s) {
      launch_pool_fwd(v->conv[v->last[s - 1]].act, v->hs[s - 1], v->ws[s - 1], v->C[s - 1], v->pooled[s - 1], st);
      in = v->pooled[s - 1];
    }
    for (int k = v->first[s]; k <= v->last[s]; ++k) {
      ConvLayer& l = v->conv[k];
      launch_conv(ConvArgs{in, v->hs[s], v->ws[s], cin_stored, l.wf, l.cout, l.bias, 1, nullptr, l.act, nullptr, 0}, st);
      in = l.act;
      cin_stored = l.cout;
    }
  }
}

}  // namespace

extern "C" {

int aph_lpips_create(const int* widths, int H, int W, aph_lpips** out) {
  APH_TRY
  if (!out || !widths) return aph_fail(APH_ERR_ARG, "aph_lpips_create: null argument");
  if (H < 1 || W < 1 || H > 16384 || W > 16384) return aph_fail(APH_ERR_ARG, "aph_lpips_create: frame %d x %d outside 1 .. 16384", H, W);
  for (int s = 0; s < 5; ++s)
    if (widths[s] < 16 || widths[s] % 16 || widths[s] > 1024)
      return aph_fail(APH_ERR_UNSUPPORTED, "aph_lpips_create: width %d of stage %d unsupported (a multiple of 16 up to 1024)", widths[s], s + 1);
  if (H / 2 < 16 || W / 2 < 16)
    return aph_fail(APH_ERR_UNSUPPORTED, "aph_lpips_create: half-size frame %d x %d unsupported (each side at least 16, so that the last stage is not empty)", H / 2, W / 2);
  auto* v = new aph_lpips();
  v->H = H; v->W = W;
  int k = 0;
  for (int s = 0; s < 5; ++s) {
    v->hs[s] = s ? v->hs[s - 1] / 2 : H / 2;
    v->ws[s] = s ? v->ws[s - 1] / 2 : W / 2;
    v->C[s] = widths[s];
    v->first[s] = k;
    for (int j = 0; j < kConvsOfStage[s]; ++j, ++k) {
      v->conv[k].cin = j ? widths[s] : (s ? widths[s - 1] : 3);
      v->conv[k].cout = widths[s];
      v->conv[k].stage = s;
    }
    v->last[s] = k - 1;
  }
  int e = 0;
  while ((1 << e) < v->hs[0] * v->ws[0]) ++e;
  v->gscale = ldexpf(1.f, e + 4);
  if (const int rc = alloc_arena("aph_lpips_create", &v->arena, &v->arena_bytes, [&](char* base) { return lpips_carve(v, base); })) { delete v; return rc; }
  *out = v;
  return APH_OK;
  APH_CATCH
}

int aph_lpips_destroy(aph_lpips* v) {
  if (!v) return APH_OK;
  (void)hipFree(v->arena);
  delete v;
  return APH_OK;
}

size_t aph_lpips_workspace_bytes(const aph_lpips* v) { return v ? v->arena_bytes : 0; }

int aph_lpips_set_weight(aph_lpips* v, const char* name, const float* data, size_t count) {
  APH_TRY
  if (!v || !name || !data) return aph_fail(APH_ERR_ARG, "aph_lpips_set_weight: null argument");
  const std::string key(name);
  for (int k = 0; k < 13; ++k) {
    ConvLayer& l = v->conv[k];
    const std::string p = "features." + std::to_string(kFeatureIdx[k]);
    if (key == p + ".weight") {
      const size_t want = (size_t)l.cout * l.cin * 9;
      if (count != want) return aph_fail(APH_ERR_ARG, "aph_lpips_set_weight(%s): %zu elements, expected %zu", name, count, want);
      const std::vector<half_t> f = pack_weights(data, l.cout, l.cin, 0), d = pack_weights(data, l.cout, l.cin, 1);
      if (hipMemcpy(l.wf, f.data(), f.size() * sizeof(half_t), hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy(l.wd, d.data(), d.size() * sizeof(half_t), hipMemcpyHostToDevice) != hipSuccess)
        return aph_fail(APH_ERR_HIP, "aph_lpips_set_weight(%s): upload failed", name);
      l.w_set = true;
      return APH_OK;
    }
    if (key == p + ".bias") {
      if (count != (size_t)l.cout) return aph_fail(APH_ERR_ARG, "aph_lpips_set_weight(%s): %zu elements, expected %d", name, count, l.cout);
      if (upload_f32(l.bias, data, 1, l.cout, false)) return aph_fail(APH_ERR_HIP, "aph_lpips_set_weight(%s): upload failed", name);
      l.b_set = true;
      return APH_OK;
    }
  }
  for (int s = 0; s < 5; ++s)
    if (key == "lin" + std::to_string(s) + ".weight") {
      if (count != (size_t)v->C[s]) return aph_fail(APH_ERR_ARG, "aph_lpips_set_weight(%s): %zu elements, expected %d", name, count, v->C[s]);
      if (upload_f32(v->lin[s], data, 1, v->C[s], false)) return aph_fail(APH_ERR_HIP, "aph_lpips_set_weight(%s): upload failed", name);
      v->lin_set[s] = true;
      return APH_OK;
    }
  return aph_fail(APH_ERR_ARG, "aph_lpips_set_weight: unknown key %s", name);
  APH_CATCH
}

int aph_lpips_set_target(aph_lpips* v, const float* d_img, int h, int w, void* stream_) {
  APH_TRY
  if (!v || !d_img) return aph_fail(APH_ERR_ARG, "aph_lpips_set_target: null argument");
  if (!((h == v->H && w == v->W) || (h == v->hs[0] && w == v->ws[0])))
    return aph_fail(APH_ERR_ARG, "aph_lpips_set_target: image %d x %d is neither the frame %d x %d nor its half size %d x %d", h, w, v->H, v->W, v->hs[0], v->ws[0]);
  if (const int rc = lpips_ready(v, "aph_lpips_set_target")) return rc;
  hipStream_t st = (hipStream_t)stream_;
  lpips_forward(v, d_img, h, w, st);
  for (int s = 0; s < 5; ++s) launch_unit_norm(v->conv[v->last[s]].act, v->hs[s] * v->ws[s], v->C[s], v->ny[s], st);
  v->target_set = true;
  return aph_check_launch("aph_lpips_set_target");
  APH_CATCH
}

// d_rgb [3][ih][iw], (ih, iw) = the full frame or its half size (the resize and its adjoint are then the identity: one tap of weight 1)
static int lpips_value_grad(aph_lpips* v, const float* d_rgb, int ih, int iw, const float* d_weight, float* d_loss, float* d_rgb_grad, void* stream_,
                            const char* who) {
  APH_TRY
  if (!v || !d_rgb || !d_weight) return aph_fail(APH_ERR_ARG, "%s: null argument", who);
  if (const int rc = lpips_ready(v, who)) return rc;
  if (!v->target_set) return aph_fail(APH_ERR_ARG, "%s: no target (aph_lpips_set_target first)", who);
  hipStream_t st = (hipStream_t)stream_;
  lpips_forward(v, d_rgb, ih, iw, st);
  HeadSums hs;
  int cur = 0;                        // v->g[cur] holds the gradient coming down
  for (int s = 4; s >= 0; --s) {
    const int P = v->hs[s] * v->ws[s], e = v->last[s], b = v->first[s];
    hs.partial[s] = v->partial + (size_t)s * kHeadBlocks; hs.count[s] = head_blocks(P); hs.P[s] = P;
    launch_head(v->conv[e].act, v->ny[s], v->lin[s], P, v->C[s], v->gscale / (float)P, d_rgb_grad ? v->hg : nullptr, v->partial + (size_t)s * kHeadBlocks, st);
    if (!d_rgb_grad) continue;
    launch_grad_merge(v->conv[e].act, v->hs[s], v->ws[s], v->C[s], s < 4 ? v->g[cur] : nullptr, v->hg, 1, v->g[cur ^ 1], st);
    cur ^= 1;
    for (int k = e; k >= b; --k) {
      const ConvLayer& l = v->conv[k];
      ConvArgs a{v->g[cur], v->hs[s], v->ws[s], l.cout, l.wd, round_up(l.cin, 16), nullptr, 0, nullptr, nullptr, nullptr, 0};
      if (k > b) { a.mask = v->conv[k - 1].act; a.out = v->g[cur ^ 1]; }
      else if (s > 0) a.out = v->g[cur ^ 1];
      else { a.out32 = v->g32; a.n32 = 3; }
      launch_conv(a, st);
      cur ^= 1;
    }
  }
  APH_LAUNCH(head_finish_kernel, dim3(1), dim3(256), 0, st, hs, d_weight, v->value, d_loss);
  if (d_rgb_grad) launch_resize_adj(v->g32, v->hs[0], v->ws[0], d_rgb_grad, ih, iw, 1.f / v->gscale, 1, d_weight, st);
  return aph_check_launch(who);
  APH_CATCH
}

int aph_lpips_value_grad(aph_lpips* v, const float* d_rgb, const float* d_weight, float* d_loss, float* d_rgb_grad, void* stream) {
  return lpips_value_grad(v, d_rgb, v ? v->H : 0, v ? v->W : 0, d_weight, d_loss, d_rgb_grad, stream, "aph_lpips_value_grad");
}
int aph_lpips_value_grad_half(aph_lpips* v, const float* d_x, const float* d_weight, float* d_loss, float* d_x_grad, void* stream) {
  return lpips_value_grad(v, d_x, v ? v->hs[0] : 0, v ? v->ws[0] : 0, d_weight, d_loss, d_x_grad, stream, "aph_lpips_value_grad_half");
}

}  // extern "C"
