// The Depth-Anything-V2 relative-depth estimator behind `illustrip.py -d` (reference depth/depth.py:20-32 loads transformers'
// DepthAnythingForDepthEstimation; tests/depthnet_ref.py is the restatement this is tested against): inference only.
//   encoder  DINOv2 S / B / L: patch rows (normalisation folded in, depth_kernels.h) -> patch-embedding GEMM with the position rows in its
//            epilogue -> per layer LN . QKV GEMM . attention (attn_long_fwd_kernel) . projection GEMM + residual . LN . fc1 GEMM + erf-GELU .
//            fc2 GEMM + residual, on the f16 GEMM of vit_gemm.h with an fp32 residual stream.  LayerScale is folded into the projection / fc2
//            weights and biases when they are uploaded.  The four tapped layers go through the final LayerNorm without their class row.
//   neck     per tap a 1 x 1 projection (dn_gemm_kernel), the resize of that tap (transpose convolution 4 / 2 as a GEMM with a pixel-shuffle
//            store, identity, 3 x 3 stride 2 as the stride-1 convolution + a subsample), a 3 x 3 convolution to the fusion width
//            (lpips_conv.h's kernel, X instantiation), then four fusion layers, coarsest first: pre-activation residual units (the first
//            convolution reads through a ReLU and writes through one, the second adds the unit's input -- and the running fused map -- in its
//            epilogue), a bilinear align_corners resize to the next tap's size (x 2 after the last), a 1 x 1 projection
//   head     3 x 3 to F / 2, resize to (h, w), 3 x 3 + ReLU to head_hidden, 1 x 1 + ReLU to one fp32 channel, optionally the per-image
//            min-max normalisation of InferDepthAny.__call__
// One arena, sized at create for max_batch images of max_h x max_w, holds weights and activations; aph_depth_forward allocates nothing and
// every launch is on the caller's stream (the first forward after a weight changed uploads the packed weights first, synchronously).
#include <algorithm>
#include <map>
#include <string>

#include "aph_device.h"
#include "aph_host.h"
#include "tower_store.h"
#include "vit_gemm.h"
#include "vit_gemm_ws.h"
#include "vit_gemm_rs.h"
#include "depth_epi.h"
#include "lpips_conv.h"
#include "depth_kernels.h"

using namespace aph;
using namespace aph::depth;
using aph::lpips::ConvArgs;
using aph::lpips::launch_conv;
using aph::lpips::pack_weights;

namespace {

struct EncLayer {
  half_t *w_qkv = nullptr, *w_o = nullptr, *w_fc1 = nullptr, *w_fc2 = nullptr;
  float *b_qkv = nullptr, *b_o = nullptr, *b_fc1 = nullptr, *b_fc2 = nullptr;
  float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
};
struct Conv3 { half_t* w = nullptr; float* b = nullptr; };      // packed [9][cout][cin] and bias [cout]
struct Fusion { half_t* pw = nullptr; float* pb = nullptr; Conv3 rl[2][2]; };
struct Spec { std::string name; size_t count; bool used; };

}  // namespace

struct aph_depth {
  int D, L, heads, F, HH, max_h, max_w, max_batch;
  int out_idx[4], neck[4];
  std::vector<Spec> specs;                                  // every checkpoint tensor this network has, in checkpoint order
  std::map<std::string, std::vector<float>> host;           // what aph_depth_set_weight was given
  bool dirty = true;                                        // host holds something the device copies do not
  int pos_gh = 0, pos_gw = 0;                               // grid of the position rows in `pos`
  // weights
  half_t* w_pe = nullptr; float *b_pe = nullptr, *cls = nullptr, *lnf_g = nullptr, *lnf_b = nullptr, *pos = nullptr;
  std::vector<EncLayer> layers;
  half_t* pj_w[4] = {}; float* pj_b[4] = {};
  half_t* rs_w[4] = {}; float* rs_b[4] = {};
  half_t* cv_w[4] = {};
  Fusion fu[4];
  Conv3 h1, h2;
  float* h3_w = nullptr; float h3_b = 0.f;
  // activations
  half_t *patches = nullptr, *hln = nullptr, *qkv = nullptr, *att = nullptr, *g = nullptr, *tap[4] = {};
  float *x = nullptr, *x_mid = nullptr, *mm = nullptr;
  half_t *pj = nullptr, *s1 = nullptr, *r[4] = {}, *f[4] = {}, *U[3] = {}, *up = nullptr, *c2 = nullptr;
  char* arena = nullptr;
  size_t arena_bytes = 0;
};

namespace {

void depth_build_specs(aph_depth* v) {
  const size_t D = v->D, F = v->F;
  std::vector<Spec>& s = v->specs;
  auto add = [&](std::string n, size_t c, bool used = true) { s.push_back(Spec{std::move(n), c, used}); };
  add("backbone.embeddings.cls_token", D);
  add("backbone.embeddings.patch_embeddings.projection.weight", D * kPatchK);
  add("backbone.embeddings.patch_embeddings.projection.bias", D);
  for (int i = 0; i < v->L; ++i) {
    const std::string p = "backbone.encoder.layer." + std::to_string(i) + ".";
    add(p + "norm1.weight", D); add(p + "norm1.bias", D);
    for (const char* n : {"query", "key", "value"}) { add(p + "attention.attention." + n + ".weight", D * D); add(p + "attention.attention." + n + ".bias", D); }
    add(p + "attention.output.dense.weight", D * D); add(p + "attention.output.dense.bias", D);
    add(p + "layer_scale1.lambda1", D);
    add(p + "norm2.weight", D); add(p + "norm2.bias", D);
    add(p + "mlp.fc1.weight", 4 * D * D); add(p + "mlp.fc1.bias", 4 * D);
    add(p + "mlp.fc2.weight", 4 * D * D); add(p + "mlp.fc2.bias", D);
    add(p + "layer_scale2.lambda1", D);
  }
  add("backbone.layernorm.weight", D); add("backbone.layernorm.bias", D);
  for (int i = 0; i < 4; ++i) {
    const std::string p = "neck.reassemble_stage.layers." + std::to_string(i) + ".";
    const size_t C = v->neck[i];
    add(p + "projection.weight", C * D); add(p + "projection.bias", C);
    if (i != 2) { add(p + "resize.weight", C * C * (i == 0 ? 16 : i == 1 ? 4 : 9)); add(p + "resize.bias", C); }
  }
  for (int i = 0; i < 4; ++i) add("neck.convs." + std::to_string(i) + ".weight", F * v->neck[i] * 9);
  for (int i = 0; i < 4; ++i) {
    const std::string p = "neck.fusion_stage.layers." + std::to_string(i) + ".";
    add(p + "projection.weight", F * F); add(p + "projection.bias", F);
    for (int u = 0; u < 2; ++u)
      for (int c = 0; c < 2; ++c) {
        const std::string q = p + "residual_layer" + std::to_string(u + 1) + ".convolution" + std::to_string(c + 1);
        // the first fusion layer has no lateral input: the checkpoint carries its residual_layer1, the network never runs it
        add(q + ".weight", F * F * 9, !(i == 0 && u == 0)); add(q + ".bias", F, !(i == 0 && u == 0));
      }
  }
  add("head.conv1.weight", (F / 2) * F * 9); add("head.conv1.bias", F / 2);
  add("head.conv2.weight", (size_t)v->HH * (F / 2) * 9); add("head.conv2.bias", v->HH);
  add("head.conv3.weight", v->HH); add("head.conv3.bias", 1);
}

size_t depth_carve(aph_depth* v, char* base) {
  Carver c{base};
  const size_t D = v->D, F = v->F, B = v->max_batch;
  const size_t gh = v->max_h / kPatch, gw = v->max_w / kPatch, P = gh * gw, T = P + 1, M = B * T, P3 = ((gh + 1) / 2) * ((gw + 1) / 2);
  v->w_pe = c.take<half_t>(D * kPatchKP); v->b_pe = c.take<float>(D); v->cls = c.take<float>(D);
  v->lnf_g = c.take<float>(D); v->lnf_b = c.take<float>(D); v->pos = c.take<float>(T * D);
  for (EncLayer& l : v->layers) {
    l.w_qkv = c.take<half_t>(3 * D * D); l.w_o = c.take<half_t>(D * D); l.w_fc1 = c.take<half_t>(4 * D * D); l.w_fc2 = c.take<half_t>(4 * D * D);
    l.b_qkv = c.take<float>(3 * D); l.b_o = c.take<float>(D); l.b_fc1 = c.take<float>(4 * D); l.b_fc2 = c.take<float>(D);
    l.ln1_g = c.take<float>(D); l.ln1_b = c.take<float>(D); l.ln2_g = c.take<float>(D); l.ln2_b = c.take<float>(D);
  }
  size_t cmax = 0;
  for (int i = 0; i < 4; ++i) {
    const size_t C = v->neck[i];
    cmax = std::max(cmax, C);
    v->pj_w[i] = c.take<half_t>(C * D); v->pj_b[i] = c.take<float>(C);
    v->rs_w[i] = c.take<half_t>(C * C * 16); v->rs_b[i] = c.take<float>(C);
    v->cv_w[i] = c.take<half_t>(9 * F * C);
    v->fu[i].pw = c.take<half_t>(F * F); v->fu[i].pb = c.take<float>(F);
    for (int u = 0; u < 2; ++u)
      for (int k = 0; k < 2; ++k) { v->fu[i].rl[u][k].w = c.take<half_t>(9 * F * F); v->fu[i].rl[u][k].b = c.take<float>(F); }
  }
  v->h1.w = c.take<half_t>(9 * (F / 2) * F); v->h1.b = c.take<float>(F / 2);
  v->h2.w = c.take<half_t>(9 * (size_t)v->HH * (F / 2)); v->h2.b = c.take<float>(v->HH);
  v->h3_w = c.take<float>(v->HH);
  // activations of max_batch images of the largest grid
  v->patches = c.take<half_t>(B * P * kPatchKP);
  v->x = c.take<float>(M * D); v->x_mid = c.take<float>(M * D);
  v->hln = c.take<half_t>(M * D); v->qkv = c.take<half_t>(M * 3 * D); v->att = c.take<half_t>(M * D); v->g = c.take<half_t>(M * 4 * D);
  for (int i = 0; i < 4; ++i) v->tap[i] = c.take<half_t>(B * P * D);
  v->pj = c.take<half_t>(B * P * cmax); v->s1 = c.take<half_t>(B * P * v->neck[3]);
  const size_t Pi[4] = {16 * P, 4 * P, P, P3};
  for (int i = 0; i < 4; ++i) { v->r[i] = c.take<half_t>(B * Pi[i] * v->neck[i]); v->f[i] = c.take<half_t>(B * Pi[i] * F); }
  for (int i = 0; i < 3; ++i) v->U[i] = c.take<half_t>(B * 64 * P * F);
  v->up = c.take<half_t>(B * 196 * P * (F / 2)); v->c2 = c.take<half_t>(B * 196 * P * v->HH);
  v->mm = c.take<float>(B * kMmBlocks * 2);
  return c.off;
}

int up_h(half_t* dst, const std::vector<half_t>& s) { return hipMemcpy(dst, s.data(), s.size() * sizeof(half_t), hipMemcpyHostToDevice) == hipSuccess ? 0 : -1; }
int up_f(float* dst, const std::vector<float>& s) { return hipMemcpy(dst, s.data(), s.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess ? 0 : -1; }
std::vector<half_t> to_h(const std::vector<float>& s) {
  std::vector<half_t> o(s.size());
  for (size_t i = 0; i < s.size(); ++i) o[i] = (half_t)s[i];
  return o;
}
// rows of w [rows][cols] and b [rows] times scale [rows] (LayerScale behind a linear layer: lambda (W x + b) = (lambda W) x + lambda b, in fp32)
void fold_rows(std::vector<float>& w, std::vector<float>& b, const std::vector<float>& scale, size_t rows, size_t cols) {
  for (size_t r = 0; r < rows; ++r) {
    for (size_t k = 0; k < cols; ++k) w[r * cols + k] *= scale[r];
    b[r] *= scale[r];
  }
}

// every device copy from the host tensors; 0 or -1 (an upload failed)
int depth_upload(aph_depth* v) {
  const size_t D = v->D, F = v->F;
  auto H = [&](const std::string& n) -> const std::vector<float>& { return v->host.at(n); };
  int bad = 0;
  {
    const std::vector<float>& w = H("backbone.embeddings.patch_embeddings.projection.weight");
    std::vector<half_t> p(D * kPatchKP, (half_t)0.f);
    for (size_t n = 0; n < D; ++n)
      for (int k = 0; k < kPatchK; ++k) p[n * kPatchKP + k] = (half_t)w[n * kPatchK + k];
    bad |= up_h(v->w_pe, p);
  }
  bad |= up_f(v->b_pe, H("backbone.embeddings.patch_embeddings.projection.bias"));
  bad |= up_f(v->cls, H("backbone.embeddings.cls_token"));
  bad |= up_f(v->lnf_g, H("backbone.layernorm.weight")); bad |= up_f(v->lnf_b, H("backbone.layernorm.bias"));
  for (int i = 0; i < v->L; ++i) {
    EncLayer& l = v->layers[i];
    const std::string p = "backbone.encoder.layer." + std::to_string(i) + ".";
    std::vector<float> wq, bq;
    for (const char* n : {"query", "key", "value"}) {
      const std::vector<float>&w = H(p + "attention.attention." + n + ".weight"), &b = H(p + "attention.attention." + n + ".bias");
      wq.insert(wq.end(), w.begin(), w.end()); bq.insert(bq.end(), b.begin(), b.end());
    }
    bad |= up_h(l.w_qkv, to_h(wq)); bad |= up_f(l.b_qkv, bq);
    std::vector<float> wo = H(p + "attention.output.dense.weight"), bo = H(p + "attention.output.dense.bias");
    fold_rows(wo, bo, H(p + "layer_scale1.lambda1"), D, D);
    bad |= up_h(l.w_o, to_h(wo)); bad |= up_f(l.b_o, bo);
    bad |= up_h(l.w_fc1, to_h(H(p + "mlp.fc1.weight"))); bad |= up_f(l.b_fc1, H(p + "mlp.fc1.bias"));
    std::vector<float> w2 = H(p + "mlp.fc2.weight"), b2 = H(p + "mlp.fc2.bias");
    fold_rows(w2, b2, H(p + "layer_scale2.lambda1"), D, 4 * D);
    bad |= up_h(l.w_fc2, to_h(w2)); bad |= up_f(l.b_fc2, b2);
    bad |= up_f(l.ln1_g, H(p + "norm1.weight")); bad |= up_f(l.ln1_b, H(p + "norm1.bias"));
    bad |= up_f(l.ln2_g, H(p + "norm2.weight")); bad |= up_f(l.ln2_b, H(p + "norm2.bias"));
  }
  auto conv3 = [&](const Conv3& c, const std::string& name, int cout, int cin) {
    bad |= up_h(c.w, pack_weights(H(name + ".weight").data(), cout, cin, 0));
    if (c.b) bad |= up_f(c.b, H(name + ".bias"));
  };
  for (int i = 0; i < 4; ++i) {
    const int C = v->neck[i];
    const std::string p = "neck.reassemble_stage.layers." + std::to_string(i) + ".";
    bad |= up_h(v->pj_w[i], to_h(H(p + "projection.weight"))); bad |= up_f(v->pj_b[i], H(p + "projection.bias"));
    if (i < 2) { bad |= up_h(v->rs_w[i], pack_convt(H(p + "resize.weight").data(), C, C, i == 0 ? 4 : 2)); bad |= up_f(v->rs_b[i], H(p + "resize.bias")); }
    if (i == 3) conv3(Conv3{v->rs_w[3], v->rs_b[3]}, p + "resize", C, C);
    conv3(Conv3{v->cv_w[i], nullptr}, "neck.convs." + std::to_string(i), (int)F, C);
    const std::string q = "neck.fusion_stage.layers." + std::to_string(i) + ".";
    bad |= up_h(v->fu[i].pw, to_h(H(q + "projection.weight"))); bad |= up_f(v->fu[i].pb, H(q + "projection.bias"));
    for (int u = (i == 0 ? 1 : 0); u < 2; ++u)
      for (int k = 0; k < 2; ++k) conv3(v->fu[i].rl[u][k], q + "residual_layer" + std::to_string(u + 1) + ".convolution" + std::to_string(k + 1), (int)F, (int)F);
  }
  conv3(v->h1, "head.conv1", (int)F / 2, (int)F);
  conv3(v->h2, "head.conv2", v->HH, (int)F / 2);
  bad |= up_f(v->h3_w, H("head.conv3.weight"));
  v->h3_b = H("head.conv3.bias")[0];
  return bad ? -1 : 0;
}

// handed to every launch_gemm: no split-K workspace and "not a small batch", so that no GEMM is split over k or takes the register-staged
// split-K kernel -- every output is one k-ordered accumulation whatever M is, and an image's depth does not depend on the batch it is in
const SplitKSpace kNoSplit{nullptr, 0, false};

// one 3 x 3 convolution (pad 1, stride 1) on `batch` maps of H x W
void conv(const half_t* in, int H, int W, int cin, const Conv3& c, int cout, int relu_in, int relu, const half_t* res, const half_t* res2, half_t* out, int batch,
          hipStream_t st) {
  ConvArgs a{in, H, W, cin, c.w, cout, c.b, relu, nullptr, out, nullptr, 0};
  a.relu_in = relu_in; a.res = res; a.res2 = res2; a.batch = batch;
  launch_conv<true>(a, st);
}

}  // namespace

extern "C" {

int aph_depth_create(int hidden, int layers, int heads, int swiglu, const int* out_indices, const int* neck_sizes, int fusion, int head_hidden, int max_h,
                     int max_w, int max_batch, aph_depth** out) {
  APH_TRY
  if (!out || !out_indices || !neck_sizes) return aph_fail(APH_ERR_ARG, "aph_depth_create: null argument");
  if (swiglu) return aph_fail(APH_ERR_UNSUPPORTED, "aph_depth_create: the SwiGLU feed-forward (the giant encoder) is not supported");
  if (hidden < 128 || hidden % 128 || hidden > 1024)
    return aph_fail(APH_ERR_UNSUPPORTED, "aph_depth_create: hidden size %d unsupported (a multiple of 128 up to 1024)", hidden);
  if (heads < 1 || heads * 64 != hidden) return aph_fail(APH_ERR_UNSUPPORTED, "aph_depth_create: hidden %d / heads %d unsupported (head dim 64)", hidden, heads);
  if (layers < 1 || layers > 64) return aph_fail(APH_ERR_ARG, "aph_depth_create: %d layers outside 1 .. 64", layers);
  for (int i = 0; i < 4; ++i) {
    if (out_indices[i] < 1 || out_indices[i] > layers || (i && out_indices[i] < out_indices[i - 1]))
      return aph_fail(APH_ERR_ARG, "aph_depth_create: out_indices must be four non-decreasing layer numbers in 1 .. %d", layers);
    if (neck_sizes[i] < 16 || neck_sizes[i] % 16 || neck_sizes[i] > 2048)
      return aph_fail(APH_ERR_UNSUPPORTED, "aph_depth_create: neck width %d unsupported (a multiple of 16 up to 2048)", neck_sizes[i]);
  }
  if (fusion < 32 || fusion % 32 || fusion > 1024) return aph_fail(APH_ERR_UNSUPPORTED, "aph_depth_create: fusion width %d unsupported (a multiple of 32 up to 1024)", fusion);
  if (head_hidden < 16 || head_hidden % 16 || head_hidden > 256)
    return aph_fail(APH_ERR_UNSUPPORTED, "aph_depth_create: head width %d unsupported (a multiple of 16 up to 256)", head_hidden);
  if (max_h < kPatch || max_w < kPatch || max_h % kPatch || max_w % kPatch || max_h > 4096 || max_w > 4096)
    return aph_fail(APH_ERR_ARG, "aph_depth_create: largest image %d x %d must be multiples of 14 in 14 .. 4096", max_h, max_w);
  if (max_batch < 1 || max_batch > 64) return aph_fail(APH_ERR_ARG, "aph_depth_create: max_batch %d outside 1 .. 64", max_batch);
  auto* v = new aph_depth();
  v->D = hidden; v->L = layers; v->heads = heads; v->F = fusion; v->HH = head_hidden; v->max_h = max_h; v->max_w = max_w; v->max_batch = max_batch;
  for (int i = 0; i < 4; ++i) { v->out_idx[i] = out_indices[i]; v->neck[i] = neck_sizes[i]; }
  v->layers.resize(layers);
  depth_build_specs(v);
  if (const int rc = alloc_arena("aph_depth_create", &v->arena, &v->arena_bytes, [&](char* base) { return depth_carve(v, base); })) { delete v; return rc; }
  *out = v;
  return APH_OK;
  APH_CATCH
}

int aph_depth_destroy(aph_depth* v) {
  if (!v) return APH_OK;
  (void)hipFree(v->arena);
  delete v;
  return APH_OK;
}

size_t aph_depth_workspace_bytes(const aph_depth* v) { return v ? v->arena_bytes : 0; }

int aph_depth_set_weight(aph_depth* v, const char* name, const float* data, size_t count) {
  APH_TRY
  if (!v || !name || !data) return aph_fail(APH_ERR_ARG, "aph_depth_set_weight: null argument");
  for (const Spec& s : v->specs)
    if (s.name == name) {
      if (count != s.count) return aph_fail(APH_ERR_ARG, "aph_depth_set_weight(%s): %zu elements, expected %zu", name, count, s.count);
      if (s.used) { v->host[s.name].assign(data, data + count); v->dirty = true; }
      return APH_OK;
    }
  return aph_fail(APH_ERR_ARG, "aph_depth_set_weight: unknown key %s", name);
  APH_CATCH
}

int aph_depth_set_pos_embed(aph_depth* v, int gh, int gw, const float* rows, size_t count) {
  APH_TRY
  if (!v || !rows) return aph_fail(APH_ERR_ARG, "aph_depth_set_pos_embed: null argument");
  if (gh < 1 || gw < 1 || gh * kPatch > v->max_h || gw * kPatch > v->max_w)
    return aph_fail(APH_ERR_ARG, "aph_depth_set_pos_embed: grid %d x %d outside 1 x 1 .. %d x %d", gh, gw, v->max_h / kPatch, v->max_w / kPatch);
  const size_t want = ((size_t)gh * gw + 1) * v->D;
  if (count != want) return aph_fail(APH_ERR_ARG, "aph_depth_set_pos_embed: %zu elements, expected %zu ((1 + %d x %d) rows of %d)", count, want, gh, gw, v->D);
  v->pos_gh = v->pos_gw = 0;
  if (hipMemcpy(v->pos, rows, count * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return aph_fail(APH_ERR_HIP, "aph_depth_set_pos_embed: upload failed");
  v->pos_gh = gh; v->pos_gw = gw;
  return APH_OK;
  APH_CATCH
}

int aph_depth_forward(aph_depth* v, const float* d_img, int B, int h, int w, int normalise, float* d_depth, void* stream_) {
  APH_TRY
  if (!v || !d_img || !d_depth) return aph_fail(APH_ERR_ARG, "aph_depth_forward: null argument");
  if (B < 1 || B > v->max_batch) return aph_fail(APH_ERR_ARG, "aph_depth_forward: batch %d outside 1..%d", B, v->max_batch);
  if (h < kPatch || w < kPatch || h % kPatch || w % kPatch) return aph_fail(APH_ERR_ARG, "aph_depth_forward: image %d x %d: both sides must be multiples of 14", h, w);
  if (h > v->max_h || w > v->max_w) return aph_fail(APH_ERR_ARG, "aph_depth_forward: image %d x %d larger than the %d x %d this estimator was created for", h, w, v->max_h, v->max_w);
  for (const Spec& s : v->specs)
    if (s.used && !v->host.count(s.name)) return aph_fail(APH_ERR_ARG, "aph_depth_forward: weight %s not set", s.name.c_str());
  const int gh = h / kPatch, gw = w / kPatch;
  if (gh != v->pos_gh || gw != v->pos_gw)
    return aph_fail(APH_ERR_ARG, "aph_depth_forward: position rows are set for a %d x %d grid, the image has %d x %d (aph_depth_set_pos_embed)", v->pos_gh, v->pos_gw, gh, gw);
  if (v->dirty) {
    if (depth_upload(v)) return aph_fail(APH_ERR_HIP, "aph_depth_forward: weight upload failed");
    v->dirty = false;
  }
  hipStream_t st = (hipStream_t)stream_;
  const int D = v->D, F = v->F, P = gh * gw, T = P + 1, M = B * T;
  const float eps = 1e-6f;

  // ---- encoder
  {
    const size_t n = (size_t)B * P * (kPatchKP / 8);
    APH_LAUNCH(dn_patch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_img, v->patches, B, h, w);
  }
  launch_gemm(v->patches, kPatchKP, v->w_pe, kPatchKP, B * P, D, kPatchKP, EpiPatchEmbedRect{v->x, v->pos, v->b_pe, D, P, T}, st, &kNoSplit);
  APH_LAUNCH(dn_cls_kernel, dim3((unsigned)((B * D + 255) / 256)), dim3(256), 0, st, (const float*)v->cls, (const float*)v->pos, v->x, B, T, D);
  int tap = 0;
  for (int li = 0; li < v->L; ++li) {
    const EncLayer& l = v->layers[li];
    launch_dn_ln<false>(v->x, l.ln1_g, l.ln1_b, v->hln, M, T, D, eps, st);
    launch_gemm(v->hln, D, l.w_qkv, D, M, 3 * D, D, EpiF16{v->qkv, 3 * D, l.b_qkv}, st, &kNoSplit);
    launch_attn_long_fwd(v->qkv, v->att, B, T, v->heads, st);
    launch_gemm(v->att, D, l.w_o, D, M, D, D, EpiResidual{v->x_mid, v->x, D, l.b_o}, st, &kNoSplit);
    launch_dn_ln<false>(v->x_mid, l.ln2_g, l.ln2_b, v->hln, M, T, D, eps, st);
    launch_gemm(v->hln, D, l.w_fc1, D, M, 4 * D, D, EpiGeluErfF16{v->g, 4 * D, l.b_fc1}, st, &kNoSplit);
    launch_gemm(v->g, 4 * D, l.w_fc2, 4 * D, M, D, 4 * D, EpiResidual{v->x, v->x_mid, D, l.b_fc2}, st, &kNoSplit);
    for (; tap < 4 && v->out_idx[tap] == li + 1; ++tap) launch_dn_ln<true>(v->x, v->lnf_g, v->lnf_b, v->tap[tap], M, T, D, eps, st);
  }

  // ---- neck: reassemble
  const int Hs[4] = {4 * gh, 2 * gh, gh, (gh + 1) / 2}, Ws[4] = {4 * gw, 2 * gw, gw, (gw + 1) / 2};
  for (int i = 0; i < 4; ++i) {
    const int C = v->neck[i];
    half_t* proj = i == 2 ? v->r[2] : v->pj;
    launch_dn_gemm(v->tap[i], D, v->pj_w[i], B * P, C, D, EpiDnBias{proj, C, v->pj_b[i]}, st);
    if (i < 2) {
      const int k = i == 0 ? 4 : 2;
      launch_dn_gemm(v->pj, C, v->rs_w[i], B * P, k * k * C, C, EpiDnShuffle{v->r[i], v->rs_b[i], gh, gw, k, C}, st);
    } else if (i == 3) {
      conv(v->pj, gh, gw, C, Conv3{v->rs_w[3], v->rs_b[3]}, C, 0, 0, nullptr, nullptr, v->s1, B, st);
      launch_dn_subsample(v->s1, gh, gw, v->r[3], C, B, st);
    }
    conv(v->r[i], Hs[i], Ws[i], C, Conv3{v->cv_w[i], nullptr}, F, 0, 0, nullptr, nullptr, v->f[i], B, st);
  }
  // ---- neck: fusion, coarsest first; the running fused map lives in U[2]
  half_t *U0 = v->U[0], *U1 = v->U[1], *U2 = v->U[2];
  for (int idx = 0; idx < 4; ++idx) {
    const int i = 3 - idx, H = Hs[i], W = Ws[i];
    const Fusion& fu = v->fu[idx];
    const half_t* hid = v->f[i];
    if (idx > 0) {      // hidden = fused + residual_layer1(tap feature)
      conv(v->f[i], H, W, F, fu.rl[0][0], F, 1, 1, nullptr, nullptr, U0, B, st);
      conv(U0, H, W, F, fu.rl[0][1], F, 0, 0, v->f[i], U2, U1, B, st);
      hid = U1;
    }
    conv(hid, H, W, F, fu.rl[1][0], F, 1, 1, nullptr, nullptr, U0, B, st);
    conv(U0, H, W, F, fu.rl[1][1], F, 0, 0, hid, nullptr, U2, B, st);
    const int Hn = idx < 3 ? Hs[i - 1] : 2 * H, Wn = idx < 3 ? Ws[i - 1] : 2 * W;
    launch_dn_resize(U2, H, W, U0, Hn, Wn, F, B, st);
    launch_dn_gemm(U0, F, fu.pw, B * Hn * Wn, F, F, EpiDnBias{U2, F, fu.pb}, st);
  }
  // ---- head
  const int Hf = 8 * gh, Wf = 8 * gw;
  conv(U2, Hf, Wf, F, v->h1, F / 2, 0, 0, nullptr, nullptr, U0, B, st);
  launch_dn_resize(U0, Hf, Wf, v->up, h, w, F / 2, B, st);
  conv(v->up, h, w, F / 2, v->h2, v->HH, 0, 1, nullptr, nullptr, v->c2, B, st);
  {
    const size_t n = (size_t)B * h * w;
    APH_LAUNCH(dn_head_out_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const half_t*)v->c2, (const float*)v->h3_w, v->h3_b, d_depth, n, v->HH);
  }
  if (normalise) launch_dn_minmax(d_depth, (size_t)h * w, B, v->mm, st);
  return aph_check_launch("aph_depth_forward");
  APH_CATCH
}

}  // extern "C"
