// CLIP ViT visual tower: `model.encode_image(x)` forward and its INPUT-gradient backward
// (clip_fft.py:254 and the autograd pass of clip_fft.py:294 through it).  Weight gradients are
// never formed -- the optimisation only updates the image parameters.
//
// fp16 operands / fp32 accumulation on the matrix cores, fp32 residual stream, fp32 LayerNorm and
// softmax statistics; the backward chain carries a static loss scale (applied by the caller to
// d_enc, removed by `out_scale`) so fp16 gradient activations do not underflow.
#include <string>

#include "aph_device.h"
#include "aph_host.h"
#include "tower_store.h"
#include "vit_gemm.h"
#include "vit_gemm_ws.h"
#include "vit_gemm_rs.h"
#include "vit_ops.h"
#include "vit_attn.h"
#include "vit_gemm_f32.h"
#include "vit_attn_f32.h"

using namespace aph;

namespace {

struct Layer {
  half_t *w_qkv = nullptr, *w_qkvT = nullptr, *w_o = nullptr, *w_oT = nullptr;
  half_t* w_qkv2 = nullptr;            // [3D, 2D]: w_qkv repeated along K (split-precision forward)
  half_t *w_fc1 = nullptr, *w_fc1T = nullptr, *w_fc2 = nullptr, *w_fc2T = nullptr;
  float *b_qkv = nullptr, *b_o = nullptr, *b_fc1 = nullptr, *b_fc2 = nullptr;
  float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
  // per-layer activations kept for the backward
  float *x_in = nullptr, *x_mid = nullptr, *lse = nullptr;
  half_t *qkv = nullptr, *att = nullptr, *u = nullptr;
  // exact path (aph_vit_enable_f32): fp32 weights [N, K] and their transposes, fp32 activations kept for the backward
  float *w_qkv32 = nullptr, *w_qkvT32 = nullptr, *w_o32 = nullptr, *w_oT32 = nullptr;
  float *w_fc1_32 = nullptr, *w_fc1T32 = nullptr, *w_fc2_32 = nullptr, *w_fc2T32 = nullptr;
  float *qkv32 = nullptr, *dg32 = nullptr;
};

constexpr size_t kGlobalWeights = 8, kLayerWeights = 12;      // table order = carve order: the global tensors, then layer by layer

}  // namespace

struct aph_vit {
  int res, patch, D, L, heads, E, T, P, Kp, max_batch;
  half_t *w_patch = nullptr, *w_patchT = nullptr, *w_patch2 = nullptr;      // w_patch2 [D, 2 Kp]: w_patch repeated along K
  float *cls = nullptr, *pos = nullptr, *ln_pre_g = nullptr, *ln_pre_b = nullptr, *ln_post_g = nullptr, *ln_post_b = nullptr;
  float *proj = nullptr, *projT = nullptr;
  std::vector<Layer> layers;
  float *x0 = nullptr, *x_last = nullptr;
  half_t *h = nullptr, *gact = nullptr;
  float* dx = nullptr;                 // fp32 residual-stream gradient
  half_t *dx16 = nullptr, *du = nullptr, *dh = nullptr, *datt = nullptr, *dqkv = nullptr, *dx0_16 = nullptr;
  SplitKSpace sk;                      // split-K partials of the small-M GEMMs (per-rank shards, class-row GEMMs)
  char* arena = nullptr;
  size_t arena_bytes = 0;
  char* arena_hilo = nullptr;          // [r6] the K-repeated weight copies of the split-precision forward (w_patch2, w_qkv2): allocated by aph_vit_enable_hilo only
  size_t arena_hilo_bytes = 0;
  // exact path (aph_vit_enable_f32): fp32 weights, the fp32 activation stash and gradient buffers, in an arena of their own
  char* arena_f32 = nullptr;
  size_t arena_f32_bytes = 0;
  float *w_patch32 = nullptr, *w_patchT32 = nullptr;
  float *h32 = nullptr, *g32 = nullptr, *att32 = nullptr, *datt32 = nullptr, *dqkv32 = nullptr, *delta32 = nullptr;
  F32Space f32sp;                      // split-K partials of the fp32 class-row GEMMs
  std::vector<Weight> weights;         // every checkpoint tensor (build_weights; tower_store.h), looked up by key
  int last_fwd = 0;                    // precision of the last forward: 0 none, 1 f16 (aph_vit_forward / _hilo), 2 fp32 (aph_vit_forward_f32)
  // optional per-launch timing of the GEMM family (bench.py roofline): HIP event pairs on the launch stream
  bool prof_on = false;
  std::vector<hipEvent_t> prof_ev;     // pairs
  size_t prof_used = 0;
  double prof_flops = 0.0;
};

namespace {

// The weight table: 8 global tensors, then 12 per layer, in the order the arenas are carved in (a layer's f16 matrices, its biases, its
// LayerNorm vectors).  v->layers must have its final size: the table points at its members.
void build_weights(aph_vit* v) {
  const size_t D = v->D;
  std::vector<Weight>& t = v->weights;
  t.reserve(kGlobalWeights + kLayerWeights * v->L);
  add_mat(t, "conv1.weight", D, v->Kp, &v->w_patch, &v->w_patchT, &v->w_patch2, &v->w_patch32, &v->w_patchT32);
  add_f32(t, "class_embedding", 1, D, &v->cls);
  add_f32(t, "positional_embedding", v->T, D, &v->pos);
  add_f32(t, "ln_pre.weight", 1, D, &v->ln_pre_g); add_f32(t, "ln_pre.bias", 1, D, &v->ln_pre_b);
  add_f32(t, "ln_post.weight", 1, D, &v->ln_post_g); add_f32(t, "ln_post.bias", 1, D, &v->ln_post_b);
  add_f32(t, "proj", D, v->E, &v->proj, &v->projT);
  for (int li = 0; li < v->L; ++li) {
    Layer& l = v->layers[li];
    const std::string p = "transformer.resblocks." + std::to_string(li) + ".";
    add_mat(t, p + "attn.in_proj_weight", 3 * D, D, &l.w_qkv, &l.w_qkvT, &l.w_qkv2, &l.w_qkv32, &l.w_qkvT32);
    add_mat(t, p + "attn.out_proj.weight", D, D, &l.w_o, &l.w_oT, nullptr, &l.w_o32, &l.w_oT32);
    add_mat(t, p + "mlp.c_fc.weight", 4 * D, D, &l.w_fc1, &l.w_fc1T, nullptr, &l.w_fc1_32, &l.w_fc1T32);
    add_mat(t, p + "mlp.c_proj.weight", D, 4 * D, &l.w_fc2, &l.w_fc2T, nullptr, &l.w_fc2_32, &l.w_fc2T32);
    add_f32(t, p + "attn.in_proj_bias", 1, 3 * D, &l.b_qkv); add_f32(t, p + "attn.out_proj.bias", 1, D, &l.b_o);
    add_f32(t, p + "mlp.c_fc.bias", 1, 4 * D, &l.b_fc1); add_f32(t, p + "mlp.c_proj.bias", 1, D, &l.b_fc2);
    add_f32(t, p + "ln_1.weight", 1, D, &l.ln1_g); add_f32(t, p + "ln_1.bias", 1, D, &l.ln1_b);
    add_f32(t, p + "ln_2.weight", 1, D, &l.ln2_g); add_f32(t, p + "ln_2.bias", 1, D, &l.ln2_b);
  }
}

// The carve functions point the handle's members into `base` and return the arena's size; base == nullptr: null pointers, the size alone.

// the second arena (aph_vit_enable_hilo): [N, 2 K] copies of the patch-embedding and QKV weights, every row twice along K -- the B operand of
// a GEMM over [hi | lo] activation rows.  85 MB at ViT-B/32 that the default (f16 everywhere) path never touches.
size_t carve_hilo(aph_vit* v, char* base) {
  Carver c{base};
  carve_weights(v->weights, c, 0, v->weights.size(), ARENA_HILO);
  return c.off;
}

// the exact path's arena (aph_vit_enable_f32): fp32 weights [N, K] and transposes, the fp32 stash (per block: qkv, dGELU/du), shared fp32
// scratch (LayerNorm outputs / their gradients, GELU outputs / du, attention output / its gradient, dqkv, attention row dots) and the split-K
// partials of the class-row GEMMs.  x_in / x_mid / lse / x0 / x_last / dx of the main arena are fp32 already and are shared with the f16 path.
size_t carve_f32(aph_vit* v, char* base) {
  Carver c{base};
  const size_t D = v->D, Mx = (size_t)v->max_batch * v->T;
  carve_weights(v->weights, c, 0, kGlobalWeights, ARENA_F32);
  for (size_t li = 0; li < v->layers.size(); ++li) {
    Layer& l = v->layers[li];
    carve_weights(v->weights, c, kGlobalWeights + li * kLayerWeights, kGlobalWeights + (li + 1) * kLayerWeights, ARENA_F32);
    l.qkv32 = c.take<float>(Mx * 3 * D); l.dg32 = c.take<float>(Mx * 4 * D);
  }
  v->h32 = c.take<float>(Mx * D); v->g32 = c.take<float>(Mx * 4 * D);
  v->att32 = c.take<float>(Mx * D); v->datt32 = c.take<float>(Mx * D); v->dqkv32 = c.take<float>(Mx * 3 * D);
  v->delta32 = c.take<float>((size_t)v->max_batch * v->heads * v->T);
  v->f32sp.ws_floats = (size_t)8 * v->max_batch * 4 * D;
  v->f32sp.ws = c.take<float>(v->f32sp.ws_floats);
  return c.off;
}

size_t carve(aph_vit* v, char* base) {
  Carver c{base};
  const size_t D = v->D, Mx = (size_t)v->max_batch * v->T, T = v->T;
  carve_weights(v->weights, c, 0, kGlobalWeights, ARENA_MAIN);
  for (size_t li = 0; li < v->layers.size(); ++li) {
    Layer& l = v->layers[li];
    carve_weights(v->weights, c, kGlobalWeights + li * kLayerWeights, kGlobalWeights + (li + 1) * kLayerWeights, ARENA_MAIN);
    l.x_in = c.take<float>(Mx * D); l.x_mid = c.take<float>(Mx * D); l.lse = c.take<float>((size_t)v->max_batch * v->heads * T);
    l.qkv = c.take<half_t>(Mx * 3 * D); l.att = c.take<half_t>(Mx * D); l.u = c.take<half_t>(Mx * 4 * D);
  }
  v->x0 = c.take<float>(Mx * D); v->x_last = c.take<float>(Mx * D);
  v->h = c.take<half_t>(Mx * 2 * D); v->gact = c.take<half_t>(Mx * 4 * D);      // h: [hi | lo] rows in the split-precision forward
  v->dx = c.take<float>(Mx * D);
  v->dx16 = c.take<half_t>(Mx * D); v->du = c.take<half_t>(Mx * 4 * D); v->dh = c.take<half_t>(Mx * D);
  v->datt = c.take<half_t>(Mx * D); v->dqkv = c.take<half_t>(Mx * 3 * D); v->dx0_16 = c.take<half_t>(Mx * D);
  v->sk.ws_floats = (size_t)256 * GemmSmall::BM * GemmSmall::BN;       // choose_splits keeps tiles * splits <= 256
  v->sk.ws = c.take<float>(v->sk.ws_floats);
  return c.off;
}

// host fp32 copy of a weight matrix -> the fp32 arena (when both exist)
int sync_f32(aph_vit* v, const Weight& w) {
  if (!v->arena_f32 || !w.m32[0] || w.host.empty()) return 0;
  return upload_f32(*w.m32[0], w.host.data(), w.rows, w.cols, false) | upload_f32(*w.m32[1], w.host.data(), w.rows, w.cols, true);
}

// a patch side that is no power of two: its patch rows come from aph_patchify_f16_win (padded to aph_patch_row_elems), not from the sampler's
// patch-major layouts.  The routing rule of the whole stack (ops.patchify / unpatchify, Engine) is this one predicate.
bool window_patch(int patch) { return (patch & (patch - 1)) != 0; }

// towers only the default f16 path serves: more than 256 tokens (the fp32 attention of vit_attn_f32.h stops there) or a window patch (the
// sampler's patch-major modes, which emit the [hi | lo] and fp32 operands, need a power-of-two patch)
int check_f16_only(const aph_vit* v, const char* who, const char* what) {
  if (v->T > 256) return aph_fail(APH_ERR_UNSUPPORTED, "%s: %s is not available for %d tokens per image (it stops at 256)", who, what, v->T);
  if (window_patch(v->patch))
    return aph_fail(APH_ERR_UNSUPPORTED, "%s: %s is not available for patch %d (not a power of two: patch rows of %d elements in %d, made by aph_patchify_f16_win)",
                    who, what, v->patch, 3 * v->patch * v->patch, v->Kp);
  return 0;
}

// a launch of the GEMM family, with its HIP event pair when the profile is on (bench.py roofline); flops = its algorithmic FLOPs
template <class F>
void vtimed(aph_vit* v, double flops, hipStream_t st, F&& launch) {
  if (!v->prof_on) { launch(); return; }
  if (v->prof_used + 2 > v->prof_ev.size()) {
    hipEvent_t a, b;
    APH_HIP(hipEventCreate(&a)); APH_HIP(hipEventCreate(&b));
    v->prof_ev.push_back(a); v->prof_ev.push_back(b);
  }
  APH_HIP(hipEventRecord(v->prof_ev[v->prof_used], st));
  launch();
  APH_HIP(hipEventRecord(v->prof_ev[v->prof_used + 1], st));
  v->prof_used += 2;
  v->prof_flops += flops;
}
// kdiv: the split-precision forward runs a GEMM over K = 2 x the algorithmic K (hi | lo operand against the weights repeated along K): the
// profile counts the ALGORITHMIC FLOPs (roofline.achieved is algorithmic work over measured time)
template <class Epi>
void vgemm(aph_vit* v, const half_t* A, int lda, const half_t* Bt, int ldb, int M, int N, int K, Epi epi, hipStream_t st, int kdiv = 1) {
  vtimed(v, 2.0 * M * N * K / kdiv, st, [&] { launch_gemm(A, lda, Bt, ldb, M, N, K, epi, st, &v->sk); });
}

// the exact path's GEMMs (vit_gemm_f32.h), timed like vgemm
template <class Epi>
void vgemm32(aph_vit* v, const float* A, int lda, const float* Bt, int ldb, int M, int N, int K, Epi epi, hipStream_t st, int a_rowP = 0) {
  vtimed(v, 2.0 * M * N * K, st, [&] { launch_gemm_f32(A, lda, Bt, ldb, M, N, K, epi, st, &v->f32sp, a_rowP); });
}

inline AttnArgs attn_args(aph_vit* v, const Layer& l, int S) {
  return AttnArgs{(const half_t*)l.qkv, l.att, l.lse, (const half_t*)v->datt, v->dqkv, S, v->T, v->heads};
}

}  // namespace

extern "C" {

// cfg mirrors clip.model.VisionTransformer(input_resolution, patch_size, width, layers, heads, output_dim)
int aph_vit_create(int input_resolution, int patch_size, int width, int layers, int heads, int output_dim, int max_batch,
                   aph_vit** out) {
  APH_TRY
  if (!out) return aph_fail(APH_ERR_ARG, "aph_vit_create: null out");
  if (width % 256 || width > 1024 || heads * kHeadDim != width)
    return aph_fail(APH_ERR_UNSUPPORTED, "aph_vit_create: width %d / heads %d unsupported (need head dim 64, width in {256,512,768,1024})", width, heads);
  // a power-of-two patch goes through the sampler's patch-major layouts, whose rows are 3 patch^2 elements and never padded: such a tower
  // needs 3 patch^2 % 128 == 0 as it always did (patch 8 and below stay refused); any other patch side gets padded rows (window_patch)
  if (patch_size < 1 || patch_size > 64 || input_resolution % patch_size || (!window_patch(patch_size) && (3 * patch_size * patch_size) % 128) ||
      output_dim < 1 || layers < 1 || max_batch < 1)
    return aph_fail(APH_ERR_UNSUPPORTED, "aph_vit_create: resolution %d / patch %d unsupported", input_resolution, patch_size);
  auto* v = new aph_vit();
  v->res = input_resolution; v->patch = patch_size; v->D = width; v->L = layers; v->heads = heads; v->E = output_dim;
  const int g = input_resolution / patch_size;
  v->P = g * g; v->T = v->P + 1; v->Kp = aph_patch_row_elems(patch_size); v->max_batch = max_batch;      // (padded to a multiple of 128: zero weight columns)
  // Tokens per image: the five-block attention (256 < T <= AT_TMAX) is admitted for the towers this library did not build before -- those
  // whose patch side is no power of two (ViT-L/14).  A power-of-two-patch tower keeps the limit of 256 it has always had: what was refused
  // stays refused (tests/test_gpu_kernels.py::test_vit_sequence_lengths[256] pins res 256 / patch 16), and its exact, split-precision and
  // f16-gradient modes stop at 256 tokens anyway.
  const int t_max = window_patch(patch_size) ? AT_TMAX : 256;
  if (v->T > t_max) { delete v; return aph_fail(APH_ERR_UNSUPPORTED, "aph_vit_create: %d tokens per image not supported", v->T); }
  v->layers.resize(layers);
  build_weights(v);
  if (const int rc = alloc_arena("aph_vit_create", &v->arena, &v->arena_bytes, [&](char* base) { return carve(v, base); })) { delete v; return rc; }
  *out = v;
  return APH_OK;
  APH_CATCH
}

int aph_vit_destroy(aph_vit* v) {
  if (!v) return APH_OK;
  for (hipEvent_t e : v->prof_ev) (void)hipEventDestroy(e);
  (void)hipFree(v->arena);
  if (v->arena_hilo) (void)hipFree(v->arena_hilo);
  if (v->arena_f32) (void)hipFree(v->arena_f32);
  delete v;
  return APH_OK;
}

// [r6] Allocates and fills the K-repeated weight copies aph_vit_forward_hilo multiplies [hi | lo] activation rows with (85 MB at ViT-B/32).
// Call once, after the weights are loaded and outside any stream capture (it allocates and copies synchronously); idempotent.  The default
// path (aph_vit_forward: f16 operands everywhere) never needs it -- round 5 carried these copies in every handle.
int aph_vit_enable_hilo(aph_vit* v) {
  APH_TRY
  if (!v) return aph_fail(APH_ERR_ARG, "aph_vit_enable_hilo: null handle");
  if (v->arena_hilo) return APH_OK;
  if (const int rc = check_f16_only(v, "aph_vit_enable_hilo", "the split-precision forward")) return rc;
  if (const int rc = check_loaded(v->weights, "aph_vit_enable_hilo")) return rc;
  return alloc_arena("aph_vit_enable_hilo", &v->arena_hilo, &v->arena_hilo_bytes, [&](char* base) { return carve_hilo(v, base); }, [&] {
    int rc = 0;
    for (const Weight& w : v->weights)
      if (w.rep) rc |= upload_f16_twice(*w.rep, w.host.data(), w.rows, w.cols);
    return rc || hipDeviceSynchronize() != hipSuccess;
  });
  APH_CATCH
}

// Allocates the exact path's arena (carve_f32) and fills its fp32 weights from the host fp32 copies aph_vit_set_weight keeps; a later
// aph_vit_set_weight refreshes them.  Once, after the weights are loaded and outside any stream capture (allocates and copies synchronously);
// idempotent.
int aph_vit_enable_f32(aph_vit* v) {
  APH_TRY
  if (!v) return aph_fail(APH_ERR_ARG, "aph_vit_enable_f32: null handle");
  if (v->arena_f32) return APH_OK;
  if (const int rc = check_f16_only(v, "aph_vit_enable_f32", "the exact fp32 path")) return rc;
  if (const int rc = check_loaded(v->weights, "aph_vit_enable_f32")) return rc;
  return alloc_arena("aph_vit_enable_f32", &v->arena_f32, &v->arena_f32_bytes, [&](char* base) { return carve_f32(v, base); }, [&] {
    int rc = 0;
    for (const Weight& w : v->weights) rc |= sync_f32(v, w);      // (reads v->arena_f32: alloc_arena has set it)
    return rc || hipDeviceSynchronize() != hipSuccess;
  });
  APH_CATCH
}

size_t aph_vit_workspace_bytes(const aph_vit* v) { return v ? v->arena_bytes + v->arena_hilo_bytes + v->arena_f32_bytes : 0; }

// Upload one tensor by its OpenAI checkpoint key (without the `visual.` prefix), fp32 host data.
// e.g. "conv1.weight", "transformer.resblocks.3.attn.in_proj_weight", "proj".
int aph_vit_set_weight(aph_vit* v, const char* name, const float* data, size_t count) {
  APH_TRY
  if (!v || !name || !data) return aph_fail(APH_ERR_ARG, "aph_vit_set_weight: null argument");
  Weight* w = find_weight(v->weights, name);
  if (!w) return aph_fail(APH_ERR_ARG, "aph_vit_set_weight: unknown key %s", name);
  const size_t rows = w->rows, cols = w->cols;
  const bool conv1 = w->key == "conv1.weight";
  const size_t pp = (size_t)v->patch * v->patch, expect = conv1 ? rows * 3 * pp : rows * cols;      // (the checkpoint's conv1.weight has no pad columns)
  if (count != expect) return aph_fail(APH_ERR_ARG, "aph_vit_set_weight(%s): %zu elements, expected %zu", name, count, expect);
  std::vector<float> perm;
  if (conv1) {
    // [D, 3, p, p] (openai/CLIP) -> K order of the sampler's patch rows: pixel-major, channel fastest (sampler.hip patch_index); the pad
    // columns 3 p^2 .. Kp of a padded row (patch 14) are zero, in W and in the transposed copy made from it
    perm.assign(rows * cols, 0.f);
    for (size_t d = 0; d < rows; ++d)
      for (size_t c = 0; c < 3; ++c)
        for (size_t q = 0; q < pp; ++q) perm[d * cols + q * 3 + c] = data[d * 3 * pp + c * pp + q];
    data = perm.data();
    count = rows * cols;
  }
  int rc = 0;
  if (w->h16[0]) {
    rc = upload_f16(*w->h16[0], data, rows, cols, false) | upload_f16(*w->h16[1], data, rows, cols, true);
    if (w->rep && *w->rep) rc |= upload_f16_twice(*w->rep, data, rows, cols);
  } else {
    rc = upload_f32(*w->f32[0], data, rows, cols, false);
    if (w->f32[1]) rc |= upload_f32(*w->f32[1], data, rows, cols, true);
  }
  if (w->h16[0]) {          // the source of the copies the enable calls allocate later
    w->host.assign(data, data + count);
    rc |= sync_f32(v, *w);
  }
  if (rc) return aph_fail(APH_ERR_HIP, "aph_vit_set_weight(%s): upload failed", name);
  w->set = true;
  return APH_OK;
  APH_CATCH
}

// encode_image: d_patches f16 [S*P, Kp] (patch-major, CLIP-normalised; Kp = aph_patch_row_elems(patch)) -> d_enc f32 [S, output_dim]
// hilo: the SPLIT-PRECISION forward -- d_patches rows are [hi (Kp) | lo (Kp)] (APH_OUT_PATCH_F16_HILO) and the first LayerNorm of every
// block writes [hi (D) | lo (D)]: the patch-embedding and the QKV GEMMs then run over K = 2 Kp / 2 D against the weights repeated along K,
// i.e. with ~22 operand bits on the two activations whose f16 rounding dominates the input-gradient error on weights with realistic
// dynamic range (profiles/r04_precision_attribution.txt).  Everything else, the backward included, is unchanged.
static int vit_forward_impl(aph_vit* v, const void* d_patches, int S, float* d_enc, bool hilo, void* stream_) {
  if (const int rc = check_call(v, d_patches, d_enc, S, "aph_vit_forward")) return rc;
  if (hilo && !v->arena_hilo)
    return aph_fail(APH_ERR_ARG, "aph_vit_forward_hilo: call aph_vit_enable_hilo(vit) once after loading the weights (the split-precision forward's "
                    "K-repeated weight copies are not allocated by default)");
  hipStream_t st = (hipStream_t)stream_;
  const int D = v->D, T = v->T, M = S * T, nv = D / 256;
  const int kx = hilo ? 2 : 1;
  v->sk.small_batch = M <= 128;   // see gemm_rs_mode(): the split-K small-M kernel only when the whole batch is small
  vgemm(v, (const half_t*)d_patches, kx * v->Kp, hilo ? v->w_patch2 : v->w_patch, kx * v->Kp, S * v->P, D, kx * v->Kp, EpiPatchEmbed{v->x0, v->pos, D, v->P, T}, st, kx);
  const bool fuse = vit_fuse_ln() != 0;
  launch_ln_fwd<false, true>(nv, {.x = v->x0, .g = v->ln_pre_g, .b = v->ln_pre_b, .out = v->layers[0].x_in, .M = M, .T = T, .cls = v->cls, .pos = v->pos, .x_fill = v->x0,
                                  .g2 = fuse ? v->layers[0].ln1_g : nullptr, .b2 = fuse ? v->layers[0].ln1_b : nullptr, .out2 = fuse ? v->h : nullptr, .hilo = hilo ? 1 : 0}, st);
  for (int li = 0; li < v->L; ++li) {
    Layer& l = v->layers[li];
    float* x_next = li + 1 < v->L ? v->layers[li + 1].x_in : v->x_last;
    if (!(fuse && li == 0)) launch_ln_fwd<true, false>(nv, {.x = l.x_in, .g = l.ln1_g, .b = l.ln1_b, .out = v->h, .M = M, .T = T, .hilo = hilo ? 1 : 0}, st);
    if (hilo) {
      // [r5] the lo half reaches the Q and K columns only; the V columns are summed over the hi half of the [hi | lo] rows alone (the first D of
      // the 2 D columns of A and of [W | W]).  What the lo half repairs is the cancellation in h . W on weights whose residual stream carries
      // large common offsets: through Q and K that error is amplified by the softmax, through V it enters the block linearly next to the f16
      // rounding V is stored with anyway (CPU model, tools/precision_attribution.py: single-step gradient error 5.2e-4 through Q / K, 1.8e-4
      // through V; on the GPU the single-step errors of the two forms are equal, profiles/r05_split_qk_only_ab.txt).  At full batch this is ONE
      // launch of the wave-specialised kernel with two k-loop lengths (vit_gemm_ws.h).  Batches below that kernel's threshold are launch-bound,
      // not MFMA-bound: they keep the plain launch over [hi | lo] on all 3 D columns (V a little more exact than it needs to be; a second
      // launch per block would cost more than the shorter sums save: C1 726 -> 690 steps/s when it was tried).
      const EpiF16 eq{l.qkv, 3 * D, l.b_qkv};
      if (D % 128 == 0 && gemm_takes_ws(M, 2 * D, 3 * D, 2 * D)) {
        vtimed(v, 2.0 * M * 3 * D * D, st, [&] { launch_gemm_ws(v->h, 2 * D, l.w_qkv2, 2 * D, M, 3 * D, 2 * D, eq, st, nullptr, D, D); });
      } else {
        vgemm(v, v->h, 2 * D, l.w_qkv2, 2 * D, M, 3 * D, 2 * D, eq, st, 2);      // (launch-bound sizes: one launch, the lo half on every column)
      }
    } else {
      vgemm(v, v->h, D, l.w_qkv, D, M, 3 * D, D, EpiF16{l.qkv, 3 * D, l.b_qkv}, st);
    }
    launch_attn_fwd(attn_args(v, l, S), st);
    // Only the class token leaves the last block (VisionTransformer.forward: ln_post(x[:, 0, :])), so everything after
    // its attention runs on the S class rows alone: the same buffers addressed with a row pitch of T rows.
    const bool cls_only = li + 1 == v->L;
    const int Mr = cls_only ? S : M, rs = cls_only ? T : 1;
    vgemm(v, l.att, rs * D, l.w_o, D, Mr, D, D, EpiResidual{l.x_mid, l.x_in, rs * D, l.b_o}, st);
    launch_ln_fwd<true, false>(nv, {.x = l.x_mid, .g = l.ln2_g, .b = l.ln2_b, .out = v->h, .M = Mr, .T = T, .xs = rs}, st);
    vgemm(v, v->h, D, l.w_fc1, D, Mr, 4 * D, D, EpiGelu{l.u, v->gact, 4 * D, l.b_fc1}, st);
    vgemm(v, v->gact, 4 * D, l.w_fc2, 4 * D, Mr, D, 4 * D, EpiResidual{x_next, l.x_mid, rs * D, l.b_fc2}, st);
  }
  launch_head_fwd(v->x_last, v->ln_post_g, v->ln_post_b, v->proj, d_enc, S, T, D, v->E, st);
  v->last_fwd = 1;
  return aph_check_launch("aph_vit_forward");
}
int aph_vit_forward(aph_vit* v, const void* d_patches, int S, float* d_enc, void* stream_) {
  APH_TRY
  return vit_forward_impl(v, d_patches, S, d_enc, false, stream_);
  APH_CATCH
}
// d_patches_hilo f16 [S*P, 2 * 3*patch*patch] (APH_OUT_PATCH_F16_HILO rows [hi | lo])
int aph_vit_forward_hilo(aph_vit* v, const void* d_patches_hilo, int S, float* d_enc, void* stream_) {
  APH_TRY
  return vit_forward_impl(v, d_patches_hilo, S, d_enc, true, stream_);
  APH_CATCH
}

// input-gradient of the last aph_vit_forward: d_genc f32 [S, output_dim] (already multiplied by the caller's
// loss scale) -> d_patch_grad f32 [S*P, Kp] multiplied by out_scale (pass 1/loss_scale).
static int vit_backward_impl(aph_vit* v, const float* d_genc, int S, void* d_patch_grad, bool grad_f16, float out_scale, void* stream_) {
  if (const int rc = check_call(v, d_genc, d_patch_grad, S, "aph_vit_backward")) return rc;
  if (v->last_fwd == 2)
    return aph_fail(APH_ERR_ARG, "aph_vit_backward: the last forward was aph_vit_forward_f32 (exact path): take its gradient with aph_vit_backward_f32");
  hipStream_t st = (hipStream_t)stream_;
  const int D = v->D, T = v->T, M = S * T, nv = D / 256;
  v->sk.small_batch = M <= 128;   // see gemm_rs_mode(): the split-K small-M kernel only when the whole batch is small
  // only the class rows carry gradient out of the head: the fp32 stream starts from zero; dx16 needs no clearing -- the
  // last block reads and writes its class rows only (row pitch T), and its ln_1 backward rewrites every row
  const bool fuse = vit_fuse_ln() != 0;      // (then the last block's ln_1 backward takes its residual from the class rows only: no fill)
  const int s16 = (vit_grad_stream_f16() != 0 && fuse) ? 1 : 0;      // f16-only gradient stream (measurement switch; needs the fused LayerNorm pairs' row conventions)
  if (!fuse) zero_fill_async(v->dx, sizeof(float) * (size_t)M * D, st);            // (a kernel node, not a memset node: see zero_fill_async)
  APH_LAUNCH(head_bwd_kernel, dim3(S), dim3(D), sizeof(float) * v->E, st, d_genc, (const float*)v->x_last,
             (const float*)v->ln_post_g, (const float*)v->projT, v->dx, v->dx16, T, D, v->E);
  for (int li = v->L - 1; li >= 0; --li) {
    Layer& l = v->layers[li];
    const bool cls_only = li + 1 == v->L;          // see aph_vit_forward: the last block's MLP / out-proj saw class rows only
    const int Mr = cls_only ? S : M, rs = cls_only ? T : 1;
    if (cls_only) zero_fill_async(v->datt, sizeof(half_t) * (size_t)M * D, st);   // no gradient into the other rows' attention output
    vgemm(v, v->dx16, rs * D, l.w_fc2T, D, Mr, 4 * D, D, EpiGeluBwd{v->du, l.u, 4 * D}, st);
    vgemm(v, v->du, 4 * D, l.w_fc1T, 4 * D, Mr, D, 4 * D, EpiF16{v->dh, D, nullptr}, st);
    if (s16) launch_ln_bwd<true, false>(nv, {.dy = v->dh, .x = l.x_mid, .g = l.ln2_g, .res = v->dx16, .out16 = v->dx16, .M = Mr, .T = T, .xs = rs, .res_f16 = 1}, st);
    else launch_ln_bwd<true, false>(nv, {.dy = v->dh, .x = l.x_mid, .g = l.ln2_g, .res = v->dx, .out32 = v->dx, .out16 = v->dx16, .M = Mr, .T = T, .xs = rs}, st);
    vgemm(v, v->dx16, rs * D, l.w_oT, D, Mr, D, D, EpiF16{v->datt, rs * D, nullptr}, st);
    launch_attn_bwd(attn_args(v, l, S), st);
    vgemm(v, v->dqkv, 3 * D, l.w_qkvT, 3 * D, M, D, 3 * D, EpiF16{v->dh, D, nullptr}, st);
    if (fuse && li == 0)      // ln_1 backward and ln_pre backward as one kernel: writes the patch rows of dx0_16 only
      launch_ln_bwd<true, false>(nv, {.dy = v->dh, .x = l.x_in, .g = l.ln1_g, .res = s16 ? (const void*)v->dx16 : (const void*)v->dx, .out16 = v->dx0_16, .M = M, .T = T,
                                      .res_T = cls_only ? T : 0, .x_b = v->x0, .g_b = v->ln_pre_g, .res_f16 = s16}, st);
    else if (s16)
      launch_ln_bwd<true, false>(nv, {.dy = v->dh, .x = l.x_in, .g = l.ln1_g, .res = v->dx16, .out16 = v->dx16, .M = M, .T = T, .res_T = cls_only ? T : 0, .res_f16 = 1}, st);
    else
      launch_ln_bwd<true, false>(nv, {.dy = v->dh, .x = l.x_in, .g = l.ln1_g, .res = v->dx, .out32 = v->dx, .out16 = v->dx16, .M = M, .T = T, .res_T = (fuse && cls_only) ? T : 0}, st);
  }
  if (!fuse) launch_ln_bwd<false, true>(nv, {.dy = v->dx, .x = v->x0, .g = v->ln_pre_g, .out16 = v->dx0_16, .M = M, .T = T}, st);
  if (grad_f16) vgemm(v, v->dx0_16, D, v->w_patchT, D, S * v->P, v->Kp, D, EpiF16Scale{(half_t*)d_patch_grad, v->Kp, out_scale}, st);
  else vgemm(v, v->dx0_16, D, v->w_patchT, D, S * v->P, v->Kp, D, EpiF32{(float*)d_patch_grad, v->Kp, out_scale}, st);
  return aph_check_launch("aph_vit_backward");
}

int aph_vit_backward(aph_vit* v, const float* d_genc, int S, float* d_patch_grad, float out_scale, void* stream_) {
  APH_TRY
  return vit_backward_impl(v, d_genc, S, d_patch_grad, false, out_scale, stream_);
  APH_CATCH
}
int aph_vit_backward_h(aph_vit* v, const float* d_genc, int S, void* d_patch_grad_f16, float out_scale, void* stream_) {
  APH_TRY
  return vit_backward_impl(v, d_genc, S, d_patch_grad_f16, true, out_scale, stream_);
  APH_CATCH
}

// ---- exact path: fp32 operands everywhere, the f32-input MFMA GEMM (vit_gemm_f32.h), fp32 attention (vit_attn_f32.h), the fp32 LayerNorm
// kernels of the f16 path with fp32 outputs / gradients.  Same block structure as vit_forward_impl (the last block on its class rows only).

// d_patches f32 [S*P, 3*patch^2] (APH_OUT_PATCH_F32) -> d_enc f32 [S, output_dim]
int aph_vit_forward_f32(aph_vit* v, const float* d_patches, int S, float* d_enc, void* stream_) {
  APH_TRY
  if (const int rc = check_call(v, d_patches, d_enc, S, "aph_vit_forward_f32")) return rc;
  if (!v->arena_f32)
    return aph_fail(APH_ERR_ARG, "aph_vit_forward_f32: call aph_vit_enable_f32(vit) once after loading the weights (the exact path's fp32 weights "
                    "and activations are not allocated by default)");
  hipStream_t st = (hipStream_t)stream_;
  const int D = v->D, T = v->T, M = S * T, nv = D / 256;
  vgemm32(v, d_patches, v->Kp, v->w_patch32, v->Kp, S * v->P, D, v->Kp, EpiPatchEmbed{v->x0, v->pos, D, v->P, T}, st);
  launch_ln_fwd<false, true>(nv, {.x = v->x0, .g = v->ln_pre_g, .b = v->ln_pre_b, .out = v->layers[0].x_in, .M = M, .T = T, .cls = v->cls, .pos = v->pos, .x_fill = v->x0}, st);
  for (int li = 0; li < v->L; ++li) {
    Layer& l = v->layers[li];
    float* x_next = li + 1 < v->L ? v->layers[li + 1].x_in : v->x_last;
    launch_ln_fwd<false, false>(nv, {.x = l.x_in, .g = l.ln1_g, .b = l.ln1_b, .out = v->h32, .M = M, .T = T}, st);
    vgemm32(v, v->h32, D, l.w_qkv32, D, M, 3 * D, D, EpiBiasF32{l.qkv32, 3 * D, l.b_qkv}, st);
    launch_attn_fwd_f32(l.qkv32, v->att32, l.lse, S, T, v->heads, st);
    const bool cls_only = li + 1 == v->L;
    const int Mr = cls_only ? S : M, rs = cls_only ? T : 1;
    vgemm32(v, v->att32, rs * D, l.w_o32, D, Mr, D, D, EpiResidual{l.x_mid, l.x_in, rs * D, l.b_o}, st);
    launch_ln_fwd<false, false>(nv, {.x = l.x_mid, .g = l.ln2_g, .b = l.ln2_b, .out = v->h32, .M = Mr, .T = T, .xs = rs}, st);
    vgemm32(v, v->h32, D, l.w_fc1_32, D, Mr, 4 * D, D, EpiGeluF32{l.dg32, v->g32, 4 * D, l.b_fc1}, st);
    vgemm32(v, v->g32, 4 * D, l.w_fc2_32, 4 * D, Mr, D, 4 * D, EpiResidual{x_next, l.x_mid, rs * D, l.b_fc2}, st);
  }
  launch_head_fwd(v->x_last, v->ln_post_g, v->ln_post_b, v->proj, d_enc, S, T, D, v->E, st);
  v->last_fwd = 2;
  return aph_check_launch("aph_vit_forward_f32");
  APH_CATCH
}

// input-gradient of the last aph_vit_forward_f32: d_genc f32 [S, output_dim] -> d_patch_grad f32 [S*P, 3*patch^2] x out_scale.  The gradient
// stream is fp32 end to end (no f16 copies); a power-of-two loss scale on d_genc and its inverse in out_scale are exact.
int aph_vit_backward_f32(aph_vit* v, const float* d_genc, int S, float* d_patch_grad, float out_scale, void* stream_) {
  APH_TRY
  if (const int rc = check_call(v, d_genc, d_patch_grad, S, "aph_vit_backward_f32")) return rc;
  if (v->last_fwd != 2 || !v->arena_f32)
    return aph_fail(APH_ERR_ARG, "aph_vit_backward_f32: the last forward was not aph_vit_forward_f32 (run the exact forward first; the f16 "
                    "forward's gradient is aph_vit_backward)");
  hipStream_t st = (hipStream_t)stream_;
  const int D = v->D, T = v->T, M = S * T, nv = D / 256;
  float* dh = v->h32;          // gradient w.r.t. a LayerNorm output [M, D]
  float* du = v->g32;          // gradient w.r.t. the fc1 pre-activation [M, 4D]
  // class rows of dx (the gradient w.r.t. the last block's output); the f16 copy the kernel also writes is not read here
  APH_LAUNCH(head_bwd_kernel, dim3(S), dim3(D), sizeof(float) * v->E, st, d_genc, (const float*)v->x_last,
             (const float*)v->ln_post_g, (const float*)v->projT, v->dx, v->dx16, T, D, v->E);
  for (int li = v->L - 1; li >= 0; --li) {
    Layer& l = v->layers[li];
    const bool cls_only = li + 1 == v->L;
    const int Mr = cls_only ? S : M, rs = cls_only ? T : 1;
    if (cls_only) zero_fill_async(v->datt32, sizeof(float) * (size_t)M * D, st);      // no gradient into the other rows' attention output
    vgemm32(v, v->dx, rs * D, l.w_fc2T32, D, Mr, 4 * D, D, EpiGeluBwdF32{du, l.dg32, 4 * D}, st);
    vgemm32(v, du, 4 * D, l.w_fc1T32, 4 * D, Mr, D, 4 * D, EpiF32{dh, D, 1.0f}, st);
    launch_ln_bwd<false, false>(nv, {.dy = dh, .x = l.x_mid, .g = l.ln2_g, .res = v->dx, .out32 = v->dx, .M = Mr, .T = T, .xs = rs}, st);
    vgemm32(v, v->dx, rs * D, l.w_oT32, D, Mr, D, D, EpiF32{v->datt32, rs * D, 1.0f}, st);
    launch_attn_bwd_f32(l.qkv32, v->datt32, l.lse, v->delta32, v->dqkv32, S, T, v->heads, st);
    vgemm32(v, v->dqkv32, 3 * D, l.w_qkvT32, 3 * D, M, D, 3 * D, EpiF32{dh, D, 1.0f}, st);
    // the last block's residual reaches its class rows only (res_T = T): the other rows of dx are not read before this writes them
    launch_ln_bwd<false, false>(nv, {.dy = dh, .x = l.x_in, .g = l.ln1_g, .res = v->dx, .out32 = v->dx, .M = M, .T = T, .res_T = cls_only ? T : 0}, st);
  }
  // ln_pre backward into dh (token rows), then the patch-embedding dgrad over its patch rows (row s*P + p <- token row s*T + 1 + p)
  launch_ln_bwd<false, false>(nv, {.dy = v->dx, .x = v->x0, .g = v->ln_pre_g, .out32 = dh, .M = M, .T = T}, st);
  vgemm32(v, dh, D, v->w_patchT32, D, S * v->P, v->Kp, D, EpiF32{d_patch_grad, v->Kp, out_scale}, st, v->P);
  return aph_check_launch("aph_vit_backward_f32");
  APH_CATCH
}

// GEMM-family timing for bench.py: enable, run steps, then read {sum of launch durations [ms], launches, flops}
int aph_vit_profile(aph_vit* v, int on) {
  APH_TRY
  if (!v) return aph_fail(APH_ERR_ARG, "aph_vit_profile: null handle");
  v->prof_on = on != 0;
  v->prof_used = 0;
  v->prof_flops = 0.0;
  return APH_OK;
  APH_CATCH
}
int aph_vit_profile_read(aph_vit* v, double* ms_total, long long* launches, double* flops) {
  APH_TRY
  if (!v || !ms_total || !launches || !flops) return aph_fail(APH_ERR_ARG, "aph_vit_profile_read: null argument");
  double total = 0.0;
  for (size_t i = 0; i + 1 < v->prof_used; i += 2) {
    if (hipEventSynchronize(v->prof_ev[i + 1]) != hipSuccess) return aph_fail(APH_ERR_HIP, "aph_vit_profile_read: event sync failed");
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, v->prof_ev[i], v->prof_ev[i + 1]) != hipSuccess) return aph_fail(APH_ERR_HIP, "aph_vit_profile_read: elapsed failed");
    total += ms;
  }
  *ms_total = total; *launches = (long long)(v->prof_used / 2); *flops = v->prof_flops;
  return APH_OK;
  APH_CATCH
}

}  // extern "C"
