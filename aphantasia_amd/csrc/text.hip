// CLIP text tower: `model.encode_text(tokens)` forward (clip_fft.py:119 and wherever a prompt becomes a target embedding).  fp32 throughout --
// the exact path's kernels: the f32-input MFMA GEMM (vit_gemm_f32.h), the fp32 LayerNorm (vit_ops.h) and the fp32 attention in its causal
// instantiation (vit_attn_f32.h) -- plus the token embedding and the head below.  No backward (a prompt is a constant of the optimisation),
// so the weights are the fp32 [N, K] matrices alone: no transposes, no f16 copies, no stash.  The tower runs once per prompt.
// Follows openai/CLIP clip/model.py CLIP.encode_text (tests/text_ref.py is the restatement it is tested against).
#include <string>

#include "aph_device.h"
#include "aph_host.h"
#include "vit_gemm.h"
#include "vit_ops.h"
#include "vit_gemm_f32.h"
#include "vit_attn_f32.h"

using namespace aph;

namespace {

// x[s, t, :] = token_embedding[ids[s, t], :] + positional_embedding[t, :]; a thread per four features.  An id outside [0, vocab) is clamped
// into it: no id reads out of bounds (the Python layer refuses such ids before they are uploaded).
__global__ __launch_bounds__(256) void text_embed_kernel(const int32_t* __restrict__ ids, const float* __restrict__ tok, const float* __restrict__ pos,
                                                         float* __restrict__ x, int M, int ctx, int vocab, int D) {
  const int d4 = D >> 2;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)M * d4) return;
  const int m = (int)(idx / d4), d = (int)(idx - (size_t)m * d4) * 4, t = m % ctx;
  int id = ids[m];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  st4(x + (size_t)m * D + d, ld4(tok + (size_t)id * D + d) + ld4(pos + (size_t)t * D + d));
}

// enc[s, :] = LN(x[s, eot_s, :]; gamma, beta) @ proj  (proj [D, E]), eot_s = the first position of the largest (clamped) id of sequence s --
// upstream's text.argmax(dim=-1).  One workgroup per prompt; every output is one thread's d-ordered fmaf chain, so a prompt's embedding does
// not depend on the batch it is in.
__global__ __launch_bounds__(256) void text_head_kernel(const int32_t* __restrict__ ids, const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const float* __restrict__ proj, float* __restrict__ enc,
                                                        int ctx, int vocab, int D, int E) {
  APH_DYN_SMEM(smem);
  float* y = reinterpret_cast<float*>(smem);      // [D]
  __shared__ float red[16];
  const int s = blockIdx.x;
  int eot = 0, best = -1;
  for (int t = 0; t < ctx; ++t) {
    int id = ids[(size_t)s * ctx + t];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    if (id > best) { best = id; eot = t; }
  }
  const float* row = x + ((size_t)s * ctx + eot) * D;
  float a = 0.f;
  for (int d = threadIdx.x; d < D; d += blockDim.x) a += row[d];
  const float mean = block_sum(a, red) / D;
  float q = 0.f;
  for (int d = threadIdx.x; d < D; d += blockDim.x) { const float c = row[d] - mean; q += c * c; }
  const float rstd = rsqrtf(block_sum(q, red) / D + kLnEps);
  for (int d = threadIdx.x; d < D; d += blockDim.x) y[d] = (row[d] - mean) * rstd * gamma[d] + beta[d];
  __syncthreads();
  for (int e = threadIdx.x; e < E; e += blockDim.x) {
    float acc = 0.f;
    for (int d = 0; d < D; ++d) acc = fmaf(y[d], proj[(size_t)d * E + e], acc);
    enc[(size_t)s * E + e] = acc;
  }
}

// fc1's epilogue without the derivative the ViT's backward wants: out = QuickGELU(acc + bias)
struct EpiGeluFwdF32 {
  float* g; int ldo; const float* bias;
  __device__ __forceinline__ void apply8(int m, int n, f32x4 a, f32x4 b) const {
    a += ld4(bias + n); b += ld4(bias + n + 4);
    f32x4 ga, da, gb, db;
    quick_gelu4_f32(a, ga, da);
    quick_gelu4_f32(b, gb, db);
    const size_t o = (size_t)m * ldo + n;
    st4(g + o, ga); st4(g + o + 4, gb);
  }
};

struct TextLayer {
  float *w_qkv = nullptr, *w_o = nullptr, *w_fc1 = nullptr, *w_fc2 = nullptr;
  float *b_qkv = nullptr, *b_o = nullptr, *b_fc1 = nullptr, *b_fc2 = nullptr;
  float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
};
struct TextWeight {
  std::string key;            // OpenAI checkpoint key (top level: the text tower has no prefix)
  size_t count;
  float** dst;
  bool set = false;
};

}  // namespace

struct aph_text {
  int ctx, vocab, D, L, heads, E, max_batch;
  float *tok = nullptr, *pos = nullptr, *lnf_g = nullptr, *lnf_b = nullptr, *proj = nullptr;
  std::vector<TextLayer> layers;
  float *x = nullptr, *x_mid = nullptr, *h = nullptr, *qkv = nullptr, *att = nullptr, *g = nullptr, *lse = nullptr;      // activations of one forward
  std::vector<TextWeight> weights;
  char* arena = nullptr;
  size_t arena_bytes = 0;
};

namespace {

void text_build_weights(aph_text* v) {
  const size_t D = v->D;
  auto add = [&](std::string key, size_t count, float** dst) { v->weights.push_back(TextWeight{std::move(key), count, dst}); };
  add("token_embedding.weight", (size_t)v->vocab * D, &v->tok);
  add("positional_embedding", (size_t)v->ctx * D, &v->pos);
  add("ln_final.weight", D, &v->lnf_g); add("ln_final.bias", D, &v->lnf_b);
  add("text_projection", D * v->E, &v->proj);
  for (int li = 0; li < v->L; ++li) {
    TextLayer& l = v->layers[li];
    const std::string p = "transformer.resblocks." + std::to_string(li) + ".";
    add(p + "attn.in_proj_weight", 3 * D * D, &l.w_qkv); add(p + "attn.in_proj_bias", 3 * D, &l.b_qkv);
    add(p + "attn.out_proj.weight", D * D, &l.w_o); add(p + "attn.out_proj.bias", D, &l.b_o);
    add(p + "mlp.c_fc.weight", 4 * D * D, &l.w_fc1); add(p + "mlp.c_fc.bias", 4 * D, &l.b_fc1);
    add(p + "mlp.c_proj.weight", 4 * D * D, &l.w_fc2); add(p + "mlp.c_proj.bias", D, &l.b_fc2);
    add(p + "ln_1.weight", D, &l.ln1_g); add(p + "ln_1.bias", D, &l.ln1_b);
    add(p + "ln_2.weight", D, &l.ln2_g); add(p + "ln_2.bias", D, &l.ln2_b);
  }
}

// every weight in table order, then the activations of max_batch prompts; base == nullptr: sizes only
size_t text_carve(aph_text* v, char* base) {
  size_t off = 0;
  auto take = [&](size_t n) {
    float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
    off += (n * sizeof(float) + 255) & ~(size_t)255;
    return p;
  };
  for (TextWeight& w : v->weights) *w.dst = take(w.count);
  const size_t D = v->D, Mx = (size_t)v->max_batch * v->ctx;
  v->x = take(Mx * D); v->x_mid = take(Mx * D); v->h = take(Mx * D);
  v->qkv = take(Mx * 3 * D); v->att = take(Mx * D); v->g = take(Mx * 4 * D);
  v->lse = take((size_t)v->max_batch * v->heads * v->ctx);
  return off;
}

}  // namespace

extern "C" {

// cfg mirrors the text half of clip.model.CLIP(embed_dim, ..., context_length, vocab_size, transformer_width, transformer_heads, transformer_layers)
int aph_text_create(int context_length, int vocab_size, int width, int layers, int heads, int output_dim, int max_batch, aph_text** out) {
  APH_TRY
  if (!out) return aph_fail(APH_ERR_ARG, "aph_text_create: null out");
  if (width < 256 || width % 256 || width > 1024)
    return aph_fail(APH_ERR_UNSUPPORTED, "aph_text_create: width %d unsupported (the LayerNorm kernel takes a multiple of 256 up to 1024)", width);
  if (heads < 1 || heads * kHeadDim != width)
    return aph_fail(APH_ERR_UNSUPPORTED, "aph_text_create: width %d / heads %d unsupported (need head dim 64: width == 64 * heads)", width, heads);
  if (context_length < 1 || context_length > 256)
    return aph_fail(APH_ERR_UNSUPPORTED, "aph_text_create: context length %d unsupported (the fp32 attention holds 1 .. 256 tokens)", context_length);
  if (vocab_size < 1 || layers < 1 || output_dim < 1 || max_batch < 1)
    return aph_fail(APH_ERR_ARG, "aph_text_create: vocab %d / layers %d / output_dim %d / max_batch %d must be positive", vocab_size, layers, output_dim,
                    max_batch);
  auto* v = new aph_text();
  v->ctx = context_length; v->vocab = vocab_size; v->D = width; v->L = layers; v->heads = heads; v->E = output_dim; v->max_batch = max_batch;
  v->layers.resize(layers);
  text_build_weights(v);
  const size_t total = text_carve(v, nullptr);
  const hipError_t me = hipMalloc((void**)&v->arena, total);
  if (me != hipSuccess) { delete v; return aph_fail(APH_ERR_HIP, "aph_text_create: cannot allocate %zu bytes (%s)", total, hipGetErrorString(me)); }
  v->arena_bytes = total;
  text_carve(v, v->arena);
  *out = v;
  return APH_OK;
  APH_CATCH
}

int aph_text_destroy(aph_text* v) {
  if (!v) return APH_OK;
  (void)hipFree(v->arena);
  delete v;
  return APH_OK;
}

size_t aph_text_workspace_bytes(const aph_text* v) { return v ? v->arena_bytes : 0; }

// one tensor by its OpenAI checkpoint key (fp32 host data, the checkpoint's own layout: matrices [N, K], text_projection [width, output_dim])
int aph_text_set_weight(aph_text* v, const char* name, const float* data, size_t count) {
  APH_TRY
  if (!v || !name || !data) return aph_fail(APH_ERR_ARG, "aph_text_set_weight: null argument");
  TextWeight* w = nullptr;
  for (TextWeight& e : v->weights)
    if (e.key == name) { w = &e; break; }
  if (!w) return aph_fail(APH_ERR_ARG, "aph_text_set_weight: unknown key %s", name);
  if (count != w->count) return aph_fail(APH_ERR_ARG, "aph_text_set_weight(%s): %zu elements, expected %zu", name, count, w->count);
  if (hipMemcpy(*w->dst, data, count * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
    return aph_fail(APH_ERR_HIP, "aph_text_set_weight(%s): upload failed", name);
  w->set = true;
  return APH_OK;
  APH_CATCH
}

// encode_text: d_tokens int32 [S, context_length] (device) -> d_enc f32 [S, output_dim].  The block structure of aph_vit_forward_f32 with the
// causal attention; every block on all rows.  No GEMM is split over k (no workspace is handed to launch_gemm_f32): the order of every sum is
// the same for any S.
int aph_text_forward(aph_text* v, const int32_t* d_tokens, int S, float* d_enc, void* stream_) {
  APH_TRY
  if (!v || !d_tokens || !d_enc) return aph_fail(APH_ERR_ARG, "aph_text_forward: null argument");
  if (S < 1 || S > v->max_batch) return aph_fail(APH_ERR_ARG, "aph_text_forward: batch %d outside 1..%d", S, v->max_batch);
  int n = 0;
  for (const TextWeight& w : v->weights) n += w.set;
  if (n != (int)v->weights.size()) return aph_fail(APH_ERR_ARG, "aph_text_forward: weights not fully loaded (%d of %zu tensors)", n, v->weights.size());
  hipStream_t st = (hipStream_t)stream_;
  const int D = v->D, T = v->ctx, M = S * T, nv = D / 256;
  const size_t n4 = (size_t)M * (D / 4);
  APH_LAUNCH(text_embed_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, d_tokens, (const float*)v->tok, (const float*)v->pos, v->x, M, T,
             v->vocab, D);
  for (int li = 0; li < v->L; ++li) {
    const TextLayer& l = v->layers[li];
    launch_ln_fwd<false, false>(nv, v->x, l.ln1_g, l.ln1_b, v->h, M, T, nullptr, nullptr, nullptr, st);
    launch_gemm_f32(v->h, D, l.w_qkv, D, M, 3 * D, D, EpiBiasF32{v->qkv, 3 * D, l.b_qkv}, st, nullptr);
    launch_attn_fwd_f32<true>(v->qkv, v->att, v->lse, S, T, v->heads, st);
    launch_gemm_f32(v->att, D, l.w_o, D, M, D, D, EpiResidual{v->x_mid, v->x, D, l.b_o}, st, nullptr);
    launch_ln_fwd<false, false>(nv, v->x_mid, l.ln2_g, l.ln2_b, v->h, M, T, nullptr, nullptr, nullptr, st);
    launch_gemm_f32(v->h, D, l.w_fc1, D, M, 4 * D, D, EpiGeluFwdF32{v->g, 4 * D, l.b_fc1}, st, nullptr);
    launch_gemm_f32(v->g, 4 * D, l.w_fc2, 4 * D, M, D, 4 * D, EpiResidual{v->x, v->x_mid, D, l.b_fc2}, st, nullptr);
  }
  APH_LAUNCH(text_head_kernel, dim3(S), dim3(256), sizeof(float) * D, st, d_tokens, (const float*)v->x, (const float*)v->lnf_g, (const float*)v->lnf_b,
             (const float*)v->proj, d_enc, T, v->vocab, D, v->E);
  return aph_check_launch("aph_text_forward");
  APH_CATCH
}

}  // extern "C"
