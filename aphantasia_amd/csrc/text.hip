// CLIP text tower: `model.encode_text(tokens)` forward (clip_fft.py:119 and wherever a prompt becomes a target embedding).  fp32 throughout --
// the exact path's kernels: the f32-input MFMA GEMM (vit_gemm_f32.h), the fp32 LayerNorm (vit_ops.h) and the fp32 attention in its causal
// instantiation (vit_attn_f32.h) -- plus the token embedding and the head below.  No backward (a prompt is a constant of the optimisation),
// so the weights are the fp32 [N, K] matrices alone: no transposes, no f16 copies, no stash.  The tower runs once per prompt.
// Follows openai/CLIP clip/model.py CLIP.encode_text (tests/text_ref.py is the restatement it is tested against).
#include <string>

#include "aph_device.h"
#include "aph_host.h"
#include "tower_store.h"
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

}  // namespace

struct aph_text {
  int ctx, vocab, D, L, heads, E, max_batch;
  float *tok = nullptr, *pos = nullptr, *lnf_g = nullptr, *lnf_b = nullptr, *proj = nullptr;
  std::vector<TextLayer> layers;
  float *x = nullptr, *x_mid = nullptr, *h = nullptr, *qkv = nullptr, *att = nullptr, *g = nullptr, *lse = nullptr;      // activations of one forward
  std::vector<Weight> weights;         // every checkpoint tensor (tower_store.h): fp32 entries, keys at the checkpoint's top level (no prefix)
  char* arena = nullptr;
  size_t arena_bytes = 0;
};

namespace {

void text_build_weights(aph_text* v) {
  const size_t D = v->D;
  std::vector<Weight>& t = v->weights;
  add_f32(t, "token_embedding.weight", v->vocab, D, &v->tok);
  add_f32(t, "positional_embedding", v->ctx, D, &v->pos);
  add_f32(t, "ln_final.weight", 1, D, &v->lnf_g); add_f32(t, "ln_final.bias", 1, D, &v->lnf_b);
  add_f32(t, "text_projection", D, v->E, &v->proj);
  for (int li = 0; li < v->L; ++li) {
    TextLayer& l = v->layers[li];
    const std::string p = "transformer.resblocks." + std::to_string(li) + ".";
    add_f32(t, p + "attn.in_proj_weight", 3 * D, D, &l.w_qkv); add_f32(t, p + "attn.in_proj_bias", 1, 3 * D, &l.b_qkv);
    add_f32(t, p + "attn.out_proj.weight", D, D, &l.w_o); add_f32(t, p + "attn.out_proj.bias", 1, D, &l.b_o);
    add_f32(t, p + "mlp.c_fc.weight", 4 * D, D, &l.w_fc1); add_f32(t, p + "mlp.c_fc.bias", 1, 4 * D, &l.b_fc1);
    add_f32(t, p + "mlp.c_proj.weight", D, 4 * D, &l.w_fc2); add_f32(t, p + "mlp.c_proj.bias", 1, D, &l.b_fc2);
    add_f32(t, p + "ln_1.weight", 1, D, &l.ln1_g); add_f32(t, p + "ln_1.bias", 1, D, &l.ln1_b);
    add_f32(t, p + "ln_2.weight", 1, D, &l.ln2_g); add_f32(t, p + "ln_2.bias", 1, D, &l.ln2_b);
  }
}

// every weight in table order, then the activations of max_batch prompts; returns the size (base == nullptr: null pointers, the size alone)
size_t text_carve(aph_text* v, char* base) {
  Carver c{base};
  carve_weights(v->weights, c, 0, v->weights.size(), ARENA_MAIN);
  const size_t D = v->D, Mx = (size_t)v->max_batch * v->ctx;
  v->x = c.take<float>(Mx * D); v->x_mid = c.take<float>(Mx * D); v->h = c.take<float>(Mx * D);
  v->qkv = c.take<float>(Mx * 3 * D); v->att = c.take<float>(Mx * D); v->g = c.take<float>(Mx * 4 * D);
  v->lse = c.take<float>((size_t)v->max_batch * v->heads * v->ctx);
  return c.off;
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
  if (const int rc = alloc_arena("aph_text_create", &v->arena, &v->arena_bytes, [&](char* base) { return text_carve(v, base); })) { delete v; return rc; }
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
  Weight* w = find_weight(v->weights, name);
  if (!w) return aph_fail(APH_ERR_ARG, "aph_text_set_weight: unknown key %s", name);
  if (count != w->rows * w->cols) return aph_fail(APH_ERR_ARG, "aph_text_set_weight(%s): %zu elements, expected %zu", name, count, w->rows * w->cols);
  if (upload_f32(*w->f32[0], data, w->rows, w->cols, false)) return aph_fail(APH_ERR_HIP, "aph_text_set_weight(%s): upload failed", name);
  w->set = true;
  return APH_OK;
  APH_CATCH
}

// encode_text: d_tokens int32 [S, context_length] (device) -> d_enc f32 [S, output_dim].  The block structure of aph_vit_forward_f32 with the
// causal attention; every block on all rows.  No GEMM is split over k (no workspace is handed to launch_gemm_f32): the order of every sum is
// the same for any S.
int aph_text_forward(aph_text* v, const int32_t* d_tokens, int S, float* d_enc, void* stream_) {
  APH_TRY
  if (const int rc = check_call(v, d_tokens, d_enc, S, "aph_text_forward")) return rc;
  hipStream_t st = (hipStream_t)stream_;
  const int D = v->D, T = v->ctx, M = S * T, nv = D / 256;
  const size_t n4 = (size_t)M * (D / 4);
  APH_LAUNCH(text_embed_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, d_tokens, (const float*)v->tok, (const float*)v->pos, v->x, M, T,
             v->vocab, D);
  for (int li = 0; li < v->L; ++li) {
    const TextLayer& l = v->layers[li];
    launch_ln_fwd<false, false>(nv, {.x = v->x, .g = l.ln1_g, .b = l.ln1_b, .out = v->h, .M = M, .T = T}, st);
    launch_gemm_f32(v->h, D, l.w_qkv, D, M, 3 * D, D, EpiBiasF32{v->qkv, 3 * D, l.b_qkv}, st, nullptr);
    launch_attn_fwd_f32<true>(v->qkv, v->att, v->lse, S, T, v->heads, st);
    launch_gemm_f32(v->att, D, l.w_o, D, M, D, D, EpiResidual{v->x_mid, v->x, D, l.b_o}, st, nullptr);
    launch_ln_fwd<false, false>(nv, {.x = v->x_mid, .g = l.ln2_g, .b = l.ln2_b, .out = v->h, .M = M, .T = T}, st);
    launch_gemm_f32(v->h, D, l.w_fc1, D, M, 4 * D, D, EpiGeluFwdF32{v->g, 4 * D, l.b_fc1}, st, nullptr);
    launch_gemm_f32(v->g, 4 * D, l.w_fc2, 4 * D, M, D, 4 * D, EpiResidual{v->x, v->x_mid, D, l.b_fc2}, st, nullptr);
  }
  APH_LAUNCH(text_head_kernel, dim3(S), dim3(256), sizeof(float) * D, st, d_tokens, (const float*)v->x, (const float*)v->lnf_g, (const float*)v->lnf_b,
             (const float*)v->proj, d_enc, T, v->vocab, D, v->E);
  return aph_check_launch("aph_text_forward");
  APH_CATCH
}

}  // extern "C"
