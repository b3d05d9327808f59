// Host side of a tower's device memory, shared by the image tower (vit.hip) and the text tower (text.hip): the table of checkpoint tensors
// with every device copy of each, the carving of an arena into 256-byte-aligned buffers, the uploads, and the one way an arena is allocated.
// Host code only: no kernel is defined here.
#pragma once
#include <string>
#include <vector>

#include "aph_device.h"
#include "aph_host.h"

namespace aph {

// Hands out consecutive 256-byte-aligned pieces of an arena.  base == nullptr: every pointer handed out is null and only `off` (the size) counts.
struct Carver {
  char* base; size_t off = 0;
  template <typename T> T* take(size_t n) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += (n * sizeof(T) + 255) & ~(size_t)255;
    return p;
  }
};

// One checkpoint tensor and every device copy of it; the pointers name the members of the tower's handle / layers that carve_weights fills.
// An f16 matrix [rows, cols] has h16 (the copy and its transpose, main arena), m32 (the fp32 copy and its transpose, the exact path's arena),
// optionally rep (the copy repeated along K, hilo arena), and keeps its fp32 data in `host`, from which the enable calls fill rep and m32.
// An fp32 tensor has f32 (the copy and, where asked for, its transpose, main arena): every tensor of the text tower is one.  Absent copies are null.
struct Weight {
  std::string key;                     // OpenAI checkpoint key (the image tower's without the `visual.` prefix)
  size_t rows, cols;
  half_t** h16[2];
  half_t** rep;
  float** m32[2];
  float** f32[2];
  std::vector<float> host;             // (conv1.weight in the sampler's K order)
  bool set = false;                    // uploaded at least once
};
// table order = carve order
inline void add_mat(std::vector<Weight>& t, std::string key, size_t rows, size_t cols, half_t** w, half_t** wT, half_t** rep, float** w32, float** wT32) {
  t.push_back(Weight{std::move(key), rows, cols, {w, wT}, rep, {w32, wT32}, {nullptr, nullptr}});
}
inline void add_f32(std::vector<Weight>& t, std::string key, size_t rows, size_t cols, float** w, float** wT = nullptr) {
  t.push_back(Weight{std::move(key), rows, cols, {nullptr, nullptr}, nullptr, {nullptr, nullptr}, {w, wT}});
}

enum Arena { ARENA_MAIN, ARENA_HILO, ARENA_F32 };
// the copies of weights [first, last) that live in arena `a`, in table order
inline void carve_weights(std::vector<Weight>& t, Carver& c, size_t first, size_t last, Arena a) {
  for (size_t i = first; i < last; ++i) {
    Weight& w = t[i];
    const size_t n = w.rows * w.cols;
    if (a == ARENA_MAIN) {
      if (w.h16[0]) { *w.h16[0] = c.take<half_t>(n); *w.h16[1] = c.take<half_t>(n); }
      else { *w.f32[0] = c.take<float>(n); if (w.f32[1]) *w.f32[1] = c.take<float>(n); }
    }
    else if (a == ARENA_HILO) { if (w.rep) *w.rep = c.take<half_t>(2 * n); }
    else if (w.m32[0]) { *w.m32[0] = c.take<float>(n); *w.m32[1] = c.take<float>(n); }
  }
}

// host fp32 [rows, cols] -> device fp16, optionally transposed
inline int upload_f16(half_t* dst, const float* src, size_t rows, size_t cols, bool transpose) {
  std::vector<half_t> tmp(rows * cols);
  if (!transpose) {
    for (size_t i = 0; i < rows * cols; ++i) tmp[i] = (half_t)src[i];
  } else {
    for (size_t r = 0; r < rows; ++r)
      for (size_t c = 0; c < cols; ++c) tmp[c * rows + r] = (half_t)src[r * cols + c];
  }
  return hipMemcpy(dst, tmp.data(), tmp.size() * sizeof(half_t), hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
// host fp32 [rows, cols] -> device fp16 [rows, 2 cols]: every row twice along K (the B operand of a hi | lo split GEMM)
inline int upload_f16_twice(half_t* dst, const float* src, size_t rows, size_t cols) {
  std::vector<half_t> tmp(rows * cols * 2);
  for (size_t r = 0; r < rows; ++r)
    for (size_t c = 0; c < cols; ++c) tmp[r * 2 * cols + c] = tmp[r * 2 * cols + cols + c] = (half_t)src[r * cols + c];
  return hipMemcpy(dst, tmp.data(), tmp.size() * sizeof(half_t), hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
inline int upload_f32(float* dst, const float* src, size_t rows, size_t cols, bool transpose) {
  if (!transpose) return hipMemcpy(dst, src, rows * cols * sizeof(float), hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
  std::vector<float> tmp(rows * cols);
  for (size_t r = 0; r < rows; ++r)
    for (size_t c = 0; c < cols; ++c) tmp[c * rows + r] = src[r * cols + c];
  return hipMemcpy(dst, tmp.data(), tmp.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}

// the entry of a checkpoint key, or null
inline Weight* find_weight(std::vector<Weight>& t, const char* key) {
  for (Weight& w : t)
    if (w.key == key) return &w;
  return nullptr;
}
// every tensor of the table uploaded at least once
inline int check_loaded(const std::vector<Weight>& t, const char* who) {
  int n = 0;
  for (const Weight& w : t) n += w.set;
  if (n == (int)t.size()) return 0;
  return aph_fail(APH_ERR_ARG, "%s: weights not fully loaded (%d of %zu tensors)", who, n, t.size());
}
// the checks every forward / backward entry of a tower (a handle with max_batch and weights) opens with: arguments, batch, check_loaded
template <class Tower>
int check_call(const Tower* v, const void* in, const void* out, int S, const char* who) {
  if (!v || !in || !out) return aph_fail(APH_ERR_ARG, "%s: null argument", who);
  if (S < 1 || S > v->max_batch) return aph_fail(APH_ERR_ARG, "%s: batch %d outside 1..%d", who, S, v->max_batch);
  return check_loaded(v->weights, who);
}

// The one way an arena comes to be.  carve(base) points the handle's members into `base` and returns the size (base == nullptr: null
// pointers, the size alone): it is called to size the arena, again on the allocation, and -- when fill() reports a failure -- a third time
// with nullptr after the arena is freed, so that a failed call leaves the handle as it found it.  *arena is set before fill() runs.
template <class Carve, class Fill>
int alloc_arena(const char* who, char** arena, size_t* bytes, Carve&& carve, Fill&& fill) {
  const size_t total = carve(nullptr);
  char* base = nullptr;
  const hipError_t me = hipMalloc((void**)&base, total);
  if (me != hipSuccess) return aph_fail(APH_ERR_HIP, "%s: cannot allocate %zu bytes (%s)", who, total, hipGetErrorString(me));
  carve(base);
  *arena = base;
  if (fill()) {
    (void)hipFree(base);
    *arena = nullptr;
    carve(nullptr);
    return aph_fail(APH_ERR_HIP, "%s: weight upload failed", who);
  }
  *bytes = total;
  return APH_OK;
}
// an arena that nothing is uploaded into yet (the create calls)
template <class Carve>
int alloc_arena(const char* who, char** arena, size_t* bytes, Carve&& carve) {
  return alloc_arena(who, arena, bytes, carve, [] { return 0; });
}

}  // namespace aph
