// GEMM epilogues of the depth estimator's encoder (depth.hip: DINOv2, forward only) for launch_gemm of vit_gemm.h: apply8 for the ring and
// register-staged kernels, ws_tile / ws_bias for the wave-specialised one (vit_gemm_ws.h; found there by argument-dependent lookup when the
// kernel is instantiated, so this header comes after it).  They live here, not in vit_gemm.h: the ViT's GEMM sources stay byte for byte what
// the committed traffic measurements were taken on, and no existing instantiation changes.
#pragma once
#include "vit_gemm.h"
#include "vit_gemm_ws.h"

namespace aph {

// exact GELU g = u (1 + erf(u / sqrt 2)) / 2 with u = acc + bias, f16; no derivative is kept
__device__ __forceinline__ float gelu_erf(float u) { return 0.5f * u * (1.0f + erff(u * 0.70710678118654752f)); }
struct EpiGeluErfF16 {
  half_t* out; int ldo; const float* bias;
  __device__ __forceinline__ void apply8(int m, int n, f32x4 a, f32x4 b) const {
    a += ld4(bias + n); b += ld4(bias + n + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { a[i] = gelu_erf(a[i]); b[i] = gelu_erf(b[i]); }
    store_h8(out + (size_t)m * ldo + n, a, b);
  }
};
// patch embedding with a bias over a rectangular token grid of P = gh x gw patches: token row s*T + 1 + p  <-  patch row s*P + p, plus the
// convolution's bias and row 1 + p of the position rows interpolated to that grid (T = P + 1)
struct EpiPatchEmbedRect {
  float* x0; const float* pos; const float* bias; int D, P, T;
  __device__ __forceinline__ void apply8(int m, int n, f32x4 a, f32x4 b) const {
    const int s = m / P, p = m - s * P;
    const float* pe = pos + (size_t)(1 + p) * D + n;
    float* o = x0 + ((size_t)s * T + 1 + p) * D + n;
    st4(o, a + ld4(bias + n) + ld4(pe));
    st4(o + 4, b + ld4(bias + n + 4) + ld4(pe + 4));
  }
};

// v[nt][r] = C[m4 + r][n4 + nt] (vit_gemm_ws.h); lb = the bias vector in LDS
__device__ __forceinline__ void ws_tile(const EpiGeluErfF16& e, int m4, int M, int n4, f32x4 (&v)[4], const float* lb) {
  const f32x4 b = *reinterpret_cast<const f32x4*>(lb + n4);
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (m4 + r < M)
      *reinterpret_cast<half4*>(e.out + (size_t)(m4 + r) * e.ldo + n4) =
          pack_h4(gelu_erf(v[0][r] + b[0]), gelu_erf(v[1][r] + b[1]), gelu_erf(v[2][r] + b[2]), gelu_erf(v[3][r] + b[3]));
}
__device__ __forceinline__ void ws_tile(const EpiPatchEmbedRect& e, int m4, int M, int n4, f32x4 (&v)[4], const float*) {
  const f32x4 b = ld4(e.bias + n4);
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (m4 + r < M) {
      const int m = m4 + r, s = m / e.P, p = m - s * e.P;
      st4(e.x0 + ((size_t)s * e.T + 1 + p) * e.D + n4, f32x4{v[0][r], v[1][r], v[2][r], v[3][r]} + b + ld4(e.pos + (size_t)(1 + p) * e.D + n4));
    }
}
__device__ __forceinline__ const float* ws_bias(const EpiGeluErfF16& e) { return e.bias; }

}  // namespace aph
