// Test entries of the depth estimator (include/aphantasia_hip_test.h): each kernel of depth_kernels.h, the X instantiation of lpips_conv.h's
// convolution and the erf-GELU GEMM epilogue alone on caller-supplied buffers, for the element-wise checks of tests/depthnet_checks.py.
#include "aph_device.h"
#include "aph_host.h"
#include "vit_gemm.h"
#include "vit_gemm_ws.h"
#include "vit_gemm_rs.h"
#include "depth_epi.h"
#include "lpips_conv.h"
#include "depth_kernels.h"

using namespace aph;
using namespace aph::depth;

extern "C" {

int aph_depth_attn_test(const void* d_qkv, void* d_att, int B, int T, int heads, void* stream) {
  APH_TRY
  if (!d_qkv || !d_att || B < 1 || T < 1 || heads < 1) return aph_fail(APH_ERR_ARG, "aph_depth_attn_test: bad argument");
  launch_attn_long_fwd((const half_t*)d_qkv, (half_t*)d_att, B, T, heads, (hipStream_t)stream);
  return aph_check_launch("aph_depth_attn_test");
  APH_CATCH
}

int aph_depth_conv_test(const void* d_in, int H, int W, int C, const void* d_wt, int N, const float* d_bias, int relu, int relu_in, const void* d_res,
                        const void* d_res2, int batch, int stride, void* d_tmp, void* d_out, void* stream) {
  APH_TRY
  if (!d_in || !d_wt || !d_out || (stride == 2 && !d_tmp)) return aph_fail(APH_ERR_ARG, "aph_depth_conv_test: null argument");
  if (H < 1 || W < 1 || C < 8 || C % 8 || N < 16 || N % 16 || batch < 1 || (stride != 1 && stride != 2))
    return aph_fail(APH_ERR_ARG, "aph_depth_conv_test: H %d W %d C %d (multiple of 8) N %d (multiple of 16) batch %d stride %d (1, 2)", H, W, C, N, batch, stride);
  lpips::ConvArgs a{(const half_t*)d_in, H, W, C, (const half_t*)d_wt, N, d_bias, relu, nullptr, (half_t*)(stride == 2 ? d_tmp : d_out), nullptr, 0};
  a.relu_in = relu_in; a.res = (const half_t*)d_res; a.res2 = (const half_t*)d_res2; a.batch = batch;
  lpips::launch_conv<true>(a, (hipStream_t)stream);
  if (stride == 2) launch_dn_subsample((const half_t*)d_tmp, H, W, (half_t*)d_out, N, batch, (hipStream_t)stream);
  return aph_check_launch("aph_depth_conv_test");
  APH_CATCH
}

// out [M][N] f16 = A [M][lda] Bt[N][K]^T + bias (nullable): the neck's 1 x 1 convolution
int aph_depth_gemm_test(const void* d_a, int lda, const void* d_bt, int M, int N, int K, const float* d_bias, void* d_out, void* stream) {
  APH_TRY
  if (!d_a || !d_bt || !d_out || M < 1 || N < 16 || N % 16 || K < 8 || K % 8 || lda < K) return aph_fail(APH_ERR_ARG, "aph_depth_gemm_test: bad argument");
  launch_dn_gemm((const half_t*)d_a, lda, (const half_t*)d_bt, M, N, K, EpiDnBias{(half_t*)d_out, N, d_bias}, (hipStream_t)stream);
  return aph_check_launch("aph_depth_gemm_test");
  APH_CATCH
}

// the transpose convolution with kernel = stride = k: h_w fp32 HOST [cin][cout][k][k] is packed by the routine aph_depth_forward uses into
// d_wpack (k k cout cin f16 of caller scratch), then d_out [B][gh k][gw k][cout] from d_in [B][gh][gw][cin]
int aph_depth_convt_test(const void* d_in, int B, int gh, int gw, int cin, const float* h_w, int cout, int k, const float* d_bias, void* d_wpack, void* d_out,
                         void* stream) {
  APH_TRY
  if (!d_in || !h_w || !d_bias || !d_wpack || !d_out) return aph_fail(APH_ERR_ARG, "aph_depth_convt_test: null argument");
  if (B < 1 || gh < 1 || gw < 1 || cin < 8 || cin % 8 || cout < 16 || cout % 16 || k < 1 || k > 4) return aph_fail(APH_ERR_ARG, "aph_depth_convt_test: bad shape");
  const std::vector<half_t> p = pack_convt(h_w, cin, cout, k);
  if (hipMemcpy(d_wpack, p.data(), p.size() * sizeof(half_t), hipMemcpyHostToDevice) != hipSuccess) return aph_fail(APH_ERR_HIP, "aph_depth_convt_test: upload failed");
  launch_dn_gemm((const half_t*)d_in, cin, (const half_t*)d_wpack, B * gh * gw, k * k * cout, cin, EpiDnShuffle{(half_t*)d_out, d_bias, gh, gw, k, cout},
                 (hipStream_t)stream);
  return aph_check_launch("aph_depth_convt_test");
  APH_CATCH
}

int aph_depth_resize_test(const void* d_in, int B, int h, int w, int C, void* d_out, int H, int W, void* stream) {
  APH_TRY
  if (!d_in || !d_out || B < 1 || h < 1 || w < 1 || H < 1 || W < 1 || C < 8 || C % 8) return aph_fail(APH_ERR_ARG, "aph_depth_resize_test: bad argument");
  launch_dn_resize((const half_t*)d_in, h, w, (half_t*)d_out, H, W, C, B, (hipStream_t)stream);
  return aph_check_launch("aph_depth_resize_test");
  APH_CATCH
}

// out [M][N] f16 = gelu_erf(A [M][K] Bt[N][K]^T + bias) through launch_gemm (N % 128 == 0, K % 64 == 0): fc1 of the encoder
int aph_depth_gelu_gemm_test(const void* d_a, const void* d_bt, int M, int N, int K, const float* d_bias, void* d_out, void* stream) {
  APH_TRY
  if (!d_a || !d_bt || !d_bias || !d_out || M < 1 || N < 128 || N % 128 || K < 64 || K % 64) return aph_fail(APH_ERR_ARG, "aph_depth_gelu_gemm_test: bad argument");
  launch_gemm((const half_t*)d_a, K, (const half_t*)d_bt, K, M, N, K, EpiGeluErfF16{(half_t*)d_out, N, d_bias}, (hipStream_t)stream);
  return aph_check_launch("aph_depth_gelu_gemm_test");
  APH_CATCH
}

}  // extern "C"
