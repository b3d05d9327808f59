// Test entries of the LPIPS term (include/aphantasia_hip_test.h): each kernel of lpips_conv.h / lpips_ops.h alone on caller-supplied buffers,
// for the element-wise checks of tests/lpips_checks.py.  Not part of the drop-in boundary.
#include "aph_device.h"
#include "aph_host.h"
#include "lpips_conv.h"
#include "lpips_ops.h"

using namespace aph;
using namespace aph::lpips;

extern "C" {

// pack_weights (the routine aph_lpips_set_weight uses) into d_out; out_elems must be the packed size
int aph_lpips_pack_test(const float* h_w, int cout, int cin, int dgrad, void* d_out, size_t out_elems) {
  APH_TRY
  if (!h_w || !d_out || cout < 1 || cin < 1) return aph_fail(APH_ERR_ARG, "aph_lpips_pack_test: bad argument");
  const std::vector<half_t> p = pack_weights(h_w, cout, cin, dgrad ? 1 : 0);
  if (p.size() != out_elems) return aph_fail(APH_ERR_ARG, "aph_lpips_pack_test: packed size is %zu elements, caller has %zu", p.size(), out_elems);
  if (hipMemcpy(d_out, p.data(), p.size() * sizeof(half_t), hipMemcpyHostToDevice) != hipSuccess) return aph_fail(APH_ERR_HIP, "aph_lpips_pack_test: upload failed");
  return APH_OK;
  APH_CATCH
}

int aph_lpips_conv_test(const void* d_in, int H, int W, int C, const void* d_wt, int N, const float* d_bias, int relu, const void* d_mask, void* d_out,
                        float* d_out32, int n32, int nf, void* stream) {
  APH_TRY
  if (!d_in || !d_wt || (!d_out && !d_out32)) return aph_fail(APH_ERR_ARG, "aph_lpips_conv_test: null argument");
  if (H < 1 || W < 1 || C < 8 || C % 8 || N < 16 || N % 16 || n32 < 0 || n32 > N || (nf != 0 && nf != 1 && nf != 2 && nf != 4))
    return aph_fail(APH_ERR_ARG, "aph_lpips_conv_test: H %d W %d C %d (multiple of 8) N %d (multiple of 16) n32 %d nf %d (0, 1, 2, 4)", H, W, C, N, n32, nf);
  launch_conv(ConvArgs{(const half_t*)d_in, H, W, C, (const half_t*)d_wt, N, d_bias, relu, (const half_t*)d_mask, (half_t*)d_out, d_out32, n32}, (hipStream_t)stream, nf);
  return aph_check_launch("aph_lpips_conv_test");
  APH_CATCH
}

// d_out (nullable) [H/2][W/2][C] = pool(d_in); d_din (nullable) [H][W][C] = the pool's backward of d_dpool [H/2][W/2][C] at d_in
int aph_lpips_pool_test(const void* d_in, int H, int W, int C, void* d_out, const void* d_dpool, void* d_din, void* stream) {
  APH_TRY
  if (!d_in || (d_din && !d_dpool)) return aph_fail(APH_ERR_ARG, "aph_lpips_pool_test: null argument");
  if (H < 2 || W < 2 || C < 8 || C % 8) return aph_fail(APH_ERR_ARG, "aph_lpips_pool_test: H %d W %d (at least 2) C %d (multiple of 8)", H, W, C);
  if (d_out) launch_pool_fwd((const half_t*)d_in, H, W, C, (half_t*)d_out, (hipStream_t)stream);
  if (d_din) launch_grad_merge((const half_t*)d_in, H, W, C, (const half_t*)d_dpool, nullptr, 0, (half_t*)d_din, (hipStream_t)stream);
  return aph_check_launch("aph_lpips_pool_test");
  APH_CATCH
}

// the head on features d_f against target features d_fy (both f16 [P][C]): d_ny [P][C] = the normalised target, *d_value = mean_p d(p),
// d_hg (nullable) [P][C] = gcoef * dd/df; d_partial: 512 doubles of scratch
int aph_lpips_head_test(const void* d_f, const void* d_fy, const float* d_lin, int P, int C, float gcoef, float* d_ny, float* d_hg, double* d_partial,
                        float* d_value, void* stream) {
  APH_TRY
  if (!d_f || !d_fy || !d_lin || !d_ny || !d_partial || !d_value) return aph_fail(APH_ERR_ARG, "aph_lpips_head_test: null argument");
  if (P < 1 || C < 8 || C % 8) return aph_fail(APH_ERR_ARG, "aph_lpips_head_test: P %d C %d (multiple of 8)", P, C);
  hipStream_t st = (hipStream_t)stream;
  launch_unit_norm((const half_t*)d_fy, P, C, d_ny, st);
  launch_head((const half_t*)d_f, d_ny, d_lin, P, C, gcoef, d_hg, d_partial, st);
  HeadSums hs;
  for (int l = 0; l < 5; ++l) { hs.partial[l] = d_partial; hs.count[l] = l ? 0 : head_blocks(P); hs.P[l] = P; }
  APH_LAUNCH(head_finish_kernel, dim3(1), dim3(256), 0, st, hs, (const float*)nullptr, d_value, (float*)nullptr);
  return aph_check_launch("aph_lpips_head_test");
  APH_CATCH
}

// adjoint == 0: d_half [3][H/2][W/2] = resize(d_full [3][H][W]);  adjoint == 1: d_full += resize^T(d_half)
int aph_lpips_resize_test(float* d_full, int H, int W, float* d_half, int adjoint, void* stream) {
  APH_TRY
  if (!d_full || !d_half) return aph_fail(APH_ERR_ARG, "aph_lpips_resize_test: null argument");
  if (H < 4 || W < 4 || H > 16384 || W > 16384) return aph_fail(APH_ERR_ARG, "aph_lpips_resize_test: frame %d x %d outside 4 .. 16384", H, W);
  if (adjoint) launch_resize_adj(d_half, H / 2, W / 2, d_full, H, W, 1.f, 0, nullptr, (hipStream_t)stream);
  else launch_resize_fwd(d_full, H, W, d_half, H / 2, W / 2, (hipStream_t)stream);
  return aph_check_launch("aph_lpips_resize_test");
  APH_CATCH
}

}  // extern "C"
