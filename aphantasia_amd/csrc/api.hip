// Error plumbing + version for the C ABI.
#include "aph_device.h"
#include "aph_host.h"

static thread_local char g_err[512] = "";

int aph_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int aph_check_launch(const char* where) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return aph_fail(APH_ERR_HIP, "%s: %s", where, hipGetErrorString(e));
  return APH_OK;
}

#ifndef APH_EMU
#include <mutex>
#include <unordered_map>
void aph_allow_smem(const void* kernel, int bytes) {
  static std::mutex mu;
  static std::unordered_map<unsigned long long, int> granted;     // (kernel, device) -> largest size granted
  int dev = 0;
  APH_HIP(hipGetDevice(&dev));
  const unsigned long long key = (unsigned long long)(uintptr_t)kernel * 64ull + (unsigned long long)(dev & 63);
  std::lock_guard<std::mutex> lk(mu);
  auto it = granted.find(key);
  if (it != granted.end() && it->second >= bytes) return;
  APH_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  granted[key] = bytes;
}
#endif

extern "C" {
int aph_version(void) { return 200; }
const char* aph_last_error(void) { return g_err; }
}

// The interpreter build (tests/emu/build_emu.py) compiles a fixed list of units that has neither vit_test.hip nor text.hip nor the LPIPS nor the
// depth estimator's units: it takes the ViT's test and measurement entries, the text tower, the LPIPS term and the depth estimator with their
// test entries from here.  The gfx950 build compiles them as units of their own (aphantasia_amd/_build.py).
#ifdef APH_EMU
#include "vit_test.hip"
#include "text.hip"
#include "lpips.hip"
#include "lpips_test.hip"
#include "depth.hip"
#include "depth_net_test.hip"
#endif
