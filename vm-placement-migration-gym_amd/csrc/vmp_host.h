// vmp_host.h — host-side plumbing of the C ABI (vmp_capi.cpp, and the
// test-only wrappers of vmp_prims.hip): the thread's error text, the counted
// device allocations, the PCG64 jump table, and the per-config Poisson setup,
// evaluated with glibc exactly as numpy's C code does.
#ifndef VMP_HOST_H
#define VMP_HOST_H

#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vmp.h"
#include "vmp_layout.h"

namespace vmp {

inline thread_local std::string g_err;

inline int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}
// fail(rc) with the failure's own message, after a cleanup that may set another
template <class F>
int fail_after(int rc, F cleanup) {
  const std::string msg = g_err;
  cleanup();
  return fail(rc, msg);
}

// fail() for a HIP error: VMP_EOOM if it is out of memory, else VMP_EDEVICE, with the
// error's text behind `who`
inline int fail_hip(const char *who, hipError_t e) {
  return fail(e == hipErrorOutOfMemory ? VMP_EOOM : VMP_EDEVICE, std::string(who) + hipGetErrorString(e));
}

#define HIP_TRY(expr)                                 \
  do {                                                \
    hipError_t _e = (expr);                           \
    if (_e != hipSuccess) return fail_hip(#expr ": ", _e); \
  } while (0)
inline int launched() {  // after a kernel launch
  HIP_TRY(hipGetLastError());
  return VMP_OK;
}

// Device allocations of the handle go through here, so the failure paths can
// be exercised (vmp_debug_fail_alloc: the n-th allocation from now fails as
// out-of-memory; tests/test_sanitizers_cpu.py, tests/native/capi_faults.cpp).
// g_live counts the library's live device allocations (vmp_debug_live_allocs),
// so a leak on a failure path is seen exactly, whatever the runtime caches.
inline std::atomic<int64_t> g_fail_alloc{0};
inline std::atomic<int64_t> g_live{0};
template <class T>
hipError_t dev_malloc(T **p, size_t bytes) {
  int64_t n = g_fail_alloc.load();
  while (n > 0 && !g_fail_alloc.compare_exchange_weak(n, n - 1)) {
  }
  if (n == 1) {
    *p = nullptr;
    return hipErrorOutOfMemory;
  }
  const hipError_t e = hipMalloc(reinterpret_cast<void **>(p), bytes);
  if (e == hipSuccess && *p) g_live++;
  else *p = nullptr;
  return e;
}
inline void dev_free(void *p) {
  if (!p) return;
  (void)hipFree(p);
  g_live--;
}

// PCG64 jump table of the lane-parallel draws (ParRng, vmp_env_common.h):
// entry j holds (A_j, M_j), each as (hi, lo), with the state after j + 1 draws
// s_j = A_j * base + M_j * inc, i.e. A_j = a^(j+1), M_j = a^j + ... + a + 1
// for the LCG multiplier a.
constexpr int kJumpWords = 64 * 4;
inline void pcg_jump_table(uint64_t jt[kJumpWords]) {
  const unsigned __int128 a = ((unsigned __int128)0x2360ED051FC65DA4ULL << 64) | 0x4385DF649FCCF645ULL;
  unsigned __int128 A = a, M = 1;
  for (int j = 0; j < 64; j++) {
    jt[4 * j + 0] = (uint64_t)(A >> 64);
    jt[4 * j + 1] = (uint64_t)A;
    jt[4 * j + 2] = (uint64_t)(M >> 64);
    jt[4 * j + 3] = (uint64_t)M;
    A *= a;
    M = M * a + 1;
  }
}

// random_loggam (numpy distributions.c), host copy for the PTRS table.
inline double loggam_host(double x) {
  static const double a[10] = {8.333333333333333e-02, -2.777777777777778e-03,
                               7.936507936507937e-04, -5.952380952380952e-04,
                               8.417508417508418e-04, -1.917526917526918e-03,
                               6.410256410256410e-03, -2.955065359477124e-02,
                               1.796443723688307e-01, -1.39243221690590e+00};
  if (x == 1.0 || x == 2.0) return 0.0;
  int64_t n = (x < 7.0) ? (int64_t)(7 - x) : 0;
  double x0 = x + n;
  double x2 = (1.0 / x0) * (1.0 / x0);
  double gl0 = a[9];
  for (int k = 8; k >= 0; k--) {
    gl0 *= x2;
    gl0 += a[k];
  }
  double gl = gl0 / x0 + 0.5 * 1.8378770664093453e+00 + (x0 - 0.5) * std::log(x0) - x0;
  if (x < 7.0)
    for (int64_t k = 1; k <= n; k++) {
      gl -= std::log(x0 - 1.0);
      x0 -= 1.0;
    }
  return gl;
}

// The constants of Poisson(lam) and the length tab_n of the loggam table its
// PTRS draws index (entry k = loggam(k), the same for every lam); loggam_tab
// is left null for the caller to point at a table of at least tab_n entries.
inline void pois_consts(double lam, PoisConst &c) {
  std::memset(&c, 0, sizeof(c));
  c.lam = lam;
  if (lam == 0) {
    c.kind = 0;
  } else if (lam < 10) {
    c.kind = 1;
    c.enlam = std::exp(-lam);
  } else {
    c.kind = 2;
    double slam = std::sqrt(lam);
    c.loglam = std::log(lam);
    c.b = 0.931 + 2.53 * slam;
    c.a = -0.059 + 0.02483 * c.b;
    c.invalpha = 1.1239 + 1.1328 / (c.b - 3.4);
    c.vr = 0.9277 - 3.6224 / (c.b - 2);
    c.log_invalpha = std::log(c.invalpha);
    int64_t n = (int64_t)(lam + 16.0 * slam + 64.0);
    if (n > (1 << 22)) n = 1 << 22;
    c.tab_n = (int32_t)n;
  }
}

// A device table loggam(k), k in [0, n).
inline int make_loggam_tab(int64_t n, double **dev_tab) {
  std::vector<double> host_tab((size_t)n);
  for (int64_t k = 0; k < n; k++) host_tab[(size_t)k] = loggam_host((double)k);
  HIP_TRY(dev_malloc(dev_tab, sizeof(double) * n));
  const hipError_t e = hipMemcpy(*dev_tab, host_tab.data(), sizeof(double) * n, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    dev_free(*dev_tab);
    *dev_tab = nullptr;
    return fail(VMP_EDEVICE, std::string("loggam table copy: ") + hipGetErrorString(e));
  }
  return VMP_OK;
}

inline int setup_pois(double lam, PoisConst &c, double **dev_tab) {
  pois_consts(lam, c);
  if (c.kind != 2) return VMP_OK;
  const int rc = make_loggam_tab(c.tab_n, dev_tab);
  c.loggam_tab = *dev_tab;  // null if it failed
  return rc;
}

}  // namespace vmp

#endif  // VMP_HOST_H
