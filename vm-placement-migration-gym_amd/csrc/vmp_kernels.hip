// vmp_kernels.hip — gfx950 kernels for the batched VmEnv hot path.
//
// One 64-lane wavefront owns one env for a whole launch (4 envs per 256-thread
// workgroup, the waves never synchronise with each other after the prologue).
// Lane l holds VM slots v = s*64 + l (s < VPT) in registers: the reference's
// per-VM Python loops (env.py:68-88, 244-293) become lane-parallel passes, and
// the only truly ordered work — resource updates on one PM, which must happen
// in VM order — runs as a wave-uniform loop over the
// ballot of the slots that carry an event. PM resources (f64) live in LDS.
//
// Exactness: all f64 arithmetic follows the reference's operation order; the
// build uses -ffp-contract=off; numpy's pairwise summation, PCG64 streams,
// Poisson samplers and np.around are restated bit-for-bit (see oracle/ for the
// CPU restatement these kernels are tested against).
//
// This file is the one translation unit of those kernels: the code is in the
// headers below, by concern, and only the host-side pieces that need the
// kernels' definitions (the block kernel's launchers, the check build's
// counter) are here.
#include <hip/hip_runtime.h>

#include "vmp_kernels.h"
#include "vmp_layout.h"

#include "vmp_dev.h"
#include "vmp_np_rng.h"
#include "vmp_stamps.h"
#include "vmp_np_sum.h"
#include "vmp_np_sort.h"
#include "vmp_env_common.h"
#include "vmp_env_wave.h"
#include "vmp_env_aux.h"
#include "vmp_env_big.h"
#include "vmp_act_obs.h"

namespace vmp {

// -> the count since the last call (reset to 0); -1 in a build without the check
int64_t quiet_violations_take() {
#ifdef VMP_CHECK_QUIET
  unsigned long long v = 0, z = 0;
  if (hipDeviceSynchronize() != hipSuccess) return -2;
  if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_quiet_violations), sizeof(v)) != hipSuccess) return -2;
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_quiet_violations), &z, sizeof(z)) != hipSuccess) return -2;
  return (int64_t)v;
#else
  return -1;
#endif
}

// host side: the block kernel's launcher (vmp_capi.cpp)
void launch_big_env(int spt, bool one, int n_env, size_t lds, hipStream_t s, const EnvParams &p,
                    const StepOut &o) {
  if (one) launch_big_one<true, kSrcConfig>(spt, n_env, lds, s, p, o);
  else launch_big_one<false, kSrcConfig>(spt, n_env, lds, s, p, o);
}
// workgroups per CU of the per-step block kernel at `lds` dynamic bytes, and
// its static LDS
int big_occupancy(int spt, size_t lds, int *static_lds) {
  const void *f = reinterpret_cast<const void *>(&k_env_big<kBigMaxSPT, true>);
  if (spt == 4) f = reinterpret_cast<const void *>(&k_env_big<4, true>);
  else if (spt == 8) f = reinterpret_cast<const void *>(&k_env_big<8, true>);
  else if (spt == 16) f = reinterpret_cast<const void *>(&k_env_big<16, true>);
  hipFuncAttributes a;
  if (hipFuncGetAttributes(&a, f) == hipSuccess) *static_lds = (int)a.sharedSizeBytes;
  int nb = -1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, f, kBigNT, lds) != hipSuccess) nb = -1;
  return nb;
}

}  // namespace vmp
