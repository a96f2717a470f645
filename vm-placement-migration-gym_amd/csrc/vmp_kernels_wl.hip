// vmp_kernels_wl.hip — the step kernels of handles with a per-env workload
// (vmp_set_workload): the WL = true instantiations of k_env, k_env_ext and
// k_env_big, which read env e's Poisson constants from p.pois[e] instead of
// the handle's one pair (env_pois, vmp_env_common.h). A translation unit of
// its own, so it compiles beside vmp_kernels.hip, whose kernels (every handle
// without a per-env workload) are the same code with or without this file.
//
// The quiet-bit check build (-DVMP_CHECK_QUIET) links this unit's normal
// object: its counter is a __device__ global of vmp_kernels.hip's code object
// and counts the launches of that unit's kernels.
#include <hip/hip_runtime.h>

#define VMP_ENV_WL true

#include "vmp_kernels.h"
#include "vmp_layout.h"

#include "vmp_dev.h"
#include "vmp_np_rng.h"
#include "vmp_stamps.h"
#include "vmp_np_sum.h"
#include "vmp_np_sort.h"
#include "vmp_env_common.h"
#include "vmp_env_wave.h"
#include "vmp_env_big.h"

namespace vmp {

void launch_big_env_wl(int spt, bool one, int n_env, size_t lds, hipStream_t s,
                       const EnvParams &p, const StepOut &o) {
  if (one) launch_big_one<true, kSrcEnv>(spt, n_env, lds, s, p, o);
  else launch_big_one<false, kSrcEnv>(spt, n_env, lds, s, p, o);
}

}  // namespace vmp
