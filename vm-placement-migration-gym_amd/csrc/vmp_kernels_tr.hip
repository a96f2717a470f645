// vmp_kernels_tr.hip — the step kernels of handles with a trace (vmp_set_trace):
// k_env_tr, k_env_ext_tr and k_env_big<.., TR = true>, the kSrcTrace
// instantiations of the bodies of k_env, k_env_ext and k_env_big. A traced env
// draws nothing: the
// prologue loads the launch's arrival counts from the env's trace
// (trace_preload, vmp_env_common.h) and the accept loops take sizes and
// runtimes from its packed requests; RNG streams 1-4 are neither read nor
// advanced. The env's TraceDesc is read from the table that rides in
// EnvParams::pois. A translation unit of its own, as vmp_kernels_wl.hip: the
// kernels of every other handle are the same code with or without this file.
#include <hip/hip_runtime.h>

#define VMP_ENV_TR 1

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

void launch_big_env_tr(int spt, bool one, int n_env, size_t lds, hipStream_t s,
                       const EnvParams &p, const StepOut &o) {
  if (one) launch_big_one<true, kSrcTrace>(spt, n_env, lds, s, p, o);
  else launch_big_one<false, kSrcTrace>(spt, n_env, lds, s, p, o);
}

}  // namespace vmp
