// vmp_kernels.h — what the host side (vmp_capi.cpp) needs of the env kernels'
// translation unit (vmp_kernels.hip): the kernels it launches and the block
// kernel's launchers (the constants both sides agree on: vmp_carve.h). Restates
// nothing of the reference. Included by vmp_kernels.hip's headers and by
// vmp_capi.cpp.
#ifndef VMP_KERNELS_H
#define VMP_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vmp_carve.h"
#include "vmp_layout.h"

namespace vmp {

constexpr int kStamps = 24;  // per-env phase clocks (diagnostic builds)

// WL = true: the instantiations for handles with a per-env workload
// (vmp_set_workload), in a translation unit of their own (vmp_kernels_wl.hip);
// handles without one run the WL = false kernels, whose code does not change
template <int VPT, bool ONE, bool WL = false>
__global__ void k_env(EnvParams p, StepOut o);
template <int VPT, bool WL = false>
__global__ void k_env_ext(EnvParams p, StepOut o);
// the kernels of handles with a trace (vmp_set_trace): vmp_kernels_tr.hip
template <int VPT, bool ONE>
__global__ void k_env_tr(EnvParams p, StepOut o);
template <int VPT>
__global__ void k_env_ext_tr(EnvParams p, StepOut o);
__global__ void k_rank(EnvParams p, int64_t *rank);
__global__ void k_target_means_lds(EnvParams p);
__global__ void k_reset(EnvParams p, const int64_t *seeds, const uint8_t *env_mask, float *obs);
__global__ void k_export(EnvParams p, int64_t *placement, double *vm_cpu, double *vm_mem,
                         double *cpu, double *mem, int64_t *remaining, int64_t *rank);
__global__ void k_counters(EnvParams p, int64_t *ctr, double *st);
__global__ void k_target_means(EnvParams p);
__global__ void k_mask_bool(int64_t rows, int A, int W, const uint32_t *bits, uint8_t *mask);
__global__ void k_act_obs(int P, int V, int policy, const float *obs, int32_t *act);
__global__ void k_launch_map(EnvParams p, int32_t *env_of_block);

// k_env_big: one workgroup per env (kBigNT threads, big_spt slots per thread:
// vmp_carve.h); its launchers live with the kernel (vmp_kernels.hip)
void launch_big_env(int spt, bool one, int n_env, size_t lds, hipStream_t s, const EnvParams &p,
                    const StepOut &o);
void launch_big_env_wl(int spt, bool one, int n_env, size_t lds, hipStream_t s,
                       const EnvParams &p, const StepOut &o);  // vmp_kernels_wl.hip
void launch_big_env_tr(int spt, bool one, int n_env, size_t lds, hipStream_t s,
                       const EnvParams &p, const StepOut &o);  // vmp_kernels_tr.hip
int big_occupancy(int spt, size_t lds, int *static_lds);

int64_t quiet_violations_take();

}  // namespace vmp

#endif  // VMP_KERNELS_H
