// vmp_kernels.h — what the host side (vmp_capi.cpp) needs of the env kernels'
// translation unit (vmp_kernels.hip): the kernels it launches, the block
// kernel's launchers, and the constants both sides must agree on. Restates
// nothing of the reference. Included by vmp_kernels.hip's headers and by
// vmp_capi.cpp.
#ifndef VMP_KERNELS_H
#define VMP_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vmp_layout.h"

namespace vmp {

constexpr int kStamps = 24;  // per-env phase clocks (diagnostic builds)

// Static LDS of the step kernels in the default build, which vmp_create adds
// to the dynamic carve when it checks a config against the 160 KB of a CU.
// Each is tied to the structs it stands for by a static_assert next to them
// (vmp_env_common.h, vmp_env_big.h).
constexpr int kEnvStaticLds = 2048;  // k_env / k_env_ext: allowance for Tables
constexpr int kBigStaticLds = 4720;  // k_env_big: Tables + BigShared, exactly
constexpr int kBigAccLds = 512;      // k_env_big: accepted sizes held in LDS

// WL = true: the instantiations for handles with a per-env workload
// (vmp_set_workload), in a translation unit of their own (vmp_kernels_wl.hip);
// handles without one run the WL = false kernels, whose code does not change
template <int VPT, bool ONE, bool WL = false>
__global__ void k_env(EnvParams p, StepOut o);
template <int VPT, bool WL = false>
__global__ void k_env_ext(EnvParams p, StepOut o);
__global__ void k_rank(EnvParams p, int64_t *rank);
__global__ void k_target_means_lds(EnvParams p);
__global__ void k_reset(EnvParams p, const int64_t *seeds, const uint8_t *env_mask, float *obs);
__global__ void k_export(EnvParams p, int64_t *placement, double *vm_cpu, double *vm_mem,
                         double *cpu, double *mem, int64_t *remaining, int64_t *rank);
__global__ void k_counters(EnvParams p, int64_t *ctr, double *st);
__global__ void k_target_means(EnvParams p);
__global__ void k_mask_bool(int64_t rows, int A, int W, const uint32_t *bits, uint8_t *mask);
__global__ void k_act_obs(int P, int V, int policy, const float *obs, int32_t *act);

// k_env_big: one workgroup per env; its geometry (threads, slots per thread)
// and launcher live with the kernel (vmp_kernels.hip)
void big_geometry(int *nt, int *spt_max);
void launch_big_env(int spt, bool one, int n_env, size_t lds, hipStream_t s, const EnvParams &p,
                    const StepOut &o);
void launch_big_env_wl(int spt, bool one, int n_env, size_t lds, hipStream_t s,
                       const EnvParams &p, const StepOut &o);  // vmp_kernels_wl.hip
int big_occupancy(int spt, size_t lds, int *static_lds);

int64_t quiet_violations_take();

}  // namespace vmp

#endif  // VMP_KERNELS_H
