// vmp_state.h — vmp_set_state: give chosen envs the state in the caller's
// reference-dtype arrays, validated per env on the device (kernel in
// vmp_state.hip). First the pure host part: which calls are refused before
// anything is launched, and the kernel's LDS size. No HIP calls:
// tests/native/state_check.cpp sweeps them on the CPU under the host
// sanitizers. Then the kernel's arguments, for vmp_state.hip and vmp_capi.cpp.
#ifndef VMP_STATE_H
#define VMP_STATE_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/vmp.h"

namespace vmp {

constexpr int kStateThreads = 256;
// k_set_state's dynamic LDS: u32 [2 P] hundredths per PM (cpu then memory),
// then kStateLdsTail words: the refusal code, #waiting, #existing, spare
constexpr int kStateLdsTail = 4;
constexpr int64_t kStateLdsMax = 64 * 1024;  // what a launch gets without opting in to more

inline int64_t state_lds_bytes(int32_t P) { return 4 * (2 * (int64_t)P + kStateLdsTail); }

// The pointers of a vmp_set_state call the host decides on (device pointers:
// only compared with null, never read)
struct StateCall {
  const void *handle;
  const void *placement, *vm_cpu, *vm_mem, *remaining;
  const void *cpu, *mem;
  int32_t P;
};

// VMP_OK, or VMP_EINVAL and in *why the reason; the handle is then untouched
inline int state_check(const StateCall *c, const char **why) {
  *why = nullptr;
  if (!c || !c->handle) {
    *why = "vmp_set_state: null handle";
    return VMP_EINVAL;
  }
  if (!c->placement || !c->vm_cpu || !c->vm_mem || !c->remaining) {
    *why = "vmp_set_state: placement, vm_cpu, vm_mem and remaining are required";
    return VMP_EINVAL;
  }
  if ((c->cpu == nullptr) != (c->mem == nullptr)) {
    *why = "vmp_set_state: cpu and mem are both given or both null";
    return VMP_EINVAL;
  }
  if (c->P < 1 || state_lds_bytes(c->P) > kStateLdsMax) {
    *why = "vmp_set_state: too many PMs for the kernel's per-PM sums in LDS";
    return VMP_EINVAL;
  }
  return VMP_OK;
}

}  // namespace vmp

#ifdef __HIP__
#include <hip/hip_runtime.h>

#include "vmp_layout.h"

namespace vmp {
struct StateArgs {
  EnvHdr *hdr;
  double *pm;
  uint32_t *vmw;
  const uint8_t *env_mask;   // [N], nullable = all
  const int64_t *placement;  // [N][V]
  const double *vm_cpu, *vm_mem;  // [N][V]
  const int64_t *remaining;  // [N][V]
  const double *cpu, *mem;   // [N][P], both or neither
  const int64_t *counters;   // [N][VMP_NCTR], nullable
  const double *totals;      // [N][2], nullable
  const int64_t *seeds;      // [N], nullable
  uint8_t *status;           // [N], nullable: VMP_SS_*
  uint8_t *imported;         // [N], nullable: 1 = the env was written (restarts its observers)
  int32_t N, P, V;
};
// grid: N workgroups of kStateThreads, state_lds_bytes(P) of dynamic LDS
__global__ void k_set_state(StateArgs a);
}  // namespace vmp
#endif

#endif  // VMP_STATE_H
