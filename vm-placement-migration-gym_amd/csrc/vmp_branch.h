// vmp_branch.h — vmp_branch: copy the state of chosen envs of one handle into
// chosen envs of another (or the same) on the device, optionally with fresh RNG
// streams (kernel in vmp_branch.hip). First the pure host part: the
// compatibility check of the two handles and the geometry of the gather (an
// env's three rows as 16-byte units, cut into chunks). No HIP calls:
// tests/native/branch_check.cpp sweeps them on the CPU under the host
// sanitizers. Then the kernel's arguments, for vmp_branch.hip and vmp_capi.cpp.
#ifndef VMP_BRANCH_H
#define VMP_BRANCH_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vmp.h"

namespace vmp {

// What vmp_branch compares of a handle
struct BranchSide {
  int32_t P, V, A;
  int32_t device;
  int32_t traced;  // the handle has a trace (vmp_set_trace)
  vmp_config cfg;  // seed excluded, as in vmp_restore
};

// VMP_OK, or the code vmp_branch returns and in *why the reason. The env counts
// are not compared: the map ranges over them. Neither are eval mode, per-env
// workloads or the traces themselves: a dst env continues under dst's own.
inline int branch_check(const BranchSide *dst, const BranchSide *src, const void *src_of_dst,
                        const char **why) {
  *why = nullptr;
  if (!dst || !src || !src_of_dst) {
    *why = "vmp_branch: null handle or map";
    return VMP_EINVAL;
  }
  if (dst->P != src->P || dst->V != src->V || dst->A != src->A) {
    *why = "vmp_branch: the handles differ in pms, vms or the action count";
    return VMP_EINVAL;
  }
  vmp_config x = dst->cfg, y = src->cfg;
  x.seed = y.seed = 0;
  if (memcmp(&x, &y, sizeof(x)) != 0) {
    *why = "vmp_branch: the handles differ in their config";
    return VMP_EINVAL;
  }
  if (dst->device != src->device) {
    *why = "vmp_branch: the handles live on different devices";
    return VMP_EINVAL;
  }
  if ((dst->traced != 0) != (src->traced != 0)) {
    *why = "vmp_branch: one handle has a trace and the other has none";
    return VMP_ESTATE;
  }
  return VMP_OK;
}

// An env is three rows, each a multiple of 16 bytes: EnvHdr (256 B), pm
// (16 P B) and the VM words (4 pitch B, pitch a multiple of 128). The gather
// moves them as 16-byte units numbered hdr | pm | vmw, kBranchChunk units per
// workgroup (256 lanes, 4 units each: 16 KB).
constexpr int kBranchThreads = 256;
constexpr int kBranchPerLane = 4;
constexpr int kBranchChunk = kBranchThreads * kBranchPerLane;
constexpr int kBranchHdrUnits = 16;  // sizeof(EnvHdr) / 16

struct BranchGeom {
  int64_t pm_units;   // P
  int64_t vm_units;   // pitch / 4
  int64_t units;      // per env
  int64_t chunks;     // per env
};

// pitch: vm_pitch(V), u32 elements
inline BranchGeom branch_geom(int32_t P, int64_t pitch) {
  BranchGeom g;
  g.pm_units = P;
  g.vm_units = pitch / 4;
  g.units = kBranchHdrUnits + g.pm_units + g.vm_units;
  g.chunks = (g.units + kBranchChunk - 1) / kBranchChunk;
  return g;
}

// Unit u of an env: which row (0 hdr, 1 pm, 2 vmw) and the unit inside it;
// k_branch calls it too
#ifdef __HIP__
__host__ __device__
#endif
inline int branch_part(int64_t u, int64_t pm_units, int64_t *at) {
  if (u < kBranchHdrUnits) {
    *at = u;
    return 0;
  }
  u -= kBranchHdrUnits;
  if (u < pm_units) {
    *at = u;
    return 1;
  }
  *at = u - pm_units;
  return 2;
}

}  // namespace vmp

#ifdef __HIP__
#include <hip/hip_runtime.h>

#include "vmp_layout.h"

namespace vmp {
struct BranchArgs {
  const uint4 *src_hdr, *src_pm, *src_vmw;  // the source rows (the staging copy when dst == src)
  uint4 *dst_hdr, *dst_pm, *dst_vmw;
  const int32_t *src_of_dst;  // [dst_n]
  const int64_t *seeds;       // [dst_n], nullable
  uint8_t *mask;              // [dst_n], nullable: 1 = the env was overwritten
  int32_t src_n, dst_n;
  int32_t pm_units, vm_units;  // 16-byte units of an env's pm and vmw rows
  int32_t units, chunks;       // per env
};
// grid: dst_n * chunks workgroups of kBranchThreads
__global__ void k_branch(BranchArgs a);
}  // namespace vmp
#endif

#endif  // VMP_BRANCH_H
