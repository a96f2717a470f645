// vmp_stamps.h — the STAMP macros of the two diagnostic builds (-DVMP_STAMPS:
// per-phase shader clocks, -DVMP_WGTIME: workgroup timing); empty otherwise.
// Restates nothing of the reference. Included by the env kernel headers.
#ifndef VMP_STAMPS_H
#define VMP_STAMPS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vmp_dev.h"
#include "vmp_kernels.h"

namespace vmp {

// Diagnostic build only (-DVMP_STAMPS): per-phase shader-clock deltas,
// accumulated per env into p.stamps[e][kStamps]. No stamp executes otherwise.
#ifdef VMP_STAMPS
// The accumulators live in LDS (one row per wave in k_env, one per block in
// k_env_big, written by one lane), not in registers: a 24-entry register
// array in the 256-VGPR block kernel spilled and distorted its timing ~7x.
#define STAMP_PARAMS , uint64_t LDSP *st_acc, uint64_t &st_prev
#define STAMP_ARGS , st_acc, st_prev
#define STAMP_DECL_AT(ptr)                                          \
  uint64_t LDSP *st_acc = (ptr);                                    \
  if (st_acc && lane_id() == 0)                                     \
    for (int _i = 0; _i < kStamps; _i++) st_acc[_i] = 0;            \
  uint64_t st_prev = __builtin_amdgcn_s_memtime();
#define STAMP(i)                                      \
  do {                                                \
    const uint64_t _t = __builtin_amdgcn_s_memtime(); \
    if (st_acc && lane_id() == 0) st_acc[i] += _t - st_prev; \
    st_prev = _t;                                     \
  } while (0)
#define STAMP_FLUSH()                                                         \
  do {                                                                        \
    if (p.stamps && st_acc && lane_id() == 0)                                 \
      for (int _i = 0; _i < kStamps; _i++) p.stamps[(int64_t)e * kStamps + _i] += st_acc[_i]; \
  } while (0)
// k_env: a wave whose launch met the idle-step predicate (idle_step) says so
// in three slots k_env stamps nowhere else: how many of the env's launches did,
// and their share of slots 7 (wall time, x1000 100 MHz ticks) and 9 (shader
// cycles). tools/stamps.py reads them.
constexpr int kStampIdleN = 8, kStampIdleWall = 10, kStampIdleCyc = 22;
// the idle path's record, straight to the env's row (it leaves before the
// first STAMP; the prologue's three LDS slots are not flushed)
__device__ __forceinline__ void stamp_idle(uint64_t *row, uint64_t t_start, uint64_t rt_start) {
  const uint64_t wall = (__builtin_amdgcn_s_memrealtime() - rt_start) * 1000;
  const uint64_t cyc = __builtin_amdgcn_s_memtime() - t_start;
  row[7] += wall;
  row[9] += cyc;
  row[kStampIdleN] += 1;
  row[kStampIdleWall] += wall;
  row[kStampIdleCyc] += cyc;
}
#elif defined(VMP_WGTIME)
// Workgroup timing build (k_env_big): thread 0 records the 100 MHz real-time
// clock at every stamp point into a block LDS row; tools/wgtime.py reads it.
__shared__ uint64_t wg_marks[24];
#define STAMP_PARAMS
#define STAMP_ARGS
#define STAMP_DECL_AT(ptr)
#define STAMP(i)                                                         \
  do {                                                                   \
    if (threadIdx.x == 0) wg_marks[i] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#define STAMP_FLUSH()
#else
#define STAMP_PARAMS
#define STAMP_ARGS
#define STAMP_DECL_AT(ptr)
#define STAMP(i)
#define STAMP_FLUSH()
#endif

}  // namespace vmp

#endif  // VMP_STAMPS_H
