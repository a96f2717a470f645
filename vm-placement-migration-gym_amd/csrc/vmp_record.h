// vmp_record.h — recorder state and kernels shared by vmp_record.hip and
// vmp_capi.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vmp_layout.h"

namespace vmp {
struct RecArgs {
  uint16_t *prev;     // [N][V] previous post-step placement
  uint32_t *life_n;   // [N][V] status count of the slot's current life
  int32_t *alloc;     // [N][V] allocated_at of the current life, -1 = none
  uint32_t *waits;    // [N][V] WAIT statuses at or after allocated_at
  uint32_t *hist;     // [N][2][VMP_REC_BINS] pending, slowdown
  double *sums;       // [N][VMP_NREC]
  const int32_t *act;      // this step's actions [N][V]
  const uint8_t *valid;    // [N][V]
  const double *reward;    // [N]
};
__global__ void k_record(EnvParams p, RecArgs r);
// env_mask (device u8 [N], nullable = all): the envs to (re)start
__global__ void k_record_init(EnvParams p, RecArgs r, const uint8_t *env_mask);
__global__ void k_record_close(EnvParams p, RecArgs r, uint32_t *hist, double *sums);

// per-request outcome log (vmp_reqlog.hip), a second observer behind the step
struct ReqArgs {
  int32_t *rows;      // [N][cap][VMP_RQ_NF] one row per request id
  int32_t *ids;       // [N][V] request id of the slot's VM, -1 = untracked
  uint16_t *prev;     // [N][V] previous post-step placement
  int64_t *meta;      // [N][VMP_RQ_NMETA]; VMP_RQ_NEXT is the kernel's prev_total
  int64_t cap;        // rows per env
  const int32_t *act;      // this step's actions [N][V]
  const uint8_t *valid;    // [N][V]
};
__global__ void k_reqlog(EnvParams p, ReqArgs q);
// adds the open waiting stretches to `rows`, a copy of q.rows
__global__ void k_reqlog_close(EnvParams p, ReqArgs q, int32_t *rows);
// env_mask (device u8 [N], nullable = all): the envs to (re)start
__global__ void k_reqlog_init(EnvParams p, ReqArgs q, const uint8_t *env_mask);
}  // namespace vmp
