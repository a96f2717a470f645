// vmp_reqlog.h — the size arithmetic of the per-request outcome log
// (vmp_reqlog_enable, kernels in vmp_reqlog.hip) as pure functions: bytes of
// the rows, the slots' tracked ids, their previous placements and the per-env
// meta, with every product checked for overflow. No HIP calls:
// tests/native/reqlog_sizes.cpp sweeps it on the CPU under the host
// sanitizers. Included by vmp_capi.cpp.
#ifndef VMP_REQLOG_H
#define VMP_REQLOG_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/vmp.h"

namespace vmp {

// a request id is kept as an int32 per slot, so a log holds ids below 2^31 - 1
constexpr int64_t kReqlogMaxCapacity = 0x7fffffffLL;
// no single buffer above 2^62 bytes: every later index computed in int64 fits
constexpr uint64_t kReqlogMaxBytes = 1ull << 62;

struct ReqlogSizes {
  size_t rows;  // int32 [n_env][capacity][VMP_RQ_NF]
  size_t ids;   // int32 [n_env][V]
  size_t prev;  // uint16 [n_env][V]
  size_t meta;  // int64 [n_env][VMP_RQ_NMETA]
};

// a * b * c in *out; false if the product does not fit kReqlogMaxBytes
inline bool reqlog_mul3(uint64_t a, uint64_t b, uint64_t c, size_t *out) {
  uint64_t ab = 0, abc = 0;
  if (__builtin_mul_overflow(a, b, &ab) || __builtin_mul_overflow(ab, c, &abc)) return false;
  if (abc > kReqlogMaxBytes || abc > (uint64_t)SIZE_MAX) return false;
  *out = (size_t)abc;
  return true;
}

// null and *s filled if a log of `capacity` rows per env is a valid request
// for a handle of n_env envs of V slots, else what is wrong with it
inline const char *reqlog_sizes(int32_t n_env, int32_t V, int64_t capacity, ReqlogSizes *s) {
  if (n_env < 1 || V < 1) return "vmp_reqlog_enable: no envs or no slots";
  if (capacity < 1) return "vmp_reqlog_enable: capacity must be >= 1";
  if (capacity > kReqlogMaxCapacity) return "vmp_reqlog_enable: capacity above 2^31 - 1";
  if (!reqlog_mul3((uint64_t)n_env, (uint64_t)capacity, VMP_RQ_NF * sizeof(int32_t), &s->rows))
    return "vmp_reqlog_enable: the log's byte size does not fit";
  if (!reqlog_mul3((uint64_t)n_env, (uint64_t)V, sizeof(int32_t), &s->ids) ||
      !reqlog_mul3((uint64_t)n_env, (uint64_t)V, sizeof(uint16_t), &s->prev) ||
      !reqlog_mul3((uint64_t)n_env, VMP_RQ_NMETA, sizeof(int64_t), &s->meta))
    return "vmp_reqlog_enable: the log's byte size does not fit";
  return nullptr;
}

// Requests of the ids [prev_total, total) that a log of `capacity` rows cannot
// hold (id >= capacity): what a step adds to VMP_RQ_LOST (k_reqlog calls it too)
#ifdef __HIP__
__host__ __device__
#endif
inline int64_t reqlog_lost(int64_t prev_total, int64_t total, int64_t capacity) {
  const int64_t from = prev_total > capacity ? prev_total : capacity;
  return total > from ? total - from : 0;
}

}  // namespace vmp

#endif  // VMP_REQLOG_H
