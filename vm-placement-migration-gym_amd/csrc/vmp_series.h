// vmp_series.h — the per-step time series log (vmp_series_enable, kernels in
// vmp_series.hip). First the size arithmetic as pure functions: bytes of the
// rows, the optional PM rows, the per-env meta and the scratch reward, with
// every product checked for overflow, and the row a step folds into. No HIP
// calls: tests/native/series_sizes.cpp sweeps them on the CPU under the host
// sanitizers. Then the kernels' arguments, for vmp_series.hip and vmp_capi.cpp.
#ifndef VMP_SERIES_H
#define VMP_SERIES_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/vmp.h"

namespace vmp {

// rows per env: the row index is COUNT / stride in int64, far below this
constexpr int64_t kSeriesMaxCapacity = 0x7fffffffLL;
// no single buffer above 2^62 bytes: every later index computed in int64 fits
constexpr uint64_t kSeriesMaxBytes = 1ull << 62;

struct SeriesSizes {
  size_t rows;    // f64 [n_env][capacity][VMP_SR_NF]
  size_t pm;      // f32 [n_env][capacity][2 P], 0 without PM rows
  size_t meta;    // int64 [n_env][VMP_SR_NMETA]
  size_t reward;  // f64 [n_env]: the step's reward where the caller passes no buffer
};

// a * b * c in *out; false if the product does not fit kSeriesMaxBytes
inline bool series_mul3(uint64_t a, uint64_t b, uint64_t c, size_t *out) {
  uint64_t ab = 0, abc = 0;
  if (__builtin_mul_overflow(a, b, &ab) || __builtin_mul_overflow(ab, c, &abc)) return false;
  if (abc > kSeriesMaxBytes || abc > (uint64_t)SIZE_MAX) return false;
  *out = (size_t)abc;
  return true;
}

// null and *s filled if a series of `capacity` rows per env, `stride` steps a
// row, is a valid request for a handle of n_env envs of P PMs, else what is
// wrong with it
inline const char *series_sizes(int32_t n_env, int32_t P, int64_t capacity, int32_t stride,
                                int32_t pm_rows, SeriesSizes *s) {
  if (n_env < 1 || P < 1) return "vmp_series_enable: no envs or no PMs";
  if (capacity < 1) return "vmp_series_enable: capacity must be >= 1";
  if (capacity > kSeriesMaxCapacity) return "vmp_series_enable: capacity above 2^31 - 1";
  if (stride < 1) return "vmp_series_enable: stride must be >= 1";
  if (pm_rows != 0 && pm_rows != 1) return "vmp_series_enable: pm_rows must be 0 or 1";
  size_t per_pm = 0;  // bytes of one PM row
  if (!series_mul3((uint64_t)P, 2, sizeof(float), &per_pm))
    return "vmp_series_enable: the series' byte size does not fit";
  s->pm = 0;
  if (!series_mul3((uint64_t)n_env, (uint64_t)capacity, VMP_SR_NF * sizeof(double), &s->rows) ||
      (pm_rows && !series_mul3((uint64_t)n_env, (uint64_t)capacity, per_pm, &s->pm)) ||
      !series_mul3((uint64_t)n_env, VMP_SR_NMETA, sizeof(int64_t), &s->meta) ||
      !series_mul3((uint64_t)n_env, 1, sizeof(double), &s->reward))
    return "vmp_series_enable: the series' byte size does not fit";
  return nullptr;
}

// The row the step observed as the env's count-th (from 0) folds into, or -1
// if the series cannot hold it (a lost step); k_series calls it too
#ifdef __HIP__
__host__ __device__
#endif
inline int64_t series_row(int64_t count, int32_t stride, int64_t capacity) {
  const int64_t r = count / stride;
  return r < capacity ? r : -1;
}

}  // namespace vmp

#ifdef __HIP__
#include "vmp_layout.h"

namespace vmp {
struct SerArgs {
  double *rows;          // [N][cap][VMP_SR_NF]
  float *pm;             // [N][cap][2P], null without PM rows
  int64_t *meta;         // [N][VMP_SR_NMETA]; the kernels take the row index from COUNT
  int64_t cap;           // rows per env
  int32_t stride;        // steps per row
  int32_t off_used;      // k_series_lds: byte offset of the used-PM bitmap in its dynamic LDS
  const double *reward;  // this step's rewards [N]
};
// V <= 1024 and P <= 1024: one wave per env, four per block, static LDS
__global__ void k_series(EnvParams p, SerArgs a);
// any shape: one wave per block on the dynamic carve of carve_target_means,
// the used-PM bitmap at a.off_used behind it
__global__ void k_series_lds(EnvParams p, SerArgs a);
// env_mask (device u8 [N], nullable = all): the envs to (re)start
__global__ void k_series_init(EnvParams p, SerArgs a, const uint8_t *env_mask);
}  // namespace vmp
#endif

#endif  // VMP_SERIES_H
