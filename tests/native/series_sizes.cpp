// series_sizes — the size arithmetic of the per-step time series
// (csrc/vmp_series.h) on the CPU, under ASan + UBSan (make series-sizes;
// tests/test_series_cpu.py). No library, no device. UBSan turns a signed
// overflow inside the header into a failure of this program.
//  1. every refusal: no envs, no PMs, capacity < 1 or above 2^31 - 1, stride
//     < 1, a pm_rows flag that is neither 0 nor 1, and products that pass 2^62
//     bytes, at the exact boundary;
//  2. a sweep of (n_env, P, capacity, stride, pm_rows), random and at the
//     extremes: accepted requests give the sizes computed here in 128-bit
//     arithmetic, and a request is refused exactly when one of them passes
//     the limit;
//  3. series_row against a step-by-step walk: rows fill in order, `stride`
//     steps each, and exactly the steps past the capacity are lost.
#include <cstdint>
#include <cstdio>
#include <random>

#include "../../vm-placement-migration-gym_amd/csrc/vmp_series.h"

using namespace vmp;

namespace {

int bad = 0;
void expect(bool ok, const char *what, int line) {
  if (!ok && bad++ < 20) std::printf("line %d: %s\n", line, what);
}
#define EXPECT(c) expect((c), #c, __LINE__)

typedef unsigned __int128 u128;

// what series_sizes must answer, in arithmetic that cannot overflow
bool model(int32_t n, int32_t P, int64_t cap, int32_t stride, int32_t pmr, SeriesSizes *s) {
  if (n < 1 || P < 1 || cap < 1 || cap > kSeriesMaxCapacity || stride < 1) return false;
  if (pmr != 0 && pmr != 1) return false;
  const u128 rows = (u128)n * (u128)cap * (VMP_SR_NF * 8), per = (u128)P * 2 * 4,
             pm = pmr ? (u128)n * (u128)cap * per : 0, meta = (u128)n * VMP_SR_NMETA * 8,
             reward = (u128)n * 8;
  for (u128 x : {rows, per, pm, meta, reward})
    if (x > (u128)kSeriesMaxBytes) return false;
  s->rows = (size_t)rows;
  s->pm = (size_t)pm;
  s->meta = (size_t)meta;
  s->reward = (size_t)reward;
  return true;
}

void check(int32_t n, int32_t P, int64_t cap, int32_t stride, int32_t pmr) {
  SeriesSizes got = {1, 2, 3, 4}, want = {0, 0, 0, 0};
  const bool ok = series_sizes(n, P, cap, stride, pmr, &got) == nullptr,
             should = model(n, P, cap, stride, pmr, &want);
  EXPECT(ok == should);
  if (ok && should)
    EXPECT(got.rows == want.rows && got.pm == want.pm && got.meta == want.meta &&
           got.reward == want.reward);
}

}  // namespace

int main() {
  SeriesSizes s;
  // 1. refusals and their boundaries
  EXPECT(series_sizes(0, 100, 10, 1, 0, &s) != nullptr);
  EXPECT(series_sizes(-1, 100, 10, 1, 0, &s) != nullptr);
  EXPECT(series_sizes(8, 0, 10, 1, 0, &s) != nullptr);
  EXPECT(series_sizes(8, 100, 0, 1, 0, &s) != nullptr);
  EXPECT(series_sizes(8, 100, -1, 1, 0, &s) != nullptr);
  EXPECT(series_sizes(8, 100, INT64_MIN, 1, 0, &s) != nullptr);
  EXPECT(series_sizes(8, 100, INT64_MAX, 1, 0, &s) != nullptr);
  EXPECT(series_sizes(8, 100, (int64_t)1 << 62, 1, 0, &s) != nullptr);
  EXPECT(series_sizes(8, 100, kSeriesMaxCapacity + 1, 1, 0, &s) != nullptr);
  EXPECT(series_sizes(8, 100, kSeriesMaxCapacity, 1, 0, &s) == nullptr);
  EXPECT(s.rows == (size_t)8 * (size_t)kSeriesMaxCapacity * 152 && s.pm == 0);
  EXPECT(series_sizes(8, 100, 10, 0, 0, &s) != nullptr);
  EXPECT(series_sizes(8, 100, 10, -3, 0, &s) != nullptr);
  EXPECT(series_sizes(8, 100, 10, INT32_MIN, 0, &s) != nullptr);
  EXPECT(series_sizes(8, 100, 10, INT32_MAX, 1, &s) == nullptr);
  EXPECT(series_sizes(8, 100, 10, 1, 2, &s) != nullptr);
  EXPECT(series_sizes(8, 100, 10, 1, -1, &s) != nullptr);
  EXPECT(series_sizes(1, 1, 1, 1, 1, &s) == nullptr && s.rows == 152 && s.pm == 8 && s.meta == 24 &&
         s.reward == 8);
  EXPECT(series_sizes(5, 100, 60, 7, 1, &s) == nullptr && s.rows == 5 * 60 * 152 &&
         s.pm == 5 * 60 * 800 && s.meta == 5 * 3 * 8 && s.reward == 40);
  EXPECT(series_sizes(5, 100, 60, 7, 0, &s) == nullptr && s.pm == 0);
  // n_env * capacity * 152 around 2^62
  EXPECT(series_sizes(INT32_MAX, 1, kSeriesMaxCapacity, 1, 0, &s) != nullptr);
  // ... the rows fit, the PM rows of 2^31 - 1 PMs do not
  EXPECT(series_sizes(1 << 10, INT32_MAX, 1 << 20, 1, 0, &s) == nullptr);
  EXPECT(series_sizes(1 << 10, INT32_MAX, 1 << 20, 1, 1, &s) != nullptr);
  {
    size_t out = 7;
    EXPECT(series_mul3(1ull << 31, 1ull << 31, 1, &out) && out == (size_t)1 << 62);
    EXPECT(!series_mul3(1ull << 31, 1ull << 31, 2, &out));
    EXPECT(!series_mul3(UINT64_MAX, UINT64_MAX, UINT64_MAX, &out));
    EXPECT(!series_mul3(1ull << 32, 1ull << 32, 1, &out));
    EXPECT(series_mul3(0, UINT64_MAX, 1, &out) && out == 0);
  }
  // 2. the sweep
  std::mt19937_64 g(20242);
  const int32_t ns[] = {1, 5, 4096, 1 << 20, INT32_MAX, 0, -5};
  const int32_t ps[] = {1, 10, 100, 1024, 1025, 65533, INT32_MAX, 0, -1};
  const int64_t cs[] = {1, 5, 60, 1 << 20, kSeriesMaxCapacity, kSeriesMaxCapacity + 1,
                        (int64_t)1 << 40, INT64_MAX, 0, -1, INT64_MIN};
  const int32_t ss[] = {1, 7, INT32_MAX, 0, -1};
  int n_checked = 0;
  for (int32_t n : ns)
    for (int32_t P : ps)
      for (int64_t c : cs)
        for (int32_t st : ss)
          for (int32_t pmr : {0, 1, 2}) {
            check(n, P, c, st, pmr);
            n_checked++;
          }
  for (int k = 0; k < 200000; k++) {
    const int32_t n = (int32_t)(g() >> (33 + g() % 31));
    const int32_t P = (int32_t)(g() >> (33 + g() % 31));
    const int64_t c = (int64_t)(g() >> (1 + g() % 63)) - (int64_t)(g() % 3);
    const int32_t st = (int32_t)(g() >> (33 + g() % 31)) - (int32_t)(g() % 2);
    check(n, P, c, st, (int32_t)(g() % 2));
    n_checked++;
  }
  // 3. the row of a step
  for (int64_t cap : {1, 5, 100})
    for (int32_t st : {1, 2, 7, 64}) {
      int64_t lost = 0, filled[101] = {0};
      for (int64_t count = 0; count < 3 * cap * st + 5; count++) {
        const int64_t r = series_row(count, st, cap);
        EXPECT(r >= -1 && r < cap);
        if (r < 0) {
          lost++;
          EXPECT(count >= cap * st);
        } else {
          EXPECT(r == count / st && filled[r] == count % st);
          filled[r]++;
        }
      }
      EXPECT(lost == 2 * cap * st + 5);
      for (int64_t r = 0; r < cap; r++) EXPECT(filled[r] == st);
    }
  EXPECT(series_row(INT64_MAX, 1, kSeriesMaxCapacity) == -1);
  EXPECT(series_row(INT64_MAX, INT32_MAX, kSeriesMaxCapacity) == -1);
  EXPECT(series_row((int64_t)INT32_MAX * 5 + 3, INT32_MAX, 6) == 5);
  std::printf("series sizes: %d requests checked, %d violations\n", n_checked, bad);
  if (bad) return 1;
  std::printf("series sizes ok\n");
  return 0;
}
