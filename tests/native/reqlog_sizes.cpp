// reqlog_sizes — the size arithmetic of the per-request outcome log
// (csrc/vmp_reqlog.h) on the CPU, under ASan + UBSan (make reqlog-sizes;
// tests/test_reqlog_cpu.py). No library, no device. UBSan turns a signed
// overflow inside the header into a failure of this program.
//  1. every refusal: no envs, no slots, capacity < 1, capacity above 2^31 - 1,
//     and products that pass 2^62 bytes, at the exact boundary;
//  2. a sweep of (n_env, V, capacity), random and at the extremes: accepted
//     requests give the sizes computed here in 128-bit arithmetic, and a
//     request is refused exactly when one of them passes the limit;
//  3. reqlog_lost against a brute-force count, and its sum over a run of steps
//     against the one-shot value.
#include <cstdint>
#include <cstdio>
#include <random>

#include "../../vm-placement-migration-gym_amd/csrc/vmp_reqlog.h"

using namespace vmp;

namespace {

int bad = 0;
void expect(bool ok, const char *what, int line) {
  if (!ok && bad++ < 20) std::printf("line %d: %s\n", line, what);
}
#define EXPECT(c) expect((c), #c, __LINE__)

typedef unsigned __int128 u128;

// what reqlog_sizes must answer, in arithmetic that cannot overflow
bool model(int32_t n, int32_t V, int64_t cap, ReqlogSizes *s) {
  if (n < 1 || V < 1 || cap < 1 || cap > kReqlogMaxCapacity) return false;
  const u128 rows = (u128)n * (u128)cap * (VMP_RQ_NF * 4), ids = (u128)n * (u128)V * 4,
             prev = (u128)n * (u128)V * 2, meta = (u128)n * VMP_RQ_NMETA * 8;
  for (u128 x : {rows, ids, prev, meta})
    if (x > (u128)kReqlogMaxBytes) return false;
  s->rows = (size_t)rows;
  s->ids = (size_t)ids;
  s->prev = (size_t)prev;
  s->meta = (size_t)meta;
  return true;
}

void check(int32_t n, int32_t V, int64_t cap) {
  ReqlogSizes got = {1, 2, 3, 4}, want = {0, 0, 0, 0};
  const bool ok = reqlog_sizes(n, V, cap, &got) == nullptr, should = model(n, V, cap, &want);
  EXPECT(ok == should);
  if (ok && should)
    EXPECT(got.rows == want.rows && got.ids == want.ids && got.prev == want.prev &&
           got.meta == want.meta);
}

}  // namespace

int main() {
  ReqlogSizes s;
  // 1. refusals and their boundaries
  EXPECT(reqlog_sizes(0, 90, 10, &s) != nullptr);
  EXPECT(reqlog_sizes(-1, 90, 10, &s) != nullptr);
  EXPECT(reqlog_sizes(8, 0, 10, &s) != nullptr);
  EXPECT(reqlog_sizes(8, 90, 0, &s) != nullptr);
  EXPECT(reqlog_sizes(8, 90, -1, &s) != nullptr);
  EXPECT(reqlog_sizes(8, 90, INT64_MIN, &s) != nullptr);
  EXPECT(reqlog_sizes(8, 90, INT64_MAX, &s) != nullptr);
  EXPECT(reqlog_sizes(8, 90, (int64_t)1 << 62, &s) != nullptr);
  EXPECT(reqlog_sizes(8, 90, kReqlogMaxCapacity + 1, &s) != nullptr);
  EXPECT(reqlog_sizes(8, 90, kReqlogMaxCapacity, &s) == nullptr);
  EXPECT(s.rows == (size_t)8 * (size_t)kReqlogMaxCapacity * 24);
  EXPECT(reqlog_sizes(1, 1, 1, &s) == nullptr && s.rows == 24 && s.ids == 4 && s.prev == 2 &&
         s.meta == 24);
  EXPECT(reqlog_sizes(8, 90, 100, &s) == nullptr && s.rows == 8 * 100 * 24 && s.ids == 8 * 90 * 4 &&
         s.prev == 8 * 90 * 2 && s.meta == 8 * 3 * 8);
  // n_env * capacity * 24 around 2^62: 2^31 - 1 envs of 2^31 - 1 rows pass it
  EXPECT(reqlog_sizes(INT32_MAX, 1, kReqlogMaxCapacity, &s) != nullptr);
  EXPECT(reqlog_sizes(INT32_MAX, INT32_MAX, 1, &s) != nullptr);  // ids: 2^64 - ...
  {
    size_t out = 7;
    EXPECT(reqlog_mul3(1ull << 31, 1ull << 31, 1, &out) && out == (size_t)1 << 62);
    EXPECT(!reqlog_mul3(1ull << 31, 1ull << 31, 2, &out));
    EXPECT(!reqlog_mul3(UINT64_MAX, UINT64_MAX, UINT64_MAX, &out));
    EXPECT(!reqlog_mul3(1ull << 32, 1ull << 32, 1, &out));
    EXPECT(!reqlog_mul3(1ull << 32, 1ull << 31, 2, &out));
    EXPECT(reqlog_mul3(0, UINT64_MAX, 1, &out) && out == 0);
    EXPECT(out == 0);
  }
  // 2. the sweep
  std::mt19937_64 g(20241);
  const int32_t ns[] = {1, 2, 8, 4096, 65536, 1 << 20, INT32_MAX - 1, INT32_MAX, 0, -5};
  const int32_t vs[] = {1, 63, 64, 65, 90, 1024, 1100, 10240, INT32_MAX, 0, -1};
  const int64_t cs[] = {1, 2, 99, 100, 1 << 20, kReqlogMaxCapacity - 1, kReqlogMaxCapacity,
                        kReqlogMaxCapacity + 1, (int64_t)1 << 40, INT64_MAX, 0, -1, INT64_MIN};
  int n_checked = 0;
  for (int32_t n : ns)
    for (int32_t V : vs)
      for (int64_t c : cs) {
        check(n, V, c);
        n_checked++;
      }
  for (int k = 0; k < 200000; k++) {
    const int32_t n = (int32_t)(g() >> (33 + g() % 31));
    const int32_t V = (int32_t)(g() >> (33 + g() % 31));
    const int64_t c = (int64_t)(g() >> (1 + g() % 63)) - (int64_t)(g() % 3);
    check(n, V, c);
    n_checked++;
  }
  // 3. the lost count
  for (int64_t cap : {1, 5, 100})
    for (int64_t a = 0; a <= 130; a++)
      for (int64_t b = a; b <= 130; b++) {
        int64_t brute = 0;
        for (int64_t id = a; id < b; id++) brute += id >= cap;
        EXPECT(reqlog_lost(a, b, cap) == brute);
      }
  for (int run = 0; run < 2000; run++) {
    const int64_t cap = 1 + (int64_t)(g() % 300);
    int64_t total = (int64_t)(g() % 200), lost = 0;
    const int64_t first = total;
    for (int step = 0; step < 50; step++) {
      const int64_t a = (int64_t)(g() % 40);
      lost += reqlog_lost(total, total + a, cap);
      total += a;
    }
    EXPECT(lost == reqlog_lost(first, total, cap));
  }
  EXPECT(reqlog_lost(INT64_MAX - 5, INT64_MAX, kReqlogMaxCapacity) == 5);
  EXPECT(reqlog_lost(0, INT64_MAX, 1) == INT64_MAX - 1);
  std::printf("reqlog sizes: %d requests checked, %d violations\n", n_checked, bad);
  if (bad) return 1;
  std::printf("reqlog sizes ok\n");
  return 0;
}
