// trace_pack — the host side of trace-driven workloads (csrc/vmp_trace.h) on
// the CPU, under ASan + UBSan (make trace-pack; tests/test_trace_cpu.py). No
// library, no device. Every array handed to the header is an exact-size heap
// allocation, so a read past what validation allows is an ASan report.
//  1. every failure class of trace_check is refused, at the first, a middle
//     and the last position it can occur, and a trace whose request arrays are
//     shorter than a bad offs would claim is refused without being read;
//  2. random valid traces pass, pack into the layout the kernels read (offs,
//     then cpu << 16 | mem << 24 | runtime << 32 per request) and unpack to
//     their fields, and the content hash moves with every field and the map.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../vm-placement-migration-gym_amd/csrc/vmp_trace.h"

using namespace vmp;

namespace {

int bad = 0;
void expect(bool ok, const char *what, int line) {
  if (!ok && bad++ < 20) std::printf("line %d: %s\n", line, what);
}
#define EXPECT(c) expect((c), #c, __LINE__)

// One trace in exact-size heap arrays
struct Owned {
  std::unique_ptr<int64_t[]> offs;
  std::unique_ptr<uint8_t[]> cpu, mem;
  std::unique_ptr<uint32_t[]> rt;
  int64_t steps = 0, n = 0;
  vmp_trace view() const { return vmp_trace{steps, offs.get(), cpu.get(), mem.get(), rt.get()}; }
};

Owned make(std::mt19937_64 &g, int64_t steps, int max_per_step) {
  Owned o;
  o.steps = steps;
  o.offs.reset(new int64_t[(size_t)steps + 1]);
  o.offs[0] = 0;
  for (int64_t s = 0; s < steps; s++)
    o.offs[s + 1] = o.offs[s] + (int64_t)(g() % (uint64_t)(max_per_step + 1));
  o.n = o.offs[steps];
  o.cpu.reset(new uint8_t[(size_t)o.n]);
  o.mem.reset(new uint8_t[(size_t)o.n]);
  o.rt.reset(new uint32_t[(size_t)o.n]);
  for (int64_t j = 0; j < o.n; j++) {
    o.cpu[j] = (uint8_t)(1 + g() % 100);
    o.mem[j] = (uint8_t)(1 + g() % 100);
    const uint64_t r = g();
    o.rt[j] = (r & 7) == 0 ? kTraceMaxRuntime : (r & 7) == 1 ? 1u : (uint32_t)(1 + (r >> 8) % kTraceMaxRuntime);
  }
  return o;
}

bool ok(const vmp_trace &t) { return trace_check(1, &t, nullptr, 4) == nullptr; }

void failure_classes(std::mt19937_64 &g) {
  Owned o = make(g, 9, 5);
  while (o.n < 3) o = make(g, 9, 5);
  const vmp_trace t = o.view();
  EXPECT(ok(t));
  // null pointers and counts
  EXPECT(trace_check(0, &t, nullptr, 4) != nullptr);
  EXPECT(trace_check(-1, &t, nullptr, 4) != nullptr);
  EXPECT(trace_check(1, nullptr, nullptr, 4) != nullptr);
  for (int f = 0; f < 4; f++) {
    vmp_trace x = t;
    if (f == 0) x.offs = nullptr;
    if (f == 1) x.cpu = nullptr;
    if (f == 2) x.mem = nullptr;
    if (f == 3) x.runtime = nullptr;
    EXPECT(!ok(x));
  }
  {
    vmp_trace x = t;
    x.steps = -1;
    EXPECT(!ok(x));
  }
  // offs[0] != 0 and a decreasing offs at every position; the request arrays
  // stay exact-size, so validation must stop before it trusts offs[steps]
  for (int64_t s = 0; s <= o.steps; s++)
    for (int64_t d : {(int64_t)-1, (int64_t)1, (int64_t)1 << 40, -((int64_t)1 << 40)}) {
      const int64_t keep = o.offs[s];
      o.offs[s] = keep + d;
      bool mono = o.offs[0] == 0;
      for (int64_t i = 0; i < o.steps; i++) mono = mono && o.offs[i + 1] >= o.offs[i];
      // a still-monotone change of the last offset claims requests that do not exist
      if (!mono) EXPECT(!ok(o.view()));
      o.offs[s] = keep;
    }
  EXPECT(ok(o.view()));
  // sizes and runtimes out of range at the first, a middle and the last request
  for (int64_t j : {(int64_t)0, o.n / 2, o.n - 1}) {
    for (int v : {0, 101, 255}) {
      uint8_t k = o.cpu[j];
      o.cpu[j] = (uint8_t)v;
      EXPECT(!ok(o.view()));
      o.cpu[j] = k;
      k = o.mem[j];
      o.mem[j] = (uint8_t)v;
      EXPECT(!ok(o.view()));
      o.mem[j] = k;
    }
    for (uint32_t v : {0u, kTraceMaxRuntime + 1u, 0xFFFFFFFFu}) {
      const uint32_t k = o.rt[j];
      o.rt[j] = v;
      EXPECT(!ok(o.view()));
      o.rt[j] = k;
    }
  }
  EXPECT(ok(o.view()));
  // too many requests for the kernels' 32-bit step counts: refused before any request is read
  {
    std::unique_ptr<int64_t[]> offs(new int64_t[2]{0, kTraceMaxRequests + 1});
    const vmp_trace x{1, offs.get(), o.cpu.get(), o.mem.get(), o.rt.get()};
    EXPECT(!ok(x));
  }
  // the env map
  const vmp_trace two[2] = {t, t};
  std::unique_ptr<int32_t[]> map(new int32_t[4]{0, 1, 1, 0});
  EXPECT(trace_check(2, two, map.get(), 4) == nullptr);
  for (int e = 0; e < 4; e++)
    for (int32_t v : {-1, 2, 0x7fffffff}) {
      const int32_t k = map[e];
      map[e] = v;
      EXPECT(trace_check(2, two, map.get(), 4) != nullptr);
      map[e] = k;
    }
  // a second trace that is bad is found too
  {
    vmp_trace x[2] = {t, t};
    x[1].offs = nullptr;
    EXPECT(trace_check(2, x, nullptr, 4) != nullptr);
  }
  // the empty traces are valid: no steps, and steps without requests
  {
    std::unique_ptr<int64_t[]> z1(new int64_t[1]{0}), z4(new int64_t[4]{0, 0, 0, 0});
    EXPECT(ok(vmp_trace{0, z1.get(), nullptr, nullptr, nullptr}));
    EXPECT(ok(vmp_trace{3, z4.get(), nullptr, nullptr, nullptr}));
  }
}

void valid_traces(std::mt19937_64 &g, int rounds) {
  for (int r = 0; r < rounds; r++) {
    const int64_t steps = (int64_t)(g() % 40);
    Owned o = make(g, steps, r % 3 == 0 ? 0 : 1 + (int)(g() % 90));
    const vmp_trace t = o.view();
    EXPECT(ok(t));
    const size_t words = trace_words(t);
    EXPECT(words == (size_t)(steps + 1 + o.n));
    std::unique_ptr<uint64_t[]> out(new uint64_t[words]);
    trace_pack(t, out.get());
    for (int64_t s = 0; s <= steps; s++) EXPECT((int64_t)out[s] == o.offs[s]);
    for (int64_t j = 0; j < o.n; j++) {
      const uint64_t q = out[steps + 1 + j];
      EXPECT((q & 0xFFFFu) == 0);  // the placement bits of the slot word stay free
      EXPECT(((q >> 16) & 0xFFu) == o.cpu[j] && ((q >> 24) & 0xFFu) == o.mem[j]);
      EXPECT((uint32_t)(q >> 32) == o.rt[j]);
    }
    // the hash: equal for equal content, moved by every field and by the map
    std::unique_ptr<int32_t[]> map(new int32_t[3]{0, 0, 0});
    const uint64_t h0 = trace_hash(1, &t, nullptr, 3);
    EXPECT(h0 == trace_hash(1, &t, map.get(), 3));  // NULL map = all trace 0
    EXPECT(h0 != trace_hash(1, &t, nullptr, 2));
    if (o.n > 0) {
      const int64_t j = (int64_t)(g() % (uint64_t)o.n);
      o.cpu[j] = (uint8_t)(o.cpu[j] % 100 + 1);
      EXPECT(h0 != trace_hash(1, &t, nullptr, 3));
      o.cpu[j] = (uint8_t)((o.cpu[j] + 98) % 100 + 1);
      EXPECT(h0 == trace_hash(1, &t, nullptr, 3));
      o.rt[j] ^= 1u << 7;
      EXPECT(h0 != trace_hash(1, &t, nullptr, 3));
      o.rt[j] ^= 1u << 7;
    }
    const vmp_trace two[2] = {t, t};
    map[1] = 1;
    const uint64_t h2 = trace_hash(2, two, map.get(), 3);
    map[1] = 0;
    EXPECT(h2 != trace_hash(2, two, map.get(), 3));
  }
}

}  // namespace

int main() {
  std::mt19937_64 g(20240611);
  for (int i = 0; i < 20; i++) failure_classes(g);
  valid_traces(g, 400);
  std::printf("trace pack: %d violations\n", bad);
  if (bad == 0) std::printf("trace pack ok\n");
  return bad ? 1 : 0;
}
