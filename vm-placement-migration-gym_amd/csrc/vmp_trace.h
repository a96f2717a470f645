// vmp_trace.h — the host side of trace-driven workloads (vmp_set_trace) as
// pure functions: validation of the caller's traces and env map, the packing of
// requests into the words the trace kernels read, and the content hash that
// snapshots carry. No HIP calls: tests/native/trace_pack.cpp sweeps it on the
// CPU under the host sanitizers. Included by vmp_capi.cpp.
#ifndef VMP_TRACE_H
#define VMP_TRACE_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/vmp.h"

namespace vmp {

constexpr uint32_t kTraceMaxRuntime = 1u << 30;      // finish key = timestep + runtime fits u32
constexpr int64_t kTraceMaxRequests = 0x7fffffffLL;  // per trace: a step's count fits i32

// A request as the kernels read it: the slot word's size bits (cpu << 16 |
// mem << 24, placement bits 0) in the low word, the runtime in the high word.
inline uint64_t trace_pack_req(uint8_t cpu, uint8_t mem, uint32_t runtime) {
  return ((uint64_t)runtime << 32) | ((uint64_t)mem << 24) | ((uint64_t)cpu << 16);
}

// null if (traces, map) is a valid argument of vmp_set_trace for n_env envs,
// else what is wrong with it. Reads nothing past what it has validated: the
// request arrays only up to offs[steps], once offs is known to be monotone.
inline const char *trace_check(int32_t n_traces, const vmp_trace *traces,
                               const int32_t *trace_of_env, int32_t n_env) {
  if (n_traces < 1 || !traces) return "vmp_set_trace: no traces";
  for (int32_t i = 0; i < n_traces; i++) {
    const vmp_trace &t = traces[i];
    if (t.steps < 0 || !t.offs) return "vmp_set_trace: a trace without offs";
    if (t.offs[0] != 0) return "vmp_set_trace: offs[0] must be 0";
    for (int64_t s = 0; s < t.steps; s++)
      if (t.offs[s + 1] < t.offs[s]) return "vmp_set_trace: offs must be non-decreasing";
    const int64_t n = t.offs[t.steps];
    if (n > kTraceMaxRequests) return "vmp_set_trace: a trace holds at most 2^31 - 1 requests";
    if (n > 0 && (!t.cpu || !t.mem || !t.runtime)) return "vmp_set_trace: null request array";
    for (int64_t j = 0; j < n; j++) {
      if (t.cpu[j] < 1 || t.cpu[j] > 100 || t.mem[j] < 1 || t.mem[j] > 100)
        return "vmp_set_trace: sizes are hundredths in 1..100";
      if (t.runtime[j] < 1 || t.runtime[j] > kTraceMaxRuntime)
        return "vmp_set_trace: runtimes must be in 1..2^30";
    }
  }
  if (trace_of_env)
    for (int32_t e = 0; e < n_env; e++)
      if (trace_of_env[e] < 0 || trace_of_env[e] >= n_traces)
        return "vmp_set_trace: trace_of_env entry out of range";
  return nullptr;
}

// 8-byte words of the device copy of a checked trace: offs, then the requests
inline size_t trace_words(const vmp_trace &t) { return (size_t)(t.steps + 1) + (size_t)t.offs[t.steps]; }

// The device copy of a checked trace into out[trace_words(t)]
inline void trace_pack(const vmp_trace &t, uint64_t *out) {
  for (int64_t s = 0; s <= t.steps; s++) out[s] = (uint64_t)t.offs[s];
  uint64_t *req = out + t.steps + 1;
  const int64_t n = t.offs[t.steps];
  for (int64_t j = 0; j < n; j++) req[j] = trace_pack_req(t.cpu[j], t.mem[j], t.runtime[j]);
}

// FNV-1a over the content of checked (traces, map): counts, every offs and
// packed request, and the map as the kernels see it (NULL = all trace 0)
inline uint64_t trace_hash(int32_t n_traces, const vmp_trace *traces, const int32_t *trace_of_env,
                           int32_t n_env) {
  uint64_t h = 0xcbf29ce484222325ULL;
  auto mix = [&h](uint64_t x) {
    for (int b = 0; b < 8; b++) {
      h ^= (x >> (8 * b)) & 0xFFu;
      h *= 0x100000001b3ULL;
    }
  };
  mix((uint64_t)n_traces);
  for (int32_t i = 0; i < n_traces; i++) {
    const vmp_trace &t = traces[i];
    mix((uint64_t)t.steps);
    for (int64_t s = 0; s <= t.steps; s++) mix((uint64_t)t.offs[s]);
    const int64_t n = t.offs[t.steps];
    for (int64_t j = 0; j < n; j++) mix(trace_pack_req(t.cpu[j], t.mem[j], t.runtime[j]));
  }
  mix((uint64_t)n_env);
  for (int32_t e = 0; e < n_env; e++) mix((uint64_t)(trace_of_env ? trace_of_env[e] : 0));
  return h;
}

}  // namespace vmp

#endif  // VMP_TRACE_H
