// vmp_state.hip — the kernel of vmp_set_state (include/vmp.h): one workgroup
// per selected env reads the caller's reference-dtype arrays, validates the env
// as a whole and, only if every rule holds, writes its VM words, PM row and
// header. A unit of its own: no env kernel is compiled with it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vmp_layout.h"
#include "vmp_np_rng.h"
#include "vmp_state.h"

namespace vmp {

static_assert(offsetof(EnvHdr, timestep) == 8 * 20 && offsetof(EnvHdr, total_requests) == 8 * 21 &&
                  offsetof(EnvHdr, dropped) == 8 * 25 && offsetof(EnvHdr, total_cpu_req) == 8 * 26 &&
                  offsetof(EnvHdr, total_mem_req) == 8 * 27 && offsetof(EnvHdr, waiting_ratio) == 8 * 28 &&
                  offsetof(EnvHdr, pad) == 8 * 31,
              "k_set_state writes the header's 64-bit words 20..28 and 31");
static_assert(VMP_CTR_TOTAL_REQUESTS == 0 && VMP_CTR_DROPPED == 4 && VMP_CTR_TIMESTEP == 5 && VMP_NCTR == 6,
              "counter j < 5 is header word 21 + j, the timestep word 20");

namespace {

constexpr int64_t kMaxRuntime = 1 << 30;   // the trace packer's bound (vmp_trace.h)
constexpr uint32_t kNoRule = 0xffffffffu;  // above every VMP_SS_* code: no rule failed

// x is bitwise (double)k / 100.0 for an integer k in [1, 100]: k, else 0.
// NaN, infinities and negatives fail the range test first.
__device__ __forceinline__ uint32_t size_hundredths(double x) {
  if (!(x > 0.0 && x <= 1.0)) return 0u;
  const uint32_t k = (uint32_t)(x * 100.0 + 0.5);
  if (k < 1u || k > 100u) return 0u;
  return __double_as_longlong((double)k / 100.0) == __double_as_longlong(x) ? k : 0u;
}

// The first failing rule of a slot, kNoRule if none; kc / km its sizes in
// hundredths (0 for a NULL slot)
__device__ __forceinline__ uint32_t slot_rule(int P, int64_t pl, double c, double m, int64_t r,
                                              uint32_t &kc, uint32_t &km) {
  kc = km = 0u;
  if (pl < 0 || pl > (int64_t)P + 1) return VMP_SS_PLACEMENT;
  if (pl == (int64_t)P + 1) return (c == 0.0 && m == 0.0 && r == 0) ? kNoRule : VMP_SS_NULL_SLOT;
  kc = size_hundredths(c);
  km = size_hundredths(m);
  if (kc == 0u || km == 0u) return VMP_SS_VM_SIZE;
  if (r < 1 || r > kMaxRuntime) return VMP_SS_RUNTIME;
  return kNoRule;
}

}  // namespace

__global__ __launch_bounds__(kStateThreads) void k_set_state(StateArgs a) {
  extern __shared__ uint32_t lds[];
  const int e = blockIdx.x, tid = threadIdx.x;
  const int P = a.P, V = a.V;
  if (e >= a.N) return;
  if (a.env_mask && !a.env_mask[e]) {  // workgroup-uniform
    if (tid == 0) {
      if (a.status) a.status[e] = VMP_SS_SKIPPED;
      if (a.imported) a.imported[e] = 0;
    }
    return;
  }
  uint32_t *sum = lds;           // [2 P] hundredths per PM: cpu, then memory
  uint32_t *tail = lds + 2 * P;  // lowest failing rule, #waiting, #existing, timestep
  for (int i = tid; i < 2 * P + kStateLdsTail; i += kStateThreads) lds[i] = i == 2 * P ? kNoRule : 0u;
  __syncthreads();

  EnvHdr *h = a.hdr + e;
  const int64_t *pl_in = a.placement + (int64_t)e * V, *rem_in = a.remaining + (int64_t)e * V;
  const double *vc_in = a.vm_cpu + (int64_t)e * V, *vm_in = a.vm_mem + (int64_t)e * V;

  // ---- phase 1: validate; nothing of the env is stored before the verdict ----
  // Lane-consecutive 8-byte loads of the four VM arrays; the per-PM hundredths
  // are integer LDS adds, so their sums do not depend on the order.
  uint32_t bad = kNoRule, waiting = 0u, existing = 0u;
  for (int v = tid; v < V; v += kStateThreads) {
    uint32_t kc, km;
    const int64_t pl = pl_in[v];
    const uint32_t r = slot_rule(P, pl, vc_in[v], vm_in[v], rem_in[v], kc, km);
    if (r != kNoRule) {
      bad = r < bad ? r : bad;
      continue;
    }
    existing += pl <= P;
    waiting += pl == P;
    if (pl < P) {  // 0 <= pl < P holds here: inside sum[]
      atomicAdd(&sum[(int)pl], kc);
      atomicAdd(&sum[P + (int)pl], km);
    }
  }
  if (tid < VMP_NCTR) {
    if (tid == VMP_CTR_TIMESTEP) {
      const int64_t ts = a.counters ? a.counters[(int64_t)e * VMP_NCTR + tid] : h->timestep;
      if (ts < 1 || ts > 0x7fffffffLL) bad = VMP_SS_TIMESTEP < bad ? VMP_SS_TIMESTEP : bad;
      else tail[3] = (uint32_t)ts;
    } else if (a.counters && a.counters[(int64_t)e * VMP_NCTR + tid] < 0) {
      bad = VMP_SS_COUNTER < bad ? VMP_SS_COUNTER : bad;
    }
  }
  if (waiting) atomicAdd(&tail[1], waiting);
  if (existing) atomicAdd(&tail[2], existing);
  __syncthreads();  // the per-PM sums are complete
  const bool loads = a.cpu != nullptr;
  for (int q = tid; q < 2 * P; q += kStateThreads) {
    const uint32_t s = sum[q];
    uint32_t r = kNoRule;
    if (s > 100u) r = VMP_SS_CAPACITY;
    else if (loads) {
      const double x = q < P ? a.cpu[(int64_t)e * P + q] : a.mem[(int64_t)e * P + (q - P)];
      if (!(x == 0.0 || x >= 1e-7)) r = VMP_SS_LOAD_FLOOR;
      else if (!(x <= 1.0)) r = VMP_SS_LOAD_MAX;
      else if (!(fabs(x - (double)s / 100.0) < 1e-7)) r = VMP_SS_LOAD_SUM;
    }
    bad = r < bad ? r : bad;
  }
  if (bad != kNoRule) atomicMin(&tail[0], bad);
  __syncthreads();
  const uint32_t verdict = tail[0];
  if (verdict != kNoRule) {  // workgroup-uniform: refused, nothing of the env written
    if (tid == 0) {
      if (a.status) a.status[e] = (uint8_t)verdict;
      if (a.imported) a.imported[e] = 0;
    }
    return;
  }

  // ---- phase 2: pack and store (the arrays are read again, from cache) ----
  const uint32_t ts = tail[3];
  uint32_t *vw = a.vmw + (int64_t)e * vm_pitch(V);
  for (int v = tid; v < V; v += kStateThreads) {
    const int64_t pl = pl_in[v];
    uint32_t slot = (uint32_t)pl, time = 0u;
    if (pl <= P) {
      const uint32_t kc = (uint32_t)(vc_in[v] * 100.0 + 0.5), km = (uint32_t)(vm_in[v] * 100.0 + 0.5);
      slot |= kc << 16 | km << 24;
      // running: the finish key, < 2^31 + 2^30; waiting: the remaining runtime
      time = (uint32_t)rem_in[v] + (pl < P ? ts : 0u);
    }
    vw[vm_slot_idx(v)] = slot;
    vw[vm_time_idx(v)] = time;
  }
  double *pm = a.pm + (int64_t)e * 2 * P;
  for (int q = tid; q < 2 * P; q += kStateThreads)
    pm[q] = loads ? (q < P ? a.cpu[(int64_t)e * P + q] : a.mem[(int64_t)e * P + (q - P)])
                  : (double)sum[q] / 100.0;
  if (tid >= 64) return;
  // the header, by lanes of the first wave
  uint64_t *hw = reinterpret_cast<uint64_t *>(h);
  if (tid < VMP_NCTR) {
    if (a.counters)
      hw[tid == VMP_CTR_TIMESTEP ? 20 : 21 + tid] = (uint64_t)a.counters[(int64_t)e * VMP_NCTR + tid];
  } else if (tid < 8) {
    if (a.totals) (tid == 6 ? h->total_cpu_req : h->total_mem_req) = a.totals[2 * (int64_t)e + (tid - 6)];
  } else if (tid == 8) {
    const uint32_t nw = tail[1], ne = tail[2];
    h->waiting_ratio = ne ? (double)nw / (double)ne : 0.0;  // env.py:112-115
  } else if (tid == 9) {
    h->pad = 0ull;  // no hint: the next step takes the general path (vmp_layout.h's invariant)
  } else if (tid == 10) {
    if (a.status) a.status[e] = VMP_SS_IMPORTED;
    if (a.imported) a.imported[e] = 1;
  }
  if (a.seeds) {  // wave-uniform
    const int64_t seed = a.seeds[e];
    if (seed >= 0 && tid < 4) {  // the four streams and sequence bases of reset(seed), as k_reset
      Pcg r;
      pcg_seed(r, (uint64_t)(seed + tid));
      h->rng[tid][0] = r.s.hi;
      h->rng[tid][1] = r.s.lo;
      h->rng[tid][2] = r.inc.hi;
      h->rng[tid][3] = r.inc.lo;
      if (tid < 2) {
        h->seqbase[tid][0] = r.s.hi;
        h->seqbase[tid][1] = r.s.lo;
      }
    }
  }
}

}  // namespace vmp
