// vmp_branch.hip — the gather kernel of vmp_branch (include/vmp.h): dst env i
// takes the three rows of src env src_of_dst[i] in 16-byte units, and where
// seeds[i] >= 0 the four PCG64 streams and the two sequence bases that k_reset
// writes for reset(seed = seeds[i]). A unit of its own: no env kernel is
// compiled with it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vmp_branch.h"
#include "vmp_layout.h"
#include "vmp_np_rng.h"

namespace vmp {

static_assert(sizeof(EnvHdr) == 16 * kBranchHdrUnits, "the header is kBranchHdrUnits units");
static_assert(offsetof(EnvHdr, rng) == 0 && offsetof(EnvHdr, seqbase) == 128,
              "k_branch patches the header's units 0..9");

// One workgroup per (dst env, chunk of kBranchChunk units). The map entry is
// read once per workgroup; an entry outside [0, src_n) keeps the env and is
// never used as an index.
__global__ __launch_bounds__(kBranchThreads) void k_branch(BranchArgs a) {
  const int64_t bid = blockIdx.x;
  const int i = (int)(bid / a.chunks);
  const int chunk = (int)(bid - (int64_t)i * a.chunks);
  if (i >= a.dst_n) return;
  const int s = a.src_of_dst[i];
  const bool take = (uint32_t)s < (uint32_t)a.src_n;
  if (chunk == 0 && threadIdx.x == 0 && a.mask) a.mask[i] = take ? 1 : 0;
  if (!take) return;

  const uint4 *sh = a.src_hdr + (int64_t)s * kBranchHdrUnits;
  const uint4 *sp = a.src_pm + (int64_t)s * a.pm_units;
  const uint4 *sv = a.src_vmw + (int64_t)s * a.vm_units;
  uint4 *dh = a.dst_hdr + (int64_t)i * kBranchHdrUnits;
  uint4 *dp = a.dst_pm + (int64_t)i * a.pm_units;
  uint4 *dv = a.dst_vmw + (int64_t)i * a.vm_units;

  uint4 val[kBranchPerLane];
  int part[kBranchPerLane];
  int64_t at[kBranchPerLane];
#pragma unroll
  for (int k = 0; k < kBranchPerLane; k++) {  // all loads first
    const int64_t u = (int64_t)chunk * kBranchChunk + k * kBranchThreads + threadIdx.x;
    part[k] = -1;
    if (u < a.units) {
      part[k] = branch_part(u, a.pm_units, &at[k]);
      const uint4 *q = part[k] == 0 ? sh + at[k] : part[k] == 1 ? sp + at[k] : sv + at[k];
      val[k] = *q;
    }
  }
  // The header is units 0..15 of chunk 0: the first wave's lanes 0..15 at k = 0.
  // Fresh streams: lanes 0..3 seed stream `lane` as k_reset does, then lane
  // 2 j takes stream j's state, lane 2 j + 1 its increment, lanes 8 and 9 the
  // states of streams 0 and 1 (the sequence bases).
  if (chunk == 0 && threadIdx.x < 64 && a.seeds) {  // wave-uniform
    const int64_t seed = a.seeds[i];
    if (seed >= 0) {
      const int lane = threadIdx.x;
      Pcg r;
      pcg_seed(r, (uint64_t)(seed + (lane & 3)));
      const int from = lane < 8 ? lane >> 1 : (lane - 8) & 3;
      const bool want_inc = lane < 8 && (lane & 1);
      const uint64_t s_hi = __shfl((unsigned long long)r.s.hi, from);
      const uint64_t s_lo = __shfl((unsigned long long)r.s.lo, from);
      const uint64_t i_hi = __shfl((unsigned long long)r.inc.hi, from);
      const uint64_t i_lo = __shfl((unsigned long long)r.inc.lo, from);
      if (lane < 10) {
        const uint64_t w0 = want_inc ? i_hi : s_hi, w1 = want_inc ? i_lo : s_lo;
        val[0] = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kBranchPerLane; k++) {
    if (part[k] < 0) continue;
    uint4 *q = part[k] == 0 ? dh + at[k] : part[k] == 1 ? dp + at[k] : dv + at[k];
    *q = val[k];
  }
}

}  // namespace vmp
