// vmp_series.hip — per-step time series on the device (include/vmp.h,
// vmp_series_*): for every env one f64[VMP_SR_NF] row per window of `stride`
// observed steps, filled after each step; no per-step host copies. The data of
// the reference Record's per-step lists (src/record.py:13-32, filled by
// Base.record_testing_step, src/agents/base.py:131-149) for N envs at once. A
// third observer beside the recorder (vmp_record.hip) and the request log
// (vmp_reqlog.hip): it reads the post-step state and the step's reward, writes
// its own buffers only, and touches neither the env state nor EnvParams memory
// (EnvHdr::tcm / tmm included: the target means are recomputed here under
// every reward function).
//
// One wave per env. The step's values are wave-uniform (ballot counts, the
// pairwise sums of vmp_np_sum.h, a shuffle reduction of the bitmap's
// popcounts), so lane f < VMP_SR_NF simply keeps field f: it loads the header
// word or the reward its field needs, selects its value, and the 19 lanes
// write the row with one coalesced store (one load and one add before it for
// the float fields of a window that is already open). Every row has one
// writer: no atomics on global memory. The row index comes from the env's
// COUNT in device memory, so a replayed graph advances through the rows.
//
// CPU_SUM / MEM_SUM go through wave_pw_sum over the PM words, as the `ut`
// reward's sums do (env.py:152), the variances are np.var's two passes with
// the mean from that sum, and the target means compact the existing VMs' size
// bytes and sum them as k_target_means does (env.py:116-121).
#include <hip/hip_runtime.h>

#include "../../include/vmp.h"
#include "vmp_carve.h"
#include "vmp_dev.h"
#include "vmp_layout.h"
#include "vmp_np_sum.h"
#include "vmp_series.h"

namespace vmp {

constexpr int kSerRows = kMaxVPT;  // slot rows of 64 whose loads are issued together
constexpr int kSerMaxP = 1024;     // k_series: P of the static used-PM bitmap
constexpr int kHdrCtr = (int)(offsetof(EnvHdr, timestep) / sizeof(int64_t));
// fields TIMESTEP .. DROPPED are the header's counters in the header's order
static_assert(offsetof(EnvHdr, total_requests) == 8 * (kHdrCtr + VMP_SR_TOTAL_REQUESTS - VMP_SR_TIMESTEP) &&
                  offsetof(EnvHdr, served) == 8 * (kHdrCtr + VMP_SR_SERVED - VMP_SR_TIMESTEP) &&
                  offsetof(EnvHdr, suspend_action) == 8 * (kHdrCtr + VMP_SR_SUSPEND - VMP_SR_TIMESTEP) &&
                  offsetof(EnvHdr, place_action) == 8 * (kHdrCtr + VMP_SR_PLACE - VMP_SR_TIMESTEP) &&
                  offsetof(EnvHdr, dropped) == 8 * (kHdrCtr + VMP_SR_DROPPED - VMP_SR_TIMESTEP) &&
                  VMP_SR_DROPPED + 1 == VMP_SR_NF,
              "lane f reads counter f - VMP_SR_TIMESTEP of the header");

__device__ __forceinline__ int wsum_i(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// Env e's step by one wave. cc / cm: LDS for the existing VMs' size bytes (V
// each), used: the wave's zeroed bitmap of ceil(P/64) words, cent: k / 100.
__device__ __forceinline__ void series_step(const EnvParams &p, const SerArgs &a, int e, uint8_t *cc,
                                            uint8_t *cm, unsigned long long *used, const double *cent,
                                            const PwLds &S) {
  const int lane = lane_id();
  const int V = p.V, P = p.P, NUL = p.P + 1;
  const int64_t *hw = reinterpret_cast<const int64_t *>(p.hdr + e);
  int64_t *meta = a.meta + (int64_t)e * VMP_SR_NMETA;
  const double *pm = p.pm + (int64_t)e * 2 * P;
  const uint32_t *vw = p.vmw + (int64_t)e * vm_pitch(V);
  // ---- the loads of the step, issued together: COUNT, the lane's header word
  // or reward, the first slot rows, the PM words
  const int64_t count = meta[VMP_SR_COUNT];
  double mine = 0.0;  // the value of the lane's field where it is read, not computed
  if (lane == VMP_SR_REWARD) mine = a.reward[e];
  if (lane == VMP_SR_WAITING_RATIO) mine = p.hdr[e].waiting_ratio;
  if (lane >= VMP_SR_TIMESTEP && lane < VMP_SR_NF) mine = (double)hw[kHdrCtr + lane - VMP_SR_TIMESTEP];
  const int64_t r = series_row(count, a.stride, a.cap);  // -1: a lost step
  const bool first = count % a.stride == 0;              // opens its window
  int n_ex = 0, n_wait = 0;
  for (int v0 = 0; v0 < V; v0 += 64 * kSerRows) {
    uint32_t w[kSerRows];
#pragma unroll
    for (int s = 0; s < kSerRows; s++) {
      const int v = v0 + 64 * s + lane;
      w[s] = v < V ? vw[vm_slot_idx(v)] : (uint32_t)NUL;  // the last row may be partial
    }
#pragma unroll
    for (int s = 0; s < kSerRows; s++) {
      if (v0 + 64 * s >= V) break;  // wave-uniform
      const int pl = (int)(w[s] & 0xFFFFu);
      const bool ex = pl <= P;  // env.py:111-121 vms_existing
      const uint64_t m = ballot(ex);
      if (ex) {
        const int rk = n_ex + below(m, lane);
        cc[rk] = (uint8_t)((w[s] >> 16) & 0xFFu);
        cm[rk] = (uint8_t)((w[s] >> 24) & 0xFFu);
      }
      if (pl < P) atomicOr(used + (pl >> 6), 1ull << (pl & 63));
      n_ex += __popcll(m);
      n_wait += __popcll(ballot(pl == P));
    }
  }
  // P - count_nonzero(cpu); with PM rows, the PM part of the observation
  // (write_obs: cpu then memory as f32) into the window's row, overwritten by
  // every step of the window
  float *prow = a.pm && r >= 0 ? a.pm + ((int64_t)e * a.cap + r) * 2 * P : nullptr;
  int n_nz = 0;
  for (int i0 = 0; i0 < 2 * P; i0 += 64) {
    const int i = i0 + lane;
    const double x = i < 2 * P ? pm[i] : 0.0;
    n_nz += __popcll(ballot(i < P && x != 0.0));
    if (prow && i < 2 * P) prow[i] = (float)x;
  }
  wsync();  // cc / cm and the bitmap are complete
  int rank = 0;
  for (int i = lane; i < (P + 63) / 64; i += 64) rank += __popcll(used[i]);
  rank = wsum_i(rank);
  // ---- the pairwise sums, one inlined body per source type; lane f keeps field f
  double val = mine;
  if (lane == VMP_SR_STEPS) val = 1.0;
  if (lane == VMP_SR_USED_PM) val = (double)rank;
  if (lane == VMP_SR_EMPTY_PM) val = (double)(P - n_nz);
  if (lane == VMP_SR_WAITING) val = (double)n_wait;
  if (lane == VMP_SR_RUNNING) val = (double)(n_ex - n_wait);
#pragma unroll 1
  for (int j = 0; j < 4; j++) {  // np.sum(cpu), np.sum(memory), then np.var of each
    const double *src = pm + (j & 1) * P;
    const bool sq = j >= 2;
    const double mean = sq ? readlane_f64(val, VMP_SR_CPU_SUM + (j & 1)) / (double)P : 0.0;
    double s = wave_pw_sum(P, [=](int i) {
      const double x = src[i];
      const double d = x - mean;
      return sq ? d * d : x;
    }, S);
    if (sq) s = s / (double)P;
    if (lane == VMP_SR_CPU_SUM + j) val = s;
  }
#pragma unroll 1
  for (int j = 0; j < 2; j++) {  // target_cpu_mean, target_memory_mean
    const uint8_t *src = j ? cm : cc;
    double t = wave_pw_sum(n_ex, [=](int i) { return cent[src[i]]; }, S) / (double)P;
    if (p.cap_target_util && t > 1) t = 1.0;
    if (lane == VMP_SR_TARGET_CPU_MEAN + j) val = t;
  }
  // ---- the row: 19 lanes, one coalesced store; a window already open adds
  // the step to its float fields (one f64 add each, in step order) and takes
  // the counters as they are now
  if (r >= 0 && lane < VMP_SR_NF) {
    double *row = a.rows + ((int64_t)e * a.cap + r) * VMP_SR_NF;
    if (!first && lane < VMP_SR_TIMESTEP) val = row[lane] + val;
    row[lane] = val;
  }
  if (lane == 0) {
    meta[VMP_SR_COUNT] = count + 1;
    if (r < 0) meta[VMP_SR_LOST] += 1;
  }
}

static_assert(VMP_SR_CPU_SUM + 1 == VMP_SR_MEM_SUM && VMP_SR_CPU_SUM + 2 == VMP_SR_CPU_VAR &&
                  VMP_SR_CPU_SUM + 3 == VMP_SR_MEM_VAR &&
                  VMP_SR_TARGET_CPU_MEAN + 1 == VMP_SR_TARGET_MEM_MEAN && VMP_SR_NF <= 64,
              "series_step's loops address the fields by offset");

// V <= 1024 and P <= 1024: one wave per env, four per block; the pairwise sums
// stay in wave_pw_sum's register plan (n <= 1928).
__global__ __launch_bounds__(256) void k_series(EnvParams p, SerArgs a) {
  __shared__ uint8_t comp[4][2][kMaxVPT * 64];
  __shared__ unsigned long long used[4][kSerMaxP / 64];
  __shared__ double cent[128];
  if (threadIdx.x < 128) cent[threadIdx.x] = (double)threadIdx.x / 100.0;
  if (threadIdx.x < 4 * (kSerMaxP / 64)) (&used[0][0])[threadIdx.x] = 0ull;
  __syncthreads();
  const int wid = threadIdx.x >> 6;
  const int e = uni(blockIdx.x * 4 + wid);
  if (e >= p.N) return;  // the block's tail waves
  const PwLds none{};
  series_step(p, a, e, comp[wid][0], comp[wid][1], used[wid], cent, none);
}

// Any shape: one wave per block on the dynamic carve of carve_target_means
// (size bytes, then the LDS plan of the pairwise sums), the bitmap behind it.
__global__ __launch_bounds__(64) void k_series_lds(EnvParams p, SerArgs a) {
  extern __shared__ __align__(16) char lds[];
  __shared__ double cent[128];
  for (int i = threadIdx.x; i < 128; i += 64) cent[i] = (double)i / 100.0;
  unsigned long long *used = reinterpret_cast<unsigned long long *>(lds + a.off_used);
  for (int i = threadIdx.x; i < (p.P + 63) / 64; i += 64) used[i] = 0ull;
  __syncthreads();
  char LDSP *base = (char LDSP *)lds;
  PwLds S;
  S.lo = reinterpret_cast<int32_t LDSP *>(base + p.off_leaf);
  S.len = S.lo + p.n_leaf;
  S.stk = S.len + p.n_leaf;
  S.val = reinterpret_cast<double LDSP *>(base + p.off_leafval);
  uint8_t *cc = reinterpret_cast<uint8_t *>(lds + p.off_ccomp);
  series_step(p, a, (int)blockIdx.x, cc, cc + p.ccomp_cap, used, cent, S);
}

// (Re)start the series of every env (of those flagged in env_mask) at row 0:
// rows and PM rows cleared, FIRST = the env's timestep, COUNT = LOST = 0.
__global__ void k_series_init(EnvParams p, SerArgs a, const uint8_t *env_mask) {
  const int64_t nrow = a.cap * VMP_SR_NF, npm = a.pm ? a.cap * 2 * p.P : 0;
  const int64_t span = nrow > npm ? nrow : npm;  // >= VMP_SR_NMETA: cap >= 1
  const int64_t n = (int64_t)p.N * span;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
    const int64_t e = k / span, j = k - e * span;
    if (env_mask && !env_mask[e]) continue;
    if (j < nrow) a.rows[e * nrow + j] = 0.0;
    if (j < npm) a.pm[e * npm + j] = 0.0f;
    if (j < VMP_SR_NMETA) a.meta[e * VMP_SR_NMETA + j] = j == VMP_SR_FIRST ? p.hdr[e].timestep : 0;
  }
}

}  // namespace vmp
