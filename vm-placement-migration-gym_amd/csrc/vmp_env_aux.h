// vmp_env_aux.h — the kernels around the step: VmEnv.reset (env.py:180-226),
// state export, _get_rank (env.py:320-325), the target means (env.py:116-121),
// counters and the bool action mask. Included by vmp_kernels.hip only.
#ifndef VMP_ENV_AUX_H
#define VMP_ENV_AUX_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vmp_dev.h"
#include "vmp_env_common.h"
#include "vmp_kernels.h"
#include "vmp_layout.h"
#include "vmp_np_rng.h"
#include "vmp_np_sum.h"

namespace vmp {

// ------------------------------------------------------------- reset -----
// VmEnv.reset (env.py:180-226) for masked envs, one wave per env.
__global__ __launch_bounds__(256) void k_reset(EnvParams p, const int64_t *seeds,
                                               const uint8_t *env_mask, float *obs) {
  const int lane = lane_id();
  const int e = uni(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
  if (e >= p.N) return;
  if (env_mask && !env_mask[e]) return;
  EnvHdr *h = p.hdr + e;
  const int V = p.V, P = p.P;
  if (lane < 4) {
    Pcg r;
    if (seeds) {
      pcg_seed(r, (uint64_t)(seeds[e] + lane));  // seed() env.py:172-178
    } else {
      r.s = U128{h->rng[lane][0], h->rng[lane][1]};
      r.inc = U128{h->rng[lane][2], h->rng[lane][3]};
      if (lane < 2) {  // sequences restart 2M draws after the last reset
        r.s = U128{h->seqbase[lane][0], h->seqbase[lane][1]};
        pcg_advance(r, (uint64_t)p.M2);
      }
    }
    h->rng[lane][0] = r.s.hi;
    h->rng[lane][1] = r.s.lo;
    h->rng[lane][2] = r.inc.hi;
    h->rng[lane][3] = r.inc.lo;
    if (lane < 2) {
      h->seqbase[lane][0] = r.s.hi;
      h->seqbase[lane][1] = r.s.lo;
    }
  }
  if (lane >= 20 && lane < 32) {
    reinterpret_cast<uint64_t *>(h)[lane] = (lane == 20) ? 1ull : 0ull;  // timestep = 1
  }
  uint32_t *vw = p.vmw + (int64_t)e * vm_pitch(V);
  for (int v = lane; v < V; v += 64) {
    vw[vm_slot_idx(v)] = (uint32_t)(P + 1);
    vw[vm_time_idx(v)] = 0u;
  }
  for (int i = lane; i < 2 * P; i += 64) p.pm[(int64_t)e * 2 * P + i] = 0.0;
  if (obs) {
    float *o = obs + (int64_t)e * p.D;
    for (int i = lane; i < p.D; i += 64) o[i] = i < V ? (float)(P + 1) : 0.0f;
  }
}

// ------------------------------------------------------- state export ----
__global__ void k_export(EnvParams p, int64_t *placement, double *vm_cpu, double *vm_mem,
                         double *cpu, double *mem, int64_t *remaining, int64_t *rank) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t nv = (int64_t)p.N * p.V;
  if (i < nv) {
    const uint32_t *vw = p.vmw + (i / p.V) * vm_pitch(p.V);
    const int v = (int)(i % p.V);
    const uint64_t w = (uint64_t)vw[vm_slot_idx(v)] | ((uint64_t)vw[vm_time_idx(v)] << 32);
    if (placement) placement[i] = (int64_t)(w & 0xFFFF);
    if (vm_cpu) vm_cpu[i] = (double)((w >> 16) & 0xFF) / 100.0;
    if (vm_mem) vm_mem[i] = (double)((w >> 24) & 0xFF) / 100.0;
    if (remaining) {  // running VMs hold their finish key F = timestep + remaining
      const int64_t hi = (int64_t)(w >> 32);
      remaining[i] = (int)(w & 0xFFFF) < p.P ? (int64_t)(uint32_t)((uint32_t)hi - (uint32_t)p.hdr[i / p.V].timestep) : hi;
    }
  }
  int64_t np_ = (int64_t)p.N * p.P;
  if (i < np_) {
    int64_t e = i / p.P, q = i % p.P;
    if (cpu) cpu[i] = p.pm[e * 2 * p.P + q];
    if (mem) mem[i] = p.pm[e * 2 * p.P + p.P + q];
  }
  if (rank && i < p.N) {  // _get_rank (env.py:320-325): distinct PMs hosting a VM
    int64_t r = 0;
    const uint32_t *row = p.vmw + i * vm_pitch(p.V);
    for (int q = 0; q < p.P; q++) {
      bool used = false;
      for (int v = 0; v < p.V && !used; v++) used = (int)(row[vm_slot_idx(v)] & 0xFFFF) == q;
      r += used;
    }
    rank[i] = r;
  }
}

// target_cpu_mean / target_memory_mean (env.py:116-121) from the stored state,
// one wave per env. Both are pure functions of the post-step state (existing =
// placement <= WAIT, their sizes in index order), so deriving them here gives
// the values step() would have left, through the same pairwise order; the step
// kernel itself computes them only for the kl reward. vmp_get_stats runs this
// before k_counters.
__global__ __launch_bounds__(256) void k_target_means(EnvParams p) {
  __shared__ uint8_t comp[kWavesPerBlock][2][kMaxVPT * 64];
  __shared__ double cent[128];
  for (int i = threadIdx.x; i < 128; i += blockDim.x) cent[i] = (double)i / 100.0;
  __syncthreads();
  const int lane = lane_id(), wid = threadIdx.x >> 6;
  const int e = uni(blockIdx.x * kWavesPerBlock + wid);
  if (e >= p.N) return;
  const int V = p.V, P = p.P;
  const uint32_t *row = p.vmw + (int64_t)e * vm_pitch(V);
  uint8_t *cc = comp[wid][0], *cm = comp[wid][1];
  int n_ex = 0;
  for (int b = 0; b < V; b += 64) {
    const int v = b + lane;
    const uint32_t w = v < V ? row[vm_slot_idx(v)] : (uint32_t)(P + 1);
    const bool ex = v < V && (int)(w & 0xFFFFu) <= P;
    const uint64_t m = ballot(ex);
    if (ex) {
      const int rk = n_ex + below(m, lane);
      cc[rk] = (uint8_t)((w >> 16) & 0xFFu);
      cm[rk] = (uint8_t)((w >> 24) & 0xFFu);
    }
    n_ex += __popcll(m);
  }
  wsync();
  const PwLds none{};  // n <= 1024: the register plan, no LDS plan needed
  const double *ct = cent;
  const double sc = wave_pw_sum(n_ex, [=](int i) { return ct[cc[i]]; }, none);
  const double sm = wave_pw_sum(n_ex, [=](int i) { return ct[cm[i]]; }, none);
  if (lane == 0) {
    double tcm = sc / (double)P, tmm = sm / (double)P;
    if (p.cap_target_util && tcm > 1) tcm = 1.0;
    if (p.cap_target_util && tmm > 1) tmm = 1.0;
    p.hdr[e].tcm = tcm;
    p.hdr[e].tmm = tmm;
  }
}

__global__ void k_counters(EnvParams p, int64_t *ctr, double *st) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.N) return;
  const EnvHdr *h = p.hdr + e;
  if (ctr) {
    int64_t *c = ctr + (int64_t)e * 6;
    c[0] = h->total_requests;
    c[1] = h->served;
    c[2] = h->suspend_action;
    c[3] = h->place_action;
    c[4] = h->dropped;
    c[5] = h->timestep;
  }
  if (st) {
    double *s = st + (int64_t)e * 5;
    s[0] = h->waiting_ratio;
    s[1] = h->tcm;
    s[2] = h->tmm;
    s[3] = h->total_cpu_req;
    s[4] = h->total_mem_req;
  }
}

__global__ void k_mask_bool(int64_t rows, int A, int W, const uint32_t *bits, uint8_t *mask) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * A) return;
  int64_t r = i / A;
  int a = (int)(i % A);
  mask[i] = (bits[r * W + (a >> 5)] >> (a & 31)) & 1u;
}

// _get_rank for any V: one wave per env, LDS bitmap of used PMs.
__global__ __launch_bounds__(64) void k_rank(EnvParams p, int64_t *rank) {
  extern __shared__ unsigned long long used[];
  const int lane = lane_id(), e = blockIdx.x;
  const int NWP = (p.P + 63) / 64;
  for (int i = lane; i < NWP; i += 64) used[i] = 0ull;
  __syncthreads();
  const uint32_t *row = p.vmw + (int64_t)e * vm_pitch(p.V);
  for (int v = lane; v < p.V; v += 64) {
    const int st = (int)(row[vm_slot_idx(v)] & 0xFFFFu);
    if (st < p.P) atomicOr(used + (st >> 6), 1ull << (st & 63));
  }
  __syncthreads();
  int64_t r = 0;
  for (int i = lane; i < NWP; i += 64) r += __popcll(used[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) r += __shfl_xor(r, o);
  if (lane == 0) rank[e] = r;
}

// target means for any V: one wave per env on the env's LDS carve (ccomp /
// mcomp and the pairwise-sum plan of make_lds).
__global__ __launch_bounds__(64) void k_target_means_lds(EnvParams p) {
  extern __shared__ __align__(16) char lds[];
  __shared__ double cent[128];
  for (int i = threadIdx.x; i < 128; i += 64) cent[i] = (double)i / 100.0;
  __syncthreads();
  const int lane = lane_id(), e = blockIdx.x;
  const Lds L = make_lds(p, (char LDSP *)lds);
  const int V = p.V, P = p.P;
  const uint32_t *row = p.vmw + (int64_t)e * vm_pitch(V);
  int n_ex = 0;
  for (int b = 0; b < V; b += 64) {
    const int v = b + lane;
    const uint32_t w = v < V ? row[vm_slot_idx(v)] : (uint32_t)(P + 1);
    const bool ex = v < V && (int)(w & 0xFFFFu) <= P;
    const uint64_t m = ballot(ex);
    if (ex) {
      const int rk = n_ex + below(m, lane);
      L.ccomp[rk] = (uint8_t)((w >> 16) & 0xFFu);
      L.mcomp[rk] = (uint8_t)((w >> 24) & 0xFFu);
    }
    n_ex += __popcll(m);
  }
  wsync();
  const double *ct = cent;
  const uint8_t LDSP *cc = L.ccomp;
  const uint8_t LDSP *cm = L.mcomp;
  const double sc = wave_pw_sum(n_ex, [=](int i) { return ct[cc[i]]; }, L.pw);
  const double sm = wave_pw_sum(n_ex, [=](int i) { return ct[cm[i]]; }, L.pw);
  if (lane == 0) {
    double tcm = sc / (double)P, tmm = sm / (double)P;
    if (p.cap_target_util && tcm > 1) tcm = 1.0;
    if (p.cap_target_util && tmm > 1) tmm = 1.0;
    p.hdr[e].tcm = tcm;
    p.hdr[e].tmm = tmm;
  }
}

// vmp_debug_launch_map: the env each workgroup of a heuristic per-step launch
// with p.pad0 takes, by the function the launch itself evaluates (one wave per
// workgroup, as there); env state is neither read nor written.
__global__ __launch_bounds__(64) void k_launch_map(EnvParams p, int32_t *env_of_block) {
  int fidx;
  const int e = uni(lo_swap_env(p, lo_position((uint32_t)p.pad0, p.N, (int)blockIdx.x), fidx));
  if (lane_id() == 0) env_of_block[blockIdx.x] = e;
}

}  // namespace vmp

#endif  // VMP_ENV_AUX_H
