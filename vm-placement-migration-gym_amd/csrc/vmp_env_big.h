// vmp_env_big.h — the block-per-env kernel k_env_big (V > 1024): the same
// heuristics and VmEnv.step (env.py) as vmp_env_wave.h, in the same arithmetic
// order, by one workgroup per env. Included by vmp_kernels.hip only.
#ifndef VMP_ENV_BIG_H
#define VMP_ENV_BIG_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vmp_dev.h"
#include "vmp_env_common.h"
#include "vmp_kernels.h"
#include "vmp_layout.h"
#include "vmp_stamps.h"

namespace vmp {

// ------------------------------------------------------- large-V env kernel
// V > 1024 (e.g. the P1000 / V10000 stress config): one workgroup of NT =
// 64 * NWV threads per env. Thread t owns VM slots v = s*NT + t (s < SPT), so
// slot order (s, t) is ascending VM order. The VM words live in LDS (W[v]),
// the remaining service times in registers (rem[s], only touched by fully
// unrolled loops, so they stay statically indexed: a dynamically indexed
// register array would live in scratch, which at 512 threads x 500 B per CU
// misses L2). PM-level work (fit bitmaps, BF sort, placements, frees, RNG
// draws, pairwise sums, reward) runs on wave 0 with the wave kernel's helpers;
// per-VM events that the reference applies in VM order are ranked across the
// block (row_counts + slot_rank: one barrier pair for all SPT slot rows) and
// applied by wave 0 in that order. Same arithmetic, same
// order as k_env: the two kernels are interchangeable (VMP_BIG_KERNEL=1
// forces this one for any V, which the parity tests use).
// Slot-row loops of the block kernel (s = 0..SPT-1), unrolled by 4: 4 LDS
// reads in flight per round trip (a full unroll hoists enough per-slot
// temporaries to grow the scratch from 496 to 3296 B per lane at SPT = 20;
// one row per iteration costs one LDS round trip per row).
#define VMP_SLOOP _Pragma("unroll 4")

// per-thread slot sets (bit s: slot s * kBigNT + t; kBigNT, kBigMaxSPT: vmp_carve.h)
typedef uint64_t SMask;
#define SBIT(s) ((SMask)1 << (s))
constexpr int kBigMaxWaves = kBigNT / 64;
static_assert(kBigNT % 64 == 0 && kBigNT <= 512 && kBigMaxSPT <= 64, "block shape");
// k_env_big's per-step helpers (pairwise-sum jobs, reward, draws): inlined
// (round 3: out of line, every call saved and restored the caller's live
// registers through scratch, 224 B per lane; inlined the kernel needs 193
// VGPRs instead of 250 and runs 8 % faster with the 4-row slot loops): hence
// __forceinline__ on big_sum_job, big_stats_final and big_predraw
struct BigShared {
  int32_t wcnt[16];   // per-wave counts of a compaction
  int32_t bc[8];      // broadcast scalars
  int64_t b64[4];
  int32_t rc[kBigMaxSPT * kBigMaxWaves];  // per slot row, per wave flag counts (row_counts)
  int32_t rtot[kBigMaxWaves];             // per wave flag totals
  double half[20];    // big_sum_phase: the two halves of a split job j at 2j, 2j + 1
  uint32_t fmax[kBigMaxWaves][128];  // big_heuristic: any-fit table per PM chunk
  int32_t wmin[kBigMaxWaves];         // block_min_1b
  int32_t klflag[2];                  // big_kl_sums: means of jobs 2 / 3 published
};
// k_env_big's static LDS is one Tables and one BigShared: kBigStaticLds is what
// the host's carve check (vmp_create) adds to the dynamic bytes, and equals the
// compiler's .group_segment_fixed_size of every instantiation (the two structs,
// rounded up to the 16-byte alignment of the dynamic carve behind them). The
// diagnostic builds add st_lds (-DVMP_STAMPS) and wg_marks (-DVMP_WGTIME) on top.
static_assert((sizeof(Tables) + sizeof(BigShared) + 15) / 16 * 16 == kBigStaticLds,
              "k_env_big static LDS");

// Rank of this thread's flag among the flagged threads of the block
// (ascending t) and the block total. Two barriers.
__device__ __forceinline__ int bcx_rank(bool flag, BigShared &B, int &total) {
  const int lane = lane_id(), wid = threadIdx.x >> 6, nwv = kBigNT >> 6;
  const uint64_t m = ballot(flag);
  __syncthreads();
  if (lane == 0) B.wcnt[wid] = __popcll(m);
  __syncthreads();
  int off = 0, tot = 0;
  for (int i = 0; i < nwv; i++) {
    const int c = B.wcnt[i];
    off += i < wid ? c : 0;
    tot += c;
  }
  total = tot;
  return off + below(m, lane);
}

// Flag counts of all SPT slot rows at once (bit s of fl = slot s*NT + t):
// B.rc[s][wave] and the block total. Two barriers for all rows.
// With xsum: *xsum (a per-thread int) is summed over the block on the same
// two barriers.
template <int SPT>
__device__ __forceinline__ int row_counts(SMask fl, BigShared &B, int *xsum = nullptr) {
  const int lane = lane_id(), wid = threadIdx.x >> 6, nwv = kBigNT >> 6;
  int x = 0;
  if (xsum) {
    x = *xsum;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  }
  __syncthreads();
  int wt = 0;
#pragma unroll
  for (int s = 0; s < SPT; s++) {
    const int c = __popcll(ballot((fl >> s) & 1u));
    wt += c;
    if (lane == 0) B.rc[s * kBigMaxWaves + wid] = c;
  }
  if (lane == 0) {
    B.rtot[wid] = wt;
    if (xsum) B.wcnt[wid] = x;
  }
  __syncthreads();
  int tot = 0, xt = 0;
  for (int i = 0; i < nwv; i++) {
    tot += B.rtot[i];
    if (xsum) xt += B.wcnt[i];
  }
  if (xsum) *xsum = xt;
  return tot;
}

// Rank (ascending VM order) of slot row s of this thread in the flag set
// counted by row_counts; `base` carries the flags of rows < s (start at 0 and
// call for s = 0, 1, ... in order). Valid for flagged slots only.
__device__ __forceinline__ int slot_rank(SMask fl, int s, const BigShared &B, int &base) {
  const int lane = lane_id(), wid = threadIdx.x >> 6;
  const uint64_t m = ballot((fl >> s) & 1u);
  int pre = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kBigMaxWaves; w++) {  // rows of absent waves stay 0
    const int c = B.rc[s * kBigMaxWaves + w];
    pre += w < wid ? c : 0;
    tot += c;
  }
  const int r = base + pre + below(m, lane);
  base += tot;
  return r;
}

// After row_counts: the block rank (VM order) of this wave's first flagged
// slot of row s, in lane s (s < SPT), and in `rowbase` the rank of row s's
// first flagged slot. One set of LDS reads per wave and a lane scan, instead
// of eight LDS reads per row in slot_rank; then the rank of a flagged slot in
// row s is readlane(result, s) + its position among the wave's flags.
template <int SPT>
__device__ __forceinline__ int row_prefix(const BigShared &B, int &rowbase) {
  static_assert(SPT <= 64, "one lane per slot row");
  const int lane = lane_id(), wid = threadIdx.x >> 6;
  int tot = 0, mine = 0;
  if (lane < SPT) {
#pragma unroll
    for (int w = 0; w < kBigMaxWaves; w++) {  // rows of absent waves stay 0
      const int c = B.rc[lane * kBigMaxWaves + w];
      tot += c;
      mine += w < wid ? c : 0;
    }
  }
  int incl = tot;
#pragma unroll
  for (int o = 1; o < (SPT > 32 ? 64 : 32); o <<= 1) {
    const int y = __shfl_up(incl, o);
    if (lane >= o) incl += y;
  }
  rowbase = incl - tot;
  return rowbase + mine;
}

__device__ __forceinline__ int block_sum_int(int x, BigShared &B) {
  const int lane = lane_id(), wid = threadIdx.x >> 6, nwv = kBigNT >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  __syncthreads();
  if (lane == 0) B.wcnt[wid] = x;
  __syncthreads();
  int s = 0;
  for (int i = 0; i < nwv; i++) s += B.wcnt[i];
  return s;
}

__device__ __forceinline__ int block_min_int(int x, BigShared &B) {
  const int lane = lane_id(), wid = threadIdx.x >> 6, nwv = kBigNT >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o));
  __syncthreads();
  if (lane == 0) B.wcnt[wid] = x;
  __syncthreads();
  int s = 0x7fffffff;
  for (int i = 0; i < nwv; i++) s = min(s, B.wcnt[i]);
  return s;
}

// Block-wide min with ONE barrier. Precondition: another block barrier lies
// between two calls (the resolve loop's choose barrier), so no wave can
// overwrite B.wmin while another still reads the previous call's values.
__device__ __forceinline__ int block_min_1b(int x, BigShared &B) {
  const int lane = lane_id(), wid = threadIdx.x >> 6, nwv = kBigNT >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o));
  if (lane == 0) B.wmin[wid] = x;
  __syncthreads();
  int s = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < nwv; i++) s = min(s, B.wmin[i]);
  return s;
}

// PM chunk c of the block (one per wave): PMs [c*CP, min((c+1)*CP, P)).
__device__ __forceinline__ int big_chunk_len(int P) { return (P + kBigMaxWaves - 1) / kBigMaxWaves; }

// The any-fit table of PM chunk c (build_fitmax over that chunk's PMs), built
// by the calling wave alone: the table of the whole env is the max over the
// chunks' tables, and a placement changes one PM, so only its chunk is rebuilt.
template <class MT>  // uint32_t * into the block's static LDS (BigShared)
__device__ __forceinline__ void big_build_chunk(const Lds &L, MT *M, int lo, int hi) {
  const int lane = lane_id();
  M[lane] = 0;
  M[lane + 64] = 0;
  wsync();
  for (int q = lo + lane; q < hi; q += 64) {
    const int tcq = (int)L.tc[q];
    if (tcq > 0) __atomic_fetch_max(&M[tcq - 1], (uint32_t)L.tm[q], __ATOMIC_RELAXED);
  }
  wsync();
  const int rlo = 63 - lane, rhi = 127 - lane;
  const bool hi_ok = rhi <= 100;
  uint32_t c1 = hi_ok ? M[rhi] : 0u, c0 = M[rlo];
  c1 = prefix_max32(c1);
  c0 = max(prefix_max32(c0), (uint32_t)__builtin_amdgcn_readlane((int)c1, 63));
  wsync();
  M[rlo] = c0;
  if (hi_ok) M[rhi] = c1;
  wsync();
}

// Does some PM accept sizes (c, m): the max over the chunk tables.
__device__ __forceinline__ bool big_anyfit(const BigShared &B, int c, int m) {
  uint32_t x = B.fmax[0][c];
#pragma unroll
  for (int i = 1; i < kBigMaxWaves; i++) x = max(x, B.fmax[i][c]);
  return x > (uint32_t)m;
}

// Wave 0's choice for sizes (kc, km): FirstFit's first fitting PM in index
// order (firstfit.py:33-37) or BestFit's fitting PM of largest f32 key
// (bestfit.py:33-39, ties by numpy's introsort in bf_choose). Lane l scans the
// 16 consecutive PMs [b + 16l, b + 16l + 16) of each 1024-PM block b with
// vector LDS reads (thresholds 16 B, f32 view 4 x 16 B per row), so a scan is
// one round trip per block instead of one per 64 PMs. -1 if nothing fits.
__device__ __forceinline__ int big_choose(const EnvParams &p, const Lds &L, bool bf, int kc, int km) {
  const int lane = lane_id();
  const int P = p.P;
  float best = -INFINITY;
  int cnt = 0, bi = -1, first = 0x7fffffff;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  f32x4 kfc[4], kfm[4];  // the last block's f32 view (the tie count reads it for P <= 1024)
  for (int b = 0; b < P; b += 1024) {
    const int q0 = b + 16 * lane;
    const u32x4 tcw = *reinterpret_cast<const u32x4 LDSP *>(L.tc + q0);
    const u32x4 tmw = *reinterpret_cast<const u32x4 LDSP *>(L.tm + q0);
    f32x4 fc[4], fm[4];
    if (bf) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        fc[j] = *reinterpret_cast<const f32x4 LDSP *>(L.fcpu + q0 + 4 * j);
        fm[j] = *reinterpret_cast<const f32x4 LDSP *>(L.fmem + q0 + 4 * j);
        kfc[j] = fc[j];
        kfm[j] = fm[j];
      }
    }
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int q = q0 + j;
      const int tcq = (int)((tcw[j >> 2] >> (8 * (j & 3))) & 0xFFu) - 1;
      const int tmq = (int)((tmw[j >> 2] >> (8 * (j & 3))) & 0xFFu) - 1;
      if (q < P && tcq >= kc && tmq >= km) {
        first = min(first, q);
        if (bf) {
          const float key = fc[j >> 2][j & 3] + fm[j >> 2][j & 3];  // the f32 sum bestfit.py sorts
          if (key > best) {
            best = key;
            cnt = 1;
            bi = q;
          } else if (key == best) {
            cnt++;
          }
        }
      }
    }
    if (!bf) {  // FirstFit: the first block with a fit decides
      const uint64_t f = ballot(first != 0x7fffffff);
      if (f) return __builtin_amdgcn_readlane(first, __ffsll((unsigned long long)f) - 1);
    }
  }
  if (!bf) return -1;
  float m = best;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  int tot = (best == m) ? cnt : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
  if (tot == 0) return -1;
  if (tot == 1) {
    const uint64_t who = ballot(best == m && cnt == 1);
    return __builtin_amdgcn_readlane(bi, __ffsll((unsigned long long)who) - 1);
  }
#ifdef VMP_WGTIME
  if (threadIdx.x == 0) wg_marks[23] += 1;  // tie count (timing build)
#endif
  if (P > 1024) return bf_choose(p, L, kc, km);  // tied top keys: numpy's order decides
  // one block: every key is still in this lane's registers
  int above = 0, eq = 0;
  {
    const int q0 = 16 * lane;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const float key = kfc[j >> 2][j & 3] + kfm[j >> 2][j & 3];
      above += (q0 + j < P) && key > m;
      eq += (q0 + j < P) && key == m;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    above += __shfl_xor(above, o);
    eq += __shfl_xor(eq, o);
  }
  return bf_tie(p, L, kc, km, above, eq);
}

// FirstFit / BestFit act fused with the action phase (heuristic_apply, block form).
// Per step: each wave builds the f32 view, thresholds and any-fit table of its
// PM chunk (no barrier until all are built), the pending VMs' hits are read
// from the chunk tables, and each placement costs two block barriers: the
// earliest winner (block_min_1b) and wave 0's choose + place + rebuild of the
// placed PM's chunk table.
template <int SPT>
__device__ __forceinline__ int64_t big_heuristic(const EnvParams &p, const Lds &L, const Tables &T,
                                                 BigShared &B, uint32_t LDSP *W, int policy,
                                                 int32_t *act_out, uint8_t *valid_out STAMP_PARAMS) {
  const int t = threadIdx.x, NT = kBigNT, lane = lane_id(), wid = t >> 6;
  const bool w0 = t < 64;
  const int P = p.P, WAIT = p.P;
  const bool bf = policy == 1;
  SMask pend = 0;
VMP_SLOOP
  for (int s = 0; s < SPT; s++)
    if (w_pl(W[s * NT + t]) == WAIT) pend |= SBIT(s);
  SMask won = 0, bad = 0;
  int64_t n_place = 0;
  const int CP = big_chunk_len(P);
  {  // this wave's PM chunk: f32 view, thresholds, any-fit table
    const int lo = wid * CP, hi = min(P, lo + CP);
    for (int i = lo + lane; i < hi; i += 64) {
      const float fcv = (float)L.cpu[i], fmv = (float)L.mem[i];
      L.fcpu[i] = fcv;
      L.fmem[i] = fmv;
      L.tc[i] = (uint8_t)(fit_threshold(fcv) + 1);
      L.tm[i] = (uint8_t)(fit_threshold(fmv) + 1);
    }
    wsync();
    big_build_chunk(L, B.fmax[wid], lo, hi);
  }
  __syncthreads();
  STAMP(22);
  SMask hit = 0;
  for (SMask r = pend; r; r &= r - 1) {
    const int s = __builtin_ctzll(r);
    const uint32_t w = W[s * NT + t];
    if (big_anyfit(B, w_cc(w), w_cm(w))) hit |= SBIT(s);
  }
  STAMP(17);
#pragma unroll 1
  for (;;) {
    // earliest VM (index order) with a fit: this thread's lowest hit slot
    const int mine = hit ? __builtin_ctzll(hit) * NT + t : 0x7fffffff;
    const int vw = block_min_1b(mine, B);
    if (vw == 0x7fffffff) break;
    {  // VMs before the winner never fit again (PM loads only grow)
      const int sm = vw >= t ? (vw - t) / NT : -1;  // slots s <= sm have s*NT + t <= vw
      if (sm >= 0) pend &= sm >= 63 ? (SMask)0 : ~(SBIT(sm + 1) - 1);
    }
    hit &= pend;
    const int ws = vw / NT, wt = vw - ws * NT;
    const uint32_t ww = W[vw];
    const int kc = w_cc(ww), km = w_cm(ww);
    STAMP(18);
    if (w0) {
      const int q = big_choose(p, L, bf, kc, km);
      const bool ok = env_place(L, T, P, q, kc, km);
      const int tc_old = (int)L.tc[q] - 1, tm_old = (int)L.tm[q] - 1;
      const float nc = L.fcpu[q] + T.fcent[kc];
      const float nm = bf ? L.fmem[q] + T.fcent[km] : L.fmem[q];
      const int tc_new = fit_threshold(nc), tm_new = bf ? fit_threshold(nm) : tm_old;
      wsync();
      if (lane == 0) {
        L.fcpu[q] = nc;
        L.tc[q] = (uint8_t)(tc_new + 1);
        if (bf) {
          L.fmem[q] = nm;
          L.tm[q] = (uint8_t)(tm_new + 1);
        }
        B.bc[1] = q;
        B.bc[2] = ok;
        B.bc[3] = tc_old;
        B.bc[4] = tc_new;
        B.bc[5] = tm_new;
        B.bc[7] = tm_old;
      }
      wsync();
      if (tc_new != tc_old || tm_new != tm_old) {  // q's chunk table
        const int c = q / CP;
        big_build_chunk(L, B.fmax[c], c * CP, min(P, c * CP + CP));
      }
    }
    __syncthreads();
    STAMP(19);
    const int q = B.bc[1];
    const bool ok = B.bc[2] != 0;
    n_place += ok;
    if (t == wt) {
      won |= SBIT(ws);
      if (ok) W[vw] = (ww & 0xFFFF0000u) | (uint32_t)q;
      else bad |= SBIT(ws);
      if (act_out) act_out[vw] = q;
    }
    {  // re-query the VMs q fitted before and not after
      const int tq = B.bc[4], tc_old = B.bc[3], tmq = B.bc[5], tm_old = B.bc[7];
      if (tq != tc_old || tmq != tm_old)
        for (SMask r = hit; r; r &= r - 1) {
          const int s = __builtin_ctzll(r);
          const uint32_t w = W[s * NT + t];
          const int c = w_cc(w), m = w_cm(w);
          if (c <= tc_old && m <= tm_old && !(c <= tq && m <= tmq) && !big_anyfit(B, c, m))
            hit &= ~SBIT(s);
        }
    }
  }
  if (act_out || valid_out) {
VMP_SLOOP
    for (int s = 0; s < SPT; s++) {
      const int v = s * NT + t;
      const uint32_t w = W[v];
      if (live(w)) {
        if (act_out && !((won >> s) & 1u)) act_out[v] = (int32_t)w_pl(w);
        if (valid_out) valid_out[v] = (uint8_t)!((bad >> s) & 1u);
      }
    }
  }
  __syncthreads();
  return n_place;
}

// External actions (external_apply, block form): per slot row s, the events
// are compacted in ascending VM order and applied by wave 0 one by one.
template <int SPT>
__device__ __forceinline__ void big_external(const EnvParams &p, const Lds &L, const Tables &T,
                                             BigShared &B, uint32_t LDSP *W,
                                             const int32_t *act_row, uint8_t *valid_out,
                                             int64_t &n_place, int64_t &n_susp) {
  const int t = threadIdx.x, NT = kBigNT, lane = lane_id();
  const int P = p.P, WAIT = p.P;
#pragma unroll 1
  for (int s = 0; s < SPT; s++) {
    const int v = s * NT + t;
    const uint32_t wv = W[v];
    const bool in = live(wv);
    const int c = w_pl(wv);
    const int tg = in ? act_row[v] : c;
    const bool isplace = in && c == WAIT && tg >= 0 && tg < P;
    const bool issusp = in && c < P && tg == WAIT;
    int nev = 0;
    const int r = bcx_rank(isplace || issusp, B, nev);
    if (isplace || issusp) {
      L.evw[r] = wv;
      L.evt[r] = tg;
    }
    __syncthreads();
    if (t < 64) {
#pragma unroll 1
      for (int i = 0; i < nev; i++) {  // ascending VM index
        const uint32_t ew = L.evw[i];
        const int et = L.evt[i];
        const int ec = w_pl(ew);
        const double vc = T.cent[w_cc(ew)], vm = T.cent[w_cm(ew)];
        const int q = (ec == WAIT) ? et : ec;
        double cq = L.cpu[q], mq = L.mem[q];
        bool eok = true;
        if (ec == WAIT) {
          eok = (cq + vc <= 1) && (mq + vm <= 1);
          if (eok) {
            cq = cq + vc;
            mq = mq + vm;
          }
        } else {
          cq = cq - vc;
          mq = mq - vm;
        }
        wsync();
        if (lane == 0) {
          L.cpu[q] = cq;
          L.mem[q] = mq;
          mark_pm(L, P, q);
          L.evok[i] = (uint8_t)eok;
        }
        wsync();
      }
    }
    __syncthreads();
    bool ok = (tg == c) || issusp;
    if (isplace) ok = L.evok[r] != 0;
    n_place += block_sum_int(isplace && ok, B);
    n_susp += block_sum_int(issusp, B);
    if (ok && tg != c && in) W[v] = (wv & 0xFFFF0000u) | (uint32_t)tg;
    if (valid_out && in) valid_out[v] = (uint8_t)ok;
  }
}

// The step's pairwise sums in k_env_big (env_tail's stats section, block
// form): job j computes res[j] with the numbers of env_tail (0,1 accepted
// sizes; 2,3 existing VM sizes; 4,5 PM cpu / memory; 6,7 PM squared
// deviations; 8,9 VM-size squared deviations), each by one whole wave in
// numpy's pairwise order. Out of line so its temporaries do not share the
// register budget with the block's slot arrays.
constexpr int kBigPwDepth = 6;       // register plan up to n = 7688 (6), 1928 (4)
constexpr bool kBigSplitA = false;   // split phase A's long sums too
// Job j over elements [o, o + m) of its source (the whole job: o = 0, m = n),
// result to *dst.
// spill: bit 0 the accepted sizes (jobs 0, 1), bit 1 the existing-VM sizes
// (jobs 2, 3, 8, 9) are in the env's HBM spill instead of LDS.
__device__ __forceinline__ void big_sum_job(const EnvParams &p, const Tables &T, char LDSP *base,
                                         int j, int n_ex, int o, int m, double LDSP *dst,
                                         uint32_t spill) {
  const Lds L = make_lds(p, base);
  const int P = p.P;
  double LDSP *res = L.jobres;
  const double *cent = T.cent;
  // job j's u8 source in the spill: accc | accm | ccomp | mcomp, V bytes each
  const int part = j < 2 ? j : 2 + (j & 1);
  const bool g = (spill >> (j < 2 ? 0 : 1)) & 1u;
  const uint8_t GLBP *gsrc = gptr(p.bigscr) + ((int64_t)blockIdx.x * 4 + part) * p.V + o;
  double r;
  if (j < 4) {
    const uint8_t LDSP *src = ((j == 0) ? L.accc : (j == 1) ? L.accm : ((j & 1) ? L.mcomp : L.ccomp)) + o;
    if (g) r = wave_pw_sum<kBigPwDepth>(m, [=](int i) { return cent[gsrc[i]]; }, L.pw);
    else r = wave_pw_sum<kBigPwDepth>(m, [=](int i) { return cent[src[i]]; }, L.pw);
  } else if (j < 8) {
    const double LDSP *src = ((j & 1) ? L.mem : L.cpu) + o;
    const double mean = j < 6 ? 0.0 : res[j - 2] / (double)P;
    const bool sq = j >= 6;
    r = wave_pw_sum<kBigPwDepth>(m, [=](int i) {
      const double x = src[i];
      const double d = x - mean;
      return sq ? d * d : x;
    }, L.pw);
  } else {
    const uint8_t LDSP *src = ((j & 1) ? L.mcomp : L.ccomp) + o;
    const double mean = res[j - 6] / (double)n_ex;
    if (g)
      r = wave_pw_sum<kBigPwDepth>(m, [=](int i) {
        const double d = cent[gsrc[i]] - mean;
        return d * d;
      }, L.pw);
    else
      r = wave_pw_sum<kBigPwDepth>(m, [=](int i) {
        const double d = cent[src[i]] - mean;
        return d * d;
      }, L.pw);
  }
  wsync();
  if (lane_id() == 0) *dst = r;
  wsync();
}

// The jobs of bit set `jobs` spread over the block's waves (all threads call
// it; returns after a barrier). A sum past the register plan uses the LDS
// plan, of which the carve holds one copy: those run on wave 0 in turn.
// halves: a job with n > kBigSplitMin runs as numpy's top-level split, pairwise(n) =
// pairwise(n2) + pairwise(n - n2) with n2 = n/2 - (n/2) % 8, the two halves on
// two waves and their sum formed by wave 0 after the barrier (so only wave 0
// may read those results).
__device__ __forceinline__ int big_sum_n(const EnvParams &p, int j, int k, int n_ex) {
  return j < 2 ? k : (j >= 4 && j < 8) ? p.P : n_ex;
}
// Number of wave tasks big_sum_phase deals for `jobs`.
// A job is split only when its halves save a pass: one wave sums 8 leaves of
// <= 128 elements per pass (8-lane groups), so n <= 1024 takes one pass whole.
constexpr int kBigSplitMin = 1024;
__device__ __forceinline__ int big_sum_ntask(const EnvParams &p, uint32_t jobs, int k, int n_ex,
                                             bool halves) {
  int n = 0;
  for (; jobs; jobs &= jobs - 1) n += (halves && big_sum_n(p, __builtin_ctz(jobs), k, n_ex) > kBigSplitMin) ? 2 : 1;
  return n;
}
// block_combine: the split results are formed before a block barrier (every
// wave may read them), else by wave 0 alone after it.
__device__ __forceinline__ void big_sum_phase(const EnvParams &p, const Tables &T, char LDSP *base,
                                              BigShared &B, uint32_t jobs, int k, int n_ex,
                                              bool halves, bool block_combine, uint32_t spill) {
  const int wid = threadIdx.x >> 6, nwv = kBigNT >> 6;
  double LDSP *res = reinterpret_cast<double LDSP *>(base + p.off_stage);  // L.jobres
  int slot = 0;
  uint32_t split = 0;
#pragma unroll 1
  while (jobs) {
    const int j = __builtin_ctz(jobs);
    jobs &= jobs - 1;
    const int n = big_sum_n(p, j, k, n_ex);
    const bool two = halves && n > kBigSplitMin;
    const int n2 = (n / 2) - (n / 2) % 8;
#pragma unroll 1
    for (int h = 0; h < (two ? 2 : 1); h++) {
      const int o = two && h ? n2 : 0, m = two ? (h ? n - n2 : n2) : n;
      const int w = m > pw_reg_cap(kBigPwDepth) ? 0 : (slot++ % nwv);
      double LDSP *dst = two ? (double LDSP *)&B.half[2 * j + h] : res + j;
      if (w == wid) big_sum_job(p, T, base, j, n_ex, o, m, dst, spill);
    }
    if (two) split |= 1u << j;
  }
#ifdef VMP_WGTIME
  STAMP(block_combine ? 18 : 19);  // wave 0: its sum tasks of phase A / B done
#endif
  __syncthreads();
  if (split && wid == 0) {
    if (lane_id() == 0)
      for (uint32_t s = split; s; s &= s - 1) {
        const int j = __builtin_ctz(s);
        res[j] = B.half[2 * j] + B.half[2 * j + 1];
      }
    wsync();
  }
  if (split && block_combine) __syncthreads();
}

// kl's ten sums on the block's four waves with no barrier between a plain sum
// and the squared deviations that need its mean: each wave runs the chain
// whose mean it computes itself (PM sums 4 -> 6 on wave 0, 5 -> 7 on wave 1,
// existing-VM sums 2 -> 8 on wave 2, 3 -> 9 on wave 3; the accepted sizes 0 /
// 1 on waves 0 / 1), and a VM-size job past one pass (n_ex > kBigSplitMin) is
// split at numpy's top level with its second half on wave 0 / 1 once wave 2 /
// 3 has published the mean (LDS flag). Same jobs, same order of additions as
// big_sum_phase: three passes on the longest wave instead of four.
__device__ __forceinline__ void big_kl_sums(const EnvParams &p, const Tables &T, char LDSP *base,
                                            BigShared &B, int k, int n_ex, uint32_t spill,
                                            int mark) {
  const int wid = threadIdx.x >> 6, lane = lane_id();
  double LDSP *res = reinterpret_cast<double LDSP *>(base + p.off_stage);  // L.jobres
  const bool split = n_ex > kBigSplitMin;
  const int n2 = (n_ex / 2) - (n_ex / 2) % 8;
  if (wid <= 1) {
    const int j = wid;  // 0 / 1: accepted sizes, then PM sums 4 / 5 and their squares 6 / 7
    if (k > 0) big_sum_job(p, T, base, j, n_ex, 0, k, res + j, spill);
    big_sum_job(p, T, base, 4 + j, n_ex, 0, p.P, res + 4 + j, spill);
    big_sum_job(p, T, base, 6 + j, n_ex, 0, p.P, res + 6 + j, spill);
    if (split) {
      while (__hip_atomic_load(&B.klflag[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != mark)
        __builtin_amdgcn_s_sleep(1);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      big_sum_job(p, T, base, 8 + j, n_ex, n2, n_ex - n2, (double LDSP *)&B.half[2 * (8 + j) + 1],
                  spill);
    }
  } else if (wid <= 3) {
    const int j = wid - 2;  // existing-VM sums 2 / 3, then their squared deviations 8 / 9
    big_sum_job(p, T, base, 2 + j, n_ex, 0, n_ex, res + 2 + j, spill);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (lane == 0) __hip_atomic_store(&B.klflag[j], mark, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (split)
      big_sum_job(p, T, base, 8 + j, n_ex, 0, n2, (double LDSP *)&B.half[2 * (8 + j)], spill);
    else
      big_sum_job(p, T, base, 8 + j, n_ex, 0, n_ex, res + 8 + j, spill);
  }
  __syncthreads();
  if (split && wid == 0) {
    if (lane == 0) {
      res[8] = B.half[16] + B.half[17];
      res[9] = B.half[18] + B.half[19];
    }
    wsync();
  }
}

// Wave 0 of k_env_big after the sums: reward, counters and termination.
__device__ __forceinline__ void big_stats_final(const EnvParams &p, BigShared &B, char LDSP *base,
                                             int64_t k, int n_ex, int n_w, int64_t n_term,
                                             int64_t arrivals) {
  const Lds L = make_lds(p, base);
  const int lane = lane_id();
  const int P = p.P;
  const bool kl = p.reward == 2;
  EnvHdr LDSP *H = L.hdr;
  double LDSP *res = L.jobres;
  double reward = 0.0;
  const double wr = n_ex > 0 ? (double)n_w / (double)n_ex : 0.0;
  const double r2 = kl ? res[2] : 0.0, r3 = kl ? res[3] : 0.0;
  double tcm = r2 / (double)P;
  if (p.cap_target_util && tcm > 1) tcm = 1.0;
  double tmm = r3 / (double)P;
  if (p.cap_target_util && tmm > 1) tmm = 1.0;
  if (n_ex > 0) {
    if (p.reward == 2) {
      double cv = res[6] / (double)P, mv = res[7] / (double)P;
      if (cv == 0) cv = 1e-6;
      if (mv == 0) mv = 1e-6;
      double tcv = res[8] / (double)n_ex, tmv = res[9] / (double)n_ex;
      if (tcv == 0) tcv = 1e-6;
      if (tmv == 0) tmv = 1e-6;
      reward = (tcm == 0 || tmm == 0)
                   ? 0.0
                   : kl_reward(tcm, tmm, tcv, tmv, res[4] / (double)P, res[5] / (double)P, cv, mv);
    } else if (p.reward == 1) {
      reward = p.beta * res[4] + (1 - p.beta) * res[5];
    } else {
      reward = -wr;
    }
  }
  const int64_t ts = H->timestep;
  const bool term = ts >= p.limit;
  const double a0 = k > 0 ? res[0] : 0.0, a1 = k > 0 ? res[1] : 0.0;
  wsync();
  if (lane == 0) {
    H->timestep = ts + 1;
    H->total_requests += arrivals;
    H->served += n_term;
    H->dropped += arrivals - k;
    H->waiting_ratio = wr;
    if (kl) {
      H->tcm = tcm;
      H->tmm = tmm;
    }
    if (k > 0) {
      H->total_cpu_req = H->total_cpu_req + a0;
      H->total_mem_req = H->total_mem_req + a1;
    }
    B.b64[0] = __double_as_longlong(reward);
    B.bc[6] = term;
  }
  wsync();
}

__device__ __forceinline__ void big_predraw(const EnvParams &p, const Tables &T, char LDSP *base,
                                         int K, const uint64_t *jt) {
  const Lds L = make_lds(p, base);
  const uint64_t GLBP *g = gptr(jt);
  const U128 JA{g[0], g[1]}, JM{g[2], g[3]};
  predraw(p, L, T, K, p.V, JA, JM);
}

// The env's outputs of the launch that are final once the step's accept
// phase is done: obs (VM part and PM part, env.py:295-296) and, with `state`,
// the VM words and PM resources. Issued before the stats so the stores drain
// while the pairwise sums run (the header follows at the end of the launch).
// With `state`: the low halves (placement, sizes) of the VM words that
// changed (the time words were written by big_tail as they changed).
template <int SPT>
__device__ __forceinline__ void big_store(const EnvParams &p, const Lds &L, const Tables &T,
                                          const uint32_t LDSP *W, SMask dirty, float *obs,
                                          bool state, int e) {
  const int t = threadIdx.x, NT = kBigNT;
  const int V = p.V, P = p.P;
  uint32_t *vmo = p.vmw + (int64_t)e * vm_pitch(V);
VMP_SLOOP
  for (int s = 0; s < SPT; s++) {
    const int v = s * NT + t;
    const uint32_t w = W[v];
    if (live(w)) {
      if (obs) {
        ST_NT(obs + v, (float)w_pl(w));
        ST_NT(obs + V + v, T.fcent[w_cc(w)]);
        ST_NT(obs + 2 * V + v, T.fcent[w_cm(w)]);
      }
      if (state && ((dirty >> s) & 1u)) ST_NT(vmo + vm_slot_idx(v), w);
    }
  }
  if (obs)
    for (int i = t; i < P; i += NT) {
      ST_NT(obs + 3 * V + i, (float)L.cpu[i]);
      ST_NT(obs + 3 * V + P + i, (float)L.mem[i]);
    }
  if (state) {  // the PM words written this launch (as env_body's store)
    double *pmo = p.pm + (int64_t)e * 2 * P;
    for (int i = t; i < 2 * P; i += NT)
      if ((L.pdirty[i >> 6] >> (i & 63)) & 1ull) ST_NT(pmo + i, (double)L.cpu[i]);
  }
}

// The state part of big_store from the owner's copy of its VM words (WR is a
// register array or the LDS words W, see big_tail).
template <int SPT, class WR>
__device__ __forceinline__ void big_store_words(const EnvParams &p, const Lds &L, const WR &wr,
                                                SMask dirty, int e) {
  const int t = threadIdx.x, NT = kBigNT;
  const int V = p.V, P = p.P;
  uint32_t *vmo = p.vmw + (int64_t)e * vm_pitch(V);
#pragma unroll
  for (int s = 0; s < SPT; s++)
    if (((dirty >> s) & 1u) && live(wr[s])) ST_NT(vmo + vm_slot_idx(s * NT + t), wr[s]);
  double *pmo = p.pm + (int64_t)e * 2 * P;
  for (int i = t; i < 2 * P; i += NT)
    if ((L.pdirty[i >> 6] >> (i & 63)) & 1ull) ST_NT(pmo + i, (double)L.cpu[i]);
}

// obs (env.py:295-296) from the LDS state by the threads [0, n) of a subset
// of the block's waves (thread i of them: slots i, i + n, ...).
__device__ __forceinline__ void big_store_obs(const EnvParams &p, const Lds &L, const Tables &T,
                                              const uint32_t LDSP *W, float *obs, int i, int n) {
  const int V = p.V, P = p.P;
  if (((uintptr_t)obs & 15) == 0 && (V & 3) == 0 && (P & 3) == 0) {
    // 4 consecutive VMs / PMs per thread: one 16-B LDS read of the VM words
    // and three 16-B streaming stores (a quarter of the store instructions)
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    typedef double f64x2 __attribute__((ext_vector_type(2)));
#pragma unroll 2
    for (int g = i; g < V / 4; g += n) {
      const u32x4 w = *reinterpret_cast<const u32x4 LDSP *>(W + 4 * g);
      f32x4 pl, cc, cm;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        pl[j] = (float)w_pl(w[j]);
        cc[j] = T.fcent[w_cc(w[j])];
        cm[j] = T.fcent[w_cm(w[j])];
      }
      __builtin_nontemporal_store(pl, reinterpret_cast<f32x4 GLBP *>(gptr(obs + 4 * g)));
      __builtin_nontemporal_store(cc, reinterpret_cast<f32x4 GLBP *>(gptr(obs + V + 4 * g)));
      __builtin_nontemporal_store(cm, reinterpret_cast<f32x4 GLBP *>(gptr(obs + 2 * V + 4 * g)));
    }
    for (int g = i; g < P / 4; g += n) {
      const f64x2 c0 = *reinterpret_cast<const f64x2 LDSP *>(L.cpu + 4 * g);
      const f64x2 c1 = *reinterpret_cast<const f64x2 LDSP *>(L.cpu + 4 * g + 2);
      const f64x2 m0 = *reinterpret_cast<const f64x2 LDSP *>(L.mem + 4 * g);
      const f64x2 m1 = *reinterpret_cast<const f64x2 LDSP *>(L.mem + 4 * g + 2);
      const f32x4 fc = {(float)c0[0], (float)c0[1], (float)c1[0], (float)c1[1]};
      const f32x4 fm = {(float)m0[0], (float)m0[1], (float)m1[0], (float)m1[1]};
      __builtin_nontemporal_store(fc, reinterpret_cast<f32x4 GLBP *>(gptr(obs + 3 * V + 4 * g)));
      __builtin_nontemporal_store(fm, reinterpret_cast<f32x4 GLBP *>(gptr(obs + 3 * V + P + 4 * g)));
    }
    return;
  }
#pragma unroll 4
  for (int v = i; v < V; v += n) {
    const uint32_t w = W[v];
    ST_NT(obs + v, (float)w_pl(w));
    ST_NT(obs + V + v, T.fcent[w_cc(w)]);
    ST_NT(obs + 2 * V + v, T.fcent[w_cm(w)]);
  }
  for (int q = i; q < P; q += n) {
    ST_NT(obs + 3 * V + q, (float)L.cpu[q]);
    ST_NT(obs + 3 * V + P + q, (float)L.mem[q]);
  }
}

// _run_vms, _accept_vm_requests, stats + reward, termination (env_tail, block form).
// out_obs / store_state: big_store right after the accept phase (last step of
// the launch only).
// The time words (high halves of the VM words: finish keys of running VMs,
// remaining runtimes of waiting ones, §2) are read from HBM at the start of
// each step and written back as they change (placed, suspended, finished,
// accepted), so no per-slot time registers live across the step; the low
// halves live in LDS (W) and are stored by big_store (`dirty`).
template <int SPT, int SRC>
__device__ __forceinline__ double big_tail(const EnvParams &p, const Lds &L, const Tables &T,
                                           BigShared &B, uint32_t LDSP *W, SMask run0,
                                           SMask &dirty, int kstep, bool &terminated,
                                           float *out_obs, bool store_state, bool heur,
                                           int e STAMP_PARAMS) {
  const int t = threadIdx.x, NT = kBigNT, lane = lane_id();
  const bool w0 = t < 64;
  const int P = p.P, WAIT = p.P, NUL = p.P + 1;
  EnvHdr LDSP *H = L.hdr;
  uint32_t *vw32 = p.vmw + (int64_t)e * vm_pitch(p.V);
  // ---- _run_vms: finish keys (env_tail), then free the finishers in ascending VM order ----
  const uint32_t t32 = (uint32_t)H->timestep;
  SMask fterm = 0;
  // this thread's VM words, in registers for the tail's per-slot passes (the
  // LDS copy W stays current for the cross-thread readers: frees, obs, mask)
  // (the tail reads its words from LDS: a 40-register copy pushed the kernel
  // to 256 VGPRs and spilled SGPRs to scratch, ~49 KB of scratch traffic
  // each way per env-step, 2 % slower)
  struct {
    uint32_t LDSP *W;
    int t;
    __device__ __forceinline__ uint32_t LDSP &operator[](int s) const { return W[s * kBigNT + t]; }
  } wr{W, t};
  {
    uint32_t hw[SPT];  // the time words, issued together, dead after this loop
#pragma unroll
    for (int s = 0; s < SPT; s++) hw[s] = gptr(vw32)[vm_time_idx(min(s * NT + t, p.V - 1))];
#pragma unroll
    for (int s = 0; s < SPT; s++) {
      const int v = s * NT + t;
      const bool running = w_pl(wr[s]) < P;
      uint32_t h = hw[s];
      if (running != (bool)((run0 >> s) & 1u)) {
        h = running ? h + t32 : h - t32;
        dirty |= SBIT(s);
      }
      if (running && (int32_t)(h - t32) <= 1) {
        fterm |= SBIT(s);
        h = 0;  // the word becomes NULL (below)
      }
      if (h != hw[s]) ST_NT(vw32 + vm_time_idx(v), h);  // padded slots never change
    }
  }
  dirty |= fterm;
  STAMP(8);
  const int n_term = row_counts<SPT>(fterm, B);
  STAMP(9);
  // heuristic actions never suspend, so only the PMs freed here can fall under
  // the precision clamp: they are clamped as they are freed (equal to the
  // reference's clamp after all frees: once a PM's value is < 1e-7 every
  // further free leaves it < 1e-7, and the clamp maps both to 0); external
  // actions keep the full clamp pass below
  const bool clamp_inline = heur;
#pragma unroll 1
  for (int j0 = 0; j0 < n_term; j0 += kEvCap) {
    if (ballot(fterm != 0)) {  // waves without finishers skip the ranking
      int rb;
      const int pre = row_prefix<SPT>(B, rb);
VMP_SLOOP
      for (int s = 0; s < SPT; s++) {
        const int r = __builtin_amdgcn_readlane(pre, s) + below(ballot((fterm >> s) & 1u), lane);
        if (((fterm >> s) & 1u) && r >= j0 && r < j0 + kEvCap) L.evw[r - j0] = wr[s];
      }
    }
    __syncthreads();
    if (w0) {
      const int nt = n_term - j0 < kEvCap ? n_term - j0 : kEvCap;
#pragma unroll 1
      for (int i = 0; i < nt; i++) {  // frees in ascending VM order
        const uint32_t ew = L.evw[i];
        const int q = w_pl(ew);
        double cq = L.cpu[q] - T.cent[w_cc(ew)];
        double mq = L.mem[q] - T.cent[w_cm(ew)];
        if (clamp_inline) {
          if (cq < 1e-7) cq = 0;
          if (mq < 1e-7) mq = 0;
        }
        wsync();
        if (lane == 0) {
          L.cpu[q] = cq;
          L.mem[q] = mq;
          mark_pm(L, P, q);
        }
        wsync();
      }
    }
    __syncthreads();
  }
  STAMP(10);
#pragma unroll
  for (int s = 0; s < SPT; s++)
    if ((fterm >> s) & 1u) {
      wr[s] = w_make(NUL, 0, 0);
    }
  STAMP(2);
  if (w0 && !clamp_inline)
    for (int i = lane; i < P; i += 64) {  // precision clamp
      if (L.cpu[i] < 1e-7) L.cpu[i] = 0;
      if (L.mem[i] < 1e-7) L.mem[i] = 0;
    }
  // ---- _accept_vm_requests: the first k NULL slots in VM order ----
  SMask fnull = 0;
#pragma unroll
  for (int s = 0; s < SPT; s++)
    if (w_pl(wr[s]) == NUL) fnull |= SBIT(s);
  const int n_null = row_counts<SPT>(fnull, B);
  STAMP(14);
  const int64_t arrivals = L.arr[kstep];
  const int64_t k = arrivals < n_null ? arrivals : n_null;
  // accepted sizes: LDS up to acc_cap, else the env's HBM spill (bigscr)
  const bool acc_g = k > p.acc_cap;
  uint8_t GLBP *gsc = gptr(p.bigscr) + (int64_t)e * 4 * p.V;
  if (k > 0) {
    Pcg r1 = ld_pcg(H, 0), r2 = ld_pcg(H, 1);
#pragma unroll 1
    for (int64_t j0 = 0; j0 < k; j0 += kEvCap) {
      const int64_t j1 = j0 + kEvCap < k ? j0 + kEvCap : k;
      if (SRC == kSrcTrace && w0) {
        // a traced env: wave 0 reads the chunk's requests, one per lane
        const uint64_t GLBP *req = gptr(env_trace(p, e).req) + L.svcfb[0];
#pragma unroll 1
        for (int64_t j = j0 + lane; j < j1; j += 64) {
          const uint64_t rq = req[j];
          if (acc_g) {
            gsc[j] = (uint8_t)rq_cc(rq);
            gsc[p.V + j] = (uint8_t)rq_cm(rq);
          } else {
            L.accc[j] = (uint8_t)rq_cc(rq);
            L.accm[j] = (uint8_t)rq_cm(rq);
          }
          L.evt[j - j0] = (int32_t)rq_rt(rq);
        }
      }
      if (SRC != kSrcTrace && w0) {
#pragma unroll 1
        for (int64_t j = j0; j < j1; j++) {
          const int cc = (int)rint((p.seq_lo + p.seq_range * next_double(r1)) * 100.0);
          const int cm = (int)rint((p.seq_lo + p.seq_range * next_double(r2)) * 100.0);
          const uint32_t rr = svc_take<SRC>(p, L, e);
          if (lane == 0) {
            if (acc_g) {
              gsc[j] = (uint8_t)cc;
              gsc[p.V + j] = (uint8_t)cm;
            } else {
              L.accc[j] = (uint8_t)cc;
              L.accm[j] = (uint8_t)cm;
            }
            L.evt[j - j0] = (int32_t)rr;
          }
        }
      }
      __syncthreads();
      int rb;
      const int pre = row_prefix<SPT>(B, rb);
#pragma unroll
      for (int s = 0; s < SPT; s++) {  // wr[] statically indexed
        if (__builtin_amdgcn_readlane(rb, s) >= j1) break;  // later rows rank past the accepted
        const int j = __builtin_amdgcn_readlane(pre, s) + below(ballot((fnull >> s) & 1u), lane);
        if (((fnull >> s) & 1u) && j >= j0 && j < j1) {
          const int cc = acc_g ? gsc[j] : L.accc[j], cm = acc_g ? gsc[p.V + j] : L.accm[j];
          wr[s] = w_make(WAIT, cc, cm);
          ST_NT(vw32 + vm_time_idx(s * NT + t), (uint32_t)L.evt[j - j0]);
          dirty |= SBIT(s);
        }
      }
      __syncthreads();
    }
    if (SRC != kSrcTrace && w0) {
      st_pcg(H, 0, r1);
      st_pcg(H, 1, r2);
    }
  }
  __syncthreads();
  // (a traced env: every request of the step is consumed, dropped ones too)
  if (SRC == kSrcTrace && t == 0) L.svcfb[0] += (uint64_t)arrivals;
  STAMP(15);
  // the VM words and PM resources are final: their owners store them now
  if (store_state) big_store_words<SPT>(p, L, wr, dirty, e);
  STAMP(3);
  // ---- stats + reward ----
  const bool kl = p.reward == 2;
  SMask fex = 0;
  int n_w = 0;
#pragma unroll
  for (int s = 0; s < SPT; s++) {
    const int c = w_pl(wr[s]);
    if (c <= WAIT) fex |= SBIT(s);
    n_w += c == WAIT;
  }
  const int n_ex = row_counts<SPT>(fex, B, &n_w);
  // existing-VM sizes: LDS up to ccomp_cap, else the env's HBM spill
  const bool cc_g = n_ex > p.ccomp_cap;
  if (kl) {
    int rb;
    const int pre = row_prefix<SPT>(B, rb);
    uint8_t LDSP *lc = L.ccomp, *lm = L.mcomp;
    uint8_t GLBP *gc = gsc + 2 * p.V, *gm = gsc + 3 * p.V;
#pragma unroll
    for (int s = 0; s < SPT; s++) {
      const int r = __builtin_amdgcn_readlane(pre, s) + below(ballot((fex >> s) & 1u), lane);
      if ((fex >> s) & 1u) {
        const uint32_t w = wr[s];
        if (cc_g) {
          gc[r] = (uint8_t)w_cc(w);
          gm[r] = (uint8_t)w_cm(w);
        } else {
          lc[r] = (uint8_t)w_cc(w);
          lm[r] = (uint8_t)w_cm(w);
        }
      }
    }
  }
  const uint32_t spill = (acc_g ? 1u : 0u) | (cc_g ? 2u : 0u);
  __syncthreads();
  STAMP(11);
  {  // phase A: plain sums; phase B (kl): squared deviations about their means
    const uint32_t ja = (k > 0 ? 0x3u : 0u) | (kl ? 0xCu : 0u) | (p.reward >= 1 ? 0x30u : 0u);
    // the observation is written by the waves that get no phase-A sum task
    // (task i runs on wave i), so its stores drain while the sums run
    const int nwv = NT >> 6, nj = big_sum_ntask(p, ja, (int)k, n_ex, kBigSplitA);
    if (out_obs) {
      const int ws = nj < nwv ? nj : 0;
      if ((t >> 6) >= ws) big_store_obs(p, L, T, W, out_obs, t - 64 * ws, NT - 64 * ws);
    }
#ifdef VMP_WGTIME
    STAMP(17);  // wave 0: obs issued
#endif
    // kl on four waves: chained, no phase barrier. Only wave 0 owns the LDS
    // plan of the deep pairwise sums, so the chains need every job of waves
    // 1-3 within the register plan (n <= pw_reg_cap): at P1000 / V10000
    // under 2 000 arrivals per step n_ex reaches ~10 000 and the block falls
    // back to the two phases (big_sum_phase sends those jobs to wave 0)
    constexpr int kCap = pw_reg_cap(kBigPwDepth);
    if (kl && kBigNT == 256 && n_ex <= kCap && (int)k <= kCap && p.P <= kCap) {
      big_kl_sums(p, T, L.base, B, (int)k, n_ex, spill, kstep + 1);
      STAMP(20);
      STAMP(21);
    } else {
      if (ja) big_sum_phase(p, T, L.base, B, ja, (int)k, n_ex, kBigSplitA, true, spill);
      STAMP(20);
      if (kl) big_sum_phase(p, T, L.base, B, 0x3C0u, (int)k, n_ex, true, false, spill);
      STAMP(21);
    }
  }
  if (w0) big_stats_final(p, B, L.base, k, n_ex, n_w, n_term, arrivals);
  __syncthreads();
  STAMP(12);
  const double reward = __longlong_as_double(B.b64[0]);
  terminated = B.bc[6] != 0;
  __syncthreads();
  return reward;
}

// ONE = true: the per-step launch (k_steps == 1), its own instantiation so the
// step's registers (rem[] above all) are dead after the state store instead of
// live around the K-step loop's back edge, which spilled them around the sums.
// (both instantiations are register-allocated for 2 waves per SIMD)
// WL = true: the kernel of handles with a per-env workload (env_pois).
// TR = true: of handles with a trace (vmp_set_trace: trace_preload, big_tail),
// instantiated by vmp_kernels_tr.hip alone.
template <int SPT, bool ONE, bool WL = false, bool TR = false>
__global__ __launch_bounds__(kBigNT, 2) void k_env_big(EnvParams p, StepOut o) {
  constexpr int SRC = TR ? kSrcTrace : WL ? kSrcEnv : kSrcConfig;
  extern __shared__ __align__(16) char lds[];
  __shared__ Tables T;
  __shared__ BigShared B;
  const int t = threadIdx.x, NT = kBigNT, lane = lane_id();
  const bool w0 = t < 64;
  const int e = blockIdx.x;
  const Lds L = make_lds(p, (char LDSP *)lds);
  uint32_t LDSP *W = reinterpret_cast<uint32_t LDSP *>((char LDSP *)lds + p.lds_wave_bytes);
  const int V = p.V, P = p.P;
#ifdef VMP_STAMPS
  __shared__ uint64_t st_lds[kStamps];
#endif
  STAMP_DECL_AT(w0 ? (uint64_t LDSP *)st_lds : nullptr)  // thread 0's clock
#ifdef VMP_WGTIME  // diagnostic: workgroup start / end (100 MHz) and its CU
  const uint64_t wg_t0 = __builtin_amdgcn_s_memrealtime();
  if (t < 24) wg_marks[t] = 0;
#endif
  for (int i = t; i < 128; i += NT) {
    T.cent[i] = (double)i / 100.0;
    T.fcent[i] = (float)((double)i / 100.0);
  }
  constexpr int kPoisWords = (int)(2 * sizeof(PoisConst) / 4);
  if (SRC != kSrcTrace && t < kPoisWords) reinterpret_cast<uint32_t *>(T.pois)[t] = gptr(reinterpret_cast<const uint32_t *>(env_pois<SRC>(p, e)))[t];
  // every global load of the env's state is issued before the first LDS store
  // (indices clamped, not branched on, so the loads are unconditional):
  // header, the first 4*NT PM words, the VM words
  const uint64_t hv = gptr(reinterpret_cast<const uint64_t *>(p.hdr + e))[t & 31];
  const double GLBP *pm = gptr(p.pm + (int64_t)e * 2 * P);
  const int n_pm = 2 * P;
  double pv[4];
#pragma unroll
  for (int j = 0; j < 4; j++) pv[j] = pm[min(j * NT + t, n_pm - 1)];
  const uint32_t GLBP *vmw = gptr(p.vmw + (int64_t)e * vm_pitch(V));
  __asm__ volatile("" ::: "memory");
  if (t < 32) reinterpret_cast<uint64_t LDSP *>(L.hdr)[t] = hv;
  if (w0) {
    // the random draws need only the header: wave 0 takes them while the
    // other waves load the VM words (the two never hold registers at once)
    if (o.k_steps > 0) {
      wsync();
      if constexpr (SRC == kSrcTrace) trace_preload(make_lds(p, L.base), env_trace(p, e), o.k_steps);
      else big_predraw(p, T, L.base, o.k_steps, p.jump + 4 * lane);
    }
  } else {
    // waves 1.. load the low halves of all VM words (placement, sizes) into W;
    // the time words are read by big_tail
    constexpr int kLd = kBigNT - 64, kLPT = (SPT * kBigNT + kLd - 1) / kLd;
    const int tl = t - 64;
    uint32_t wl[kLPT];
#pragma unroll
    for (int j = 0; j < kLPT; j++) wl[j] = vmw[vm_slot_idx(min(j * kLd + tl, V - 1))];
#pragma unroll
    for (int j = 0; j < kLPT; j++) {
      const int v = j * kLd + tl;
      if (v < SPT * kBigNT) W[v] = v < V ? wl[j] : (uint32_t)kPad;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (j * NT + t < n_pm) L.cpu[j * NT + t] = pv[j];
  for (int i = 4 * NT + t; i < n_pm; i += NT) L.cpu[i] = pm[i];  // P > 2 * NT
  for (int i = t; i < (n_pm + 63) / 64; i += NT) L.pdirty[i] = 0;
  for (int i = t; i < kBigMaxSPT * kBigMaxWaves; i += NT) B.rc[i] = 0;
  if (t < 2) B.klflag[t] = 0;
  __syncthreads();
  STAMP(13);
  bool term = false;
  int64_t ndone = 0;
  SMask dirty = 0;  // bit s: this thread's VM word s changed (stored by big_store)
  const int k_steps = ONE ? 1 : o.k_steps;
#pragma unroll 1
  for (int k = 0; k < k_steps; k++) {
    const bool last = k == k_steps - 1;
    uint8_t *valid_row = (last && o.valid) ? o.valid + (int64_t)e * V : nullptr;
    int32_t *act_row = (last && o.act_out) ? o.act_out + (int64_t)e * V : nullptr;
    int64_t n_place = 0, n_susp = 0;
    SMask run0 = 0;
VMP_SLOOP
    for (int s = 0; s < SPT; s++) run0 |= (SMask)(w_pl(W[s * NT + t]) < P) << s;
    if (o.policy >= 0)
      n_place = big_heuristic<SPT>(p, L, T, B, W, o.policy, act_row, valid_row STAMP_ARGS);
    else
      big_external<SPT>(p, L, T, B, W, o.actions + (int64_t)e * V, valid_row, n_place, n_susp);
    __syncthreads();
    STAMP(16);
    if (t == 0) {
      L.hdr->place_action += n_place;
      L.hdr->suspend_action += n_susp;
    }
    __syncthreads();
    const double r = big_tail<SPT, SRC>(p, L, T, B, W, run0, dirty, k, term,
                                   last && o.obs ? o.obs + (int64_t)e * p.D : nullptr, last,
                                   o.policy >= 0, e
                                   STAMP_ARGS);
    if (o.reward && t == 0) gptr(o.reward)[(int64_t)k * p.N + e] = r;
    ndone += term;
  }
  if (o.k_steps > 0) {
    if (SRC != kSrcTrace && w0) svc_commit(L);
  }
  if (o.k_steps == 0 && o.policy >= 0 && o.act_out) {
    big_heuristic<SPT>(p, L, T, B, W, o.policy, o.act_out + (int64_t)e * V, nullptr STAMP_ARGS);
    __syncthreads();
    for (int v = t; v < V; v += NT) W[v] = vmw[vm_slot_idx(v)];  // act only: placements unchanged
  }
  __syncthreads();
  STAMP(4);
  // a stepping launch stored obs and state after its last accept phase
  if (o.obs && o.k_steps == 0) big_store<SPT>(p, L, T, W, 0u, o.obs + (int64_t)e * p.D, false, e);
  if (o.mask_bits) {
    uint32_t *bits = o.mask_bits + (int64_t)e * V * p.W32;
    const int A = p.A, NW32 = p.W32, WAIT = p.P, NUL = p.P + 1;
VMP_SLOOP
    for (int s = 0; s < SPT; s++) {
      const int v = s * NT + t;
      const uint32_t wv = W[v];
      const bool in = live(wv);
      const int c = in ? w_pl(wv) : NUL;
      const double vc = T.cent[w_cc(wv)], vm = T.cent[w_cm(wv)];
      const bool waiting = in && c == WAIT;
#pragma unroll 1
      for (int w = 0; w < NW32; w++) {
        uint32_t word = 0xFFFFFFFFu;
        const int a0 = w * 32;
        if (c >= a0 && c < a0 + 32 && c < A) word &= ~(1u << (c - a0));
        if (c < P && WAIT >= a0 && WAIT < a0 + 32) word &= ~(1u << (WAIT - a0));
        if (waiting) {
          const int hi = min(a0 + 32, P);
#pragma unroll 1
          for (int q = a0; q < hi; q++) {
            const bool fit = (L.cpu[q] + vc <= 1) && (L.mem[q] + vm <= 1);
            if (fit) word &= ~(1u << (q - a0));
          }
        }
        if (in) bits[(int64_t)v * NW32 + w] = word;
      }
    }
  }
  if (o.k_steps > 0) {
    if (o.done && t == 0) gptr(o.done)[e] = (uint8_t)term;
    if (o.done_count && t == 0) gptr(o.done_count)[e] += ndone;
    if (t < 32)  // (no draw hint: EnvHdr::pad = 0)
      gptr(reinterpret_cast<uint64_t *>(p.hdr + e))[t] = t == 31 ? 0ull : reinterpret_cast<uint64_t LDSP *>(L.hdr)[t];
  }
  STAMP(6);
  STAMP_FLUSH();
#ifdef VMP_WGTIME
  __syncthreads();
  if (t == 0 && p.stamps) {
    // slots: 0 start, 1 end, 5 HW_ID, 7 XCC_ID, else the clock at STAMP(slot)
    uint64_t *o = p.stamps + (int64_t)e * 24;
    for (int i = 2; i < 24; i++) o[i] = wg_marks[i];
    o[0] = wg_t0;
    o[1] = __builtin_amdgcn_s_memrealtime();
    o[5] = (uint32_t)__builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_ID
    o[7] = (uint32_t)__builtin_amdgcn_s_getreg((31 << 11) | 20);  // XCC_ID
  }
#endif
}

// host side: launch the instantiation for `spt` slots per thread
template <bool ONE, int SRC>
static void launch_big_one(int spt, int n_env, size_t lds, hipStream_t s, const EnvParams &p,
                           const StepOut &o) {
  constexpr bool WL = SRC == kSrcEnv, TR = SRC == kSrcTrace;
  const dim3 grid(n_env), block(kBigNT);
  if (spt == 4) hipLaunchKernelGGL((k_env_big<4, ONE, WL, TR>), grid, block, lds, s, p, o);
  else if (spt == 8) hipLaunchKernelGGL((k_env_big<8, ONE, WL, TR>), grid, block, lds, s, p, o);
  else if (spt == 16) hipLaunchKernelGGL((k_env_big<16, ONE, WL, TR>), grid, block, lds, s, p, o);
  else
  hipLaunchKernelGGL((k_env_big<kBigMaxSPT, ONE, WL, TR>), grid, block, lds, s, p, o);
}

}  // namespace vmp

#endif  // VMP_ENV_BIG_H
