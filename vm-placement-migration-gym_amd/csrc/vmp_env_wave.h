// vmp_env_wave.h — the wave-per-env kernels k_env / k_env_ext (V <= 1024):
// FirstFitAgent.act / BestFitAgent.act (firstfit.py, bestfit.py) fused with
// VmEnv.step (env.py:68-163, 244-293). Included by vmp_kernels.hip only.
#ifndef VMP_ENV_WAVE_H
#define VMP_ENV_WAVE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vmp_dev.h"
#include "vmp_env_common.h"
#include "vmp_kernels.h"
#include "vmp_launch_order.h"
#include "vmp_layout.h"
#include "vmp_stamps.h"

namespace vmp {

// FirstFitAgent.act / BestFitAgent.act (firstfit.py:21-38, bestfit.py:21-40)
// on the pre-step f32 observation, fused with the action phase of step().
// Exact w.r.t. the reference's sequential loop because:
//  - a waiting VM's choice is "first visiting position whose PM fits", answered
//    in O(P/64) from per-size fit bitmaps; the earliest VM (index order) with a
//    fit wins; VMs before it never fit again (loads only grow);
//  - after a FirstFit win on PM q only q's cpu threshold drops, so the cached
//    "has a fit" bit of a later VM can change only if q fitted it before and
//    not after (its first fit was then q or earlier; re-querying is exact
//    either way); BestFit changes both of q's thresholds and re-queries the
//    VMs q fitted before and not after; its target is bf_choose's argmax;
//  - the heuristic's state (f32 view) and the env's state (f64) are disjoint,
//    so applying each winner's env event as soon as it is decided equals
//    deciding every action first and stepping afterwards (env.py:68-88).
template <int VPT>
__device__ __forceinline__ int64_t heuristic_apply(const EnvParams &p, const Lds &L,
                                                   const Tables &T, uint32_t (&wa)[VPT],
                                                   int policy, int32_t *act_out,
                                                   uint8_t *valid_out, bool quiet, int qkind,
                                                   bool &fit_any, bool count_wait,
                                                   int &n_wait STAMP_PARAMS) {
  const int lane = lane_id();
  const int P = p.P, WAIT = p.P;
  const bool bf = policy == 1;
  uint32_t pend = 0;
#pragma unroll
  for (int s = 0; s < VPT; s++)
    if (w_pl(wa[s]) == WAIT) pend |= 1u << s;
  // count_wait (a launch's first step): the number of waiting VMs before the
  // action phase, the start of the n_w that env_tail carries
  if (count_wait) n_wait = (int)wave_sum32((uint32_t)__popc(pend));
  uint32_t won = 0, bad = 0;
  int64_t n_place = 0;
  fit_any = false;
  // quiet: skip the heuristic. qkind 1 (EnvHdr::pad bit 62): the previous
  // step found no pending VM that fits any PM, and since then no VM finished
  // (no PM load fell) and none arrived (no new pending VM): nothing fits now
  // either, so the heuristic places nothing and the any-fit table need not
  // be built. qkind 2 (bit 60): the previous step's placements were all
  // invalid in f64 (the f32 observation said they fit: a PM loaded to within
  // rounding of 1) and nothing finished or arrived, so the step sees the same
  // observation, makes the same decisions and the env rejects them again -
  // env_body takes this skip only where no actions / validity flags are
  // returned. The check build (-DVMP_CHECK_QUIET) runs the heuristic anyway
  // and counts the skippable steps in which some pending VM fits (qkind 1)
  // or some placement is valid (qkind 2) (vmp_debug_quiet_violations): 0
  // unless a writer of the env state left a stale bit (see EnvHdr::pad).
#ifdef VMP_CHECK_QUIET
  if (ballot(pend != 0)) {
#else
  if (!quiet && ballot(pend != 0)) {
#endif
    for (int i = lane; i < P; i += 64) {
      const float fcv = (float)L.cpu[i], fmv = (float)L.mem[i];
      L.fcpu[i] = fcv;
      L.fmem[i] = fmv;
      L.tc[i] = (uint8_t)(fit_threshold(fcv) + 1);
      L.tm[i] = (uint8_t)(fit_threshold(fmv) + 1);
    }
    wsync();
    STAMP(16);
    uint32_t hit = 0;  // bit s: VM slot s of this lane is pending and some PM fits it
    // the any-fit table M (build_fitmax) answers "does some PM accept (c, m)";
    // it is rebuilt after each placement (only the placed PM's thresholds move)
    uint32_t LDSP *M = reinterpret_cast<uint32_t LDSP *>(L.bc);
    build_fitmax(p, L, M);
#pragma unroll
    for (int s = 0; s < VPT; s++)
      hit |= (uint32_t)(((pend >> s) & 1u) && M[w_cc(wa[s])] > (uint32_t)w_cm(wa[s])) << s;
    const bool anyfit = ballot(hit != 0) != 0;
    fit_any = anyfit;
#ifdef VMP_CHECK_QUIET
    if (quiet && qkind == 1 && anyfit && lane == 0)
      __hip_atomic_fetch_add(gptr(&g_quiet_violations), 1ull, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
#endif
    STAMP(17);
#pragma unroll 1
    for (; anyfit;) {
      // earliest VM (index order s * 64 + lane) with a fit: each lane's lowest
      // hit slot, then a DPP max over the wave of (2047 - index)
      const int mine = hit ? (__builtin_ctz(hit) << 6) | lane : 2047;
      const int best = 2047 - (int)__builtin_amdgcn_readlane(
                                  (int)prefix_max32((uint32_t)(2047 - mine)), 63);
      STAMP(18);
      if (best == 2047) break;
      const int ws = best >> 6, wl = best & 63;
      uint32_t own = 0;
#pragma unroll
      for (int s = 0; s < VPT; s++)
        if (s == ws) own = wa[s];
      const uint32_t ww = rdlane(own, wl);
      // everything up to and including the winner is decided
#pragma unroll
      for (int s = 0; s < VPT; s++)
        if (s < ws || (s == ws && lane <= wl)) pend &= ~(1u << s);
      hit &= pend;
      const int kc = w_cc(ww), km = w_cm(ww);
      const int q = bf ? bf_choose(p, L, kc, km) : ff_scan(p, L, kc, km);  // wave-uniform
      // the env event (env.py:55-64: _resource_valid in f64, _place_vm) and the
      // heuristic's own f32 update (FF: cpu only, firstfit.py:36) read and
      // write disjoint state: one LDS round trip, one write-back
      const double cq = L.cpu[q], mq = L.mem[q];
      const float fq = L.fcpu[q], fmq = L.fmem[q];
      const int tc_old = (int)L.tc[q] - 1, tm_old = (int)L.tm[q] - 1;
      const double vc = T.cent[kc], vm = T.cent[km];
      const bool ok = (cq + vc <= 1) && (mq + vm <= 1);
      const float nc = fq + T.fcent[kc];
      const float nm = fmq + T.fcent[km];
      const int t = fit_threshold(nc);
      const int tmq = bf ? fit_threshold(nm) : tm_old;
      wsync();
      if (lane == 0) {
        if (ok) {
          L.cpu[q] = cq + vc;
          L.mem[q] = mq + vm;
          mark_pm(L, P, q);
        }
        L.fcpu[q] = nc;
        L.tc[q] = (uint8_t)(t + 1);
        if (bf) {
          L.fmem[q] = nm;
          L.tm[q] = (uint8_t)(tmq + 1);
        }
      }
      wsync();
      n_place += ok;
      STAMP(20);
      if (lane == wl) {
#pragma unroll
        for (int s = 0; s < VPT; s++)
          if (s == ws) {
            won |= 1u << s;
            if (ok) wa[s] = (wa[s] & 0xFFFF0000u) | (uint32_t)q;
            else bad |= 1u << s;
          }
        if (act_out) gptr(act_out)[ws * 64 + wl] = q;
      }
      STAMP(21);
      if (t < tc_old || tmq < tm_old) {  // q's thresholds fell: the table changes
        build_fitmax(p, L, M);
        STAMP(23);
        // re-query the VMs still pending with a fit (M is exact: "some PM
        // accepts (c, m)"), table reads batched four slots at a time
#pragma unroll
        for (int s0 = 0; s0 < VPT; s0 += 4) {
          uint32_t mc[4];
#pragma unroll
          for (int j = 0; j < 4; j++) mc[j] = s0 + j < VPT ? M[w_cc(wa[s0 + j])] : 0u;
#pragma unroll
          for (int j = 0; j < 4; j++)
            if (s0 + j < VPT && !(mc[j] > (uint32_t)w_cm(wa[s0 + j]))) hit &= ~(1u << (s0 + j));
        }
      }
      STAMP(19);
    }
  }
#ifdef VMP_CHECK_QUIET
  if (quiet && qkind == 2 && n_place > 0 && lane == 0)
    __hip_atomic_fetch_add(gptr(&g_quiet_violations), 1ull, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
#endif
  if (act_out || valid_out) {
    const int ln = fresh_lane();
#pragma unroll
    for (int s = 0; s < VPT; s++) {
      const int v = s * 64 + ln;
      if (live(wa[s])) {
        if (act_out && !((won >> s) & 1u)) gptr(act_out)[v] = (int32_t)w_pl(wa[s]);
        if (valid_out) gptr(valid_out)[v] = (uint8_t)!((bad >> s) & 1u);
      }
    }
  }
  return n_place;
}

// Action phase of step() for external actions (env.py:68-88): per slot of 64
// VMs, the events (WAIT -> PM place attempts, PM -> WAIT suspends) are applied
// in ascending VM order by a wave-uniform loop over the ballot.
template <int VPT>
__device__ __forceinline__ void external_apply(const EnvParams &p, const Lds &L, const Tables &T,
                                               uint32_t (&wa)[VPT], const int32_t *act_row,
                                               uint8_t *valid_out, int64_t &n_place,
                                               int64_t &n_susp, int &n_wait) {
  const int lane = lane_id();
  const int P = p.P, WAIT = p.P;
  int n_wait0 = 0;
  // all action loads issued at once, unconditionally (clamped index) and
  // through the global address space: one wait for all of them instead of a
  // conditional load + wait per slot row
  const int32_t GLBP *ar = gptr(act_row);
  int32_t tv[VPT];
  __asm__ volatile("" ::: "memory");  // not hoisted above the prologue's draws
#pragma unroll
  for (int s = 0; s < VPT; s++) tv[s] = ar[min(s * 64 + lane, p.V - 1)];
#pragma unroll
  for (int s = 0; s < VPT; s++) {
    const int v = s * 64 + lane;
    const bool in = live(wa[s]);
    const int c = w_pl(wa[s]);
    const int t = in ? tv[s] : c;
    // the waiting VMs before the action phase (a pad word's placement is
    // kPad); a scalar count: this kernel has no VGPR to spare at VPT 1
    n_wait0 += __popcll(ballot(c == WAIT));
    const bool isplace = in && c == WAIT && t >= 0 && t < P;
    const bool issusp = in && c < P && t == WAIT;
    uint64_t evm = ballot(isplace || issusp);
    uint64_t okm = 0;
    const uint32_t me = wa[s];
#pragma unroll 1
    while (evm) {  // wave-uniform, ascending lane = ascending VM index
      const int l = __ffsll((unsigned long long)evm) - 1;
      evm &= evm - 1;
      const uint32_t ew = rdlane(me, l);
      const int et = __builtin_amdgcn_readlane(t, l);
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
      }
      okm |= (uint64_t)eok << l;
      wsync();
    }
    bool ok = (t == c) || issusp;
    if (isplace) ok = (okm >> lane) & 1ull;
    n_place += __popcll(okm & ballot(isplace));
    n_susp += __popcll(ballot(issusp));
    if (ok && t != c && in) wa[s] = (wa[s] & 0xFFFF0000u) | (uint32_t)t;
    if (valid_out && in) gptr(valid_out)[v] = (uint8_t)ok;
  }
  n_wait = n_wait0;
}

// Everything of step() after the action phase: _run_vms, _accept_vm_requests,
// stats + reward, termination (env.py:101, 108-163, 244-293).
// LAZY (the per-step launch): the high words are not held in registers. `fb`
// bit s says whether slot s finishes this step if it runs (running: F - t <= 1;
// waiting: remaining <= 1, i.e. placed now it finishes now), accepted words are
// stored at once through `vmo`, and the caller fixes the finish keys of placed /
// suspended VMs in memory; rem[] is then unused.
// The VM counts of the stats come from the step's events, not from a sweep of
// the slot words: n_w (in: the waiting VMs before this step's action phase;
// out: after the step) moves by the n_susp suspensions, the n_place accepted
// placements and the k accepted requests, and null_left (out) = n_null - k is
// the number of NULL slots the step leaves, so V - null_left VMs exist.
template <int VPT, bool LAZY, int SRC, bool EXTK>
__device__ __forceinline__ double env_tail(const EnvParams &p, const Lds &L, const Tables &T,
                                           uint32_t (&wa)[VPT], uint32_t (&rem)[VPT],
                                           uint32_t run0, uint32_t fb, uint32_t &dirty,
                                           uint32_t *vmo, int kstep,
                                           bool quiet_in, int64_t n_place, int64_t n_susp,
                                           int &n_w, int &null_left, bool &terminated,
                                           bool &calm, bool &has_ex, int e STAMP_PARAMS) {
  const int lane = lane_id();
  const int P = p.P, WAIT = p.P, NUL = p.P + 1;
  EnvHdr LDSP *H = L.hdr;
  // ---- _run_vms (env.py:244-268) ----
  // A running VM's word holds its finish key F = t + remaining (t = this
  // step's timestep), so the per-step decrement of every running VM is implicit
  // and its word is not rewritten; waiting VMs hold the remaining runtime
  // itself. The action phase only moves VMs between WAIT and a PM (external
  // migrations PM -> PM' are invalid, env.py:35-44), so run0 (running before the
  // action phase) tells which words switch representation.
  const uint32_t t32 = (uint32_t)H->timestep;
  int64_t n_term = 0;
  // LAZY: the running slots after the action phase as a mask. The step's only
  // WAIT -> PM / PM -> WAIT moves are its n_place accepted placements and
  // n_susp suspensions, so without either the mask is run0 and no word
  // switches representation; and where no lane has a finish bit among its
  // running slots (one ballot) no VM finishes, and the per-slot loop is skipped.
  uint32_t run1 = run0;
  bool any_fin = true;
  if (LAZY) {
    if (n_place != 0 || n_susp != 0) {
      run1 = 0;
#pragma unroll
      for (int s = 0; s < VPT; s++) run1 |= (uint32_t)(w_pl(wa[s]) < P) << s;
      dirty |= run1 ^ run0;
    }
    any_fin = ballot((fb & run1) != 0u) != 0;
  }
  if (any_fin) {
#pragma unroll
  for (int s = 0; s < VPT; s++) {
    const bool running = LAZY ? (bool)((run1 >> s) & 1u) : w_pl(wa[s]) < P;
    if (!LAZY && running != (bool)((run0 >> s) & 1u)) {
      rem[s] = running ? rem[s] + t32 : rem[s] - t32;  // placed : suspended
      dirty |= 1u << s;
    }
    // remaining r = F - t: decrement if r > 0, finish if it reaches 0
    const bool term = running && (LAZY ? (bool)((fb >> s) & 1u) : (int32_t)(rem[s] - t32) <= 1);
    uint64_t it = ballot(term);
    n_term += __popcll(it);
    const uint32_t me = wa[s];
#pragma unroll 1
    while (it) {  // frees in ascending VM order (env.py:260-262)
      const int l = __ffsll((unsigned long long)it) - 1;
      it &= it - 1;
      const uint32_t ew = rdlane(me, l);
      const int q = w_pl(ew);
      const double cq = L.cpu[q] - T.cent[w_cc(ew)];
      const double mq = L.mem[q] - T.cent[w_cm(ew)];
      wsync();
      if (lane == 0) {
        L.cpu[q] = cq;
        L.mem[q] = mq;
        mark_pm(L, P, q);
      }
      wsync();
    }
    if (term) {
      wa[s] = w_make(NUL, 0, 0);
      if (!LAZY) rem[s] = 0;
      dirty |= 1u << s;
    }
  }
  }
  // precision clamp (env.py:267-268): every stored load is 0 or >= 1e-7 after
  // the previous step's clamp and placements only add, so only a free or a
  // suspension (external actions) can leave a value below 1e-7
  if (n_term > 0 || n_susp > 0)
    for (int i = lane; i < P; i += 64) {
      if (L.cpu[i] < 1e-7) L.cpu[i] = 0;
      if (L.mem[i] < 1e-7) L.mem[i] = 0;
    }
  STAMP(2);
  // ---- _accept_vm_requests (env.py:271-293) ----
  // only a finish makes a NULL slot: none if the previous per-step launch left
  // none (EnvHdr::pad bit 32 clear under bit 63; the launch's first step: the
  // header's hint is the state before it) and none finished now
  const uint64_t ph = H->pad;
  const bool no_null = kstep == 0 && (ph >> 63) && !((ph >> 32) & 1u) && n_term == 0;
  int n_null = 0;
  if (!no_null) {
#pragma unroll
    for (int s = 0; s < VPT; s++) {
      const int v = s * 64 + lane;
      const bool isnull = w_pl(wa[s]) == NUL;
      const uint64_t nm = ballot(isnull);
      if (isnull) L.nulls[n_null + below(nm, lane)] = (uint16_t)v;
      n_null += __popcll(nm);
    }
  }
  const int64_t arrivals = L.arr[kstep];  // rng3.poisson(lambda), drawn in the prologue
  const int64_t k = arrivals < n_null ? arrivals : n_null;
  wsync();
  if (k > 0) {
    // to_accept = the first k NULL slots; sizes popped from the rng1/rng2
    // sequences, planned runtimes from rng4 (env.py:276-290)
    Pcg r1 = ld_pcg(H, 0), r2 = ld_pcg(H, 1);
    // (a traced env: the step's requests in order, 64 at a time through the
    // staging words; the launch's first chunk was staged by trace_preload)
    const uint64_t GLBP *req = nullptr;
    if constexpr (SRC == kSrcTrace) req = gptr(env_trace(p, e).req) + L.svcfb[0];
#pragma unroll 1
    for (int j = 0; j < k; j++) {
      int cc, cm;
      uint32_t rr;
      if constexpr (SRC == kSrcTrace) {
        if ((j & 63) == 0 && (j | kstep) != 0) {
          wsync();
          L.svcst[lane] = j + lane < k ? req[j + lane] : 0ull;
          wsync();
        }
        const uint64_t rq = L.svcst[j & 63];
        cc = rq_cc(rq);
        cm = rq_cm(rq);
        rr = rq_rt(rq);
      } else {
        cc = (int)rint((p.seq_lo + p.seq_range * next_double(r1)) * 100.0);
        cm = (int)rint((p.seq_lo + p.seq_range * next_double(r2)) * 100.0);
        rr = svc_take<SRC>(p, L, e);
      }
      const int v = L.nulls[j];
      if (lane == (v & 63)) {
#pragma unroll
        for (int s = 0; s < VPT; s++)
          if (s == (v >> 6)) {
            wa[s] = w_make(WAIT, cc, cm);
            if (LAZY) {  // final for this launch: stored now, skipped at the end
              ST_NT(vmo + vm_slot_idx(v), wa[s]);
              ST_NT(vmo + vm_time_idx(v), rr);
              dirty &= ~(1u << s);
            } else {
              rem[s] = rr;
              dirty |= 1u << s;
            }
          }
      }
      if (lane == 0) {
        L.accc[j] = (uint8_t)cc;
        L.accm[j] = (uint8_t)cm;
      }
    }
    if constexpr (SRC != kSrcTrace) {
      st_pcg(H, 0, r1);
      st_pcg(H, 1, r2);
    }
  }
  wsync();
  STAMP(3);
  // ---- stats + reward (env.py:112-156) ----
  // target_cpu/memory_mean (env.py:116-121) feed only the kl reward and the
  // eval-mode info; for wr/ut they are derived on demand from the stored state
  // by k_target_means (vmp_get_stats), so the step skips the two V-long sums.
  const bool kl = p.reward == 2;
  // The counts, from the step's events. n_null is exact: the NULL list above
  // was built, or no_null proved that there is no NULL slot. Every live slot
  // holds a VM or is NULL, so n_ex = V - (n_null - k), on the V live slots and
  // not the padded rows. A waiting VM leaves WAIT only by an accepted placement
  // and a VM enters WAIT only by a suspension or as an accepted request (a VM
  // placed and finished in this step was waiting before and is NULL after).
  null_left = n_null - (int)k;
  n_w += (int)n_susp - (int)n_place + (int)k;
  int n_ex = p.V - null_left;
  // (0 <= null_left <= V <= 64 VPT: the range the popcounts of a sweep made
  // plain to the compiler; without it the pairwise sums below are compiled
  // for any n, at 30-40 more VGPRs in the trace kernels)
  __builtin_assume(n_ex >= 0 && n_ex <= VPT * 64);
  // wr after a quiet step in which nothing finished, arrived or was placed:
  // the VM set is the previous step's, so is its waiting ratio (stored in the
  // header) and whether any VM exists (has_ex: carried by the caller, from
  // EnvHdr::pad bit 61 at the launch's start); n_w stays as it was
  const bool same_vms = p.reward == 0 && quiet_in && n_term == 0 && k == 0;
  // kl: the existing VMs' sizes, compressed in slot order. EXTK (the
  // external-action kernels) keeps the sweep's own n_ex, the same number: with
  // the derived one k_env_ext<1> (128 VGPRs at 4 waves per SIMD) spills VGPRs
  // and k_env_ext_tr<8> needs 15 more
  if (EXTK || kl) {
    int off = 0;
#pragma unroll
    for (int s = 0; s < VPT; s++) {
      const bool ex = w_pl(wa[s]) <= WAIT;
      const uint64_t em = ballot(ex);
      if (kl && ex) {
        const int rk = off + below(em, lane);
        L.ccomp[rk] = (uint8_t)w_cc(wa[s]);
        L.mcomp[rk] = (uint8_t)w_cm(wa[s]);
      }
      off += __popcll(em);
    }
    if (EXTK) n_ex = off;
  }
  if (!same_vms) has_ex = n_ex > 0;
  wsync();
  STAMP(11);
  // the pairwise reductions of the step, one inlined body per source type:
  //  0,1  sum of the accepted sizes (total_*_requested, env.py:280/285)
  //  2,3  sum of existing VM sizes (target means, env.py:116-121)
  //  4,5  sum of PM cpu / memory (ut reward; kl means)
  //  6,7  PM squared-deviation sums (kl, np.var(cpu/memory))
  //  8,9  VM-size squared-deviation sums (kl, np.var(vm_cpu/vm_memory[existing]))
  double LDSP *res = L.jobres;
  const double *cent = T.cent;
  {  // VM-size sources: accepted sizes, existing sizes, their deviations
#pragma unroll 1
    for (int j = (k > 0 ? 0 : 2); j < (kl ? 4 : 2); j++) {
      const uint8_t LDSP *src = (j == 0) ? L.accc : (j == 1) ? L.accm : ((j & 1) ? L.mcomp : L.ccomp);
      const int n = j < 2 ? (int)k : n_ex;
      const double r = wave_pw_sum(n, [=](int i) { return cent[src[i]]; }, L.pw);
      wsync();
      if (lane == 0) res[j] = r;
      wsync();
    }
  }
  if (p.reward >= 1) {  // PM sources (ut, kl)
    const int jend = p.reward == 2 ? 8 : 6;
#pragma unroll 1
    for (int j = 4; j < jend; j++) {
      const double LDSP *src = (j & 1) ? L.mem : L.cpu;
      const double mean = j < 6 ? 0.0 : res[j - 2] / (double)P;
      const bool sq = j >= 6;
      const double r = wave_pw_sum(P, [=](int i) {
        const double x = src[i];
        const double d = x - mean;
        return sq ? d * d : x;
      }, L.pw);
      wsync();
      if (lane == 0) res[j] = r;
      wsync();
    }
  }
  if (p.reward == 2) {  // VM-size deviations (kl)
#pragma unroll 1
    for (int j = 8; j < 10; j++) {
      const uint8_t LDSP *src = (j & 1) ? L.mcomp : L.ccomp;
      const double mean = res[j - 6] / (double)n_ex;
      const double r = wave_pw_sum(n_ex, [=](int i) {
        const double d = cent[src[i]] - mean;
        return d * d;
      }, L.pw);
      wsync();
      if (lane == 0) res[j] = r;
      wsync();
    }
  }
  STAMP(12);
  const double wr = same_vms ? H->waiting_ratio : n_ex > 0 ? (double)n_w / (double)n_ex : 0.0;
  if (!kl) res[2] = res[3] = 0.0;  // unused below
  double tcm = res[2] / (double)P;
  if (p.cap_target_util && tcm > 1) tcm = 1.0;
  double tmm = res[3] / (double)P;
  if (p.cap_target_util && tmm > 1) tmm = 1.0;
  double reward = 0.0;
  if (has_ex) {
    if (p.reward == 2) {  // kl (env.py:124-149)
      double cv = res[6] / (double)P, mv = res[7] / (double)P;
      if (cv == 0) cv = 1e-6;
      if (mv == 0) mv = 1e-6;
      double tcv = res[8] / (double)n_ex, tmv = res[9] / (double)n_ex;
      if (tcv == 0) tcv = 1e-6;
      if (tmv == 0) tmv = 1e-6;
      reward = (tcm == 0 || tmm == 0)
                   ? 0.0
                   : kl_reward(tcm, tmm, tcv, tmv, res[4] / (double)P, res[5] / (double)P, cv, mv);
    } else if (p.reward == 1) {  // ut (env.py:150-151)
      reward = p.beta * res[4] + (1 - p.beta) * res[5];
    } else {  // wr (env.py:152-153)
      reward = -wr;
    }
  }
  STAMP(4);
  // ---- counters, termination (env.py:160-163, 101) ----
  const int64_t ts = H->timestep;
  terminated = ts >= p.limit;
  calm = n_term == 0 && k == 0;  // no PM load fell, no new pending VM
  (void)n_ex;
  wsync();
  if (lane == 0) {
    H->timestep = ts + 1;
    H->total_requests += arrivals;
    H->served += n_term;
    H->dropped += arrivals - k;
    if constexpr (SRC == kSrcTrace) L.svcfb[0] += (uint64_t)arrivals;  // dropped requests are consumed
    H->waiting_ratio = wr;
    if (kl) {
      H->tcm = tcm;
      H->tmm = tmm;
    }
    if (k > 0) {
      H->total_cpu_req = H->total_cpu_req + res[0];
      H->total_mem_req = H->total_mem_req + res[1];
    }
  }
  wsync();
  return reward;
}

template <int VPT>
__device__ __forceinline__ void write_obs(const EnvParams &p, const Lds &L, const Tables &T,
                                          const uint32_t (&wa)[VPT], float *obs) {
  const int lane = fresh_lane();
  const int V = p.V, P = p.P;
#pragma unroll
  for (int s = 0; s < VPT; s++) {
    const int v = s * 64 + lane;
    if (live(wa[s])) {
      ST_NT(obs + v, (float)w_pl(wa[s]));
      ST_NT(obs + V + v, T.fcent[w_cc(wa[s])]);
      ST_NT(obs + 2 * V + v, T.fcent[w_cm(wa[s])]);
    }
  }
  for (int i = lane; i < P; i += 64) {
    ST_NT(obs + 3 * V + i, (float)L.cpu[i]);
    ST_NT(obs + 3 * V + P + i, (float)L.mem[i]);
  }
}

// get_invalid_action_mask(masked=True) (env.py:45-53), bit-packed, 1 = invalid.
template <int VPT>
__device__ __forceinline__ void write_mask(const EnvParams &p, const Lds &L, const Tables &T,
                                           const uint32_t (&wa)[VPT], uint32_t *bits) {
  const int lane = fresh_lane();
  const int P = p.P, A = p.A, W = p.W32, WAIT = p.P, NUL = p.P + 1;
#pragma unroll
  for (int s = 0; s < VPT; s++) {
    const int v = s * 64 + lane;
    const bool in = live(wa[s]);
    const int c = in ? w_pl(wa[s]) : NUL;
    const double vc = T.cent[w_cc(wa[s])], vm = T.cent[w_cm(wa[s])];
    const bool waiting = in && c == WAIT;
    const bool anyw = ballot(waiting) != 0;
#pragma unroll 1
    for (int w = 0; w < W; w++) {
      uint32_t word = 0xFFFFFFFFu;
      const int a0 = w * 32;
      if (c >= a0 && c < a0 + 32 && c < A) word &= ~(1u << (c - a0));  // stay
      if (c < P && WAIT >= a0 && WAIT < a0 + 32) word &= ~(1u << (WAIT - a0));  // suspend
      if (anyw) {
        const int hi = min(a0 + 32, P);
#pragma unroll 1
        for (int q = a0; q < hi; q++) {  // uniform q: LDS broadcast reads
          const bool fit = (L.cpu[q] + vc <= 1) && (L.mem[q] + vm <= 1);
          if (waiting && fit) word &= ~(1u << (q - a0));
        }
      }
      if (in) bits[(int64_t)v * W + w] = word;
    }
  }
}

// ---- launch order of the per-step launches (vmp_launch_order.h) -----------
// The two flag buffers lie behind the handle's headers, [parity][chunk][rank].
__device__ __forceinline__ uint8_t *lo_flags(const EnvParams &p, int parity) {
  return reinterpret_cast<uint8_t *>(p.hdr + p.N) + (int64_t)parity * lo_flag_bytes(p.N);
}
// The env that dispatch position q of the heuristic per-step kernel runs
// (wave-uniform, scalar but for the one flag byte per lane and its ballot):
// the tail ranks exchange busy and idle envs; fidx = the env's byte in a flag
// buffer (-1 outside mode 2).
__device__ __forceinline__ int lo_swap_env(const EnvParams &p, int q, int &fidx) {
  const uint32_t w = (uint32_t)p.pad0;
  fidx = -1;
  if (lo_mode(w) == kLoIdleLast) {
    const int C = lo_chunks(p.N), T = lo_T(w), nr = lo_nr(w);
    int r = q / C;
    const int c = q - r * C;
    if (lo_in_tail(r, T, nr)) {
      const int lane = lane_id();
      const uint8_t GLBP *line = gptr(lo_flags(p, lo_parity(w))) + (int64_t)c * kLoChunk;
      const bool in = lane < 2 * T;
      const uint8_t f = in ? line[lo_lane_rank(lane, T, nr)] : (uint8_t)0;
      const uint32_t busy = (uint32_t)ballot(in && f != 0);
      r = uni(lo_partner(busy, T, nr, lo_parity(w), r));
      q = r * C + c;
    }
    fidx = c * kLoChunk + r;
  }
  return q;
}
// The env's flag for the launch after this one: 0 where the header written
// back (hint word ph, clock t) meets idle_step's header terms, else 1.
__device__ __forceinline__ void lo_store_flag(const EnvParams &p, int fidx, uint64_t ph, int64_t t) {
  if (fidx < 0) return;
  const uint32_t nf = (uint32_t)ph;
  const bool q1 = (ph >> 62) & 1u, q2 = (ph >> 60) & 1u;
  const bool idle = (ph >> 63) && q1 != q2 && (ph & 0x0FFFFFFF00000000ull) == 0 && nf != 0u &&
                    (int32_t)(nf - (uint32_t)t) > 1;
  gptr(lo_flags(p, lo_parity((uint32_t)p.pad0) ^ 1))[fidx] = (uint8_t)!idle;
}

// ---- the idle step of a per-step heuristic launch -------------------------
// A per-step launch whose header says that the step changes nothing of the
// env but its clock: the heuristic is skipped (EnvHdr::pad bit 62 or 60, see
// heuristic_apply), the previous per-step launch left no NULL slot (bit 63
// set, bit 32 clear: no request can be accepted) and the smallest running
// finish key nf is past this step (nf > t + 1: no VM finishes). Such a step
// draws its arrival count and drops all of it, repeats the stored wr reward
// and re-emits the observation; the VM words, the PM words, rng1/2/4 and the
// whole pad word stay as they are (the hint carries nf, bit 32 stays 0, bits
// 60-62 carry over: the step is calm and quiet). It is the predicate of
// env_body's skip_time plus the conditions under which nothing else leaves
// the step (wr reward, no actions / validity flags / mask returned). The pad
// word must be exactly what the general path would write back (one of bits
// 62 / 60, bits 33-59 clear), so leaving it alone is the same store.
// Wave-uniform (readfirstlane: a scalar branch).
// 2P <= 256: idle_body reads the PM words from LDS and would serve any P; the
// limit is the one the path was specified and is tested with (larger P keeps
// the general path, tests/test_gpu_idle_step.py row p130v64).
// The skip_time terms are written out here and again in env_body, on
// purpose: env_body's own expression stays where the parent has it (moving
// it moves the general path's register allocation), and a
// step that is idle here is one env_body would give skip_time; the
// twin-handle tests hold the two together.
__device__ __forceinline__ bool idle_step(const EnvParams &p, const StepOut &o, const Lds &L) {
#ifdef VMP_CHECK_QUIET
  return false;  // as skip_time: the audited state must evolve as the product's
#else
  const uint64_t ph = L.hdr->pad;
  const uint32_t t32 = (uint32_t)L.hdr->timestep;
  const uint32_t nf = (uint32_t)ph;
  const bool q1 = (ph >> 62) & 1u, q2 = (ph >> 60) & 1u;
  const bool idle = o.k_steps == 1 && p.reward == 0 && !o.act_out && !o.valid && !o.mask_bits &&
                    2 * p.P <= 256 && (ph >> 63) && q1 != q2 &&
                    (ph & 0x0FFFFFFF00000000ull) == 0 && nf != 0u && (int32_t)(nf - t32) > 1;
  return uni((int)idle) != 0;
#endif
}

// The idle step itself, behind the general path's prologue (header, PM words
// and the launch's draws are in LDS: L.arr[0] is the arrival count, rng3 is
// advanced): env_tail's counters / reward / done, write_obs, and the 32-lane
// header write-back (storing only the five changed words measured slower).
template <int VPT>
__device__ __forceinline__ void idle_body(const EnvParams &p, const StepOut &o, const Lds &L,
                                          const float LDSP *fcent, int e,
                                          const uint32_t (&wa)[VPT], int fidx) {
  const int lane = lane_id();
  const int V = p.V;
  EnvHdr LDSP *H = L.hdr;
  const int64_t a = L.arr[0];
  const uint64_t ph = H->pad;
  const int64_t ts = H->timestep;
  const bool term = ts >= p.limit;
  if (lane == 0) {
    if (o.reward) gptr(o.reward)[e] = ((ph >> 61) & 1u) ? -H->waiting_ratio : 0.0;
    if (o.done) gptr(o.done)[e] = (uint8_t)term;
    if (o.done_count) gptr(o.done_count)[e] += (int64_t)term;
  }
  if (o.obs) {
    float *obs = o.obs + (int64_t)e * p.D;
#pragma unroll
    for (int s = 0; s < VPT; s++) {
      const int v = s * 64 + lane;
      if (live(wa[s])) {
        ST_NT(obs + v, (float)w_pl(wa[s]));
        ST_NT(obs + V + v, fcent[w_cc(wa[s])]);
        ST_NT(obs + 2 * V + v, fcent[w_cm(wa[s])]);
      }
    }
    // L.cpu is [cpu P][memory P], the obs tail's order
    for (int i = lane; i < 2 * p.P; i += 64) ST_NT(obs + 3 * V + i, (float)L.cpu[i]);
  }
  wsync();
  if (lane == 0) {
    H->timestep = ts + 1;
    H->total_requests += a;
    H->dropped += a;
    lo_store_flag(p, fidx, ph, ts + 1);
  }
  wsync();
  if (lane < 32)
    gptr(reinterpret_cast<uint64_t *>(p.hdr + e))[lane] = reinterpret_cast<uint64_t LDSP *>(H)[lane];
}

// ONE = true is the per-step launch (k_steps == 1, the Base.test loop body); it
// is a separate instantiation so profiles tell it apart from fused rollouts.
// EXT = true: the external-action step (vmp_step), its own kernel k_env_ext so
// the heuristic's registers do not weigh on it and vice versa.
// SRC = kSrcEnv (WL = true): the handle has a per-env workload
// (vmp_set_workload); the only difference is where the env's Poisson constants
// are read from (env_pois). SRC = kSrcTrace: the handle has a trace
// (vmp_set_trace); nothing is drawn, the prologue loads the launch's arrival
// counts from the env's trace (trace_preload) and the accept loop its requests.
template <int VPT, bool ONE, bool EXT, int SRC>
__device__ __forceinline__ void env_body(const EnvParams &p, const StepOut &o) {
  extern __shared__ __align__(16) char lds[];
  __shared__ Tables T;
#ifdef VMP_STAMPS
  const uint64_t t_start = __builtin_amdgcn_s_memtime();
  const uint64_t rt_start = __builtin_amdgcn_s_memrealtime();
#endif
  const int lane = lane_id();
  const int wid = threadIdx.x >> 6;
  // per-step launches take their env from the launch-order layer: the
  // dispatch position here, the heuristic kernel's exchange behind the header load
  int fidx = -1;
  int e_raw = uni(blockIdx.x * kEnvWavesPerBlock + wid);
  if constexpr (ONE) e_raw = uni(lo_position((uint32_t)p.pad0, p.N, e_raw));
  int e = e_raw < p.N ? e_raw : p.N - 1;  // tail waves load a valid env, then leave
  char LDSP *base = (char LDSP *)lds + wid * p.lds_wave_bytes;
  const Lds L = make_lds(p, base);
  const int V = p.V, P = p.P;
  // ---- every global load of the env's state is issued up front: header and
  // PM resources (needed first, to LDS), then the VM words (to registers),
  // whose latency the random draws below overlap ----
  // (indices are clamped instead of branched on, so no load is conditional and
  // the waits below can count: a skipped load would force vmcnt(0))
  // a starting wave's state loads issue ahead of the running waves' work: its
  // critical path starts at their latency (burst launches -1.1-1.6 %,
  // profiles/r04_prio_prologue_ab.log)
  __builtin_amdgcn_s_setprio(2);
  uint64_t hv = gptr(reinterpret_cast<const uint64_t *>(p.hdr + e))[lane & 31];
  // idle envs last: the flags are read while the position's own header is in
  // flight (the exchange then costs a wave that keeps its env no load latency
  // of its own); a wave that takes another env loads that header instead
  if constexpr (ONE && !EXT && SRC != kSrcTrace) {
    const int e2 = uni(lo_swap_env(p, e, fidx));
    if (e2 != e) {
      e = e_raw = e2;
      hv = gptr(reinterpret_cast<const uint64_t *>(p.hdr + e))[lane & 31];
    }
  }
  // Poisson constants for the block's LDS copy (issued before the state loads,
  // so waiting for them never waits on the state): the env's own pair, one
  // env per workgroup (e is wave-uniform: scalar address arithmetic)
  static_assert(kEnvWavesPerBlock == 1, "Tables::pois holds one env's Poisson constants");
  constexpr int kPoisWords = (int)(2 * sizeof(PoisConst) / 4);
  uint32_t pw = 0;
  if constexpr (SRC != kSrcTrace)
    pw = gptr(reinterpret_cast<const uint32_t *>(env_pois<SRC>(p, e)))[threadIdx.x % kPoisWords];
  // a traced env's descriptor instead: a function of e alone (scalar loads
  // beside the header's, no link in the header -> offsets -> requests chain)
  TraceDesc td{nullptr, nullptr, 0, 0};
  if constexpr (SRC == kSrcTrace) td = env_trace(p, e);
  // this lane's PCG64 jump entry (lane-parallel draws), right behind the header
  U128 JA{0, 0}, JM{0, 0};
  if (SRC != kSrcTrace && o.k_steps > 0) {
    const uint64_t GLBP *jt = gptr(p.jump + 4 * lane);
    JA = U128{jt[0], jt[1]};
    JM = U128{jt[2], jt[3]};
  }
  const double *pm = p.pm + (int64_t)e * 2 * P;
  const int n_pm = 2 * P;
  double pv[4];
#pragma unroll
  for (int j = 0; j < 4; j++) pv[j] = pm[min(j * 64 + lane, n_pm - 1)];
  __asm__ volatile("" ::: "memory");  // keep the issue order: header/PM first
  // ONE: only the slot words (placement, sizes) go to registers here; the
  // finish keys are read after the draws and folded into one bit per slot
  // (slot and time words sit in separate 256-B runs of each 64-slot block)
  const uint32_t GLBP *vlo = gptr(p.vmw + (int64_t)e * vm_pitch(V));
  uint32_t wa[VPT], rem[VPT];
#pragma unroll
  for (int s = 0; s < VPT; s++) {
    const int v = s * 64 + lane;
    const uint32_t x = vlo[vw_row(s, lane)];
    wa[s] = v < V ? x : (uint32_t)kPad;
    if (ONE) {
      rem[s] = 0;
    } else {
      const uint32_t y = vlo[vw_row(s, lane) + 64];
      rem[s] = v < V ? y : 0u;
    }
  }
  __asm__ volatile("" ::: "memory");  // ... and the VM words before any wait
  __builtin_amdgcn_s_setprio(0);
  // size tables (k/100 in f64 and f32) while the loads are in flight; the only
  // block-wide barrier: waves are independent below
  for (int i = threadIdx.x; i < 128; i += blockDim.x) {
    T.cent[i] = (double)i / 100.0;
    T.fcent[i] = (float)((double)i / 100.0);
  }
  if (SRC != kSrcTrace && threadIdx.x < kPoisWords)
    reinterpret_cast<uint32_t *>(T.pois)[threadIdx.x] = pw;
  __syncthreads();
  if (e_raw >= p.N) return;
  if (lane < 32) reinterpret_cast<uint64_t LDSP *>(L.hdr)[lane] = hv;
  wsync();
#ifdef VMP_STAMPS
  const uint64_t t_loaded = __builtin_amdgcn_s_memtime();
#endif
  // the external kernel parks the PM words in LDS before the draws (issued
  // right behind the header, they are in by then): live across the draws
  // they spilled to scratch there
  if (EXT) {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (j * 64 + lane < n_pm) L.cpu[j * 64 + lane] = pv[j];
  }
  // the draws need only the header: they run while the PM / VM loads land
  if constexpr (SRC == kSrcTrace) {
    if (o.k_steps > 0) trace_preload(L, td, o.k_steps);
  } else {
    if (o.k_steps > 0) predraw(p, L, T, o.k_steps, V, JA, JM);
  }
#ifdef VMP_STAMPS
  const uint64_t t_drawn = __builtin_amdgcn_s_memtime();
#endif
  if (!EXT) {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (j * 64 + lane < n_pm) L.cpu[j * 64 + lane] = pv[j];
  }
  for (int i = 256 + lane; i < n_pm; i += 64) L.cpu[i] = pm[i];  // P > 128
  for (int i = lane; i < (n_pm + 63) / 64; i += 64) L.pdirty[i] = 0;
  wsync();
#ifdef VMP_STAMPS
  __shared__ uint64_t st_lds[kEnvWavesPerBlock * kStamps];
#endif
  STAMP_DECL_AT((uint64_t LDSP *)st_lds + wid * kStamps)
#ifdef VMP_STAMPS
  if (lane == 0) {
    st_acc[13] = t_loaded - t_start;
    st_acc[14] = t_drawn - t_loaded;
    st_acc[15] = st_prev - t_drawn;
  }
#endif
  // the idle step (see idle_step) leaves here: behind the prologue, which is
  // the general path's own up to this point (no load depends on the branch).
  // Traced envs keep the general path.
  if constexpr (ONE && !EXT && SRC != kSrcTrace) {
  if (idle_step(p, o, L)) {
    idle_body<VPT>(p, o, L, (const float LDSP *)T.fcent, e, wa, fidx);
#ifdef VMP_STAMPS
    if (p.stamps && lane == 0) stamp_idle(p.stamps + (int64_t)e * kStamps, t_start, rt_start);
#endif
    return;
  }
  }
  bool term = false;
  int64_t ndone = 0;
  uint32_t dirty = 0;  // bit s: this lane's VM word s changed (stored at the end)
  uint32_t fb = 0;     // ONE: bit s = slot s finishes this step if it runs
  uint32_t hiv[VPT];   // ONE: the finish keys / remaining runtimes, in flight
  uint32_t nf = 0u;  // ONE: smallest finish key running on (EnvHdr::pad hint; 0: unknown)
  bool want_nf = false;
  // ONE, heuristic: a quiet step (EnvHdr::pad bit 62, or bit 60 where no
  // actions / validity flags are returned: it places nothing) whose
  // hint records the smallest finish key nf of the running VMs (the previous
  // launch left no NULL slot) with nf > t + 1 needs no time word: no VM
  // finishes and none is placed, so every finish bit is 0 and nf carries over
  // (heuristic launches suspend nothing). Its 16 time-word loads then all read
  // one line (the loads stay unconditional, so the counted waits before their
  // use are the same on both paths): 4 KB less HBM per such env-step.
  bool skip_time = false;
  uint32_t nf_carry = 0u;
  if (ONE && !EXT) {
    // (off in the check build: its quiet steps still run the fit loop and
    // may place, which a skipped step's carried nf and zero finish bits
    // would leave stale: the audited state must evolve as the product's)
#ifndef VMP_CHECK_QUIET
    const uint64_t ph = L.hdr->pad;
    nf_carry = (uint32_t)ph;
    const bool skip_h = ((ph >> 62) & 1u) || (((ph >> 60) & 1u) && !o.act_out && !o.valid);
    skip_time = skip_h && (ph >> 63) && ((ph >> 32) & 1u) == 0u && nf_carry != 0u &&
                (int32_t)(nf_carry - (uint32_t)L.hdr->timestep) > 1;
#endif
    // issued before the action phase, consumed after it (latency hidden by it)
    const uint32_t GLBP *hb = vlo + 64 + (skip_time ? 0 : lane);
    const int hs = skip_time ? 0 : 128;
#pragma unroll
    for (int s = 0; s < VPT; s++) hiv[s] = hb[s * hs];
    __asm__ volatile("" ::: "memory");
  }
  uint32_t *vmo = p.vmw + (int64_t)e * vm_pitch(V);
  const int k_steps = ONE ? 1 : o.k_steps;
  // EnvHdr::pad bits 62 / 60 (qkind 1 / 2, see heuristic_apply); the
  // external-action kernel neither uses nor keeps them
  int qkind = EXT ? 0 : (((L.hdr->pad >> 62) & 1u) ? 1 : (((L.hdr->pad >> 60) & 1u) ? 2 : 0));
  bool has_ex = (L.hdr->pad >> 61) & 1u;  // bit 61: some VM exists (read with bit 62 only)
  // the waiting VMs, counted once by the first step's action phase and carried
  // through the launch by env_tail; the NULL slots the last step left
  int n_w = 0, null_left = 0;
#pragma unroll 1
  for (int k = 0; k < k_steps; k++) {
    const bool last = k == k_steps - 1;
    uint8_t *valid_row = (last && o.valid) ? o.valid + (int64_t)e * V : nullptr;
    int32_t *act_row = (last && o.act_out) ? o.act_out + (int64_t)e * V : nullptr;
    int64_t n_place = 0, n_susp = 0;
    uint32_t run0 = 0;
#pragma unroll
    for (int s = 0; s < VPT; s++) run0 |= (uint32_t)(w_pl(wa[s]) < P) << s;
    bool fit_any = false;
    // qkind 2 repeats rejected placements: skipped only where no actions or
    // validity flags leave this step
    const bool quiet = qkind == 1 || (qkind == 2 && !act_row && !valid_row);
    if (!EXT)
      n_place = heuristic_apply<VPT>(p, L, T, wa, o.policy, act_row, valid_row, quiet, qkind,
                                     fit_any, k == 0, n_w STAMP_ARGS);
    else {
      // the external kernel loads the time words after its action phase: live
      // across it beside the 16 action words they spilled 10 VGPRs
      external_apply<VPT>(p, L, T, wa, o.actions + (int64_t)e * V, valid_row, n_place, n_susp,
                          n_w);
      if (ONE) {
        const int ln = fresh_lane();
#pragma unroll
        for (int s = 0; s < VPT; s++) hiv[s] = vlo[vw_row(s, ln) + 64];
      }
    }
    STAMP(1);
    if (ONE) {  // the time words' last use: bit s = slot s finishes this step if it runs
      const uint32_t t32 = (uint32_t)L.hdr->timestep;
      // the next launch's draw hint needs the smallest finish key of the VMs
      // that run on only where the last step left no NULL slot (else nf = 0)
      const uint64_t ph = L.hdr->pad;
      want_nf = !((ph >> 63) && ((ph >> 32) & 1u));
      nf = want_nf ? 0xFFFFFFFFu : 0u;
      if (skip_time) {  // (want_nf holds: the hint's NULL bit is 0)
        nf = nf_carry;
      } else {
#pragma unroll
      for (int s = 0; s < VPT; s++) {  // by the placement before the action phase
        const bool was_run = (run0 >> s) & 1u;
        const bool f = was_run ? (int32_t)(hiv[s] - t32) <= 1 : hiv[s] <= 1u;
        fb |= (uint32_t)f << s;
      }
      }
      if (want_nf && !skip_time) {
#pragma unroll
        for (int s = 0; s < VPT; s++) {
          const bool was_run = (run0 >> s) & 1u;
          const bool f = (fb >> s) & 1u;
          if (w_pl(wa[s]) < P && !f) nf = min(nf, was_run ? hiv[s] : hiv[s] + t32);
        }
      }
    }
    wsync();
    if (lane == 0) {
      L.hdr->place_action += n_place;
      L.hdr->suspend_action += n_susp;
    }
    wsync();
    bool calm = false;
    const double r = env_tail<VPT, ONE, SRC, EXT>(p, L, T, wa, rem, run0, fb, dirty, vmo, k, quiet,
                                        n_place, n_susp, n_w, null_left, term, calm, has_ex,
                                        e STAMP_ARGS);
    // the next step's skip: nothing fit (1), or every placement was rejected
    // (2); a skipped step passes its kind on while nothing changes
    qkind = (EXT || !calm) ? 0 : quiet ? qkind : (!fit_any ? 1 : (n_place == 0 ? 2 : 0));
    if (o.reward && lane == 0) gptr(o.reward)[(int64_t)k * p.N + e] = r;
    ndone += term;
  }
  if (SRC != kSrcTrace && o.k_steps > 0) svc_commit(make_lds(p, opaque_base(base)));
  if (!EXT && o.k_steps == 0 && o.policy >= 0 && o.act_out) {
    // act only: decide on a scratch copy of the VM words; nothing is stored
    uint32_t wt[VPT];
#pragma unroll
    for (int s = 0; s < VPT; s++) wt[s] = wa[s];
    bool fit_any;
    heuristic_apply<VPT>(p, L, T, wt, o.policy, o.act_out + (int64_t)e * V, nullptr, qkind == 1,
                         qkind, fit_any, false, n_w STAMP_ARGS);
  }
  STAMP(0);
  if (o.obs) write_obs<VPT>(p, L, T, wa, o.obs + (int64_t)e * p.D);
  if (o.mask_bits) write_mask<VPT>(p, L, T, wa, o.mask_bits + (int64_t)e * V * p.W32);
  STAMP(5);
  if (o.k_steps > 0) {
    if (o.done && lane == 0) gptr(o.done)[e] = (uint8_t)term;
    if (o.done_count && lane == 0) gptr(o.done_count)[e] += ndone;
    const uint32_t t32 = (uint32_t)(L.hdr->timestep - 1);  // this launch's step
    const int ln = fresh_lane();
    // (per-step launch: most steps change no VM word but the accepted ones,
    // stored already; one ballot then skips the 16 predicated store blocks)
    if (!ONE || ballot(dirty != 0u) != 0) {
#pragma unroll
    for (int s = 0; s < VPT; s++) {
      if (live(wa[s]) && ((dirty >> s) & 1u)) {  // unchanged words stay as they are
        const int iw = (s << 7) + ln;  // live: slot 64 s + ln < V, so its vm_slot_idx
        if (!ONE) {
          ST_NT(vmo + iw, wa[s]);
          ST_NT(vmo + iw + 64, rem[s]);
        } else if (w_pl(wa[s]) == P + 1) {  // finished: NULL, remaining 0
          ST_NT(vmo + iw, wa[s]);
          ST_NT(vmo + iw + 64, 0u);
        } else {  // placed (r -> F = t + r) or suspended (F -> r = F - t)
          uint32_t GLBP *w32 = gptr(vmo);
          w32[iw] = wa[s];
          __hip_atomic_fetch_add(w32 + iw + 64, w_pl(wa[s]) < P ? t32 : 0u - t32,
                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
    }
    // only the PM words written this launch (place / suspend / free: the
    // precision clamp changes no other value, as every stored value is 0 or
    // >= 1e-7 after the previous launch's clamp)
    double *pmo = p.pm + (int64_t)e * 2 * P;
    for (int i = lane, j = 0; i < 2 * P; i += 64, j++)
      if ((L.pdirty[j] >> lane) & 1ull) ST_NT(pmo + i, (double)L.cpu[i]);
    {  // the next launch's draw hint (predraw): per-step launches only
      uint64_t hint = 0;
      if (ONE) {  // (the NULL count is recorded as 0 or 1: only "none" is read)
        uint32_t m = nf;
        bool nn = null_left > 0;  // env_tail's count: exact (see there)
        if (EXT) {  // (the external kernels keep the sweep, as for n_ex in env_tail)
          bool anynull = false;
#pragma unroll
          for (int s = 0; s < VPT; s++) anynull |= w_pl(wa[s]) == P + 1;
          nn = ballot(anynull) != 0;
        }
        if (!nn && want_nf) {
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, o));
        }
        hint = (1ull << 63) | ((uint64_t)nn << 32) | m;
      }
      hint |= ((uint64_t)(qkind == 1) << 62) | ((uint64_t)(qkind == 2) << 60) |
              ((uint64_t)has_ex << 61);
      wsync();
      if (lane == 0) {
        L.hdr->pad = hint;
        if constexpr (ONE && !EXT && SRC != kSrcTrace) lo_store_flag(p, fidx, hint, L.hdr->timestep);
      }
      wsync();
    }
    if (lane < 32)
      gptr(reinterpret_cast<uint64_t *>(p.hdr + e))[lane] = reinterpret_cast<uint64_t LDSP *>(L.hdr)[lane];
  }
  STAMP(6);
#ifdef VMP_STAMPS
  if (lane == 0) {
    st_acc[7] = (__builtin_amdgcn_s_memrealtime() - rt_start) * 1000;  // x1000 (100 MHz ticks)
    st_acc[9] = __builtin_amdgcn_s_memtime() - t_start;
  }
#endif
  STAMP_FLUSH();
}

template <int VPT, bool ONE, bool WL>
__global__ __launch_bounds__(64 * kEnvWavesPerBlock, ONE ? VMP_WAVES_PER_EU_ONE : VMP_WAVES_PER_EU) void k_env(EnvParams p, StepOut o) {
  env_body<VPT, ONE, false, WL ? kSrcEnv : kSrcConfig>(p, o);
}
// VPT 1 (V <= 64, the PPO eval's config/10.yml): 4 waves per SIMD, so a
// 4 096-env step is one round of waves on the 256 CUs (at 3, 131 VGPRs, a
// third of the envs ran in a second round)
template <int VPT, bool WL>
__global__ __launch_bounds__(64 * kEnvWavesPerBlock, VPT == 1 ? 4 : VMP_WAVES_PER_EU_ONE) void k_env_ext(EnvParams p, StepOut o) {
  env_body<VPT, true, true, WL ? kSrcEnv : kSrcConfig>(p, o);
}
// The kernels of handles with a trace (vmp_set_trace), same launch bounds
template <int VPT, bool ONE>
__global__ __launch_bounds__(64 * kEnvWavesPerBlock, ONE ? VMP_WAVES_PER_EU_ONE : VMP_WAVES_PER_EU) void k_env_tr(EnvParams p, StepOut o) {
  env_body<VPT, ONE, false, kSrcTrace>(p, o);
}
template <int VPT>
__global__ __launch_bounds__(64 * kEnvWavesPerBlock, VPT == 1 ? 4 : VMP_WAVES_PER_EU_ONE) void k_env_ext_tr(EnvParams p, StepOut o) {
  env_body<VPT, true, true, kSrcTrace>(p, o);
}

// One translation unit instantiates one workload variant: vmp_kernels.hip the
// kernels of handles with the config's one workload, vmp_kernels_wl.hip
// (VMP_ENV_WL = true) those of handles with a per-env workload,
// vmp_kernels_tr.hip (VMP_ENV_TR) those of handles with a trace.
#ifdef VMP_ENV_TR
template __global__ void k_env_ext_tr<1>(EnvParams, StepOut);
template __global__ void k_env_ext_tr<2>(EnvParams, StepOut);
template __global__ void k_env_ext_tr<4>(EnvParams, StepOut);
template __global__ void k_env_ext_tr<8>(EnvParams, StepOut);
template __global__ void k_env_ext_tr<16>(EnvParams, StepOut);
template __global__ void k_env_tr<1, false>(EnvParams, StepOut);
template __global__ void k_env_tr<1, true>(EnvParams, StepOut);
template __global__ void k_env_tr<2, false>(EnvParams, StepOut);
template __global__ void k_env_tr<2, true>(EnvParams, StepOut);
template __global__ void k_env_tr<4, false>(EnvParams, StepOut);
template __global__ void k_env_tr<4, true>(EnvParams, StepOut);
template __global__ void k_env_tr<8, false>(EnvParams, StepOut);
template __global__ void k_env_tr<8, true>(EnvParams, StepOut);
template __global__ void k_env_tr<16, false>(EnvParams, StepOut);
template __global__ void k_env_tr<16, true>(EnvParams, StepOut);
#else
#ifndef VMP_ENV_WL
#define VMP_ENV_WL false
#endif
template __global__ void k_env_ext<1, VMP_ENV_WL>(EnvParams, StepOut);
template __global__ void k_env_ext<2, VMP_ENV_WL>(EnvParams, StepOut);
template __global__ void k_env_ext<4, VMP_ENV_WL>(EnvParams, StepOut);
template __global__ void k_env_ext<8, VMP_ENV_WL>(EnvParams, StepOut);
template __global__ void k_env_ext<16, VMP_ENV_WL>(EnvParams, StepOut);
template __global__ void k_env<1, false, VMP_ENV_WL>(EnvParams, StepOut);
template __global__ void k_env<1, true, VMP_ENV_WL>(EnvParams, StepOut);
template __global__ void k_env<2, false, VMP_ENV_WL>(EnvParams, StepOut);
template __global__ void k_env<2, true, VMP_ENV_WL>(EnvParams, StepOut);
template __global__ void k_env<4, false, VMP_ENV_WL>(EnvParams, StepOut);
template __global__ void k_env<4, true, VMP_ENV_WL>(EnvParams, StepOut);
template __global__ void k_env<8, false, VMP_ENV_WL>(EnvParams, StepOut);
template __global__ void k_env<8, true, VMP_ENV_WL>(EnvParams, StepOut);
template __global__ void k_env<16, false, VMP_ENV_WL>(EnvParams, StepOut);
template __global__ void k_env<16, true, VMP_ENV_WL>(EnvParams, StepOut);
#endif  // VMP_ENV_TR

}  // namespace vmp

#endif  // VMP_ENV_WAVE_H
