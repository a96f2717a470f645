// vmp_carve.h — the per-env LDS carve of k_env, k_env_ext, k_env_big,
// k_target_means_lds and k_act_obs, once: the sizes and sub-offsets the host
// (vmp_capi.cpp) and the kernels (make_lds) must agree on, and pure functions
// of (P, V) that lay the regions out, size a launch and decide whether a config
// fits a CU. No HIP calls: tests/native/carve_sweep.cpp checks it on the CPU.
#ifndef VMP_CARVE_H
#define VMP_CARVE_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "vmp_layout.h"

namespace vmp {

constexpr int kCuLdsBytes = 160 * 1024;  // LDS of one gfx950 CU (and of one workgroup)

// Static LDS of the step kernels in the default build (lds_fits), each tied to
// its structs by a static_assert (vmp_env_common.h, vmp_env_big.h)
constexpr int kEnvStaticLds = 2048;  // k_env / k_env_ext: allowance for Tables
constexpr int kBigStaticLds = 4720;  // k_env_big: Tables + BigShared, exactly

// k_env_big's workgroup: a compile-time thread count, so slot s of a thread
// sits at the constant LDS offset s * kBigNT * 4 behind the env's carve, and
// up to kBigMaxSPT slots per thread (V <= kBigNT * kBigMaxSPT)
constexpr int kBigNT = 256;
constexpr int kBigMaxSPT = (10240 + kBigNT - 1) / kBigNT;
constexpr int kBigAccLds = 512;  // k_env_big: accepted sizes held in LDS

// stage: f64 reduction results of the step, then the draw bookkeeping
constexpr int kStageBytes = 8 * 16;
constexpr int kStageSvcInfo = 8 * 12;  // i32 [0] speculative count, [1] consumed
constexpr int kStageSvcFb = 8 * 14;    // u64 [2] rng4 state for fallback draws
// BF tie sort: i32 [kSortStackWords] introsort stacks, then u16 [2P] partition lists
constexpr int kSortStackWords = 256;
constexpr int kAnyFitBytes = 512;  // wave kernels: any-fit table u32 [128]
// LDS plan of the pairwise sums: i32 lo / len [n_leaf], lane 0's stack i32
// [kPwStackWords]; f64 leaf sums and value stack [2 n_leaf + kPwValStack]
constexpr int kPwStackWords = 192;
constexpr int kPwValStack = 64;
// k_env_big event lists: u32 [kEvCap] VM words, i32 [kEvCap] targets, u8 [kEvCap] results
constexpr int kEvCap = 512;
constexpr int kEvBytes = 4 + 4 + 1;
// per-launch region at off_pre: per speculative service draw the rng4 state
// u64 [2] and the value u32 (two arrays), then i32 arrivals per step
constexpr int kSpecStateBytes = 16;
constexpr int kSpecDrawBytes = kSpecStateBytes + 4;
constexpr int kStepBytes = 4;
constexpr int kActObsF32Rows = 3;  // k_act_obs: f32 cpu, memory, keys [P]; sort; order u16 [P]

inline int64_t align16(int64_t x) { return (x + 15) & ~(int64_t)15; }
inline int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

// numpy's pairwise split n2 = n/2 - (n/2)%8 down to leaves of <= 128: the most
// leaves and the deepest recursion (kernel limit 12) of any n <= m
struct PwWorst {
  int leaves, depth;
};
inline PwWorst pw_worst(int m) {
  std::vector<int> l((size_t)m + 1, 1), d((size_t)m + 1, 0);
  PwWorst w{1, 0};
  for (int n = 129; n <= m; n++) {
    const int n2 = n / 2 - (n / 2) % 8;
    l[n] = l[n2] + l[n - n2];
    d[n] = 1 + (int)max64(d[n2], d[n - n2]);
    w = {(int)max64(w.leaves, l[n]), (int)max64(w.depth, d[n])};
  }
  return w;
}

// k_env_big's slots per thread: the fewest of its instantiations that hold V
inline int big_spt(int64_t V) {
  return V <= 4 * kBigNT ? 4 : V <= 8 * kBigNT ? 8 : V <= 16 * kBigNT ? 16 : kBigMaxSPT;
}

inline int64_t sort_bytes(int64_t P) { return 4 * kSortStackWords + 4 * P; }
inline int64_t pdirty_bytes(int64_t P) { return 8 * ((2 * P + 63) / 64); }
inline int64_t pw_plan_bytes(int64_t n_leaf) { return 8 * n_leaf + 4 * kPwStackWords; }
inline int64_t pw_val_bytes(int64_t n_leaf) { return 8 * (2 * n_leaf + kPwValStack); }

// Regions are laid out one after another, each 16-byte aligned.
struct CarveCursor {
  int64_t off;
  int32_t take(int64_t bytes) {
    const int64_t at = off;
    off = align16(off + bytes);
    return (int32_t)at;
  }
};

// The carve fields of p for (P, V): carve_wave for k_env / k_env_ext
// (V <= 1024), carve_big for k_env_big. Only recursions deeper than the
// register plan (n > 1928, wave_pw_sum) use the LDS plan of the pairwise sums.
inline void carve_wave(int64_t P, int64_t V, EnvParams &p) {
  const bool deep = V > 1928 || P > 1928;
  p.NW = (int32_t)((P + 63) / 64);  // reserved (no kernel reads it)
  p.n_leaf = deep ? pw_worst((int)max64(V, P)).leaves + 8 : 1;
  CarveCursor c{0};
  p.off_hdr = c.take(sizeof(EnvHdr));
  p.off_pm = c.take(16 * P);   // cpu, mem f64
  p.off_fpm = c.take(12 * P);  // fcpu, fmem f32 (+ P spare: the measured layout)
  p.off_thr = c.take(2 * P);   // tc, tm u8
  p.fmem_off = (int32_t)P;
  p.tm_off = (int32_t)P;
  p.off_ord = c.take(2 * P);   // BF visiting order u16
  // any-fit table; after the heuristic: the NULL list u16 [V], then the accepted sizes
  p.off_bits = c.take(max64(4 * V, kAnyFitBytes));
  p.off_acc = p.off_bits + (int32_t)(2 * V);
  p.acc_cap = (int32_t)V;
  p.off_stage = c.take(kStageBytes);
  // ccomp, mcomp u8 (stats, after the action phase) share their region with
  // the BF introsort stacks + partition lists (action phase only)
  p.off_ccomp = p.off_sort = c.take(max64(2 * V, sort_bytes(P)));
  p.ccomp_cap = (int32_t)V;
  p.off_leaf = c.take(deep ? pw_plan_bytes(p.n_leaf) : 0);
  p.off_leafval = c.take(deep ? pw_val_bytes(p.n_leaf) : 0);
  // changed-PM bitmap: only the PM words written this launch are stored back
  p.off_pdirty = c.take(pdirty_bytes(P));
  p.off_ev = 0;  // k_env_big only
  p.off_pre = p.lds_wave_bytes = (int32_t)c.off;  // the per-launch region follows
}

// k_env_big's carve, sized for two workgroups per CU at P1000 / V10000 (≤ 80 KB
// with the VM words): the regions of the action phase and of the tail share
// one union. Heuristic side: the f32 view fcpu/fmem, thresholds tc/tm, the BF
// tie sort's order and stacks. Tail side: the pairwise-sum LDS plan, the
// event lists, the accepted sizes (≤ kBigAccLds in LDS) and the existing-VM
// sizes (as many as the rest of the union holds). Steps with more accepted or
// existing VMs than that use the handle's HBM spill (p.bigscr).
inline void carve_big(int64_t P, int64_t V, EnvParams &p) {
  carve_wave(P, V, p);  // NW, n_leaf; every other field is laid out anew
  const bool deep = p.n_leaf > 1;
  CarveCursor c{0};
  p.off_hdr = c.take(sizeof(EnvHdr));
  p.off_pm = c.take(16 * P);
  p.off_stage = c.take(kStageBytes);
  p.off_pdirty = c.take(pdirty_bytes(P));
  const int64_t u0 = c.off;
  // heuristic side: 16-B aligned rows (vector reads in big_choose)
  p.fmem_off = (int32_t)((P + 3) & ~3);
  p.tm_off = (int32_t)align16(P);
  p.off_fpm = c.take(8 * (int64_t)p.fmem_off);
  p.off_thr = c.take(2 * (int64_t)p.tm_off);
  p.off_ord = c.take(2 * P);
  p.off_sort = c.take(sort_bytes(P));
  const int64_t heur_end = c.off;
  p.off_bits = p.off_fpm;  // the wave kernel's any-fit table / NULL list: unused here
  // tail side
  c.off = u0;
  p.off_leaf = c.take(deep ? pw_plan_bytes(p.n_leaf) : 0);
  p.off_leafval = c.take(deep ? pw_val_bytes(p.n_leaf) : 0);
  p.off_ev = c.take(kEvCap * kEvBytes);
  p.acc_cap = (int32_t)(V < kBigAccLds ? V : kBigAccLds);
  p.off_acc = c.take(2 * (int64_t)p.acc_cap);
  p.off_ccomp = (int32_t)c.off;
  const int64_t cap = max64((heur_end - c.off) / 2, V < 1024 ? V : 1024);
  p.ccomp_cap = (int32_t)(cap > V ? V : cap);
  c.take(2 * (int64_t)p.ccomp_cap);
  p.off_pre = p.lds_wave_bytes = (int32_t)max64(c.off, heur_end);
}

// k_target_means_lds at V > 1024: a private carve from 0 (ccomp | mcomp of V
// bytes each, then the pairwise-sum plan; carve_big places ccomp after regions
// this kernel does not allocate and caps it below V) in q, a copy of the
// handle's parameters; -> the launch's dynamic LDS.
inline size_t carve_target_means(EnvParams &q) {
  q.off_ccomp = 0;
  q.ccomp_cap = q.V;
  q.off_leaf = (int32_t)align16(2 * (int64_t)q.V);
  q.off_leafval = (int32_t)(q.off_leaf + align16(pw_plan_bytes(q.n_leaf)));
  return (size_t)q.off_leafval + (size_t)pw_val_bytes(q.n_leaf);
}

// k_act_obs's dynamic LDS: the whole PM view of one env
inline size_t act_obs_lds(int64_t P) {
  return (size_t)(4 * kActObsF32Rows * P + sort_bytes(P) + 2 * P);
}

// One env's region of a launch of k_steps steps (EnvParams::lds_wave_bytes of
// that launch): the carve, then the per-launch region.
inline int32_t launch_wave_bytes(const EnvParams &p, int k_steps) {
  return (int32_t)align16(p.off_pre + (int64_t)kSpecDrawBytes * kSpecDraws +
                          (int64_t)kStepBytes * (k_steps > 0 ? k_steps : 1));
}
// The dynamic LDS of that launch: a workgroup's envs; behind k_env_big's one
// env, the VM words of its spt slots per thread.
inline size_t launch_lds(const EnvParams &p, int k_steps, bool big, int spt) {
  const size_t wave = (size_t)launch_wave_bytes(p, k_steps);
  return big ? wave + 4 * (size_t)spt * kBigNT : wave * kEnvWavesPerBlock;
}
// Do `dyn` dynamic bytes and the kernel's static LDS fit a CU?
inline bool lds_fits(size_t dyn, bool big) {
  return dyn + (size_t)(big ? kBigStaticLds : kEnvStaticLds) <= (size_t)kCuLdsBytes;
}
// Does the carved config (p.V set) fit at the longest launch (vmp_create's check)?
inline bool carve_fits(const EnvParams &p, bool big) {
  return lds_fits(launch_lds(p, kMaxStepsPerLaunch, big, big_spt(p.V)), big);
}

}  // namespace vmp

#endif  // VMP_CARVE_H
