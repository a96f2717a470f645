// vmp_env_common.h — what the wave-per-env and the block-per-env kernel share:
// the per-env LDS carve, the VM-word helpers, the f32 fit thresholds and the
// FirstFit / BestFit choices (firstfit.py, bestfit.py), PM updates of step()
// (env.py), the arrival / service draws and kl_divergence (env.py:8-17).
// Included by vmp_env_wave.h, vmp_env_big.h and vmp_env_aux.h.
#ifndef VMP_ENV_COMMON_H
#define VMP_ENV_COMMON_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "vmp_dev.h"
#include "vmp_kernels.h"
#include "vmp_layout.h"
#include "vmp_np_rng.h"
#include "vmp_np_sort.h"
#include "vmp_np_sum.h"
#include "vmp_stamps.h"

namespace vmp {

// --------------------------------------------------------- env kernel ----
// Per-wave LDS carve (offsets from EnvParams, computed by the host: vmp_carve.h).
struct Lds {
  EnvHdr LDSP *hdr;                  // the env's 256-B header (scalars, RNG streams)
  double LDSP *cpu, *mem;       // f64[P] PM resources (the env state)
  float LDSP *fcpu, *fmem;      // f32[P] observation view used by the heuristics
  uint8_t LDSP *tc, *tm;        // per-PM largest fitting size (hundredths), f32 semantics
  uint16_t LDSP *ord;                // BF ascending argsort, then reversed into visiting order
  uint64_t LDSP *bc;                 // action phase: the any-fit table (u32 [128] at bc)
  int32_t LDSP *sortstk;             // introsort stacks
  uint16_t LDSP *nulls;              // NULL slot indices (aliases the fit bitmaps)
  uint8_t LDSP *accc, *accm;    // accepted sizes (alias the fit bitmaps)
  double LDSP *jobres;               // reduction results of the step
  int32_t LDSP *arr;                 // per-step arrivals of the launch (prologue draws)
  uint32_t LDSP *svc;                // speculative planned runtimes
  uint64_t LDSP *svcst;              // rng4 state after each speculative draw
  uint64_t LDSP *svcfb;              // rng4 state for fallback draws
  int32_t LDSP *svcinfo;             // [0] speculative count, [1] consumed
  uint8_t LDSP *ccomp, *mcomp;  // compressed sizes of existing VMs [ccomp_cap]
  uint64_t LDSP *pdirty;             // bit i: PM double i (cpu | memory) changed
  uint32_t LDSP *evw;                // k_env_big event lists [kEvCap]: VM word,
  int32_t LDSP *evt;                 //   target / value,
  uint8_t LDSP *evok;                //   result
  PwLds pw;
  char LDSP *base;                   // the wave's LDS region
};

// The wave's LDS view, rebuilt from its base address (cheap; avoids passing
// the pointer struct by value into out-of-line helpers).
__device__ __forceinline__ Lds make_lds(const EnvParams &p, char LDSP *base) {
  Lds L;
  L.hdr = reinterpret_cast<EnvHdr LDSP *>(base + p.off_hdr);
  L.cpu = reinterpret_cast<double LDSP *>(base + p.off_pm);
  L.mem = L.cpu + p.P;
  L.fcpu = reinterpret_cast<float LDSP *>(base + p.off_fpm);
  L.fmem = L.fcpu + p.fmem_off;  // k_env_big: 16-B aligned rows (vector reads in big_choose)
  L.tc = reinterpret_cast<uint8_t LDSP *>(base + p.off_thr);
  L.tm = L.tc + p.tm_off;
  L.ord = reinterpret_cast<uint16_t LDSP *>(base + p.off_ord);
  L.bc = reinterpret_cast<uint64_t LDSP *>(base + p.off_bits);
  L.sortstk = reinterpret_cast<int32_t LDSP *>(base + p.off_sort);
  L.nulls = reinterpret_cast<uint16_t LDSP *>(base + p.off_bits);
  L.accc = reinterpret_cast<uint8_t LDSP *>(base + p.off_acc);
  L.accm = L.accc + p.acc_cap;
  L.jobres = reinterpret_cast<double LDSP *>(base + p.off_stage);
  L.svcinfo = reinterpret_cast<int32_t LDSP *>(base + p.off_stage + kStageSvcInfo);
  L.svcfb = reinterpret_cast<uint64_t LDSP *>(base + p.off_stage + kStageSvcFb);
  L.svcst = reinterpret_cast<uint64_t LDSP *>(base + p.off_pre);
  L.svc = reinterpret_cast<uint32_t LDSP *>(base + p.off_pre + kSpecStateBytes * p.scap);
  L.arr = reinterpret_cast<int32_t LDSP *>(base + p.off_pre + kSpecDrawBytes * p.scap);
  L.pdirty = reinterpret_cast<uint64_t LDSP *>(base + p.off_pdirty);
  L.ccomp = reinterpret_cast<uint8_t LDSP *>(base + p.off_ccomp);
  L.mcomp = L.ccomp + p.ccomp_cap;
  L.evw = reinterpret_cast<uint32_t LDSP *>(base + p.off_ev);
  L.evt = reinterpret_cast<int32_t LDSP *>(L.evw + kEvCap);
  L.evok = reinterpret_cast<uint8_t LDSP *>(L.evt + kEvCap);
  L.pw.lo = reinterpret_cast<int32_t LDSP *>(base + p.off_leaf);
  L.pw.len = L.pw.lo + p.n_leaf;
  L.pw.stk = L.pw.len + p.n_leaf;
  L.pw.val = reinterpret_cast<double LDSP *>(base + p.off_leafval);
  L.base = base;
  return L;
}

// Exact k/100 for k = 0..127 (np.around(., 2) values), per block.
struct Tables {
  double cent[128];
  float fcent[128];
  PoisConst pois[2];  // block copy of p.pois, read by the prologue draws
};
// k_env's static LDS is one Tables per workgroup; the host's carve check
// (vmp_create) allows kEnvStaticLds for it. The diagnostic builds add st_lds
// (-DVMP_STAMPS) and wg_marks (-DVMP_WGTIME) on top.
static_assert(sizeof(Tables) == 1696 && sizeof(Tables) <= kEnvStaticLds, "k_env static LDS");

__device__ __forceinline__ int w_pl(uint32_t w) { return (int)(w & 0xFFFFu); }
// Register slots past V hold placement kPad: no test for running (< P), WAIT,
// NULL or existing (<= WAIT) matches it, so the per-slot loops need no lane
// range mask (keeping 16 64-bit masks live would spill SGPRs); only stores
// test live().
constexpr int kPad = 0xFFFF;
__device__ __forceinline__ bool live(uint32_t w) { return w_pl(w) != kPad; }
__device__ __forceinline__ int w_cc(uint32_t w) { return (int)((w >> 16) & 0xFFu); }
__device__ __forceinline__ int w_cm(uint32_t w) { return (int)(w >> 24); }
__device__ __forceinline__ uint32_t w_make(int pl, int cc, int cm) {
  return (uint32_t)pl | ((uint32_t)cc << 16) | ((uint32_t)cm << 24);
}

__device__ __forceinline__ Pcg ld_pcg(const EnvHdr LDSP *h, int k) {
  Pcg r;
  r.s = U128{h->rng[k][0], h->rng[k][1]};
  r.inc = U128{h->rng[k][2], h->rng[k][3]};
  return r;
}
__device__ __forceinline__ void st_pcg(EnvHdr LDSP *h, int k, const Pcg &r) {
  if (lane_id() == 0) {
    h->rng[k][0] = r.s.hi;
    h->rng[k][1] = r.s.lo;
  }
}

// FC(k) = (float)(k / 100.0), the f32 obs value of a size of k hundredths;
// (float)(k * 0.01) equals it for every k in [0, 127] (checked exhaustively).
__device__ __forceinline__ float fcent_of(int k) { return (float)((double)k * 0.01); }

// Largest k in [0, 100] with f + FC(k) <= 1 in f32 (monotone in k), or -1.
// For every f32 f in [0, 1] (PM loads, env.py:267-268 keeps them >= 0) the
// answer is one of k0 - 1, k0, k0 + 1 with k0 = (int)((1 - f) * 100): checked
// exhaustively over all 1 065 353 217 such f.
__device__ __forceinline__ int fit_threshold(float f) {
  int k0 = (int)((1.0f - f) * 100.0f);
  k0 = k0 < 0 ? 0 : (k0 > 100 ? 100 : k0);
  const bool up = k0 < 100 && f + fcent_of(k0 + 1) <= 1.0f;
  const bool at = f + fcent_of(k0) <= 1.0f;
  return up ? k0 + 1 : (at ? k0 : k0 - 1);
}

// Inclusive prefix OR across the wave (lane i: OR of lanes 0..i) with DPP row
// shifts and the GFX9 row broadcasts: 6 VALU steps, no LDS traffic.
__device__ __forceinline__ uint32_t prefix_or32(uint32_t x) {
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false);  // row_shr:1
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false);  // row_shr:2
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false);  // row_shr:4
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false);  // row_shr:8
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);  // row_bcast:15
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);  // row_bcast:31
  return x;
}
__device__ __forceinline__ uint64_t prefix_or64(uint64_t x) {
  return ((uint64_t)prefix_or32((uint32_t)(x >> 32)) << 32) | prefix_or32((uint32_t)x);
}

// Inclusive prefix max across the wave for values >= 0 (0 is the identity).
__device__ __forceinline__ uint32_t prefix_max32(uint32_t x) {
  x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false));
  x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false));
  x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false));
  x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false));
  x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false));
  x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false));
  return x;
}

// Sum of x over the wave (wave-uniform result), the same six DPP steps.
__device__ __forceinline__ uint32_t wave_sum32(uint32_t x) {
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false);
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false);
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false);
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false);
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);
  return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

__device__ __forceinline__ uint64_t readlane_u64(uint64_t x, int l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}

// The any-fit table: M[k] = max of the +1-encoded memory thresholds tm over
// the PMs whose cpu threshold is >= k (0: none). A VM of sizes (kc, km) fits
// some PM iff M[kc] > km (firstfit.py:33, bestfit.py:35: cpu and memory both
// fit). Built per step and after each placement (only the placed PM's
// thresholds move); the heuristics' choices are then wave scans over the
// thresholds (ff_scan, bf_choose). Levels are mapped to lanes in reverse
// (row 63-i, and 127-i for levels 64..100), so the suffix max over k is a
// DPP lane prefix max.
__device__ __forceinline__ void build_fitmax(const EnvParams &p, const Lds &L, uint32_t LDSP *M) {
  const int lane = lane_id();
  M[lane] = 0;
  M[lane + 64] = 0;
  wsync();
  for (int q = lane; q < p.P; q += 64) {
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

// FirstFit's PM for sizes (kc, km) (firstfit.py:33-37): the first PM in index
// order whose f32 thresholds accept both, by a wave scan over the PMs' u8
// thresholds (P/64 ballots; no fit bitmaps to build or maintain). -1 if none.
__device__ __forceinline__ int ff_scan(const EnvParams &p, const Lds &L, int kc, int km) {
  const int lane = lane_id();
  for (int b = 0; b < p.P; b += 64) {
    const int i = b + lane;
    const bool f = i < p.P && (int)L.tc[i] - 1 >= kc && (int)L.tm[i] - 1 >= km;
    const uint64_t m = ballot(f);
    if (m) return b + __ffsll((unsigned long long)m) - 1;
  }
  return -1;
}

// BestFit's choice for sizes (kc, km) (bestfit.py:33-39): the first PM in
// visiting order flip(argsort(fcpu + fmem)) that fits, i.e. the fitting PM of
// largest key. Fast path: a wave argmax over the PMs; only when two or more
// fitting PMs share the largest key m does their order matter. The keys equal
// to m occupy the ascending positions [P - above - eq, P - above) (above =
// keys > m, none of which fits); the scalar introsort (numpy's tie order,
// SURVEY App. C) is run for that block only, and its highest fitting position
// (the first in visiting order) is taken. Returns -1 if nothing fits.
__device__ __forceinline__ int bf_tie(const EnvParams &p, const Lds &L, int kc, int km, int above,
                                   int eq);
__device__ __forceinline__ int bf_choose(const EnvParams &p, const Lds &L, int kc, int km) {
  const int lane = lane_id();
  const int P = p.P;
  float best = -INFINITY;
  int cnt = 0, bi = -1;
  for (int i = lane; i < P; i += 64) {
    if ((int)L.tc[i] - 1 >= kc && (int)L.tm[i] - 1 >= km) {
      const float key = L.fcpu[i] + L.fmem[i];
      if (key > best) {
        best = key;
        cnt = 1;
        bi = i;
      } else if (key == best) {
        cnt++;
      }
    }
  }
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
  // ties at the top: numpy's order decides
  int above = 0, eq = 0;
  for (int i = lane; i < P; i += 64) {
    const float key = L.fcpu[i] + L.fmem[i];
    above += key > m;
    eq += key == m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    above += __shfl_xor(above, o);
    eq += __shfl_xor(eq, o);
  }
  return bf_tie(p, L, kc, km, above, eq);
}

// BestFit's choice when eq >= 2 PMs share the largest fitting key m and
// `above` keys exceed it (none of which fits): the tied keys occupy the
// ascending positions [P - above - eq, P - above) of numpy's argsort; only the
// quicksort partitions that intersect that block are sorted, and the highest
// fitting position in it (the first in visiting order) is taken.
__device__ __forceinline__ int bf_tie(const EnvParams &p, const Lds &L, int kc, int km, int above,
                                   int eq) {
  const int lane = lane_id();
  const int P = p.P;
  for (int i = lane; i < P; i += 64) L.ord[i] = (uint16_t)i;
  const int hi = P - above - 1, lo = P - above - eq;
  wsync();
  const uint8_t LDSP *tc = L.tc, *tm = L.tm;
  const int pos = wave_aqselect_top(
      KeySum{L.fcpu, L.fmem}, L.ord, P, L.sortstk, lo, hi,
      reinterpret_cast<uint16_t LDSP *>(L.sortstk + kSortStackWords),
      [=](int q) { return (int)tc[q] - 1 >= kc && (int)tm[q] - 1 >= km; });
  return pos >= 0 ? (int)L.ord[pos] : -1;  // visiting order: descending positions
}

// Record that PM q's cpu and memory were written (one lane: the callers'
// writes are single-lane); the state store writes back only marked PM words.
__device__ __forceinline__ void mark_pm(const Lds &L, int P, int q) {
  L.pdirty[q >> 6] |= 1ull << (q & 63);
  L.pdirty[(P + q) >> 6] |= 1ull << ((P + q) & 63);
}

// One VM placement event of the env (env.py:74-84 for a WAIT -> PM move):
// _resource_valid in f64, then _place_vm. Returns validity (wave-uniform).
__device__ __forceinline__ bool env_place(const Lds &L, const Tables &T, int P, int q, int kc,
                                          int km) {
  double cq = L.cpu[q], mq = L.mem[q];
  double vc = T.cent[kc], vm = T.cent[km];
  bool ok = (cq + vc <= 1) && (mq + vm <= 1);
  wsync();
  if (ok && lane_id() == 0) {
    L.cpu[q] = cq + vc;
    L.mem[q] = mq + vm;
    mark_pm(L, P, q);
  }
  wsync();
  return ok;
}

// ---- random draws of a launch (prologue) ---------------------------------
// All Poisson draws a launch can need are taken BEFORE the VM state is loaded
// into registers, so the samplers never share the register budget with it:
// the K arrival counts (rng3, one per step, all consumed) and up to scap
// service lengths (rng4), speculative: only the first `used` are consumed and
// rng4 is committed to the state recorded after draw used-1 (draws past scap
// come from the out-of-line fallback below).
__device__ __noinline__ uint32_t svc_fallback(uint64_t LDSP *st, const uint64_t LDSP *inc,
                                              const PoisConst *c) {
  Pcg r;
  r.s = U128{st[0], st[1]};
  r.inc = U128{inc[0], inc[1]};
  const int64_t x = poisson(r, *c);
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if ((threadIdx.x & 63) == 0) {
    st[0] = r.s.hi;
    st[1] = r.s.lo;
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  return (uint32_t)(x + 1);
}

// Lane-parallel PCG64: lane j of a chunk holds the state after j+1 draws from
// the chunk's base state, s_j = A_j*base + M_j*inc (jump table p.jump), and
// its uniform next_double. Draws are consumed in stream order; the committed
// state after `pos` draws of the chunk is the base (pos = 0) or lane pos-1's.
struct ParRng {
  U128 base, inc;  // wave-uniform
  U128 st;         // lane j: state after j+1 draws of the chunk
  double u;        // lane j: uniform j of the chunk
  int pos;         // draws consumed in this chunk (wave-uniform)
};
__device__ __forceinline__ U128 rl128(U128 x, int l) {
  return U128{readlane_u64(x.hi, l), readlane_u64(x.lo, l)};
}
__device__ __forceinline__ void par_fill(ParRng &g, const U128 &JA, const U128 &JM) {
  g.st = add128(mul128(JA, g.base), mul128(JM, g.inc));
  const uint64_t x = g.st.hi ^ g.st.lo;
  const unsigned rot = (unsigned)(g.st.hi >> 58);
  const uint64_t out = (x >> rot) | (x << ((64 - rot) & 63));
  g.u = (double)(out >> 11) * (1.0 / 9007199254740992.0);
  g.pos = 0;
}
__device__ __forceinline__ void par_next_chunk(ParRng &g, const U128 &JA, const U128 &JM) {
  g.base = rl128(g.st, 63);
  par_fill(g, JA, JM);
}
__device__ __forceinline__ U128 par_state(const ParRng &g) {
  return g.pos == 0 ? g.base : rl128(g.st, uni(g.pos - 1));
}

// random_poisson, mult method (lam < 10): the running product is formed in
// stream order (same rounding as the sequential loop), uniforms by readlane.
__device__ __forceinline__ int64_t par_poisson_mult(ParRng &g, double enlam, const U128 &JA,
                                                    const U128 &JM) {
  double prod = 1.0;
  int64_t X = 0;
#pragma unroll 1
  for (;;) {
    if (g.pos == 64) par_next_chunk(g, JA, JM);
    prod *= readlane_f64(g.u, uni(g.pos));
    g.pos++;
    if (prod > enlam)
      X += 1;
    else
      return X;
  }
}

// random_poisson_ptrs (lam >= 10): every loop iteration consumes one (U, V)
// pair and its outcome depends on that pair only, so lanes i < 32 evaluate
// pair i of the chunk at once; the n-th draw is the n-th accepting pair.
struct PtrsChunk {
  uint64_t acc;  // accepting pairs of the chunk
  int64_t k;     // lane i: k of pair i
  bool valid;
};
__device__ __forceinline__ void par_ptrs_eval(const ParRng &g, const PoisConst &c, PtrsChunk &pc) {
  const int lane = lane_id();
  const int i = lane & 31;
  const double U = __shfl(g.u, 2 * i) - 0.5;
  const double V = __shfl(g.u, 2 * i + 1);
  const double us = 0.5 - fabs(U);
  const int64_t k = (int64_t)floor((2 * c.a / us + c.b) * U + c.lam + 0.43);
  bool ok;
  if ((us >= 0.07) && (V <= c.vr))
    ok = true;
  else if ((k < 0) || ((us < 0.013) && (V > us)))
    ok = false;
  else
    ok = ptrs_accept(V, us, k, c.lam, c.a, c.b, c.loglam, c.log_invalpha, c.loggam_tab, c.tab_n);
  pc.acc = ballot(ok && lane < 32);
  pc.k = k;
  pc.valid = true;
}
__device__ __forceinline__ int64_t par_poisson_ptrs(ParRng &g, const PoisConst &c, PtrsChunk &pc,
                                                    const U128 &JA, const U128 &JM) {
#pragma unroll 1
  for (;;) {
    if (g.pos == 64) {
      par_next_chunk(g, JA, JM);
      pc.valid = false;
    }
    if (!pc.valid) par_ptrs_eval(g, c, pc);
    const uint64_t m = pc.acc & (~0ull << (g.pos >> 1));
    if (m == 0) {
      g.pos = 64;
      continue;
    }
    const int i = uni(__builtin_ctzll(m));
    g.pos = 2 * i + 2;
    return (int64_t)readlane_u64((uint64_t)pc.k, i);
  }
}

__device__ __forceinline__ int64_t par_poisson(ParRng &g, const PoisConst &c, PtrsChunk &pc,
                                               const U128 &JA, const U128 &JM) {
  if (c.kind == 0) return 0;  // lam == 0: no draw consumed
  if (c.kind == 1) return par_poisson_mult(g, c.enlam, JA, JM);
  return par_poisson_ptrs(g, c, pc, JA, JM);
}

__device__ __forceinline__ void predraw(const EnvParams &p, const Lds &L, const Tables &T,
                                        int K, int V, const U128 &JA, const U128 &JM) {
  const int lane = lane_id();
  EnvHdr LDSP *H = L.hdr;
  ParRng g;
  PtrsChunk pc;
  pc.valid = false;
  // K arrival counts, rng3 (env.py:272)
  Pcg r3 = ld_pcg(H, 2);
  g.base = r3.s;
  g.inc = r3.inc;
  par_fill(g, JA, JM);
  int64_t need = 0;
#pragma unroll 1
  for (int k = 0; k < K; k++) {
    const int64_t a = par_poisson(g, T.pois[0], pc, JA, JM);
    if (lane == 0) L.arr[k] = (int32_t)(a < 0x7fffffff ? a : 0x7fffffff);
    need += a < V ? a : V;
  }
  r3.s = par_state(g);
  st_pcg(H, 2, r3);
  // up to scap speculative service lengths, rng4 (env.py:289), with the state
  // after each draw for the commit
  Pcg r4 = ld_pcg(H, 3);
  // a one-step launch after a step that left no NULL slot and no running VM
  // due to finish accepts nothing (_accept_vm_requests fills NULL slots only):
  // no service length is drawn. The hint (EnvHdr::pad, written by the
  // previous per-step launch) only gates this speculation: a draw it wrongly
  // skipped would come from svc_fallback, from the same stream position.
  const uint64_t hint = H->pad;
  const bool none_free = K == 1 && (hint >> 63) && ((hint >> 32) & 1u) == 0 &&
                         (uint32_t)hint > (uint32_t)H->timestep + 1u;
  const int S = none_free ? 0 : (int)(need < p.scap ? need : p.scap);
  g.base = r4.s;
  g.inc = r4.inc;
  pc.valid = false;
  if (S > 0) par_fill(g, JA, JM);
#pragma unroll 1
  for (int j = 0; j < S; j++) {
    const int64_t x = par_poisson(g, T.pois[1], pc, JA, JM);
    const U128 sj = par_state(g);
    if (lane == 0) {
      L.svc[j] = (uint32_t)(x + 1);
      L.svcst[2 * j] = sj.hi;
      L.svcst[2 * j + 1] = sj.lo;
    }
  }
  const U128 fb = S > 0 ? par_state(g) : r4.s;
  if (lane == 0) {
    L.svcfb[0] = fb.hi;  // fallback continues after the last speculative draw
    L.svcfb[1] = fb.lo;
    L.svcinfo[0] = S;
    L.svcinfo[1] = 0;  // consumed
  }
  wsync();
}

// The Poisson records of env e: the handle's one pair, or (WL, the kernels of
// handles with a per-env workload) the env's own pair of p.pois[N][2]. e is
// wave-uniform, so this is scalar address arithmetic.
// (SRC: where an env's requests come from. kSrcConfig / kSrcEnv are the WL =
// false / true instantiations; kSrcTrace never calls this.)
constexpr int kSrcConfig = 0, kSrcEnv = 1, kSrcTrace = 2;
template <int SRC>
__device__ __forceinline__ const PoisConst *env_pois(const EnvParams &p, int e) {
  return SRC == kSrcEnv ? p.pois + 2 * (int64_t)e : p.pois;
}

// Next planned runtime (rng4.poisson(L) + 1, env.py:289) for an accepted VM
// of env e (the fallback reads that env's service-length record).
template <int SRC>
__device__ __forceinline__ uint32_t svc_take(const EnvParams &p, const Lds &L, int e) {
  const int S = L.svcinfo[0], used = L.svcinfo[1];
  uint32_t x;
  if (used < S) {
    x = L.svc[used];
  } else {
    x = svc_fallback(L.svcfb, &L.hdr->rng[3][2], env_pois<SRC>(p, e) + 1);
  }
  wsync();
  if (lane_id() == 0) L.svcinfo[1] = used + 1;
  wsync();
  return x;
}

// Commit rng4 to the state after the last consumed draw.
__device__ __forceinline__ void svc_commit(const Lds &L) {
  const int S = L.svcinfo[0], used = L.svcinfo[1];
  if (used == 0) return;
  uint64_t hi, lo;
  if (used <= S) {
    hi = L.svcst[2 * (used - 1)];
    lo = L.svcst[2 * (used - 1) + 1];
  } else {
    hi = L.svcfb[0];
    lo = L.svcfb[1];
  }
  wsync();
  if (lane_id() == 0) {
    L.hdr->rng[3][0] = hi;
    L.hdr->rng[3][1] = lo;
  }
  wsync();
}

// ---- trace-fed requests (kSrcTrace: the kernels of vmp_kernels_tr.hip) ----
// A traced env draws nothing: the step at timestep s + 1 is offered the
// requests [offs[s], offs[s+1]) of its trace (none from step `steps` on), so
// the prologue's draws are replaced by one lane-parallel load of the launch's
// offsets. The per-launch draw region (off_pre) is idle on this path: its first
// 512 B (svcst) stage up to 64 packed requests, and svcfb[0] holds the index
// of the current step's first request (a dropped request is consumed: every
// step advances it by its whole arrival count).
__device__ __forceinline__ TraceDesc env_trace(const EnvParams &p, int e) {
  const TraceDesc *d = reinterpret_cast<const TraceDesc *>(p.pois) + e;  // e: wave-uniform
  return TraceDesc{d->offs, d->req, d->steps, 0};
}
__device__ __forceinline__ int rq_cc(uint64_t rq) { return (int)((rq >> 16) & 0xFFu); }
__device__ __forceinline__ int rq_cm(uint64_t rq) { return (int)((rq >> 24) & 0xFFu); }
__device__ __forceinline__ uint32_t rq_rt(uint64_t rq) { return (uint32_t)(rq >> 32); }

// L.arr[0..K) of a launch that starts at the header's timestep, and the first
// step's first 64 requests staged (the accept loop of step 0 finds them there).
// Every index is clamped into [0, steps], so no load is conditional.
__device__ __forceinline__ void trace_preload(const Lds &L, const TraceDesc &d, int K) {
  const int lane = lane_id();
  const int64_t GLBP *offs = gptr(d.offs);
  const int64_t ts = L.hdr->timestep;
  const int64_t s0 = ts > 1 ? ts - 1 : 0;
  uint64_t first = 0;
  int a0 = 0;
#pragma unroll 1
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int k = k0 + lane;
    const int64_t i0 = s0 + k < d.steps ? s0 + k : d.steps;
    const int64_t i1 = i0 < d.steps ? i0 + 1 : d.steps;
    const int64_t o0 = offs[i0], o1 = offs[i1];
    if (k < K) L.arr[k] = (int32_t)(o1 - o0);  // < 2^31 per trace (trace_check)
    if (k0 == 0) {
      first = readlane_u64((uint64_t)o0, 0);
      a0 = __builtin_amdgcn_readlane((int)(o1 - o0), 0);
    }
  }
  const uint64_t GLBP *req = gptr(d.req);
  L.svcst[lane] = lane < a0 ? req[first + (uint64_t)lane] : 0ull;
  if (lane == 0) L.svcfb[0] = first;
  wsync();
}

// kl_divergence (env.py:8-17) in numpy/LAPACK/OpenBLAS evaluation order.
__device__ __forceinline__ double kl_reward(double tcm, double tmm, double tcv, double tmv,
                                            double cm, double mm, double cv, double mv) {
  double det_q = exp((0.0 + log(cv)) + log(mv));
  double det_p = exp((0.0 + log(tcv)) + log(tmv));
  double qi0 = 1.0 / cv, qi1 = 1.0 / mv;
  double tr = qi0 * tcv + qi1 * tmv;
  double d0 = tcm - cm, d1 = tmm - mm;
  double m1 = fma(d1 * qi1, d1, (d0 * qi0) * d0);
  double kl = 0.5 * ((((log(det_q / det_p) - 2) + tr) + m1) - tr);
  return -kl;
}

}  // namespace vmp

#endif  // VMP_ENV_COMMON_H
