// vmp_prims.hip — test-only library (vmp/libvmp_prims.so, tests/test_gpu_prims.py):
// the device's restatements of numpy, each behind a small kernel of its own so
// that a test reaches it with inputs of its choosing. One wave per case, grid =
// number of cases. Nothing of the algorithms is restated here: the kernels
// call PCG64 and random_poisson (vmp_np_rng.h), the lane-parallel draws
// (vmp_env_common.h), the pairwise sum (vmp_np_sum.h) and the scalar introsort
// (vmp_np_sort.h) as the env kernels do, with the host-side setup the library
// uses (vmp_host.h, vmp_carve.h). libvmp.so does not link this unit.
//
// Every entry point takes device pointers, checks the cases' sizes and ranges
// on the host before it launches, runs on the null stream and returns after
// the kernel has finished. 0 on success; vmp_prims_last_error() has the text.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/vmp.h"
#include "vmp_carve.h"
#include "vmp_env_common.h"
#include "vmp_host.h"

using namespace vmp;

namespace {

constexpr int kMaxCases = 1 << 20;

// A device array of the caller's, on the host (the cases' sizes and offsets).
template <class T>
int fetch(const T *dev, int64_t n, std::vector<T> &out) {
  if (!dev && n > 0) return fail(VMP_EINVAL, "null argument");
  out.resize((size_t)n);
  if (n > 0) HIP_TRY(hipMemcpy(out.data(), dev, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost));
  return VMP_OK;
}
int finished() {
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  return VMP_OK;
}
int check_cases(int32_t n_cases) {
  if (n_cases < 1 || n_cases > kMaxCases) return fail(VMP_EINVAL, "n_cases out of range");
  return VMP_OK;
}

// The stream of `seed`, `offset` raw draws in.
__device__ __forceinline__ Pcg stream_at(uint64_t seed, uint64_t offset) {
  Pcg r;
  pcg_seed(r, seed);
  pcg_advance(r, offset);
  return r;
}

// ------------------------------------------------------------------ RNG ----
__global__ __launch_bounds__(64) void k_prims_seed(const uint64_t *seeds, uint64_t *out) {
  Pcg r;
  pcg_seed(r, seeds[blockIdx.x]);
  if (lane_id() == 0) {
    uint64_t *o = out + 4 * (int64_t)blockIdx.x;
    o[0] = r.s.hi;
    o[1] = r.s.lo;
    o[2] = r.inc.hi;
    o[3] = r.inc.lo;
  }
}

__global__ __launch_bounds__(64) void k_prims_draws(const uint64_t *seeds, const uint64_t *deltas,
                                                    int32_t nd, uint64_t *raw, double *dbl) {
  Pcg r = stream_at(seeds[blockIdx.x], deltas[blockIdx.x]);
  Pcg q = r;
  for (int i = 0; i < nd; i++) {
    const uint64_t x = pcg_next(r);
    const double u = next_double(q);
    if (lane_id() == 0) {
      raw[(int64_t)blockIdx.x * nd + i] = x;
      dbl[(int64_t)blockIdx.x * nd + i] = u;
    }
  }
}

// -------------------------------------------------------------- Poisson ----
// nd draws of poisson() by the serial sampler (every lane alike, as
// svc_fallback runs it), the state after each, and the raw draw that follows.
__global__ __launch_bounds__(64) void k_prims_poisson_serial(const uint64_t *seeds,
                                                             const uint64_t *offsets,
                                                             const PoisConst *pois, int32_t nd,
                                                             int64_t *draws, uint64_t *states,
                                                             uint64_t *after) {
  const int64_t c0 = blockIdx.x;
  Pcg r = stream_at(seeds[c0], offsets[c0]);
  const PoisConst c = pois[c0];
  for (int i = 0; i < nd; i++) {
    const int64_t x = poisson(r, c);
    if (lane_id() == 0) {
      draws[c0 * nd + i] = x;
      states[2 * (c0 * nd + i)] = r.s.hi;
      states[2 * (c0 * nd + i) + 1] = r.s.lo;
    }
  }
  const uint64_t x = pcg_next(r);
  if (lane_id() == 0) after[c0] = x;
}

// The same through the lane-parallel form, as predraw runs it: ParRng filled
// from the stream's state, par_poisson per draw, par_state after each.
__global__ __launch_bounds__(64) void k_prims_poisson_par(const uint64_t *seeds,
                                                          const uint64_t *offsets,
                                                          const PoisConst *pois,
                                                          const uint64_t *jump, int32_t nd,
                                                          int64_t *draws, uint64_t *states) {
  const int64_t c0 = blockIdx.x;
  const int lane = lane_id();
  const uint64_t GLBP *jt = gptr(jump + 4 * lane);
  const U128 JA{jt[0], jt[1]}, JM{jt[2], jt[3]};
  const Pcg r = stream_at(seeds[c0], offsets[c0]);
  const PoisConst c = pois[c0];
  ParRng g;
  PtrsChunk pc;
  pc.valid = false;
  g.base = r.s;
  g.inc = r.inc;
  par_fill(g, JA, JM);
  for (int i = 0; i < nd; i++) {
    const int64_t x = par_poisson(g, c, pc, JA, JM);
    const U128 s = par_state(g);
    if (lane == 0) {
      draws[c0 * nd + i] = x;
      states[2 * (c0 * nd + i)] = s.hi;
      states[2 * (c0 * nd + i) + 1] = s.lo;
    }
  }
}

// ---------------------------------------------------------- pairwise sum ----
extern __shared__ __attribute__((aligned(16))) char prims_lds[];

template <int RD>
__global__ __launch_bounds__(64) void k_prims_pw_sum(const double *a, const int32_t *off,
                                                     const int32_t *n, int32_t n_leaf,
                                                     int32_t off_leafval, double *out) {
  char LDSP *base = (char LDSP *)prims_lds;
  PwLds S;  // as make_lds lays it out
  S.lo = reinterpret_cast<int32_t LDSP *>(base);
  S.len = S.lo + n_leaf;
  S.stk = S.len + n_leaf;
  S.val = reinterpret_cast<double LDSP *>(base + off_leafval);
  const double GLBP *src = gptr(a + off[blockIdx.x]);
  const double r = wave_pw_sum<RD>(n[blockIdx.x], [=](int i) { return src[i]; }, S);
  if (lane_id() == 0) out[blockIdx.x] = r;
}

// ----------------------------------------------------------------- sort ----
// LDS of one case: the order u16 [n], the introsort stacks i32
// [kSortStackWords] with the partition lists u16 [2 n] behind them (bf_tie's
// layout), then the keys f32 [n] (KeySum: two rows).
struct SortCase {
  int32_t key_off, n, lo, hi;  // keys at key_off of the pool; positions lo..hi wanted
  int32_t fit_off;             // form 2: the fit bytes at fit_off of the pool
  int32_t out_off;             // forms 0, 1: order[lo..hi] goes to out + out_off
};
constexpr int kSortSerial = 0, kSortWave = 1, kSortSelect = 2;

// offsets of the stacks and of the keys behind the order; host and device alike
__host__ __device__ constexpr int64_t up16(int64_t x) { return (x + 15) & ~(int64_t)15; }
__host__ __device__ constexpr int64_t sort_off_stk(int64_t n) { return up16(2 * n); }
__host__ __device__ constexpr int64_t sort_off_keys(int64_t n) {
  return sort_off_stk(n) + up16(4 * kSortStackWords + 4 * n);  // sort_bytes(n)
}
size_t sort_lds(int64_t n, bool sum) { return (size_t)(sort_off_keys(n) + 4 * n * (sum ? 2 : 1)); }

template <int FORM, bool SUM>
__global__ __launch_bounds__(64) void k_prims_sort(const float *ka, const float *kb,
                                                   const SortCase *cases, const uint8_t *fit,
                                                   uint16_t *order_out, int32_t *sel_out) {
  const SortCase c = cases[blockIdx.x];
  const int lane = lane_id();
  char LDSP *base = (char LDSP *)prims_lds;
  uint16_t LDSP *ord = reinterpret_cast<uint16_t LDSP *>(base);
  int32_t LDSP *stk = reinterpret_cast<int32_t LDSP *>(base + sort_off_stk(c.n));
  uint16_t LDSP *scr = reinterpret_cast<uint16_t LDSP *>(stk + kSortStackWords);
  float LDSP *fa = reinterpret_cast<float LDSP *>(base + sort_off_keys(c.n));
  float LDSP *fb = fa + c.n;
  for (int i = lane; i < c.n; i += 64) {
    ord[i] = (uint16_t)i;
    fa[i] = ka[c.key_off + i];
    if (SUM) fb[i] = kb[c.key_off + i];
  }
  wsync();
  auto run = [&](auto kv) {
    if constexpr (FORM == kSortSerial) {
      if (lane == 0) aquicksort_lds(kv, ord, c.n, stk, c.lo, c.hi);
      wsync();
    } else if constexpr (FORM == kSortWave) {
      wave_aquicksort(kv, ord, c.n, stk, c.lo, c.hi, scr);
    } else {
      const uint8_t GLBP *f = gptr(fit + c.fit_off);
      const int pos = wave_aqselect_top(kv, ord, c.n, stk, c.lo, c.hi, scr,
                                        [=](int q) { return f[q] != 0; });
      if (lane == 0) {
        sel_out[2 * (int64_t)blockIdx.x] = pos;
        sel_out[2 * (int64_t)blockIdx.x + 1] = pos >= 0 ? (int)ord[pos] : -1;
      }
    }
  };
  if constexpr (SUM) run(KeySum{fa, fb});
  else run(KeyArr{fa});
  if (FORM != kSortSelect)
    for (int i = c.lo + lane; i <= c.hi; i += 64) order_out[c.out_off + (i - c.lo)] = ord[i];
}

// leaves of numpy's reduction of n elements (one recursion per buffer of 8192)
int64_t np_leaves(int64_t n) {
  int64_t leaves = 0;
  for (int64_t base = 0; base < n; base += 8192) {
    std::vector<int64_t> st{n - base < 8192 ? n - base : 8192};
    while (!st.empty()) {
      const int64_t m = st.back();
      st.pop_back();
      if (m <= 128) {
        leaves++;
      } else {
        const int64_t n2 = m / 2 - (m / 2) % 8;
        st.push_back(n2);
        st.push_back(m - n2);
      }
    }
  }
  return leaves;
}

struct DevBuf {  // a counted device allocation freed at scope exit
  void *p = nullptr;
  ~DevBuf() { dev_free(p); }
};

}  // namespace

extern "C" {

const char *vmp_prims_last_error(void) { return g_err.c_str(); }

// pcg_seed of n seeds -> out u64 [n][4]: state hi, lo, inc hi, lo
int vmp_prims_pcg_seed(int32_t n_cases, const uint64_t *seeds, uint64_t *out) {
  if (check_cases(n_cases) != VMP_OK) return VMP_EINVAL;
  if (!seeds || !out) return fail(VMP_EINVAL, "null argument");
  hipLaunchKernelGGL(k_prims_seed, dim3(n_cases), dim3(64), 0, nullptr, seeds, out);
  return finished();
}

// per case: pcg_seed, pcg_advance(delta), then nd raw draws -> raw u64 [n][nd]
// and, from the same position, nd doubles -> dbl f64 [n][nd]
int vmp_prims_pcg_draws(int32_t n_cases, const uint64_t *seeds, const uint64_t *deltas, int32_t nd,
                        uint64_t *raw, double *dbl) {
  if (check_cases(n_cases) != VMP_OK) return VMP_EINVAL;
  if (!seeds || !deltas || !raw || !dbl || nd < 1 || nd > (1 << 20))
    return fail(VMP_EINVAL, "null argument or nd out of range");
  hipLaunchKernelGGL(k_prims_draws, dim3(n_cases), dim3(64), 0, nullptr, seeds, deltas, nd, raw, dbl);
  return finished();
}

// per case (seed, offset, lam, tab_n override): nd Poisson(lam) draws from the
// seed's stream `offset` raw draws in -> draws i64 [n][nd] and the state after
// every draw, states u64 [n][nd][2] (hi, lo). parallel = 0: poisson(), which
// also gives after u64 [n], the raw draw behind the last one; parallel = 1:
// ParRng / par_fill / par_poisson / par_state (after is not written). The
// constants are pois_consts' and the table make_loggam_tab's, as vmp_create
// sets them up; tab_n[i] > 0 replaces the record's table length (1: every
// accepted k goes through loggam_far) and must not exceed it.
int vmp_prims_poisson(int32_t parallel, int32_t n_cases, const uint64_t *seeds,
                      const uint64_t *offsets, const double *lams, const int32_t *tab_n,
                      int32_t nd, int64_t *draws, uint64_t *states, uint64_t *after) {
  if (check_cases(n_cases) != VMP_OK) return VMP_EINVAL;
  if (!seeds || !offsets || !draws || !states || (!parallel && !after) || nd < 1 || nd > (1 << 20))
    return fail(VMP_EINVAL, "null argument or nd out of range");
  std::vector<double> lam;
  std::vector<int32_t> tn;
  if (fetch(lams, n_cases, lam) != VMP_OK || fetch(tab_n, n_cases, tn) != VMP_OK) return VMP_EINVAL;
  std::vector<PoisConst> rec((size_t)n_cases);
  int32_t need = 0;
  for (int i = 0; i < n_cases; i++) {
    if (!(lam[i] >= 0) || lam[i] > 1e6) return fail(VMP_EINVAL, "lam out of range");
    pois_consts(lam[i], rec[i]);
    if (tn[i] < 0 || (tn[i] > 0 && tn[i] > rec[i].tab_n))
      return fail(VMP_EINVAL, "tab_n override beyond the record's table");
    if (rec[i].tab_n > need) need = rec[i].tab_n;
    if (tn[i] > 0 && rec[i].kind == 2) rec[i].tab_n = tn[i];
  }
  DevBuf tab, recs, jump;
  if (need > 0) {
    double *t = nullptr;
    const int rc = make_loggam_tab(need, &t);
    if (rc != VMP_OK) return rc;
    tab.p = t;
    for (auto &r : rec)
      if (r.kind == 2) r.loggam_tab = t;
  }
  PoisConst *drec = nullptr;
  HIP_TRY(dev_malloc(&drec, sizeof(PoisConst) * rec.size()));
  recs.p = drec;
  HIP_TRY(hipMemcpy(drec, rec.data(), sizeof(PoisConst) * rec.size(), hipMemcpyHostToDevice));
  if (parallel) {
    uint64_t jt[kJumpWords], *djt = nullptr;
    pcg_jump_table(jt);
    HIP_TRY(dev_malloc(&djt, sizeof(jt)));
    jump.p = djt;
    HIP_TRY(hipMemcpy(djt, jt, sizeof(jt), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_prims_poisson_par, dim3(n_cases), dim3(64), 0, nullptr, seeds, offsets, drec,
                       djt, nd, draws, states);
  } else {
    hipLaunchKernelGGL(k_prims_poisson_serial, dim3(n_cases), dim3(64), 0, nullptr, seeds, offsets,
                       drec, nd, draws, states, after);
  }
  return finished();
}

// wave_pw_sum<rd> (rd 4 or 6) of a[off[i] .. off[i] + n[i]) -> out f64 [n_cases];
// a has a_len elements. The LDS plan's arrays are sized as carve_wave sizes
// them for a config whose larger dimension is cap (n[i] <= cap).
int vmp_prims_pw_sum(int32_t rd, int32_t n_cases, const double *a, int64_t a_len, const int32_t *off,
                     const int32_t *n, int32_t cap, double *out) {
  if (check_cases(n_cases) != VMP_OK) return VMP_EINVAL;
  if ((rd != 4 && rd != 6) || !a || !out || cap < 1 || cap > 65533)
    return fail(VMP_EINVAL, "rd must be 4 or 6, cap in [1, 65533]");
  std::vector<int32_t> o, m;
  if (fetch(off, n_cases, o) != VMP_OK || fetch(n, n_cases, m) != VMP_OK) return VMP_EINVAL;
  const bool deep = cap > 1928;
  const int32_t n_leaf = deep ? pw_worst(cap).leaves + 8 : 1;
  if (pw_worst(cap).depth > 12) return fail(VMP_EINVAL, "cap exceeds the recursion depth");
  for (int i = 0; i < n_cases; i++) {
    if (m[i] < 0 || m[i] > cap || o[i] < 0 || (int64_t)o[i] + m[i] > a_len)
      return fail(VMP_EINVAL, "case outside the array or beyond cap");
    if (m[i] > pw_reg_cap(rd) && np_leaves(m[i]) > n_leaf)
      return fail(VMP_EINVAL, "case needs more leaves than the carve holds");
  }
  const int32_t off_leafval = (int32_t)align16(deep ? pw_plan_bytes(n_leaf) : 0);
  const size_t lds = (size_t)off_leafval + (size_t)(deep ? pw_val_bytes(n_leaf) : 0) + 16;
  if (lds > (size_t)kCuLdsBytes) return fail(VMP_EINVAL, "cap too large for the LDS");
  if (rd == 4)
    hipLaunchKernelGGL(k_prims_pw_sum<4>, dim3(n_cases), dim3(64), lds, nullptr, a, off, n, n_leaf,
                       off_leafval, out);
  else
    hipLaunchKernelGGL(k_prims_pw_sum<6>, dim3(n_cases), dim3(64), lds, nullptr, a, off, n, n_leaf,
                       off_leafval, out);
  return finished();
}

// The scalar introsort of keys ka[key_off .. key_off + n) (kb non-null, form 1
// only: of the f32 sums ka[i] + kb[i], formed at each read as BestFit's KeySum does), for
// positions lo..hi. cases: i32 [n_cases][6] = key_off, n, lo, hi, fit_off,
// out_off. form 0: aquicksort_lds on one lane; 1: wave_aquicksort; both write
// order[lo..hi] to order_out + out_off (u16, order_len elements in all).
// form 2: wave_aqselect_top with the fit bytes fit[fit_off + element] (fit_len
// bytes in all) -> sel_out i32 [n_cases][2]: the position (or -1) and the
// element there.
int vmp_prims_sort(int32_t form, int32_t n_cases, const float *ka, const float *kb, int64_t key_len,
                   const int32_t *cases, const uint8_t *fit, int64_t fit_len, uint16_t *order_out,
                   int64_t order_len, int32_t *sel_out) {
  if (check_cases(n_cases) != VMP_OK) return VMP_EINVAL;
  if (form < 0 || form > 2 || !ka || !cases) return fail(VMP_EINVAL, "bad form or null argument");
  if (form == kSortSelect ? (!fit || !sel_out) : !order_out) return fail(VMP_EINVAL, "null output");
  std::vector<int32_t> cs;
  if (fetch(cases, 6 * (int64_t)n_cases, cs) != VMP_OK) return VMP_EINVAL;
  int64_t n_max = 0;
  for (int i = 0; i < n_cases; i++) {
    const int64_t ko = cs[6 * i], n = cs[6 * i + 1], lo = cs[6 * i + 2], hi = cs[6 * i + 3];
    const int64_t fo = cs[6 * i + 4], oo = cs[6 * i + 5];
    if (n < 1 || n > 65533 || ko < 0 || ko + n > key_len || lo < 0 || hi < lo || hi >= n)
      return fail(VMP_EINVAL, "sort case outside its keys");
    if (form == kSortSelect ? (fo < 0 || fo + n > fit_len) : (oo < 0 || oo + (hi - lo + 1) > order_len))
      return fail(VMP_EINVAL, "sort case outside its fit bytes or its output");
    if (n > n_max) n_max = n;
  }
  const bool sum = kb != nullptr;
  if (sum && form != kSortWave) return fail(VMP_EINVAL, "two key rows: wave_aquicksort only");
  const size_t lds = sort_lds(n_max, sum);
  if (lds > (size_t)kCuLdsBytes) return fail(VMP_EINVAL, "n too large for the LDS");
  const SortCase *sc = reinterpret_cast<const SortCase *>(cases);
  static_assert(sizeof(SortCase) == 24, "SortCase is six i32");
  const dim3 grid(n_cases), block(64);
#define PRIMS_SORT(FORM, SUM) \
  hipLaunchKernelGGL((k_prims_sort<FORM, SUM>), grid, block, lds, nullptr, ka, kb, sc, fit, order_out, sel_out)
  if (form == kSortSerial) {
    PRIMS_SORT(kSortSerial, false);
  } else if (form == kSortWave) {
    if (sum) PRIMS_SORT(kSortWave, true);
    else PRIMS_SORT(kSortWave, false);
  } else {
    PRIMS_SORT(kSortSelect, false);
  }
#undef PRIMS_SORT
  return finished();
}

}  // extern "C"
