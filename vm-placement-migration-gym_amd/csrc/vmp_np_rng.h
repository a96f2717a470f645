// vmp_np_rng.h — numpy's PCG64 bit generator (pcg64.h, SeedSequence seeding,
// advance) and random_poisson / random_loggam of numpy's distributions.c,
// restated bit for bit. Included by vmp_env_common.h and vmp_env_aux.h.
#ifndef VMP_NP_RNG_H
#define VMP_NP_RNG_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "vmp_dev.h"
#include "vmp_layout.h"

namespace vmp {

// ------------------------------------------------------------- PCG64 -----
// numpy PCG64 (pcg64.h): 128-bit LCG, XSL-RR output, next_double = (u64>>11)*2^-53.
struct U128 {
  uint64_t hi, lo;
};
constexpr uint64_t kMulHi = 0x2360ED051FC65DA4ULL, kMulLo = 0x4385DF649FCCF645ULL;

__device__ __forceinline__ U128 mul128(U128 a, U128 b) {
  U128 r;
  r.lo = a.lo * b.lo;
  r.hi = __umul64hi(a.lo, b.lo) + a.lo * b.hi + a.hi * b.lo;
  return r;
}
__device__ __forceinline__ U128 add128(U128 a, U128 b) {
  U128 r;
  r.lo = a.lo + b.lo;
  r.hi = a.hi + b.hi + (r.lo < a.lo);
  return r;
}
struct Pcg {
  U128 s, inc;
};
__device__ __forceinline__ uint64_t pcg_next(Pcg &r) {
  r.s = add128(mul128(r.s, U128{kMulHi, kMulLo}), r.inc);
  uint64_t x = r.s.hi ^ r.s.lo;
  unsigned rot = (unsigned)(r.s.hi >> 58);
  return (x >> rot) | (x << ((64 - rot) & 63));
}
__device__ __forceinline__ double next_double(Pcg &r) {
  return (double)(pcg_next(r) >> 11) * (1.0 / 9007199254740992.0);
}
// pcg_advance_lcg_128: jump by delta draws.
__device__ void pcg_advance(Pcg &r, uint64_t delta) {
  U128 cur_mult{kMulHi, kMulLo}, cur_plus = r.inc, acc_mult{0, 1}, acc_plus{0, 0};
  while (delta > 0) {
    if (delta & 1) {
      acc_mult = mul128(acc_mult, cur_mult);
      acc_plus = add128(mul128(acc_plus, cur_mult), cur_plus);
    }
    cur_plus = mul128(add128(cur_mult, U128{0, 1}), cur_plus);
    cur_mult = mul128(cur_mult, cur_mult);
    delta >>= 1;
  }
  r.s = add128(mul128(acc_mult, r.s), acc_plus);
}
// SeedSequence(seed).generate_state(4, uint64) -> pcg64_set_seed (bit_generator.pyx).
__device__ void pcg_seed(Pcg &r, uint64_t seed) {
  const uint32_t INIT_A = 0x43b0d7e5u, MULT_A = 0x931e8875u, INIT_B = 0x8b51f9ddu,
                 MULT_B = 0x58f38dedu, MIX_L = 0xca01f9ddu, MIX_R = 0x4973f715u;
  uint32_t ent0 = (uint32_t)seed, ent1 = (uint32_t)(seed >> 32);
  int n_ent = (seed >> 32) ? 2 : 1;
  uint32_t pool[4];
  uint32_t hc = INIT_A;
  auto hashmix = [&](uint32_t v) {
    v ^= hc;
    hc *= MULT_A;
    v *= hc;
    v ^= v >> 16;
    return v;
  };
#pragma unroll
  for (int i = 0; i < 4; i++) pool[i] = hashmix(i == 0 ? ent0 : (i == 1 && n_ent == 2 ? ent1 : 0u));
#pragma unroll
  for (int s = 0; s < 4; s++)
#pragma unroll
    for (int d = 0; d < 4; d++)
      if (s != d) {
        uint32_t h = hashmix(pool[s]);
        uint32_t x = MIX_L * pool[d] - MIX_R * h;
        pool[d] = x ^ (x >> 16);
      }
  uint32_t w[8];
  uint32_t hb = INIT_B;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint32_t d = pool[i & 3];
    d ^= hb;
    hb *= MULT_B;
    d *= hb;
    w[i] = d ^ (d >> 16);
  }
  uint64_t v0 = w[0] | ((uint64_t)w[1] << 32), v1 = w[2] | ((uint64_t)w[3] << 32);
  uint64_t v2 = w[4] | ((uint64_t)w[5] << 32), v3 = w[6] | ((uint64_t)w[7] << 32);
  U128 s{v0, v1}, inc{v2, v3};
  r.inc = U128{(inc.hi << 1) | (inc.lo >> 63), (inc.lo << 1) | 1};
  r.s = U128{0, 0};
  r.s = add128(mul128(r.s, U128{kMulHi, kMulLo}), r.inc);
  r.s = add128(r.s, s);
  r.s = add128(mul128(r.s, U128{kMulHi, kMulLo}), r.inc);
}

// random_loggam (distributions.c) — device fallback outside the host table.
__device__ double loggam_dev(double x) {
  const double a[10] = {8.333333333333333e-02, -2.777777777777778e-03, 7.936507936507937e-04,
                        -5.952380952380952e-04, 8.417508417508418e-04, -1.917526917526918e-03,
                        6.410256410256410e-03, -2.955065359477124e-02, 1.796443723688307e-01,
                        -1.39243221690590e+00};
  if (x == 1.0 || x == 2.0) return 0.0;
  int64_t n = (x < 7.0) ? (int64_t)(7 - x) : 0;
  double x0 = x + n;
  double x2 = (1.0 / x0) * (1.0 / x0);
  double gl0 = a[9];
  for (int k = 8; k >= 0; k--) {
    gl0 *= x2;
    gl0 += a[k];
  }
  double gl = gl0 / x0 + 0.5 * 1.8378770664093453e+00 + (x0 - 0.5) * log(x0) - x0;
  if (x < 7.0)
    for (int64_t k = 1; k <= n; k++) {
      gl -= log(x0 - 1.0);
      x0 -= 1.0;
    }
  return gl;
}

// loggam beyond the host table (k > lam + 16 sqrt(lam) + 64): never reached in
// practice; out of line so it costs the env kernel no registers.
__device__ __noinline__ double loggam_far(double x) { return loggam_dev(x); }

// PTRS acceptance test of random_poisson_ptrs (distributions.c), the branch
// taken by ~14% of draws: out of line so its log()s do not hold registers in
// the env kernel. loggam(k+1) comes from the host table (glibc) when in range.
__device__ __forceinline__ bool ptrs_accept(double V, double us, int64_t k, double lam, double a,
                                         double b, double loglam, double log_invalpha,
                                         const double *tab, int tab_n) {
  const double lg = (k + 1 < tab_n) ? gptr(tab)[k + 1] : loggam_far((double)(k + 1));
  return (log(V) + log_invalpha - log(a / (us * us) + b)) <= (-lam + k * loglam - lg);
}

// random_poisson (distributions.c): mult method (lam < 10) / PTRS (lam >= 10).
__device__ __forceinline__ int64_t poisson(Pcg &r, const PoisConst &c) {
  if (c.kind == 2) {
#pragma unroll 1
    for (;;) {
      const double U = next_double(r) - 0.5;
      const double V = next_double(r);
      const double us = 0.5 - fabs(U);
      const int64_t k = (int64_t)floor((2 * c.a / us + c.b) * U + c.lam + 0.43);
      if ((us >= 0.07) && (V <= c.vr)) return k;
      if ((k < 0) || ((us < 0.013) && (V > us))) continue;
      if (ptrs_accept(V, us, k, c.lam, c.a, c.b, c.loglam, c.log_invalpha, c.loggam_tab, c.tab_n))
        return k;
    }
  } else if (c.kind == 0) {
    return 0;
  }
  double prod = 1.0;
  int64_t X = 0;
#pragma unroll 1
  for (;;) {
    prod *= next_double(r);
    if (prod > c.enlam)
      X += 1;
    else
      return X;
  }
}

}  // namespace vmp

#endif  // VMP_NP_RNG_H
