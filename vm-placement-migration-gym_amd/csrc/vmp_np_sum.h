// vmp_np_sum.h — numpy's pairwise summation (DOUBLE_pairwise_sum,
// loops_utils.h.src) by one wave, in numpy's order of additions. Included by
// vmp_env_common.h and vmp_env_aux.h.
#ifndef VMP_NP_SUM_H
#define VMP_NP_SUM_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vmp_carve.h"
#include "vmp_dev.h"

namespace vmp {

// ---------------------------------------------------- pairwise summation --
// numpy DOUBLE_pairwise_sum (loops_utils.h.src, PW_BLOCKSIZE 128) of
// f(0..n-1) by one wave. Leaves (<= 128 elements: 8 interleaved accumulator
// chains, an ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) combine, a sequential tail)
// run lane-parallel (8 lanes per leaf); the split n2 = n/2 - (n/2)%8 is
// enumerated and the partial sums combined by lane 0 alone on small LDS
// stacks, so no cross-lane hand-off happens inside the recursion.
struct PwLds {
  int32_t LDSP *lo, *len;  // leaf list (DFS order), n_leaf entries
  int32_t LDSP *stk;            // lane-0 stack, 3 * 64 ints
  double LDSP *val;             // leaf sums, + value stack
};

// numpy's add.reduce hands DOUBLE_pairwise_sum one iterator buffer at a time
// (NPY_BUFSIZE = 8192 elements of a contiguous array): the result is
// 0.0 + pw(a[0:8192]) + pw(a[8192:16384]) + ..., the buffers added in order.
// One buffer (n <= 8192) is the plain recursion over n.
constexpr int kNpBufSize = 8192;

// lane 0 only: leaves of the recursions for n, left to right (buffer by buffer).
// Out of line, as pw_combine: the LDS plan is the rare path of the wave
// kernels, and inlined its loops cost the common path registers.
__device__ __noinline__ int pw_plan(int n, PwLds S) {
  int nl = 0;
  for (int base = 0; base < n; base += kNpBufSize) {
    int sp = 2;
    S.stk[0] = base;
    S.stk[1] = n - base < kNpBufSize ? n - base : kNpBufSize;
    while (sp > 0) {
      sp -= 2;
      const int o = S.stk[sp], m = S.stk[sp + 1];
      if (m <= 128) {
        S.lo[nl] = o;
        S.len[nl] = m;
        nl++;
      } else {
        int n2 = m / 2;
        n2 -= n2 % 8;
        S.stk[sp] = o + n2;  // right, popped second
        S.stk[sp + 1] = m - n2;
        S.stk[sp + 2] = o;   // left, popped first
        S.stk[sp + 3] = n2;
        sp += 4;
      }
    }
  }
  return nl;
}

// lane 0 only: per buffer, pw(m) = pw(n2) + pw(m - n2) over the leaf sums in
// val[]; the buffers' sums are added in order onto 0.0 (one buffer: its sum).
__device__ __noinline__ double pw_combine(int n, PwLds S, int nl) {
  double LDSP *vs = S.val + nl;  // value stack after the leaf sums
  int leaf = 0;
  double acc = 0.0;
  for (int base = 0; base < n; base += kNpBufSize) {
    int sp = 2, vsp = 0;
    S.stk[0] = n - base < kNpBufSize ? n - base : kNpBufSize;
    S.stk[1] = 0;
    while (sp > 0) {
      sp -= 2;
      const int m = S.stk[sp], ph = S.stk[sp + 1];
      if (m <= 128) {
        vs[vsp++] = S.val[leaf++];
      } else if (ph == 0) {
        int n2 = m / 2;
        n2 -= n2 % 8;
        S.stk[sp + 1] = 1;  // revisit after both children
        S.stk[sp + 2] = m - n2;
        S.stk[sp + 3] = 0;
        S.stk[sp + 4] = n2;
        S.stk[sp + 5] = 0;
        sp += 6;
      } else {
        const double b = vs[--vsp];
        const double a = vs[--vsp];
        vs[vsp++] = a + b;
      }
    }
    if (n <= kNpBufSize) return vs[0];
    acc += vs[0];
  }
  return acc;
}

__device__ __forceinline__ double readlane_f64(double x, int l) {
  const int64_t b = __double_as_longlong(x);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), l);
  return __longlong_as_double((int64_t)(((uint64_t)hi << 32) | lo));
}

// Register-resident plan (depth <= RD): leaf cnt's (offset, size) lands in
// lane cnt; the combine reads leaf sums by readlane. pw_reg_cap(RD) is the
// largest n such that every n' <= n splits into at most RD levels and 64
// leaves (1928 for RD = 4, 7688 for RD = 6; host check: vmp_capi.cpp pw_depth).
constexpr int kPwRegDepth = 4;
constexpr int pw_reg_cap(int rd) { return rd <= 4 ? 1928 : rd == 5 ? 3848 : 7688; }
template <int D>
__device__ __forceinline__ void pw_enum_r(int o, int n, int &cnt, int lane, int &my_o,
                                          int &my_m) {
  if (D == 0 || n <= 128) {
    if (lane == cnt) {
      my_o = o;
      my_m = n;
    }
    cnt++;
    return;
  }
  int n2 = n / 2;
  n2 -= n2 % 8;
  pw_enum_r<(D > 0 ? D - 1 : 0)>(o, n2, cnt, lane, my_o, my_m);
  pw_enum_r<(D > 0 ? D - 1 : 0)>(o + n2, n - n2, cnt, lane, my_o, my_m);
}
template <int D>
__device__ __forceinline__ double pw_comb_r(int n, int &cnt, double myval) {
  if (D == 0 || n <= 128) return readlane_f64(myval, cnt++);
  int n2 = n / 2;
  n2 -= n2 % 8;
  const double a = pw_comb_r<(D > 0 ? D - 1 : 0)>(n2, cnt, myval);
  const double b = pw_comb_r<(D > 0 ? D - 1 : 0)>(n - n2, cnt, myval);
  return a + b;
}

// One leaf [o, o+m) by the 8-lane group of the calling lane; the value is
// valid in the group's lane j == 0. Chain loads are issued 8 at a time.
template <class F>
__device__ __forceinline__ double pw_leaf_group(int o, int m, F &f) {
  const int j = lane_id() & 7;
  const int full = m - (m % 8);
  const int cnt = full >> 3;  // elements per accumulator chain (<= 16)
  double r = 0.0;
  if (cnt > 0) {
    double x[8];
#pragma unroll
    for (int t = 0; t < 8; t++) x[t] = t < cnt ? f(o + j + 8 * t) : 0.0;
    r = x[0];
#pragma unroll
    for (int t = 1; t < 8; t++)
      if (t < cnt) r += x[t];
    if (cnt > 8) {
#pragma unroll
      for (int t = 0; t < 8; t++) x[t] = t + 8 < cnt ? f(o + j + 8 * (t + 8)) : 0.0;
#pragma unroll
      for (int t = 0; t < 8; t++)
        if (t + 8 < cnt) r += x[t];
    }
  }
  // ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)): xor-pairs reproduce the tree exactly
  // (f64 addition is commutative)
  r = r + __shfl_xor(r, 1);
  r = r + __shfl_xor(r, 2);
  r = r + __shfl_xor(r, 4);
  double res = cnt > 0 ? r : 0.0;
  if (j == 0) {
    double tl[7];
#pragma unroll
    for (int t = 0; t < 7; t++) tl[t] = full + t < m ? f(o + full + t) : 0.0;
#pragma unroll
    for (int t = 0; t < 7; t++)
      if (full + t < m) res += tl[t];
  }
  return res;
}

template <int RD = kPwRegDepth, class F>
__device__ __forceinline__ double wave_pw_sum(int n, F f, const PwLds &S) {
  static_assert(RD >= 4 && RD <= 6, "register plan depth");
  const int lane = lane_id();
  if (n < 8) {  // pairwise_sum's direct loop, evaluated by every lane alike
    double r = 0.0;
#pragma unroll 1
    for (int i = 0; i < n; i++) r += f(i);
    return r;
  }
  if (n <= 128) return readlane_f64(pw_leaf_group(0, n, f), 0);
  if (n <= pw_reg_cap(RD)) {
    int my_o = 0, my_m = 0, nl = 0;
    pw_enum_r<RD>(0, n, nl, lane, my_o, my_m);
    double myval = 0.0;
    for (int b = 0; b < nl; b += 8) {
      const int l = b + (lane >> 3);
      // both shuffles unconditional: a ds_bpermute under a partial exec mask
      // must not read a source lane that the mask left out
      const int o = __shfl(my_o, l & 63), m_src = __shfl(my_m, l & 63);
      const int m = l < nl ? m_src : 0;
      const double v = pw_leaf_group(o, m, f);
      const double moved = __shfl(v, ((lane - b) & 7) * 8);
      if (lane >= b && lane < b + 8) myval = moved;
    }
    int cnt = 0;
    return pw_comb_r<RD>(n, cnt, myval);
  }
  // deeper recursion (n > pw_reg_cap(RD), P-sized sums of big configs): LDS
  // plan, which also splits n > kNpBufSize into numpy's buffers
  int nl = 1;
  if (lane == 0) S.stk[kPwStackWords - 1] = pw_plan(n, S);
  wsync();
  nl = S.stk[kPwStackWords - 1];
  for (int b = 0; b < nl; b += 8) {
    const int l = b + (lane >> 3);
    const int o = l < nl ? S.lo[l] : 0, m = l < nl ? S.len[l] : 0;
    const double v = pw_leaf_group(o, m, f);
    if (l < nl && (lane & 7) == 0) S.val[l] = v;
  }
  wsync();
  if (lane == 0) S.val[nl] = pw_combine(n, S, nl);
  wsync();
  const double r = S.val[nl];
  wsync();
  return r;
}

}  // namespace vmp

#endif  // VMP_NP_SUM_H
