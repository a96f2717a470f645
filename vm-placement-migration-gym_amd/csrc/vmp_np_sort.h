// vmp_np_sort.h — numpy's scalar argsort (npysort quicksort.cpp: introsort
// with its tie order) for the BestFit visiting order, by one wave. Included by
// vmp_env_common.h and vmp_act_obs.h.
#ifndef VMP_NP_SORT_H
#define VMP_NP_SORT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vmp_dev.h"

namespace vmp {

// ------------------------------------------- numpy scalar argsort (BF) ----
// aquicksort_<float_tag> / aheapsort_ (npysort), run by ONE lane on LDS
// arrays (index form of the pointer algorithm); stack arrays live in LDS.
__device__ __forceinline__ bool fless(float a, float b) { return a < b || (b != b && a == a); }
// Sort keys: an f32 array, or BestFit's fcpu[i] + fmem[i] formed at each read
// (the same f32 sum bestfit.py:31 sorts; no key array in LDS).
struct KeyArr {
  const float LDSP *a;
  __device__ __forceinline__ float operator[](int i) const { return a[i]; }
};
struct KeySum {
  const float LDSP *a, *b;
  __device__ __forceinline__ float operator[](int i) const { return a[i] + b[i]; }
};

template <class KV>
__device__ void aheapsort_lds(KV v, uint16_t LDSP *tosort, int n) {
  uint16_t LDSP *a = tosort - 1;
  int i, j, l;
  uint16_t tmp;
  for (l = n >> 1; l > 0; --l) {
    tmp = a[l];
    for (i = l, j = l << 1; j <= n;) {
      if (j < n && fless(v[a[j]], v[a[j + 1]])) j += 1;
      if (fless(v[tmp], v[a[j]])) {
        a[i] = a[j];
        i = j;
        j += j;
      } else
        break;
    }
    a[i] = tmp;
  }
  for (; n > 1;) {
    tmp = a[n];
    a[n] = a[1];
    n -= 1;
    for (i = 1, j = 2; j <= n;) {
      if (j < n && fless(v[a[j]], v[a[j + 1]])) j++;
      if (fless(v[tmp], v[a[j]])) {
        a[i] = a[j];
        i = j;
        j += j;
      } else
        break;
    }
    a[i] = tmp;
  }
}

// Only the sorted positions lo..hi are needed (BF's tie block): numpy sorts
// every partition independently of the others, so a partition that does not
// intersect [lo, hi] is dropped instead of sorted, and positions lo..hi come
// out exactly as the full sort leaves them (a quickselect-shaped walk:
// ~2n element visits instead of ~n log n).
template <class KV>
__device__ __noinline__ void aquicksort_lds(KV v, uint16_t LDSP *t, int num,
                                            int32_t LDSP *stack, int lo, int hi) {
  int32_t LDSP *depth = stack + 128;
  int pl = 0, pr = num - 1;
  int sp = 0, dp = 0;
  int cdepth = 0;
  for (int u = num; u >>= 1;) cdepth++;
  cdepth *= 2;
  for (;;) {
    if (pr < lo || pl > hi) goto stack_pop;
    if (cdepth < 0) {
      aheapsort_lds(v, t + pl, pr - pl + 1);
      goto stack_pop;
    }
    while ((pr - pl) > 15) {
      int pm = pl + ((pr - pl) >> 1);
      uint16_t x;
      if (fless(v[t[pm]], v[t[pl]])) { x = t[pm]; t[pm] = t[pl]; t[pl] = x; }
      if (fless(v[t[pr]], v[t[pm]])) { x = t[pr]; t[pr] = t[pm]; t[pm] = x; }
      if (fless(v[t[pm]], v[t[pl]])) { x = t[pm]; t[pm] = t[pl]; t[pl] = x; }
      float vp = v[t[pm]];
      int pi = pl, pj = pr - 1;
      x = t[pm]; t[pm] = t[pj]; t[pj] = x;
      for (;;) {
        do ++pi; while (fless(v[t[pi]], vp));
        do --pj; while (fless(vp, v[t[pj]]));
        if (pi >= pj) break;
        x = t[pi]; t[pi] = t[pj]; t[pj] = x;
      }
      int pk = pr - 1;
      x = t[pi]; t[pi] = t[pk]; t[pk] = x;
      if (pi - pl < pr - pi) {
        stack[sp++] = pi + 1;
        stack[sp++] = pr;
        pr = pi - 1;
      } else {
        stack[sp++] = pl;
        stack[sp++] = pi - 1;
        pl = pi + 1;
      }
      depth[dp++] = --cdepth;
      if (pr < lo || pl > hi) goto stack_pop;
    }
    for (int pi = pl + 1; pi <= pr; ++pi) {
      uint16_t vi = t[pi];
      float vp = v[vi];
      int pj = pi, pk = pi - 1;
      while (pj > pl && fless(vp, v[t[pk]])) t[pj--] = t[pk--];
      t[pj] = vi;
    }
  stack_pop:
    if (sp == 0) break;
    pr = stack[--sp];
    pl = stack[--sp];
    cdepth = depth[--dp];
  }
}

// Wave-parallel form of the same sort (all 64 lanes, uniform control flow),
// identical result. numpy's partition loop
//   do ++pi while v[pi] < vp;  do --pj while vp < v[pj];  if (pi >= pj) break;  swap
// pairs the k-th left stop A[k] (ascending positions in (pl, pr-1] with
// v >= vp; pr-1 holds the pivot) with the k-th right stop B[k] (descending
// positions in [pl, pr-2] with v <= vp; pl holds a value <= vp) while
// A[k] < B[k]: up to that point each scan only crosses unmodified positions,
// so both lists follow from the values before the loop. With K = #{k : A[k] <
// B[k]} (a prefix, A rising and B falling), the K swaps are disjoint, and the
// final left stop is min(A[K], B[K-1]) (B[K-1] holds a swapped-in value >= vp).
// Stops are ranked with ballots; the lists live in `scr` (u16, 2 x n). Small
// partitions (<= 16) get numpy's insertion sort as a stable rank sort; the
// depth-limit heapsort stays on lane 0.
//
// One partition step of numpy's loop on [pl, pr] (pr - pl > 15): median of
// three, the stops, the swaps and the pivot's final move; returns its
// position pi ([pl, pi - 1] <= pivot <= [pi + 1, pr]).
template <class KV>
__device__ __forceinline__ int wave_partition(KV v, uint16_t LDSP *t, int pl, int pr,
                                              uint16_t LDSP *scr) {
  const int lane = threadIdx.x & 63;
  const uint64_t lt = (1ull << lane) - 1ull;
  const int pm = pl + ((pr - pl) >> 1);
  uint16_t tl = t[pl], tm = t[pm], tr = t[pr], x;
  if (fless(v[tm], v[tl])) { x = tm; tm = tl; tl = x; }
  if (fless(v[tr], v[tm])) { x = tr; tr = tm; tm = x; }
  if (fless(v[tm], v[tl])) { x = tm; tm = tl; tl = x; }
  const float vp = v[tm];
  const uint16_t tq = t[pr - 1];
  wsync();
  if (lane == 0) {
    t[pl] = tl;
    t[pm] = tq;
    t[pr] = tr;
    t[pr - 1] = tm;
  }
  wsync();
  // A (ascending stops in [pl+1, pr-1]) and B (stops in [pl, pr-2], kept
  // ascending in bas: B[k] = bas[nb-1-k]) from ONE pass over [pl, pr-1]
  // reading each key once, two 64-position batches per round trip
  uint16_t LDSP *apos = scr;
  uint16_t LDSP *bas = scr + (pr - pl + 1);
  int na = 0, nb = 0;
  for (int c = pl; c <= pr - 1; c += 128) {
    const int q0 = c + lane, q1 = c + 64 + lane;
    const bool in0 = q0 <= pr - 1, in1 = q1 <= pr - 1;
    const int i0 = t[in0 ? q0 : pl], i1 = t[in1 ? q1 : pl];
    const float x0 = v[i0], x1 = v[i1];
    const bool fa0 = in0 && q0 >= pl + 1 && !fless(x0, vp), fb0 = in0 && q0 <= pr - 2 && !fless(vp, x0);
    const bool fa1 = in1 && q1 >= pl + 1 && !fless(x1, vp), fb1 = in1 && q1 <= pr - 2 && !fless(vp, x1);
    const uint64_t ma0 = ballot(fa0), mb0 = ballot(fb0), ma1 = ballot(fa1), mb1 = ballot(fb1);
    if (fa0) apos[na + __popcll(ma0 & lt)] = (uint16_t)q0;
    if (fb0) bas[nb + __popcll(mb0 & lt)] = (uint16_t)q0;
    na += __popcll(ma0);
    nb += __popcll(mb0);
    if (fa1) apos[na + __popcll(ma1 & lt)] = (uint16_t)q1;
    if (fb1) bas[nb + __popcll(mb1 & lt)] = (uint16_t)q1;
    na += __popcll(ma1);
    nb += __popcll(mb1);
  }
  wsync();
  int kk = 0;  // K: A[k] < B[k] holds for a prefix of k
  for (int c = 0; c < na && c < nb; c += 64) {
    const int k = c + lane;
    const bool sw = k < na && k < nb && (int)apos[k] < (int)bas[nb - 1 - k];
    kk += __popcll(ballot(sw));
  }
  for (int c = 0; c < kk; c += 64) {
    const int k = c + lane;
    uint16_t xa = 0, xb = 0;
    int qa = 0, qb = 0;
    if (k < kk) {
      qa = apos[k];
      qb = bas[nb - 1 - k];
      xa = t[qa];
      xb = t[qb];
    }
    wsync();
    if (k < kk) {
      t[qa] = xb;
      t[qb] = xa;
    }
    wsync();
  }
  int pi = apos[kk];
  if (kk > 0 && (int)bas[nb - kk] < pi) pi = bas[nb - kk];
  wsync();
  if (lane == 0) {
    x = t[pi];
    t[pi] = t[pr - 1];
    t[pr - 1] = x;
  }
  wsync();
  return pi;
}

// numpy's insertion sort of [pl, pr] (<= 16 elements) = a stable rank sort.
template <class KV>
__device__ __forceinline__ void wave_leaf_sort(KV v, uint16_t LDSP *t, int pl, int pr) {
  const int lane = threadIdx.x & 63;
  const int n = pr - pl + 1;
  uint16_t me = 0;
  float vm = 0.f;
  if (lane < n) {
    me = t[pl + lane];
    vm = v[me];
  }
  int rank = 0;
  for (int j = 0; j < n; j++) {
    const float vj = __shfl(vm, j);
    rank += (fless(vj, vm) || (j < lane && !fless(vm, vj))) ? 1 : 0;
  }
  wsync();
  if (lane < n) t[pl + rank] = me;
  wsync();
}

template <class KV>
__device__ __noinline__ void wave_aquicksort(KV v, uint16_t LDSP *t, int num,
                                             int32_t LDSP *stack, int lo, int hi,
                                             uint16_t LDSP *scr) {
  const int lane = threadIdx.x & 63;
  int32_t LDSP *depth = stack + 128;
  int pl = 0, pr = num - 1;
  int sp = 0, dp = 0;
  int cdepth = 0;
  for (int u = num; u >>= 1;) cdepth++;
  cdepth *= 2;
  for (;;) {
    if (pr < lo || pl > hi) goto stack_pop;
    if (cdepth < 0) {
      if (lane == 0) aheapsort_lds(v, t + pl, pr - pl + 1);
      wsync();
      goto stack_pop;
    }
    while ((pr - pl) > 15) {
      const int pi = wave_partition(v, t, pl, pr, scr);
      if (pi - pl < pr - pi) {
        if (lane == 0) {
          stack[sp] = pi + 1;
          stack[sp + 1] = pr;
        }
        sp += 2;
        pr = pi - 1;
      } else {
        if (lane == 0) {
          stack[sp] = pl;
          stack[sp + 1] = pi - 1;
        }
        sp += 2;
        pl = pi + 1;
      }
      --cdepth;
      if (lane == 0) depth[dp] = cdepth;
      dp++;
      wsync();
      if (pr < lo || pl > hi) goto stack_pop;
    }
    wave_leaf_sort(v, t, pl, pr);
  stack_pop:
    if (sp == 0) break;
    wsync();
    sp -= 2;
    pl = stack[sp];
    pr = stack[sp + 1];
    cdepth = depth[--dp];
  }
  wsync();
}

// BestFit's tie block needs only the HIGHEST position in [lo, hi] whose PM
// fits (the first in visiting order). The walk processes the same partitions
// as wave_aquicksort(lo, hi), each with the same depth, so every position in
// [lo, hi] settles to numpy's element; partitions of disjoint ranges do not
// interact, so the order they are processed in is free. Here the upper part
// is always processed first and the lower part waits on the stack (a reverse
// in-order walk: positions settle in descending order, a partition's pivot
// after its upper part, checked when the lower part is popped), and the walk
// stops at the first settled position that fits. A tie block of e PMs whose
// highest member fits costs one root-to-leaf path (~2n element visits)
// instead of sorting the block (~e log e more partitions). The stack holds
// the pending lower parts of one path: at most 2 log2(n) + 1 entries (the
// depth limit ends a path in heapsort). Returns the position, or -1.
//
// The depth limit: numpy tests cdepth < 0 only on a part it pops, i.e. the
// LARGER part of its partition; the smaller part, which it goes on with, is
// partitioned whatever its depth. Which part this walk goes on with is not
// numpy's choice, so every part carries that bit (`cont`: numpy goes on with
// it, no depth test; bit 0 of its depth entry while it waits), and a part is
// heapsorted exactly where numpy heapsorts it.
template <class KV, class Fit>
__device__ __noinline__ int wave_aqselect_top(KV v, uint16_t LDSP *t, int num,
                                              int32_t LDSP *stack, int lo, int hi,
                                              uint16_t LDSP *scr, Fit fit) {
  const int lane = threadIdx.x & 63;
  int32_t LDSP *depth = stack + 128;
  int pl = 0, pr = num - 1;
  int sp = 0, dp = 0;
  int cdepth = 0;
  for (int u = num; u >>= 1;) cdepth++;
  cdepth *= 2;
  // highest fitting position of the settled range [a, b] within [lo, hi]
  auto scan = [&](int a, int b) -> int {
    const int a0 = a > lo ? a : lo;
    for (int c = b < hi ? b : hi; c >= a0; c -= 64) {
      const int pos = c - lane;
      const uint64_t f = ballot(pos >= a0 && fit((int)t[pos >= a0 ? pos : a0]));
      if (f) return c - (__ffsll((unsigned long long)f) - 1);
    }
    return -1;
  };
  int found = -1;
  bool cont = false;
  for (;;) {
    if (pr < lo || pl > hi) goto stack_pop;
    if (cdepth < 0 && !cont) {
      if (lane == 0) aheapsort_lds(v, t + pl, pr - pl + 1);
      wsync();
      found = scan(pl, pr);
      if (found >= 0) break;
      goto stack_pop;
    }
    while ((pr - pl) > 15) {
      const int pi = wave_partition(v, t, pl, pr, scr);
      const bool lower_small = pi - pl < pr - pi;  // numpy goes on with the lower part
      --cdepth;
      if (lane == 0) {  // the lower part waits; the upper part goes on
        stack[sp] = pl;
        stack[sp + 1] = pi - 1;
        depth[dp] = cdepth * 2 + (lower_small ? 1 : 0);
      }
      sp += 2;
      dp++;
      pl = pi + 1;
      cont = !lower_small;
      wsync();
      if (pr < lo || pl > hi) goto stack_pop;
      if (!cont && cdepth < 0) break;  // numpy pops this part: heapsort
    }
    if (!cont && cdepth < 0) continue;  // of any size, as numpy's test after a pop
    wave_leaf_sort(v, t, pl, pr);
    found = scan(pl, pr);
    if (found >= 0) break;
  stack_pop:
    if (sp == 0) break;
    wsync();
    sp -= 2;
    pl = stack[sp];
    pr = stack[sp + 1];
    {
      const int d = depth[--dp];
      cdepth = d >> 1;
      cont = (d & 1) != 0;
    }
    // the popped range is the lower part of a partition whose pivot sits at
    // pr + 1, settled, and every position above it has been checked
    if (pr + 1 >= lo && pr + 1 <= hi && fit((int)t[pr + 1])) {
      found = pr + 1;
      break;
    }
  }
  wsync();
  return found;
}

}  // namespace vmp

#endif  // VMP_NP_SORT_H
