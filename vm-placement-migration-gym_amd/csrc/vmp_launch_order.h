// vmp_launch_order.h — which env a workgroup of a per-step wave launch takes
// (k_env<VPT, true, *>, k_env_ext, k_env_tr<VPT, true>, k_env_ext_tr; DESIGN.md
// §3.1 "Launch order"). Results do not depend on it: every launch is a
// bijection blocks -> envs, whatever the flag bytes hold.
//
// Direction: the handle counts these launches and every other one walks the
// envs downwards, so the state the previous launch touched last is the state
// this one reads first (Infinity Cache reuse).
//
// Idle envs last (heuristic per-step kernel only): the envs are cut into
// C = ceil(N / 64) chunks, env e being rank e / C of chunk e % C, and the
// dispatch positions likewise, rank-major. Inside a chunk the T ranks
// dispatched last hand their busy envs (flag byte != 0: the header the
// previous launch wrote back does not meet idle_step's header terms) to the T
// ranks dispatched first, in exchange for idle ones. The flags of one chunk
// are one 64-byte line [chunk][rank]; a launch reads the buffer of its own
// parity and writes the other, so what it reads is constant while it runs.
//
// The index arithmetic is __host__ __device__ and shared with the CPU sweep
// (tests/native/launch_order.cpp), which holds it against lo_ref_chunk, the
// rule written out with lists.
#ifndef VMP_LAUNCH_ORDER_H
#define VMP_LAUNCH_ORDER_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VMP_LO_HD __host__ __device__
#else
#define VMP_LO_HD
#endif

namespace vmp {

constexpr int kLoIndex = 0, kLoDirection = 1, kLoIdleLast = 2;
constexpr int kLoChunk = 64;  // ranks per chunk at most: one line of flag bytes
// what a new handle starts with (vmp_debug_launch_order changes the mode)
constexpr int kLoDefaultMode = kLoIdleLast;
constexpr int kLoDefaultDiv = 4;  // T = nr / 4

// The launch word (EnvParams::pad0): bit 0 parity, bits 1-2 mode, bits 8-15 T,
// bits 16-23 nr. 0 is index order.
VMP_LO_HD inline int lo_chunks(int N) { return (N + kLoChunk - 1) / kLoChunk; }
VMP_LO_HD inline int lo_ranks(int N) { return N / lo_chunks(N); }  // full ranks, <= 64
// ranks at each end that take part: nr / div, none below 8 ranks
VMP_LO_HD inline int lo_tail(int N, int div) {
  const int nr = lo_ranks(N);
  return (nr < 8 || div <= 0) ? 0 : nr / div;
}
VMP_LO_HD inline uint32_t lo_word(int mode, int parity, int N, int T) {
  if (mode == kLoIndex) return 0u;
  return (uint32_t)(parity & 1) | ((uint32_t)mode << 1) | ((uint32_t)T << 8) |
         ((uint32_t)lo_ranks(N) << 16);
}
VMP_LO_HD inline int lo_parity(uint32_t w) { return (int)(w & 1u); }
VMP_LO_HD inline int lo_mode(uint32_t w) { return (int)((w >> 1) & 3u); }
VMP_LO_HD inline int lo_T(uint32_t w) { return (int)((w >> 8) & 0xFFu); }
VMP_LO_HD inline int lo_nr(uint32_t w) { return (int)((w >> 16) & 0xFFu); }
// bytes of one flag buffer; the handle keeps two behind its headers
VMP_LO_HD inline int64_t lo_flag_bytes(int N) { return (int64_t)kLoChunk * lo_chunks(N); }

// dispatch position of block b
VMP_LO_HD inline int lo_position(uint32_t w, int N, int b) { return lo_parity(w) ? N - 1 - b : b; }

// rank r of a chunk takes part in the exchange
VMP_LO_HD inline bool lo_in_tail(int r, int T, int nr) { return r < nr && (r < T || r >= nr - T); }
// the rank whose flag lane i < 2T reads: the low end, then the high end, ascending
VMP_LO_HD inline int lo_lane_rank(int i, int T, int nr) { return i < T ? i : nr - 2 * T + i; }

VMP_LO_HD inline int lo_kth_bit(uint32_t m, int k) {  // index of the k-th set bit, k < popcount(m)
  for (; k > 0; k--) m &= m - 1u;
  return __builtin_ctz(m);
}

// The rank whose env rank r (in a tail) runs. busy: bit i = the flag of rank
// lo_lane_rank(i) is non-zero, i < 2T. Late ranks are the T dispatched last:
// the high end of an upward launch (parity 0), the low end of a downward one.
// A = late ranks that are busy, B = early ranks that are not, both ascending;
// the k-th of A and the k-th of B take each other's env, k < min(|A|, |B|).
VMP_LO_HD inline int lo_partner(uint32_t busy, int T, int nr, int parity, int r) {
  const uint32_t ends = (1u << T) - 1u;  // T <= 16
  const uint32_t lo = busy & ends, hi = (busy >> T) & ends;
  const uint32_t A = parity ? lo : hi;
  const uint32_t B = (parity ? ~hi : ~lo) & ends;
  const int base_lo = 0, base_hi = nr - T;
  const bool r_low = r < T;
  const int j = r_low ? r : r - base_hi;
  const bool late = r_low == (parity != 0);
  const uint32_t mine = late ? A : B, other = late ? B : A;
  if (!((mine >> j) & 1u)) return r;
  const int k = __builtin_popcount(mine & ((1u << j) - 1u));
  if (k >= __builtin_popcount(other)) return r;
  return (r_low ? base_hi : base_lo) + lo_kth_bit(other, k);
}

// env of dispatch position q, from the line of chunk q % C (flags: the whole
// buffer the launch reads; null: no exchange). The scalar form of what a
// workgroup evaluates with one byte per lane and a ballot.
VMP_LO_HD inline int lo_env_of_position(uint32_t w, int N, int q, const uint8_t *flags) {
  if (lo_mode(w) != kLoIdleLast || !flags) return q;
  const int C = lo_chunks(N), T = lo_T(w), nr = lo_nr(w);
  const int r = q / C, c = q - r * C;
  if (!lo_in_tail(r, T, nr)) return q;
  uint32_t busy = 0;
  for (int i = 0; i < 2 * T; i++)
    busy |= (uint32_t)(flags[(int64_t)c * kLoChunk + lo_lane_rank(i, T, nr)] != 0) << i;
  return lo_partner(busy, T, nr, lo_parity(w), r) * C + c;
}

// Reference of the exchange in one chunk, with lists: map[r] = the rank whose
// env rank r runs, r < nr (ranks outside the tails map to themselves).
VMP_LO_HD inline void lo_ref_chunk(const uint8_t *line, int T, int nr, int parity, int *map) {
  int A[kLoChunk], B[kLoChunk], na = 0, nb = 0;
  for (int r = 0; r < nr; r++) map[r] = r;
  const int late0 = parity ? 0 : nr - T, early0 = parity ? nr - T : 0;
  for (int i = 0; i < T; i++) {
    if (line[late0 + i] != 0) A[na++] = late0 + i;
    if (line[early0 + i] == 0) B[nb++] = early0 + i;
  }
  for (int k = 0; k < na && k < nb; k++) {
    map[A[k]] = B[k];
    map[B[k]] = A[k];
  }
}

}  // namespace vmp

#endif  // VMP_LAUNCH_ORDER_H
