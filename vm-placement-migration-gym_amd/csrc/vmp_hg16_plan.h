// vmp_hg16_plan.h — the launch plan of the bf16 fused actor head
// (csrc/vmp_headgemm_bf16.hip, k_hg16<TS, BWD, 8, SMP>): which segment width,
// how many column tiles and M blocks, which of the two grid plans (M groups or
// XCD teams), how many workgroups, and how many floats of bias-gradient
// partials the backward may write. Host only, plain C++ with no HIP types, so
// the CPU sweep tests/native/hg16_plan.cpp (make hg16-plan) runs the very code
// launch_hg16 runs; tests/hg16_cases.py restates it in Python.
//
// A workgroup owns one column tile (S = 14 / TS whole action segments of TS
// 16-column tiles) and walks the M blocks g, g + m_groups, ... of 256 samples.
//   M groups (team 0):  grid = n_tiles x m_groups, block b -> tile b % n_tiles,
//                       g = b / n_tiles.
//   XCD teams (team 8, from 8 M blocks on): blocks b and b + 8 share an XCD;
//                       the grid is padded to whole teams on every XCD, and a
//                       block whose team index is >= teams does nothing
//                       (hg16_tile in the .hip file).
#ifndef VMP_HG16_PLAN_H
#define VMP_HG16_PLAN_H

#include <stdint.h>

namespace vmp {

constexpr int kHg16BM = 256;    // samples per M block
constexpr int kHg16MaxNT = 14;  // 16-column accumulator tiles per workgroup
constexpr int kHg16Team = 8;    // XCD team size

struct Hg16Plan {
  int TS, S;              // tiles per segment, segments per column tile
  int n_tiles, m_blocks;  // column tiles, M blocks of kHg16BM samples
  int team, teams;        // team 0: the M-group plan
  int m_groups;           // a workgroup walks M blocks g, g + m_groups, ...
  int64_t grid;           // workgroups launched (padding blocks included)
};

inline int hg16_pick_ts(int A) { return (A + 15) / 16; }  // segment width: 16 TS columns, TS = ceil(A / 16)

// M groups: the grid is n_tiles x m_groups workgroups at one per CU; pick the
// group count whose last dispatch round is fullest (ties: fewer workgroups)
inline int hg16_pick_groups(int n_tiles, int m_blocks) {
  int best = 1;
  double best_eff = -1.0;
  for (int g = 1; g <= m_blocks && g <= 64; g++) {
    const int64_t wg = (int64_t)n_tiles * g;
    const double rounds = (double)((wg + 255) / 256);
    const double eff = (double)wg / (rounds * 256.0);
    if (eff > best_eff + 1e-9) {
      best_eff = eff;
      best = g;
    }
    if (eff > 0.97) break;
  }
  return best;
}

inline int64_t hg16_grid(int team, int teams, int n_tiles, int m_groups) {
  return team > 0 ? (int64_t)(teams + 7) / 8 * 8 * team : (int64_t)n_tiles * m_groups;
}

inline Hg16Plan hg16_plan(int B, int V, int A) {
  Hg16Plan p{};
  p.TS = hg16_pick_ts(A);
  p.S = kHg16MaxNT / p.TS;
  p.n_tiles = (V + p.S - 1) / p.S;
  p.m_blocks = (B + kHg16BM - 1) / kHg16BM;
  const int team = kHg16Team;
  p.team = 0;
  if (team > 0 && p.m_blocks >= team) {
    // r walks per team member: the grid n_tiles x team x r (rounded to whole
    // teams per XCD) whose last round of 256 one-per-CU workgroups is fullest
    int best = 1;
    double best_eff = -1.0;
    for (int r = 1; r * team <= p.m_blocks && r <= 64; r++) {
      const int64_t teams = (int64_t)p.n_tiles * r;
      const int64_t wg = (teams + 7) / 8 * 8 * team;
      const double eff = (double)(teams * team) / ((double)((wg + 255) / 256) * 256.0);
      if (eff > best_eff + 1e-9) {
        best_eff = eff;
        best = r;
      }
      if (eff > 0.97) break;
    }
    p.team = team;
    p.teams = p.n_tiles * best;
    p.m_groups = team * best;
  } else {
    p.m_groups = hg16_pick_groups(p.n_tiles, p.m_blocks);
  }
  p.grid = hg16_grid(p.team, p.teams, p.n_tiles, p.m_groups);
  return p;
}

// floats of bias-gradient partials vmp_actor_head_bf16_bwd may use: V*A per M
// group, at most 64 groups x 8 (XCD teams) of 256-sample blocks
inline int64_t hg16_bwd_workspace(int B, int V, int A) {
  const int64_t blocks = ((int64_t)B + kHg16BM - 1) / kHg16BM;
  const int64_t groups = blocks < 512 ? blocks : 512;
  return (groups < 1 ? 1 : groups) * (int64_t)V * A;
}

}  // namespace vmp

#endif
