// hg16_plan — the launch plan of the bf16 fused actor head
// (csrc/vmp_hg16_plan.h) on the CPU, under ASan + UBSan (make hg16-plan;
// tests/test_hg16_cases_cpu.py). No library, no device.
// Sweep: B = 1..20, the 256-borders (256 k - 1, 256 k, 256 k + 1) up to 20 000
// and a few sizes between, V = 1..600, every A = 1..128. A grid depends on B
// through m_blocks and on A through S only, so each distinct (m_blocks, V, S)
// is walked once and every other plan is compared with the walked one. For
// every plan, with block -> (column tile, first M block) as hg16_tile of
// csrc/vmp_headgemm_bf16.hip maps it (restated below) and the kernel's walk
// mb = g, g + m_groups, ... < m_blocks:
//  1. every (column tile, M block) pair is owned by exactly one (workgroup,
//     walk step);
//  2. padding blocks own nothing, and every other block owns at least one pair;
//  3. every first M block g is below min(m_groups, m_blocks), the number of
//     partial rows k_dsum reduces, and that many rows of V A floats fit in
//     hg16_bwd_workspace;
//  4. the grid is at least 1 and fits in 32 bits (dim3 takes unsigned).
// `hg16_plan print B V A ...` prints the plans of the given shapes, one line
// each, for the Python restatement (tests/hg16_cases.py plan()).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../vm-placement-migration-gym_amd/csrc/vmp_hg16_plan.h"

using namespace vmp;

namespace {

int bad = 0;
long checked = 0, walks = 0;
void expect(bool ok, const char *what, int line, int B, int V, int A) {
  if (!ok && bad++ < 20) std::printf("line %d: %s (B %d, V %d, A %d)\n", line, what, B, V, A);
}
#define EXPECT(c) expect((c), #c, __LINE__, B, V, A)

// hg16_tile: the workgroup's column tile and first M block; false: nothing to do
bool tile_of(const Hg16Plan &p, int64_t b, int &n_tile, int &g) {
  if (p.team > 0) {
    const int64_t i = b >> 3;
    const int64_t T = (i / p.team) * 8 + (b & 7);
    if (T >= p.teams) return false;
    n_tile = (int)(T % p.n_tiles);
    g = (int)(T / p.n_tiles) * p.team + (int)(i % p.team);
  } else {
    n_tile = (int)(b % p.n_tiles);
    g = (int)(b / p.n_tiles);
  }
  return g < p.m_blocks;
}

int64_t padding_blocks(const Hg16Plan &p) {
  int64_t n = 0;
  int t, g;
  for (int64_t b = 0; b < p.grid; b++) n += !tile_of(p, b, t, g);
  return n;
}

bool same_grid(const Hg16Plan &a, const Hg16Plan &b) {
  return a.n_tiles == b.n_tiles && a.m_blocks == b.m_blocks && a.team == b.team &&
         (a.team == 0 || a.teams == b.teams) && a.m_groups == b.m_groups && a.grid == b.grid;
}

// walked[(m_blocks, V, S)]: the plan whose ownership (1., 2.) has been walked;
// a plan with the same grid fields owns the same pairs and is not walked again
// (B enters through m_blocks and A through S only, which the comparison checks)
std::vector<Hg16Plan> walked;
constexpr int kMaxMB = 80, kMaxV = 600;
int s_index(int S) { return S == 14 ? 0 : S == 7 ? 1 : S == 4 ? 2 : S == 3 ? 3 : S == 2 ? 4 : 5; }

void check(int B, int V, int A, std::vector<int> &owner) {
  const Hg16Plan p = hg16_plan(B, V, A);
  EXPECT(p.TS == (A + 15) / 16 && p.TS >= 1 && p.TS <= 8 && p.S == 14 / p.TS);
  EXPECT(p.n_tiles >= 1 && (int64_t)p.n_tiles * p.S >= V && (int64_t)(p.n_tiles - 1) * p.S < V);
  EXPECT(p.m_blocks >= 1 && (int64_t)p.m_blocks * kHg16BM >= B && (int64_t)(p.m_blocks - 1) * kHg16BM < B);
  EXPECT(p.m_groups >= 1 && p.m_groups <= p.m_blocks);
  EXPECT((p.team == 0) == (p.m_blocks < kHg16Team));
  if (p.team > 0) EXPECT(p.team == kHg16Team && p.teams % p.n_tiles == 0 && p.m_groups == p.team * (p.teams / p.n_tiles));
  EXPECT(p.grid >= 1 && p.grid <= (int64_t)UINT32_MAX);                               // 4.
  const int64_t G = p.m_groups < p.m_blocks ? p.m_groups : p.m_blocks;
  EXPECT(G * (int64_t)V * A <= hg16_bwd_workspace(B, V, A));                          // 3.
  checked++;
  EXPECT(p.m_blocks < kMaxMB && V <= kMaxV);
  if (p.m_blocks >= kMaxMB || V > kMaxV) return;
  Hg16Plan &w = walked[((size_t)p.m_blocks * (kMaxV + 1) + V) * 6 + s_index(p.S)];
  if (w.grid != 0) {
    EXPECT(same_grid(w, p));
    return;
  }
  w = p;
  walks++;
  owner.assign((size_t)p.n_tiles * p.m_blocks, 0);
  for (int64_t b = 0; b < p.grid; b++) {
    int t = -1, g = -1;
    if (!tile_of(p, b, t, g)) continue;                                               // 2.
    EXPECT(t >= 0 && t < p.n_tiles && g >= 0 && g < G);                               // 3.
    int steps = 0;
    for (int mb = g; mb < p.m_blocks; mb += p.m_groups, steps++) owner[(size_t)t * p.m_blocks + mb]++;
    EXPECT(steps >= 1);                                                               // 2.
  }
  bool once = true;
  for (int n : owner) once = once && n == 1;
  EXPECT(once);                                                                       // 1.
}

void print_plan(int B, int V, int A) {
  const Hg16Plan p = hg16_plan(B, V, A);
  std::printf("plan B %d V %d A %d TS %d S %d n_tiles %d m_blocks %d team %d teams %d m_groups %d "
              "padding %lld grid %lld workspace %lld\n",
              B, V, A, p.TS, p.S, p.n_tiles, p.m_blocks, p.team, p.team > 0 ? p.teams : 0, p.m_groups,
              (long long)padding_blocks(p), (long long)p.grid, (long long)hg16_bwd_workspace(B, V, A));
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1 && argv[1][0] == 'p') {
    for (int i = 2; i + 2 < argc; i += 3) print_plan(std::atoi(argv[i]), std::atoi(argv[i + 1]), std::atoi(argv[i + 2]));
    return 0;
  }
  std::vector<int> Bs, As;
  for (int B = 1; B <= 20; B++) Bs.push_back(B);
  for (int k = 1; 256 * k <= 20000; k++)
    for (int d = -1; d <= 1; d++) Bs.push_back(256 * k + d);
  for (int B : {100, 135, 1000, 3000, 10000, 19999, 20000}) Bs.push_back(B);
  for (int A = 1; A <= 128; A++) As.push_back(A);
  walked.assign((size_t)kMaxMB * (kMaxV + 1) * 6, Hg16Plan{});
  std::vector<int> owner;
  for (int B : Bs)
    for (int V = 1; V <= kMaxV; V++)
      for (int A : As) check(B, V, A, owner);
  if (bad) {
    std::printf("hg16_plan: %d failures\n", bad);
    return 1;
  }
  std::printf("hg16_plan ok: %ld plans (%zu B x %d V x %zu A), %ld grids walked\n", checked, Bs.size(), kMaxV,
              As.size(), walks);
  return 0;
}
