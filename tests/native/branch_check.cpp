// branch_check — vmp_branch's host part (csrc/vmp_branch.h) on the CPU, under
// ASan + UBSan (make branch-check; tests/test_branch_cpu.py). No library, no
// device.
//  1. branch_check: every single-field difference between two handles gives
//     the documented code (EINVAL; ESTATE for traced against plain), the seed
//     alone does not, null arguments are EINVAL, and the refusal order is
//     shape, config, device, trace;
//  2. the gather geometry over every vm_pitch a handle can have (V 1..10240) and
//     a spread of P: walking the launch as k_branch does (chunks x 4 x 256
//     lanes, units below `units` only) touches every 16-byte unit of the three
//     rows exactly once and nothing outside them, the rows' sizes are those of
//     the snapshot layout (256 B, 16 P B, 4 pitch B), and the header is the
//     first wave's lanes 0..15 at its first unit.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../vm-placement-migration-gym_amd/csrc/vmp_branch.h"
#include "../../vm-placement-migration-gym_amd/csrc/vmp_layout.h"

using namespace vmp;

namespace {

int bad = 0;
void expect(bool ok, const char *what, int line) {
  if (!ok && bad++ < 20) std::printf("line %d: %s\n", line, what);
}
#define EXPECT(c) expect((c), #c, __LINE__)

BranchSide side() {
  BranchSide s;
  std::memset(&s, 0, sizeof(s));
  s.P = 100, s.V = 1000, s.A = 102;
  s.device = 0;
  s.traced = 0;
  s.cfg.arrival_rate = 1.8182;
  s.cfg.service_length = 1000;
  s.cfg.pms = 100, s.cfg.vms = 1000;
  s.cfg.training_steps = 10000, s.cfg.eval_steps = 100000;
  s.cfg.seed = 3;
  s.cfg.reward_function = VMP_REWARD_KL;
  s.cfg.sequence = VMP_SEQ_UNIFORM;
  s.cfg.cap_target_util = 1, s.cfg.allow_null_action = 1;
  s.cfg.beta = 0.5;
  return s;
}

int code(const BranchSide &d, const BranchSide &s) {
  const char *why = nullptr;
  int map = 0;
  const int rc = branch_check(&d, &s, &map, &why);
  EXPECT((rc == VMP_OK) == (why == nullptr));
  return rc;
}

int64_t n_checks = 0, n_units = 0;

void geometry(int32_t P, int32_t V) {
  const int64_t pitch = vm_pitch(V);
  const BranchGeom g = branch_geom(P, pitch);
  EXPECT(pitch % 4 == 0);
  EXPECT(g.pm_units * 16 == 16 * (int64_t)P && g.vm_units * 16 == 4 * pitch);
  EXPECT(g.units == kBranchHdrUnits + g.pm_units + g.vm_units);
  EXPECT(g.chunks >= 1 && (g.chunks - 1) * kBranchChunk < g.units && g.units <= g.chunks * kBranchChunk);
  EXPECT(g.units <= 0x7fffffff);
  std::vector<uint8_t> hit[3] = {std::vector<uint8_t>(kBranchHdrUnits), std::vector<uint8_t>((size_t)g.pm_units),
                                 std::vector<uint8_t>((size_t)g.vm_units)};
  for (int64_t chunk = 0; chunk < g.chunks; chunk++)
    for (int k = 0; k < kBranchPerLane; k++)
      for (int t = 0; t < kBranchThreads; t++) {
        const int64_t u = chunk * kBranchChunk + k * kBranchThreads + t;
        if (u >= g.units) continue;
        int64_t at = -1;
        const int part = branch_part(u, g.pm_units, &at);
        EXPECT(part >= 0 && part <= 2);
        if (part < 0 || part > 2) continue;
        EXPECT(at >= 0 && at < (int64_t)hit[part].size());
        if (at < 0 || at >= (int64_t)hit[part].size()) continue;
        if (part == 0) EXPECT(chunk == 0 && k == 0 && t == at && t < 16);
        hit[part][(size_t)at]++;
        n_units++;
      }
  for (const auto &h : hit)
    for (uint8_t c : h) EXPECT(c == 1);
  n_checks++;
}

}  // namespace

int main() {
  const BranchSide a = side();
  EXPECT(code(a, a) == VMP_OK);
  {
    BranchSide b = a;
    b.cfg.seed = 77;  // the seed alone is no difference
    EXPECT(code(a, b) == VMP_OK && code(b, a) == VMP_OK);
  }
  {
    const char *why = nullptr;
    int map = 0;
    EXPECT(branch_check(nullptr, &a, &map, &why) == VMP_EINVAL && why);
    EXPECT(branch_check(&a, nullptr, &map, &why) == VMP_EINVAL && why);
    EXPECT(branch_check(&a, &a, nullptr, &why) == VMP_EINVAL && why);
  }
  // one field at a time, both directions
  BranchSide v[16];
  for (auto &x : v) x = a;
  int n = 0;
  v[n++].P = 101;
  v[n++].V = 999;
  v[n++].A = 101;
  v[n++].device = 1;
  v[n++].cfg.arrival_rate = 1.8183;
  v[n++].cfg.service_length = 999;
  v[n++].cfg.pms = 101;
  v[n++].cfg.vms = 999;
  v[n++].cfg.training_steps = 10001;
  v[n++].cfg.eval_steps = 100001;
  v[n++].cfg.reward_function = VMP_REWARD_WR;
  v[n++].cfg.sequence = VMP_SEQ_LOWUNIFORM;
  v[n++].cfg.cap_target_util = 0;
  v[n++].cfg.allow_null_action = 0;
  v[n++].cfg.beta = 0.25;
  for (int i = 0; i < n; i++) {
    EXPECT(code(a, v[i]) == VMP_EINVAL);
    EXPECT(code(v[i], a) == VMP_EINVAL);
    EXPECT(code(v[i], v[i]) == VMP_OK);
  }
  {
    BranchSide t = a;
    t.traced = 1;
    EXPECT(code(a, t) == VMP_ESTATE && code(t, a) == VMP_ESTATE && code(t, t) == VMP_OK);
    t.traced = 7;  // any non-zero flag
    BranchSide u = a;
    u.traced = 1;
    EXPECT(code(t, u) == VMP_OK);
    // a shape, config or device difference is reported before the trace
    for (int i = 0; i < n; i++) EXPECT(code(t, v[i]) == VMP_EINVAL);
  }

  for (int32_t V = 1; V <= 10240; V++) geometry(V % 7 == 0 ? 65533 : (V * 37) % 2000 + 1, V);
  for (int32_t P : {1, 2, 15, 16, 17, 100, 1007, 1008, 1009, 4096, 65533})
    for (int32_t V : {1, 30, 64, 65, 300, 1000, 1024, 1025, 1100, 10000, 10240}) geometry(P, V);

  if (bad) {
    std::printf("branch_check FAILED: %d\n", bad);
    return 1;
  }
  std::printf("branch_check ok: %lld geometries, %lld units\n", (long long)n_checks, (long long)n_units);
  return 0;
}
