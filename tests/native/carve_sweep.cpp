// carve_sweep.cpp — CPU check of csrc/vmp_carve.h, the per-env LDS carve of the
// step kernels. No device, no library; built with ASan + UBSan by the package
// Makefile's `carve-sweep` target and run by tests/test_carve_cpu.py.
//
//   carve_sweep <tests/golden/carve_fields.csv>   check against the fixture
//   carve_sweep --emit                            print a fixture from this header
//
// (a) invariants of every config of the grid that fits: alignment, bounds,
//     disjoint regions per phase; (b) the carve fields of the fixture's configs
//     and a hash of the fields over the whole grid equal the fixture's, which
//     was emitted from the carve()/carve_big() of vmp_capi.cpp before this
//     header replaced them; (c) the launch, fit-check and occupancy sizes
//     agree; (d) the refused configs are those of that vmp_create (its
//     formulas restated below in literals; counted and hashed in the fixture).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../vm-placement-migration-gym_amd/csrc/vmp_carve.h"

using namespace vmp;

namespace {

struct Cfg {
  int P, V;
  bool big;  // k_env_big: V > 1024, or forced (VMP_BIG_KERNEL=1)
};

struct Field {
  const char *name;
  int32_t EnvParams::*m;
};
#define F(x) {#x, &EnvParams::x}
const Field kFields[] = {F(NW),        F(n_leaf),      F(off_hdr),  F(off_pm),   F(off_fpm),
                         F(off_thr),   F(off_ord),     F(off_bits), F(off_sort), F(off_ccomp),
                         F(off_leaf),  F(off_leafval), F(off_stage), F(off_pre), F(off_pdirty),
                         F(off_acc),   F(acc_cap),     F(ccomp_cap), F(off_ev),  F(fmem_off),
                         F(tm_off),    F(lds_wave_bytes)};
#undef F

EnvParams carved(const Cfg &c) {
  EnvParams p;
  std::memset(&p, 0, sizeof(p));
  p.P = c.P;
  p.V = c.V;
  if (c.big) carve_big(c.P, c.V, p);
  else carve_wave(c.P, c.V, p);
  return p;
}

// The grid of the sweep, in hash order.
template <class Fn>
void for_grid(Fn fn) {
  for (int P = 1; P <= 9000; P = P < 300 ? P + 1 : P + 97) {
    for (int V = 1; V <= 1024; V = V < 140 ? V + 1 : V + 61) {
      fn(Cfg{P, V, false});
      fn(Cfg{P, V, true});
    }
    for (int V = 1025; V <= 10240; V += 307) fn(Cfg{P, V, true});
    fn(Cfg{P, 1024, false});
    fn(Cfg{P, 10240, true});
  }
}

struct GridSum {
  long configs = 0, fit = 0;
  uint64_t hash = 1469598103934665603ull;  // FNV-1a over the fields and the fit flag
  void add(const EnvParams &p, bool fits) {
    configs++;
    fit += fits;
    auto byte = [&](uint8_t b) { hash = (hash ^ b) * 1099511628211ull; };
    for (const Field &f : kFields) {
      const uint32_t v = (uint32_t)(p.*f.m);
      for (int i = 0; i < 4; i++) byte((uint8_t)(v >> (8 * i)));
    }
    byte(fits);
  }
};

// The configs of the field table: the shipped and headline configs, both sides
// of every threshold of the carve (V 64 / 1024: wave rows and kernel choice;
// 1928: LDS pairwise plan; V 1024 / 2048 / 4096: slots per thread), forced-big
// small V, and the largest P that fits with the one above it.
template <class Fits>
std::vector<Cfg> table_configs(Fits fits) {
  std::vector<Cfg> c = {
      {10, 10, false},     {100, 1000, false},  {1000, 10000, true}, {100, 64, false},
      {100, 65, false},    {100, 1024, false},  {100, 1025, true},   {1928, 100, false},
      {1929, 100, false},  {100, 1928, true},   {100, 1929, true},   {1928, 1928, true},
      {1929, 1929, true},  {10, 10, true},      {100, 300, true},    {100, 1000, true},
      {1, 1, false},       {1, 1, true},        {64, 64, false},     {65, 128, false},
      {128, 129, false},   {300, 300, false},   {1000, 1024, false}, {1000, 1024, true},
      {1000, 1025, true},  {2000, 500, false},  {2000, 500, true},   {5000, 5000, true},
      {100, 10240, true},  {1, 10240, true},    {3000, 1024, false}, {4000, 10240, true},
      {100, 2048, true},   {100, 2049, true},   {100, 4096, true},   {100, 4097, true}};
  const Cfg at[] = {{0, 1, false}, {0, 1024, false}, {0, 1, true}, {0, 10240, true}};
  for (Cfg a : at) {
    int P = 1;
    while (a.P = P + 1, fits(a)) P++;
    c.push_back(Cfg{P, a.V, a.big});
    c.push_back(Cfg{P + 1, a.V, a.big});
  }
  return c;
}

template <class Carve, class Fits>
void emit(FILE *out, Carve carve, Fits fits) {
  std::fprintf(out, "P,V,big");
  for (const Field &f : kFields) std::fprintf(out, ",%s", f.name);
  std::fprintf(out, ",fits\n");
  for (const Cfg &c : table_configs(fits)) {
    const EnvParams p = carve(c);
    std::fprintf(out, "%d,%d,%d", c.P, c.V, (int)c.big);
    for (const Field &f : kFields) std::fprintf(out, ",%d", (int)(p.*f.m));
    std::fprintf(out, ",%d\n", (int)fits(c));
  }
  GridSum g;
  for_grid([&](const Cfg &c) { g.add(carve(c), fits(c)); });
  std::fprintf(out, "grid,%ld,%ld,%016llx\n", g.configs, g.fit, (unsigned long long)g.hash);
}

int bad = 0;
void violation(const Cfg &c, const std::string &what) {
  if (bad++ < 20) std::printf("P%d V%d big%d: %s\n", c.P, c.V, (int)c.big, what.c_str());
}

struct Region {
  const char *name;
  int64_t lo, size;
};
void check_set(const Cfg &c, const EnvParams &p, const char *set, const std::vector<Region> &rs) {
  for (const Region &r : rs)
    if (r.lo < 0 || r.lo + r.size > p.off_pre)
      violation(c, std::string(set) + ": " + r.name + " ends beyond off_pre");
  for (size_t i = 0; i < rs.size(); i++)
    for (size_t j = i + 1; j < rs.size(); j++)
      if (rs[i].size && rs[j].size && rs[i].lo < rs[j].lo + rs[j].size &&
          rs[j].lo < rs[i].lo + rs[i].size)
        violation(c, std::string(set) + ": " + rs[i].name + " overlaps " + rs[j].name);
}

// (a)
void check_invariants(const Cfg &c, const EnvParams &p) {
  const int64_t P = c.P, V = c.V;
  const bool deep = p.n_leaf > 1;
  // every offset is 16-byte aligned; but the wave carve's accepted sizes, a
  // byte array, directly follow the u16 NULL list of V entries
  for (const Field &f : kFields) {
    if (std::strncmp(f.name, "off_", 4) != 0) continue;
    const int al = !c.big && f.m == &EnvParams::off_acc ? 2 : 16;
    if ((p.*f.m) % al) violation(c, std::string(f.name) + " misaligned");
  }
  const std::vector<Region> live = {{"hdr", p.off_hdr, (int64_t)sizeof(EnvHdr)},
                                    {"pm", p.off_pm, 16 * P},
                                    {"stage", p.off_stage, kStageBytes},
                                    {"pdirty", p.off_pdirty, pdirty_bytes(P)}};
  const Region leaf = {"leaf", p.off_leaf, deep ? pw_plan_bytes(p.n_leaf) : 0};
  const Region leafval = {"leafval", p.off_leafval, deep ? pw_val_bytes(p.n_leaf) : 0};
  std::vector<Region> act = live, tail = live;
  act.push_back({"fcpu", p.off_fpm, 4 * P});
  act.push_back({"fmem", p.off_fpm + 4 * (int64_t)p.fmem_off, 4 * P});
  act.push_back({"tc", p.off_thr, P});
  act.push_back({"tm", p.off_thr + (int64_t)p.tm_off, P});
  act.push_back({"ord", p.off_ord, 2 * P});
  act.push_back({"sort", p.off_sort, sort_bytes(P)});
  if (!c.big) {
    act.push_back({"anyfit", p.off_bits, kAnyFitBytes});
    act.push_back(leaf);
    act.push_back(leafval);
  }
  tail.push_back({"acc", p.off_acc, 2 * (int64_t)p.acc_cap});
  tail.push_back({"ccomp", p.off_ccomp, 2 * (int64_t)p.ccomp_cap});
  tail.push_back(leaf);
  tail.push_back(leafval);
  if (c.big) tail.push_back({"ev", p.off_ev, (int64_t)kEvCap * kEvBytes});
  else tail.push_back({"nulls", p.off_bits, 2 * V});
  check_set(c, p, "action", act);
  check_set(c, p, "tail", tail);
}

// (c), (d): vmp_create's, launch_env's and vmp_debug_occupancy's sizes as they
// stood before vmp_carve.h, in literals
int old_spt(int V) { return V <= 1024 ? 4 : V <= 2048 ? 8 : V <= 4096 ? 16 : 40; }
void check_sizes(const Cfg &c, const EnvParams &p, bool fits) {
  const int spt = old_spt(c.V);
  const int64_t per_env = (int64_t)p.off_pre + 20 * 64 + 4 * 256;
  const int64_t need = c.big ? per_env + 4720 + 4 * (int64_t)spt * 256 : per_env + 2048;
  if (fits != (need <= 160 * 1024)) violation(c, "fit differs from vmp_create's need > 160 KB");
  if (big_spt(c.V) != spt) violation(c, "slots per thread");
  const size_t at_max = launch_lds(p, kMaxStepsPerLaunch, c.big, spt);
  if ((int64_t)at_max + (c.big ? 4720 : 2048) > need) violation(c, "launch larger than the fit check assumed");
  for (int k : {0, 1, 2, 17, kMaxStepsPerLaunch - 1})
    if (launch_lds(p, k, c.big, spt) > at_max) violation(c, "launch grows beyond k = kMaxStepsPerLaunch");
  const int64_t wave1 = (p.off_pre + 20 * 64 + 4 + 15) & ~(int64_t)15;
  if (launch_wave_bytes(p, 1) != wave1) violation(c, "one-step region");
  if (c.big && (int64_t)launch_lds(p, 1, true, spt) != wave1 + 4 * (int64_t)spt * 256)
    violation(c, "occupancy query's size differs from the one-step launch");
  // launch_env's own limit refuses nothing that vmp_create accepted
  if (fits && !lds_fits(at_max, c.big)) violation(c, "launch_env refuses a created config");
}

int check(const char *path) {
  FILE *f = std::fopen(path, "r");
  if (!f) {
    std::printf("cannot open %s\n", path);
    return 2;
  }
  char line[1024];
  int rows = 0;
  long g_configs = -1, g_fit = -1;
  unsigned long long g_hash = 0;
  while (std::fgets(line, sizeof(line), f)) {
    if (line[0] == 'P' || line[0] == '#' || line[0] == '\n') continue;
    if (std::sscanf(line, "grid,%ld,%ld,%llx", &g_configs, &g_fit, &g_hash) == 3) continue;
    std::vector<long> v;
    for (char *s = std::strtok(line, ",\n"); s; s = std::strtok(nullptr, ",\n")) v.push_back(std::atol(s));
    const size_t nf = sizeof(kFields) / sizeof(kFields[0]);
    if (v.size() != 3 + nf + 1) {
      std::printf("malformed fixture row %d\n", rows);
      std::fclose(f);
      return 2;
    }
    const Cfg c{(int)v[0], (int)v[1], v[2] != 0};
    const EnvParams p = carved(c);
    for (size_t i = 0; i < nf; i++)
      if ((p.*kFields[i].m) != v[3 + i])
        violation(c, std::string(kFields[i].name) + " = " + std::to_string(p.*kFields[i].m) +
                         ", fixture " + std::to_string(v[3 + i]));
    if (carve_fits(p, c.big) != (v[3 + nf] != 0)) violation(c, "fits differs from the fixture");
    rows++;
  }
  std::fclose(f);
  GridSum g;
  for_grid([&](const Cfg &c) {
    const EnvParams p = carved(c);
    const bool fits = carve_fits(p, c.big);
    g.add(p, fits);
    check_sizes(c, p, fits);
    if (fits) check_invariants(c, p);
  });
  if (rows < 40) violation(Cfg{0, 0, false}, "fixture has fewer than 40 configs");
  if (g.configs != g_configs || g.fit != g_fit || g.hash != g_hash) {
    bad++;
    std::printf("grid: %ld configs, %ld fit, hash %016llx; fixture %ld, %ld, %016llx\n", g.configs,
                g.fit, (unsigned long long)g.hash, g_configs, g_fit, g_hash);
  }
  std::printf("carve sweep: %d table rows, %ld configs, %ld fit, %d violations\n", rows, g.configs,
              g.fit, bad);
  if (bad == 0) std::printf("carve sweep ok\n");
  return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 2 && std::strcmp(argv[1], "--emit") == 0) {
    emit(stdout, carved, [](const Cfg &c) { return carve_fits(carved(c), c.big); });
    return 0;
  }
  if (argc != 2) {
    std::printf("usage: carve_sweep <carve_fields.csv> | --emit\n");
    return 2;
  }
  return check(argv[1]);
}
