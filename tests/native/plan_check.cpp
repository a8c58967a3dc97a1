// plan_check: the launch planner (csrc/mcpt_plan.h) against a table of cases.
//   plan_check <cases.txt>
// One case per line: the PlanIn fields, then the expected PlanOut fields, as
// whitespace-separated integers ('#' starts a comment line).  Prints every
// case whose outputs differ; exits non-zero on any difference.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "mcpt_plan.h"

int main(int argc, char **argv) {
  if (argc != 2) return std::fprintf(stderr, "usage: plan_check <cases.txt>\n"), 2;
  std::ifstream f(argv[1]);
  if (!f) return std::fprintf(stderr, "plan_check: cannot open %s\n", argv[1]), 2;
  std::string line;
  int n = 0, bad = 0, lineno = 0;
  while (std::getline(f, line)) {
    ++lineno;
    if (line.empty() || line[0] == '#') continue;
    std::istringstream s(line);
    long long v[26];
    for (long long &x : v)
      if (!(s >> x)) return std::fprintf(stderr, "plan_check: line %d: expected 26 integers\n", lineno), 2;
    mcpt::PlanIn in;
    in.width = (int32_t)v[0], in.height = (int32_t)v[1], in.frames = (int32_t)v[2];
    in.frames_per_launch = (int32_t)v[3];
    in.stripe_rows = (int32_t)v[4], in.stripe_index = (int32_t)v[5], in.stripe_count = (int32_t)v[6];
    in.block_entries = (int32_t)v[7], in.max_block_frames = (int32_t)v[8];
    in.last_block_frames = (int32_t)v[9], in.pixel_spread = (int32_t)v[10];
    in.resident_wg = v[11], in.wg_waves = (int32_t)v[12];
    const mcpt::PlanOut o = mcpt::plan_launches(in);
    const long long got[13] = {o.local_rows, o.tiles_x, o.tiles,        o.grid_wg,  o.fpl,           o.fpl_head, o.nb_head,
                               o.fpl_tail,   o.max_blocks, o.n_blocks_all, o.n_launch, o.no_handoff, o.spread};
    static const char *const names[13] = {"local_rows", "tiles_x",    "tiles",        "grid_wg",  "fpl",        "fpl_head", "nb_head",
                                          "fpl_tail",   "max_blocks", "n_blocks_all", "n_launch", "no_handoff", "spread"};
    bool differs = false;
    for (int k = 0; k < 13; ++k)
      if (got[k] != v[13 + k]) {
        if (!differs) std::printf("line %d: %s\n", lineno, line.c_str());
        std::printf("  %s: got %lld, expected %lld\n", names[k], got[k], v[13 + k]);
        differs = true;
      }
    bad += differs;
    ++n;
  }
  if (n == 0) return std::fprintf(stderr, "plan_check: no cases\n"), 2;
  if (bad) return std::printf("%d of %d cases differ\n", bad, n), 1;
  std::printf("ok %d cases\n", n);
  return 0;
}
