// Test driver of ritz_expand_plan (diaglib_amd/csrc/hip_plans.h), built with g++ and no ROCm include (tests/test_ritz_expand_plans.py):
// reads one request per line from standard input and prints the plan's fields as key=value tokens and, behind " | ", the name the
// engine would book for the launch.
//
//   env NCU LDS_LIMIT T0                            the device and knob 0 of the requests that follow
//   plan N M NB FIRST0 VEC2                         ritz_expand_plan
//   instances                                       RITZ_EXPAND_TILES
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "../diaglib_amd/csrc/hip_plans.h"

using namespace dla_plans;

int main()
{
  Knobs knobs;
  int ncu = 256;
  size_t lds_limit = (size_t)160 * 1024;
  std::string line, what;
  while (std::getline(std::cin, line)) {
    std::istringstream ss(line);
    if (!(ss >> what)) continue;
    const PlanEnv env{ncu, lds_limit, knobs};
    if (what == "env") {
      int t0 = 0;
      ss >> ncu >> lds_limit >> t0;
      knobs.set(0, t0);
    } else if (what == "plan") {
      int n, m, nb, first0; bool vec2;
      ss >> n >> m >> nb >> first0 >> vec2;
      const RitzExpandPlan p = ritz_expand_plan(env, n, m, nb, first0, vec2);
      std::printf("tx=%d staged_tiles=%d lds=%zu fits=%d blocks=%d rows=%d ncol=%d nslots=%d gram_slots=%d small=%zu | %s\n", p.tx, p.staged_tiles, p.lds,
                  p.fits ? 1 : 0, p.blocks, p.rows, p.ncol, p.nslots, p.gram_slots, p.small_doubles(), p.name().c_str());
    } else if (what == "instances") {
      std::printf("tiles=");
      bool first = true;
      for (int t : RITZ_EXPAND_TILES) { std::printf(first ? "%d" : ",%d", t); first = false; }
      std::printf("\n");
    } else {
      std::fprintf(stderr, "unknown request: %s\n", line.c_str());
      return 2;
    }
  }
  return 0;
}
