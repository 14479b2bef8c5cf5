// Test driver of dense_t_plan (diaglib_amd/csrc/hip_plans.h), built with g++ and no ROCm include (tests/test_dense_t_plan.py): reads
// one request "NCU N M" per line from standard input and prints the plan's fields as key=value tokens and, behind " | ", the name
// the engine would book for the launch.  The planner is called twice per request and the two answers are compared field by field.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "../diaglib_amd/csrc/hip_plans.h"

using namespace dla_plans;

static bool same(const DenseTPlan& a, const DenseTPlan& b)
{
  return a.n_pad == b.n_pad && a.row_tiles == b.row_tiles && a.col_blocks == b.col_blocks && a.strips == b.strips && a.acc_groups == b.acc_groups &&
         a.row_chunks == b.row_chunks && a.chunk_tiles == b.chunk_tiles && a.ws_doubles == b.ws_doubles;
}

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream ss(line);
    int ncu, n, m;
    if (!(ss >> ncu >> n >> m)) { std::fprintf(stderr, "bad request: %s\n", line.c_str()); return 2; }
    const DenseTPlan p = dense_t_plan(ncu, n, m);
    if (!same(p, dense_t_plan(ncu, n, m))) { std::fprintf(stderr, "two answers to: %s\n", line.c_str()); return 3; }
    std::printf("n_pad=%d row_tiles=%d col_blocks=%d strips=%d acc_groups=%d row_chunks=%d chunk_tiles=%d ws_doubles=%zu wave_blocks=%d min_chunk_tiles=%d ws_share=%d | %s\n",
                p.n_pad, p.row_tiles, p.col_blocks, p.strips, p.acc_groups, p.row_chunks, p.chunk_tiles, p.ws_doubles, DENSE_T_WAVE_BLOCKS,
                DENSE_T_MIN_CHUNK_TILES, DENSE_WS_SHARE, p.name().c_str());
  }
  return 0;
}
