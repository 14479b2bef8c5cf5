// tests/sell_layout_split_driver.cpp -- the two halves of the sliced-ELLPACK builder (dla::sell_layout and dla::sell_fill in
// diaglib_amd/csrc/dla_internal.h) against dla::sell_build, and the launch shapes of the set-up from device arrays
// (dla_plans::spmm_setup_plan in diaglib_amd/csrc/hip_plans.h), on the CPU with g++ and no ROCm include.  The assertions are in
// tests/test_sell_layout_split.py.
//
//   driver layout IN     IN: int64 n, nnz | int64 rowptr[n + 1] | int32 colind[nnz] | double values[nnz]
//                        prints one line "field=0|1" per field of dla::SellLayout (1: sell_layout + sell_fill give sell_build's),
//                        "layout_only_empty=0|1" (sell_layout alone leaves col, val, diag, long_col and long_val empty) and the counts.
//                        sell_layout has no parameter for columns or values: it is handed the row pointers alone.
//   driver plan          reads "NCU N NNZ SLICES SEGMENTS" per line from standard input, prints the four block counts and the cap
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../diaglib_amd/csrc/hip_plans.h"

template <class T>
static bool get(FILE* f, std::vector<T>& v, size_t count)
{
  v.resize(count);
  return count == 0 || fread(v.data(), sizeof(T), count, f) == count;
}

static int layout(const char* path)
{
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); return 2; }
  std::vector<int64_t> head, rowptr64;
  std::vector<int32_t> colind;
  std::vector<double> values;
  if (!get(f, head, 2)) return 2;
  const int n = (int)head[0];
  const size_t nnz = (size_t)head[1];
  if (!get(f, rowptr64, (size_t)n + 1) || !get(f, colind, nnz) || !get(f, values, nnz)) return 2;
  fclose(f);
  std::vector<long long> rowptr(rowptr64.begin(), rowptr64.end());

  dla::SellLayout whole, split;
  dla::sell_build(n, rowptr.data(), colind.data(), values.data(), whole);
  dla::sell_layout(n, rowptr.data(), split);     // (the row pointers alone: there is no parameter a column or a value could come through)
  const bool only_empty = split.col.empty() && split.val.empty() && split.diag.empty() && split.long_col.empty() && split.long_val.empty();
  dla::sell_fill(n, rowptr.data(), colind.data(), values.data(), split);

  auto bits = [](const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0);
  };
#define SAME(field) std::printf(#field "=%d\n", whole.field == split.field ? 1 : 0)
  SAME(n); SAME(slices); SAME(nnz); SAME(stored); SAME(long_entries); SAME(slice_ptr); SAME(perm); SAME(col);
  SAME(long_row); SAME(long_ptr); SAME(long_col); SAME(long_segments); SAME(multi_segments); SAME(seg_ptr); SAME(seg_row); SAME(seg_part);
  SAME(multi_row); SAME(part_ptr);
#undef SAME
  std::printf("val=%d\ndiag=%d\nlong_val=%d\n", bits(whole.val, split.val), bits(whole.diag, split.diag), bits(whole.long_val, split.long_val));
  std::printf("layout_only_empty=%d\n", only_empty ? 1 : 0);
  std::printf("count_long_rows=%zu\ncount_long_segments=%d\ncount_multi_segments=%d\ncount_stored=%lld\ncount_slices=%d\n", split.long_row.size(),
              split.long_segments, split.multi_segments, split.stored, split.slices);
  return 0;
}

static int plan()
{
  dla_plans::Knobs knobs;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream ss(line);
    int ncu; long long n, nnz, slices, segs;
    if (!(ss >> ncu >> n >> nnz >> slices >> segs)) continue;
    const dla_plans::PlanEnv env{ncu, (size_t)160 * 1024, knobs};
    const dla_plans::SpmmSetupPlan p = dla_plans::spmm_setup_plan(env, n, nnz, slices, segs);
    std::printf("entry_blocks=%d row_blocks=%d slice_blocks=%d seg_blocks=%d cap=%d\n", p.entry_blocks, p.row_blocks, p.slice_blocks, p.seg_blocks,
                ncu * 8);
  }
  return 0;
}

int main(int argc, char** argv)
{
  if (argc == 3 && std::string(argv[1]) == "layout") return layout(argv[2]);
  if (argc == 2 && std::string(argv[1]) == "plan") return plan();
  std::fprintf(stderr, "usage: %s layout IN | plan\n", argv[0]);
  return 2;
}
