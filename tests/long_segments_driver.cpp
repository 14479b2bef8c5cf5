// tests/long_segments_driver.cpp -- the segments of the sliced format's CSR tail (dla::sell_build in diaglib_amd/csrc/dla_internal.h)
// and the plan of their launches (dla_plans::long_rows_plan in diaglib_amd/csrc/hip_plans.h) on the CPU: reads a CSR matrix and a
// block x, builds the layout with the product's own code, multiplies the TAIL rows by walking the segment table the way
// csr_long_segments_kernel and long_rows_combine_kernel do (64 strided partial sums per segment with one fused multiply-add per
// entry, a butterfly, then the partials of a row added in segment order) and writes what it saw.  The assertions are in
// tests/test_long_row_segments.py.  A plain program: it may be built with -fsanitize=address,undefined.
//
//   long_segments_driver constants      prints "SEG LONG_ROW"
//   long_segments_driver in out
//   in : int64 n, m, nnz, nplans | int64 rowptr[n + 1] | int32 colind[nnz] | double values[nnz] | double x[n * m] (column-major) |
//        int64 (ncu, m_plan)[nplans]
//   out: int64 n, m, SEG, LONG_ROW, long_rows, long_entries, long_segments, multi_segments, multi_rows |
//        int32 long_row[long_rows] | int64 long_ptr[long_rows + 1] | int64 seg_ptr[long_segments + 1] | int32 seg_row[long_segments] |
//        int32 seg_part[long_segments] | int32 multi_row[multi_rows] | int32 part_ptr[multi_rows + 1] |
//        double ax[n * m] (7.0 where nothing was stored) | int32 ax_writes[n] | int32 part_writes[multi_segments] |
//        int64 (seg_blocks, combine_blocks, part_doubles, name is "csr_long_segments_kernel<4>")[nplans]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../diaglib_amd/csrc/hip_plans.h"

template <class T>
static bool get(FILE* f, std::vector<T>& v, size_t count)
{
  v.resize(count);
  return count == 0 || fread(v.data(), sizeof(T), count, f) == count;
}
template <class T>
static void put(FILE* f, const T* p, size_t count) { if (count) fwrite(p, sizeof(T), count, f); }

int main(int argc, char** argv)
{
  if (argc == 2 && !strcmp(argv[1], "constants")) { printf("%d %d\n", dla::SELL_LONG_SEG, dla::SELL_LONG_ROW); return 0; }
  if (argc != 3) { fprintf(stderr, "usage: %s constants | in out\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<int64_t> head, rowptr64, plans_in;
  std::vector<int32_t> colind;
  std::vector<double> values, x;
  if (!get(f, head, 4)) return 2;
  const int n = (int)head[0], m = (int)head[1];
  const size_t nnz_in = (size_t)head[2], nplans = (size_t)head[3];
  if (n <= 0 || m <= 0) return 2;
  if (!get(f, rowptr64, (size_t)n + 1) || !get(f, colind, nnz_in) || !get(f, values, nnz_in) || !get(f, x, (size_t)n * m) || !get(f, plans_in, 2 * nplans)) return 2;
  fclose(f);
  std::vector<long long> rowptr(rowptr64.begin(), rowptr64.end());
  int w = 0; long long nnz = 0;
  std::string err;
  if (dla::spmm_csr_check(n, rowptr.data(), colind.data(), values.data(), DLA_SPMM_SELL, &w, &nnz, err)) { fprintf(stderr, "refused: %s\n", err.c_str()); return 2; }

  dla::SellLayout L;
  dla::sell_build(n, rowptr.data(), colind.data(), values.data(), L);
  const size_t ns = L.seg_row.size(), nm = L.multi_row.size();
  if ((size_t)L.long_segments != ns || L.seg_part.size() != ns || L.seg_ptr.size() != ns + 1 || L.part_ptr.size() != nm + 1) { fprintf(stderr, "the segment tables have inconsistent lengths\n"); return 1; }

  // the two kernels, on the CPU: out-of-range slots or rows end the program (under the sanitizers: loudly)
  std::vector<double> ax((size_t)n * m, 7.0), part((size_t)L.multi_segments * m, 7.0);
  std::vector<int32_t> ax_writes((size_t)n, 0), part_writes((size_t)L.multi_segments, 0);
  for (size_t g = 0; g < ns; ++g) {
    const int row = L.long_row.at((size_t)L.seg_row[g]), slot = L.seg_part[g];
    for (int c = 0; c < m; ++c) {
      double acc[64] = {0.0}, next[64];
      for (int lane = 0; lane < 64; ++lane)
        for (long long p = L.seg_ptr[g] + lane; p < L.seg_ptr[g + 1]; p += 64) acc[lane] = std::fma(L.long_val.at((size_t)p), x[(size_t)c * n + L.long_col.at((size_t)p)], acc[lane]);
      for (int off = 32; off > 0; off >>= 1) {
        for (int lane = 0; lane < 64; ++lane) next[lane] = acc[lane] + acc[lane ^ off];
        for (int lane = 0; lane < 64; ++lane) acc[lane] = next[lane];
      }
      if (slot < 0) ax.at((size_t)c * n + row) = acc[0];
      else part.at((size_t)slot * m + c) = acc[0];
    }
    if (slot < 0) ++ax_writes.at((size_t)row);
    else ++part_writes.at((size_t)slot);
  }
  for (size_t j = 0; j < nm; ++j) {
    for (int c = 0; c < m; ++c) {
      double sum = part.at((size_t)L.part_ptr[j] * m + c);
      for (int sg = L.part_ptr[j] + 1; sg < L.part_ptr[j + 1]; ++sg) sum += part.at((size_t)sg * m + c);
      ax.at((size_t)c * n + L.multi_row[j]) = sum;
    }
    ++ax_writes.at((size_t)L.multi_row[j]);
  }

  FILE* o = fopen(argv[2], "wb");
  if (!o) { perror(argv[2]); return 2; }
  const int64_t out_head[9] = {n, m, dla::SELL_LONG_SEG, dla::SELL_LONG_ROW, (int64_t)L.long_row.size(), L.long_entries, L.long_segments, L.multi_segments, (int64_t)nm};
  put(o, out_head, 9);
  std::vector<int64_t> lp(L.long_ptr.begin(), L.long_ptr.end()), sp(L.seg_ptr.begin(), L.seg_ptr.end());
  put(o, L.long_row.data(), L.long_row.size());
  put(o, lp.data(), lp.size());
  put(o, sp.data(), sp.size());
  put(o, L.seg_row.data(), ns);
  put(o, L.seg_part.data(), ns);
  put(o, L.multi_row.data(), nm);
  put(o, L.part_ptr.data(), nm + 1);
  put(o, ax.data(), ax.size());
  put(o, ax_writes.data(), ax_writes.size());
  put(o, part_writes.data(), part_writes.size());
  const dla_plans::Knobs knobs;
  for (size_t i = 0; i < nplans; ++i) {
    const dla_plans::PlanEnv env{(int)plans_in[2 * i], (size_t)64 * 1024, knobs};
    const dla_plans::LongRowsPlan p = dla_plans::long_rows_plan(env, L.long_segments, (int)nm, L.multi_segments, (int)plans_in[2 * i + 1], 4);
    const int64_t rec[4] = {p.seg_blocks, p.combine_blocks, (int64_t)p.part_doubles, p.name() == "csr_long_segments_kernel<4>" ? 1 : 0};
    put(o, rec, 4);
  }
  fclose(o);
  return 0;
}
