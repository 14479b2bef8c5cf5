// tests/sell_layout_driver.cpp -- the sliced-ELLPACK layout builder of the product (dla::sell_build, dla::spmm_csr_check and
// dla::spmm_pick_format in diaglib_amd/csrc/dla_internal.h) on the CPU: reads a CSR matrix and a block x, checks and builds the
// layout with the product's own code, multiplies by walking the structure the way sell_spmm_kernel and csr_long_rows_kernel do
// (slices of 64 lanes in stored order with one fused multiply-add per entry, perm, then the tail with 64 strided partial sums
// and a butterfly), and writes what it saw.  The assertions are in tests/test_sell_layout.py.
//
//   in : int64 n, m, nnz, format | int64 rowptr[n + 1] | int32 colind[nnz] | double values[nnz] | double x[n * m] (column-major)
//   out: int64 status, and when status == 0:
//        int64 n, m, slices, stored, long_entries, long_rows, nnz, C, sigma, long_row_threshold, picked format |
//        double ax[n * m] | double diag[n] | int32 writes[n] | int32 perm[n] | int64 slice_ptr[slices + 1] |
//        int32 long_row[long_rows] | int64 long_ptr[long_rows + 1]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "../diaglib_amd/csrc/dla_internal.h"

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
  if (argc != 3) { fprintf(stderr, "usage: %s in out\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<int64_t> head, rowptr64;
  std::vector<int32_t> colind;
  std::vector<double> values, x;
  if (!get(f, head, 4)) return 2;
  const int n = (int)head[0], m = (int)head[1], format = (int)head[3];
  const size_t nnz_in = (size_t)head[2], rows = (size_t)(n > 0 ? n : 0);
  if (!get(f, rowptr64, rows + 1) || !get(f, colind, nnz_in) || !get(f, values, nnz_in) || !get(f, x, rows * (size_t)m)) return 2;
  fclose(f);
  std::vector<long long> rowptr(rowptr64.begin(), rowptr64.end());

  FILE* o = fopen(argv[2], "wb");
  if (!o) { perror(argv[2]); return 2; }
  int w = 0; long long nnz = 0;
  std::string err;
  const int64_t status = dla::spmm_csr_check(n, rowptr.data(), colind.data(), values.data(), format, &w, &nnz, err);
  put(o, &status, 1);
  if (status) { fclose(o); printf("refused: %s\n", err.c_str()); return 0; }

  dla::SellLayout L;
  dla::sell_build(n, rowptr.data(), colind.data(), values.data(), L);
  constexpr int C = dla::SELL_C;
  std::vector<double> ax((size_t)n * m, 7.0);
  std::vector<int32_t> writes((size_t)n, 0);
  for (int s = 0; s < L.slices; ++s) {
    const long long p0 = L.slice_ptr[s];
    const int width = (int)((L.slice_ptr[s + 1] - p0) / C);
    for (int lane = 0; lane < C; ++lane) {
      const int slot = s * C + lane;
      const int row = slot < n ? L.perm[slot] : -1;
      for (int c = 0; c < m; ++c) {
        double acc = 0.0;
        for (int q = 0; q < width; ++q) acc = std::fma(L.val[(size_t)(p0 + (long long)q * C + lane)], x[(size_t)c * n + L.col[(size_t)(p0 + (long long)q * C + lane)]], acc);
        if (row >= 0) ax[(size_t)c * n + row] = acc;
      }
      if (row >= 0) ++writes[row];
    }
  }
  for (size_t r = 0; r < L.long_row.size(); ++r) {
    const int row = L.long_row[r];
    for (int c = 0; c < m; ++c) {
      double part[64] = {0.0}, next[64];
      for (int lane = 0; lane < 64; ++lane)
        for (long long p = L.long_ptr[r] + lane; p < L.long_ptr[r + 1]; p += 64) part[lane] = std::fma(L.long_val[(size_t)p], x[(size_t)c * n + L.long_col[(size_t)p]], part[lane]);
      for (int off = 32; off > 0; off >>= 1) {
        for (int lane = 0; lane < 64; ++lane) next[lane] = part[lane] + part[lane ^ off];
        for (int lane = 0; lane < 64; ++lane) part[lane] = next[lane];
      }
      ax[(size_t)c * n + row] = part[0];
    }
    ++writes[row];
  }
  const int64_t out_head[11] = {n, m, L.slices, L.stored, L.long_entries, (int64_t)L.long_row.size(), L.nnz, C, dla::SELL_SIGMA,
                                dla::SELL_LONG_ROW, dla::spmm_pick_format(DLA_SPMM_AUTO, w, n, nnz)};
  put(o, out_head, 11);
  put(o, ax.data(), ax.size());
  put(o, L.diag.data(), L.diag.size());
  put(o, writes.data(), writes.size());
  put(o, L.perm.data(), L.perm.size());
  std::vector<int64_t> sp(L.slice_ptr.begin(), L.slice_ptr.end()), lp(L.long_ptr.begin(), L.long_ptr.end());
  put(o, sp.data(), sp.size());
  put(o, L.long_row.data(), L.long_row.size());
  put(o, lp.data(), lp.size());
  fclose(o);
  return 0;
}
