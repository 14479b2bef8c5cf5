// tests/spmm_transpose_driver.cpp -- the transposed index of the sparse operator (dla::spmm_transpose_build and what it calls, in
// diaglib_amd/csrc/dla_internal.h) on the CPU: reads a CSR matrix A and a block x, lays A out in format_a and builds the index in
// format_t with the product's own host code, forms y = A^T x by walking the index the way ell_spmm_t_kernel, sell_spmm_t_kernel and
// csr_long_segments_t_kernel / long_rows_combine_kernel do (values fetched from A's stored array through the positions, padding
// skipped, one fused multiply-add per entry, 64 strided partial sums and the butterfly per segment, segments added in order),
// forms z = (A^T) x by the forward walk over the explicitly, stably transposed CSR arrays stored in the index's format, and writes
// what it saw.  The assertions are in tests/test_spmm_transpose_index.py.
//
//   in : int64 n, m, nnz, format_a, format_t | int64 rowptr[n + 1] | int32 colind[nnz] | double values[nnz] | double x[n * m]
//   out: int64 status (a refusal's message goes to stdout), and when status == 0:
//        int64 n, m, nnz, a_fmt, a_stored, a_total, t_fmt, t_w, t_stored, t_slices, t_long_rows, t_long_entries, t_long_segments,
//              t_multi_segments, entries |
//        double y[n * m] | double z[n * m] | int32 writes[n] | int32 row[entries] | int32 pos[entries] | double a_val[a_total] |
//        int64 colptr[n + 1] | int32 perm[n] (SELL) | int64 slice_ptr[slices + 1] (SELL) | int32 long_row[long_rows] |
//        int64 long_ptr[long_rows + 1] | int64 seg_ptr[long_segments + 1] | int32 seg_part[long_segments] |
//        int64 ref slice_ptr[slices + 1] | int32 ref perm[n]      (sell_layout of the column lengths, computed here once more)
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

// what a slot stores of a matrix: ELLPACK (w) or a sliced layout, and the value array with the tail behind `stored`
struct Stored {
  int fmt = -1, w = 0;
  dla::SellLayout L;
  std::vector<int> col;
  std::vector<double> val;
  long long stored = 0, total = 0;
};
static void store(int n, const long long* rowptr, const int* colind, const double* values, int format, Stored& s)
{
  int w = 0;
  for (int i = 0; i < n; ++i) w = std::max(w, (int)(rowptr[i + 1] - rowptr[i]));
  s.fmt = dla::spmm_pick_format(format, w, n, rowptr[n] - rowptr[0]);
  if (s.fmt == DLA_SPMM_ELL) {
    s.w = w; s.stored = s.total = (long long)w * n;
    s.col.assign((size_t)s.total, 0); s.val.assign((size_t)s.total, 0.0);
    for (int i = 0; i < n; ++i)
      for (int q = 0; q < w; ++q) {
        const bool in = rowptr[i] + q < rowptr[i + 1];
        s.col[(size_t)q * n + i] = in ? colind[rowptr[i] + q] : i;
        s.val[(size_t)q * n + i] = in ? values[rowptr[i] + q] : 0.0;
      }
    return;
  }
  dla::sell_build(n, rowptr, colind, values, s.L);
  s.stored = s.L.stored; s.total = s.L.stored + s.L.long_entries;
  s.col = s.L.col; s.val = s.L.val;
  s.col.insert(s.col.end(), s.L.long_col.begin(), s.L.long_col.end());
  s.val.insert(s.val.end(), s.L.long_val.begin(), s.L.long_val.end());
}

// one segment of a tail: 64 strided partial sums from 0.0, then the butterfly; entry(p, &value, &gathered row)
template <class Entry>
static double segment_sum(long long p0, long long p1, const double* xc, Entry entry)
{
  double part[64] = {0.0}, next[64];
  for (int lane = 0; lane < 64; ++lane)
    for (long long p = p0 + lane; p < p1; p += 64) {
      double v = 0.0; int r = 0;
      entry(p, &v, &r);
      part[lane] = std::fma(v, xc[r], part[lane]);
    }
  for (int off = 32; off > 0; off >>= 1) {
    for (int lane = 0; lane < 64; ++lane) next[lane] = part[lane] + part[lane ^ off];
    for (int lane = 0; lane < 64; ++lane) part[lane] = next[lane];
  }
  return part[0];
}
// the walk of a layout: ELLPACK rows, or slices, then the tail in segments with the rows of more than one combined in order.
// entry(d, &value, &gathered row) returns false for padding that is to be skipped; tail entries are never padding
template <class Entry>
static void walk(int n, int m, int fmt, int w, const dla::SellLayout& L, const std::vector<double>& x, Entry entry, std::vector<double>& y,
                 std::vector<int32_t>* writes)
{
  if (fmt == DLA_SPMM_ELL) {
    for (int i = 0; i < n; ++i) {
      for (int c = 0; c < m; ++c) {
        double s = 0.0;
        for (int q = 0; q < w; ++q) {
          double v = 0.0; int r = 0;
          if (entry((size_t)q * n + i, &v, &r)) s = std::fma(v, x[(size_t)c * n + r], s);
        }
        y[(size_t)c * n + i] = s;
      }
      if (writes) ++(*writes)[i];
    }
    return;
  }
  constexpr int C = dla::SELL_C;
  for (int sl = 0; sl < L.slices; ++sl) {
    const long long p0 = L.slice_ptr[sl];
    const int width = (int)((L.slice_ptr[sl + 1] - p0) / C);
    for (int lane = 0; lane < C; ++lane) {
      const int slot = sl * C + lane;
      const int out = slot < n ? L.perm[slot] : -1;
      for (int c = 0; c < m; ++c) {
        double acc = 0.0;
        for (int q = 0; q < width; ++q) {
          double v = 0.0; int r = 0;
          if (entry((size_t)(p0 + (long long)q * C + lane), &v, &r)) acc = std::fma(v, x[(size_t)c * n + r], acc);
        }
        if (out >= 0) y[(size_t)c * n + out] = acc;
      }
      if (out >= 0 && writes) ++(*writes)[out];
    }
  }
  std::vector<double> part((size_t)std::max(1, L.multi_segments) * m, 0.0);
  for (int g = 0; g < L.long_segments; ++g) {
    const int out = L.long_row[L.seg_row[g]];
    for (int c = 0; c < m; ++c) {
      const double s = segment_sum(L.seg_ptr[g], L.seg_ptr[g + 1], x.data() + (size_t)c * n, [&](long long p, double* v, int* r) {
        entry((size_t)(L.stored + p), v, r);
      });
      if (L.seg_part[g] < 0) y[(size_t)c * n + out] = s;
      else part[(size_t)L.seg_part[g] * m + c] = s;
    }
    if (L.seg_part[g] < 0 && writes) ++(*writes)[out];
  }
  for (size_t j = 0; j < L.multi_row.size(); ++j) {
    for (int c = 0; c < m; ++c) {
      double sum = part[(size_t)L.part_ptr[j] * m + c];
      for (int sg = L.part_ptr[j] + 1; sg < L.part_ptr[j + 1]; ++sg) sum += part[(size_t)sg * m + c];
      y[(size_t)c * n + L.multi_row[j]] = sum;
    }
    if (writes) ++(*writes)[L.multi_row[j]];
  }
}

int main(int argc, char** argv)
{
  if (argc != 3) { fprintf(stderr, "usage: %s in out\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<int64_t> head, rowptr64;
  std::vector<int32_t> colind;
  std::vector<double> values, x;
  if (!get(f, head, 5)) return 2;
  const int n = (int)head[0], m = (int)head[1], format_a = (int)head[3], format_t = (int)head[4];
  const size_t nnz_in = (size_t)head[2], rows = (size_t)(n > 0 ? n : 0);
  if (!get(f, rowptr64, rows + 1) || !get(f, colind, nnz_in) || !get(f, values, nnz_in) || !get(f, x, rows * (size_t)m)) return 2;
  fclose(f);
  std::vector<long long> rowptr(rowptr64.begin(), rowptr64.end());

  FILE* o = fopen(argv[2], "wb");
  if (!o) { perror(argv[2]); return 2; }
  int w = 0; long long nnz = 0;
  std::string err;
  int64_t status = dla::spmm_csr_check(n, rowptr.data(), colind.data(), values.data(), format_a, &w, &nnz, err);
  Stored A;
  dla::TransposeIndex T;
  if (!status) {
    store(n, rowptr.data(), colind.data(), values.data(), format_a, A);
    status = dla::spmm_transpose_build(n, rowptr.data(), colind.data(), A.fmt, A.w, &A.L, format_t, T, err);
  }
  put(o, &status, 1);
  if (status) { fclose(o); printf("refused: %s\n", err.c_str()); return 0; }

  // y = A^T x through the index
  std::vector<double> y((size_t)n * m, 7.0), z((size_t)n * m, 7.0);
  std::vector<int32_t> writes((size_t)n, 0);
  walk(n, m, T.fmt, T.w, T.lay, x, [&](size_t d, double* v, int* r) {
    if (T.pos[d] < 0) return false;
    *v = A.val[(size_t)T.pos[d]]; *r = T.row[d];
    return true;
  }, y, &writes);

  // z: the forward walk over the explicitly transposed arrays (a stable counting sort of the triplets by column) in the index's format
  std::vector<long long> tptr((size_t)n + 1, 0);
  for (long long p = rowptr[0]; p < rowptr[n]; ++p) ++tptr[(size_t)colind[p] + 1];
  for (int j = 0; j < n; ++j) tptr[(size_t)j + 1] += tptr[j];
  std::vector<long long> next(tptr.begin(), tptr.end() - 1);
  std::vector<int> tcol((size_t)nnz);
  std::vector<double> tval((size_t)nnz);
  for (int i = 0; i < n; ++i)
    for (long long p = rowptr[i]; p < rowptr[i + 1]; ++p) {
      const size_t k = (size_t)next[(size_t)colind[p]]++;
      tcol[k] = i; tval[k] = values[p];
    }
  Stored B;
  store(n, tptr.data(), tcol.data(), tval.data(), T.fmt, B);
  walk(n, m, B.fmt, B.w, B.L, x, [&](size_t d, double* v, int* r) { *v = B.val[d]; *r = B.col[d]; return true; }, z, nullptr);

  dla::SellLayout R;
  if (T.fmt == DLA_SPMM_SELL) dla::sell_layout(n, tptr.data(), R);
  const int64_t out_head[15] = {n, m, nnz, A.fmt, A.stored, A.total, T.fmt, T.w, T.lay.stored, T.lay.slices, (int64_t)T.lay.long_row.size(),
                                T.lay.long_entries, T.lay.long_segments, T.lay.multi_segments, T.entries()};
  put(o, out_head, 15);
  put(o, y.data(), y.size());
  put(o, z.data(), z.size());
  put(o, writes.data(), writes.size());
  put(o, T.row.data(), T.row.size());
  put(o, T.pos.data(), T.pos.size());
  put(o, A.val.data(), A.val.size());
  std::vector<int64_t> cp(T.colptr.begin(), T.colptr.end());
  put(o, cp.data(), cp.size());
  if (T.fmt == DLA_SPMM_SELL) {
    std::vector<int64_t> sp(T.lay.slice_ptr.begin(), T.lay.slice_ptr.end()), lp(T.lay.long_ptr.begin(), T.lay.long_ptr.end()),
        gp(T.lay.seg_ptr.begin(), T.lay.seg_ptr.end()), rsp(R.slice_ptr.begin(), R.slice_ptr.end());
    put(o, T.lay.perm.data(), T.lay.perm.size());
    put(o, sp.data(), sp.size());
    put(o, T.lay.long_row.data(), T.lay.long_row.size());
    put(o, lp.data(), lp.size());
    put(o, gp.data(), gp.size());
    put(o, T.lay.seg_part.data(), T.lay.seg_part.size());
    put(o, rsp.data(), rsp.size());
    put(o, R.perm.data(), R.perm.size());
  }
  fclose(o);
  return 0;
}
