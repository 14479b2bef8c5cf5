// tests/dense_sym_layout_driver.cpp -- CPU driver of tests/test_dense_sym_layout.py: the triangular copy of a symmetric dense
// matrix and the plan of its product (diaglib_amd/csrc/hip_plans.h: dense_sym_index, dense_sym_pack, dense_sym_plan), compiled with
// g++ and no ROCm include.  It packs a column-major array with the product's own code and multiplies by walking the STORED array
// the way dense_sym_mfma_kernel and dense_sym_combine_kernel do: passes of at most 48 columns; per pass the panels and their chunks;
// per column block the four wavefronts' tiles (a block is read at its stored position, not through dense_sym_index), the forward
// sums kept per (panel, chunk), the transposed sums of the four wavefronts added in wavefront order; everything through the
// workspace at the offsets the plan states, added per element in the combine order (forward chunks ascending, then panels).
//   in : int64 n, lda, m, ncu, uplo ('L' or 'U') | a (lda x n doubles, column-major) | x (n x m doubles, column-major)
//        (lda = 0: nothing follows; out is the first ten plan fields of one pass of m <= 48 columns)
//   out: int64 n_pad, stored doubles, bad_pad, bad_value, bad_roundtrip, bad_index, nan_stored, passes |
//        per pass int64 m, acc_groups, panels, chunk_panels, chunk_blocks, max_chunks, items, max_partials, t_base, ws_doubles,
//        items walked, largest number of partials the walk added into one element, workspace elements not written exactly once |
//        y (n x m) | diag (n) | writes (n x m int32: how often each element of y was stored)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../diaglib_amd/csrc/hip_plans.h"

using namespace dla_plans;

template <class T>
static bool get(FILE* f, std::vector<T>& v, size_t count)
{
  v.resize(count);
  return count == 0 || std::fread(v.data(), sizeof(T), count, f) == count;
}
template <class T>
static void put(FILE* f, const std::vector<T>& v) { if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char** argv)
{
  if (argc != 3) return 2;
  FILE* fi = std::fopen(argv[1], "rb");
  if (!fi) return 2;
  std::vector<int64_t> head;
  if (!get(fi, head, 5)) return 2;
  const int n = (int)head[0], lda = (int)head[1], m = (int)head[2], ncu = (int)head[3];
  const char uplo = (char)head[4];
  if (lda == 0) {   // the plan alone (sizes too large to walk): the ten plan fields of one pass of m columns
    const DenseSymPlan p = dense_sym_plan(ncu, n, m);
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) return 2;
    put(fo, std::vector<int64_t>{m, p.acc_groups, p.panels, p.chunk_panels, p.chunk_blocks, p.max_chunks, p.items, p.max_partials, (int64_t)p.t_base,
                                 (int64_t)p.ws_doubles});
    std::fclose(fo);
    return 0;
  }
  std::vector<double> a, x;
  if (!get(fi, a, (size_t)lda * n) || !get(fi, x, (size_t)n * m)) return 2;
  std::fclose(fi);

  const int n_pad = dense_n_pad(n), nt = n_pad / DENSE_TILE;
  const size_t total = dense_sym_doubles(n_pad);
  std::vector<double> stored(total, -1.0), diag((size_t)n, -1.0);
  dense_sym_pack(n, a.data(), (size_t)lda, uplo, stored.data(), diag.data());
  // ---- the index: a bijection from {(i, k): k / 16 <= i / 16} onto [0, total), the inverse pair returns (i, k)
  int64_t bad_pad = 0, bad_value = 0, bad_roundtrip = 0, bad_index = 0, nan_stored = 0;
  {
    std::vector<uint8_t> seen(total, 0);
    size_t pairs = 0;
    for (int i = 0; i < n_pad; ++i)
      for (int k = 0; k < (i / DENSE_TILE + 1) * DENSE_TILE; ++k, ++pairs) {
        const size_t d = dense_sym_index(i, k);
        if (d >= total || seen[d]) { ++bad_index; continue; }
        seen[d] = 1;
        if (dense_sym_row_of(d) != i || dense_sym_col_of(d) != k) ++bad_roundtrip;
      }
    bad_index += pairs != total;
  }
  for (size_t d = 0; d < total; ++d) {
    const int i = dense_sym_row_of(d), k = dense_sym_col_of(d);
    nan_stored += std::isnan(stored[d]);
    uint64_t bits;
    std::memcpy(&bits, &stored[d], 8);
    if (i >= n || k >= n) { bad_pad += bits != 0; continue; }                        // +0.0, bit for bit
    const bool lower = uplo == 'L';
    const double want = (i >= k) == lower ? a[(size_t)k * lda + i] : a[(size_t)i * lda + k];
    bad_value += std::memcmp(&stored[d], &want, 8) != 0;
  }

  std::vector<double> y((size_t)n * m, 0.0);
  std::vector<int32_t> writes((size_t)n * m, 0);
  std::vector<int64_t> plans;
  int64_t passes = 0;
  for (int c0 = 0; c0 < m; c0 += DENSE_MAX_COLS, ++passes) {
    const int mp = std::min(DENSE_MAX_COLS, m - c0);
    const DenseSymPlan p = dense_sym_plan(ncu, n, mp);
    std::vector<double> ws(p.ws_doubles, 0.0);
    std::vector<int32_t> ws_writes(p.ws_doubles, 0);
    const double* xc = x.data() + (size_t)c0 * n;
    double* yc = y.data() + (size_t)c0 * n;
    int32_t* wc = writes.data() + (size_t)c0 * n;
    const auto xat = [&](int col, int row) { return row < n ? xc[(size_t)col * n + row] : 0.0; };
    const bool direct = nt == 1;
    int64_t items = 0, ws_bad = 0, most = 0;
    const int cp = p.chunk_panels;
    for (int P = p.panels - 1; P >= 0; --P)
      for (int c = 0; c <= P / cp; ++c, ++items) {
        const int last = std::min(16 * P + 15, nt - 1);
        const int b0 = 16 * cp * c, b1 = std::min(last + 1, b0 + 16 * cp);
        std::vector<double> acc_f((size_t)256 * mp, 0.0);                            // [column][row of the panel]
        for (int b = b0; b < b1; ++b) {
          std::vector<double> acc_t((size_t)4 * 16 * mp, 0.0);                       // [wavefront][column][row of block b]
          for (int w = 0; w < 4; ++w)
            for (int t = 0; t < DENSE_WAVE_TILES; ++t) {
              const int T = 16 * P + DENSE_WAVE_TILES * w + t;
              if (T > last || b > T) continue;
              const double* blk = stored.data() + ((size_t)T * (T + 1) + (size_t)(2 * b)) * 128;
              for (int h = 0; h < 2; ++h)
                for (int e = 0; e < 2; ++e)
                  for (int kk = 0; kk < 4; ++kk)
                    for (int li = 0; li < 16; ++li) {
                      const double av = blk[(size_t)h * 128 + (size_t)(16 * kk + li) * 2 + e];
                      const int j = 8 * h + 4 * e + kk;                              // a(16 T + li, 16 b + j)
                      for (int col = 0; col < mp; ++col) {
                        double& f = acc_f[(size_t)col * 256 + (size_t)(16 * (T - 16 * P) + li)];
                        f = std::fma(av, xat(col, 16 * b + j), f);
                        if (T > b) {
                          double& s = acc_t[((size_t)w * mp + col) * 16 + j];
                          s = std::fma(av, xat(col, 16 * T + li), s);
                        }
                      }
                    }
            }
          if (b < last)
            for (int col = 0; col < mp; ++col)
              for (int j = 0; j < 16; ++j) {
                const auto part = [&](int w) { return acc_t[((size_t)w * mp + col) * 16 + j]; };
                const size_t at = p.t_base + (size_t)16 * mp * ((size_t)8 * P * P + (size_t)7 * P + (size_t)b) + (size_t)col * 16 + j;
                if (at >= ws.size()) { ++ws_bad; continue; }
                ws[at] = ((part(0) + part(1)) + part(2)) + part(3);
                ++ws_writes[at];
              }
        }
        const int rows = std::min(256, n - 256 * P);
        for (int col = 0; col < mp; ++col)
          for (int r = 0; r < rows; ++r) {
            if (direct) { yc[(size_t)col * n + r] = acc_f[(size_t)col * 256 + r]; ++wc[(size_t)col * n + r]; continue; }
            const size_t at = (size_t)mp * ((size_t)256 * (size_t)dense_sym_chunks_before(P, cp) + (size_t)c * rows) + (size_t)col * rows + r;
            if (at >= ws.size()) { ++ws_bad; continue; }
            ws[at] = acc_f[(size_t)col * 256 + r];
            ++ws_writes[at];
          }
      }
    if (!direct) {
      for (int col = 0; col < mp; ++col)
        for (int i = 0; i < n; ++i) {
          const int P = i / 256, b = i / 16, rows = std::min(256, n - 256 * P);
          const double* f = ws.data() + (size_t)mp * 256 * (size_t)dense_sym_chunks_before(P, cp) + (size_t)col * rows + (i - 256 * P);
          double s = f[0];
          int64_t count = 1;
          for (int c = 1; c <= P / cp; ++c, ++count) s += f[(size_t)c * mp * rows];
          for (int q = dense_sym_first_panel(nt, b); q < p.panels; ++q, ++count)
            s += ws[p.t_base + (size_t)16 * mp * ((size_t)8 * q * q + (size_t)7 * q + (size_t)b) + (size_t)col * 16 + (i & 15)];
          yc[(size_t)col * n + i] = s;
          ++wc[(size_t)col * n + i];
          most = std::max(most, count);
        }
      for (int32_t w : ws_writes) ws_bad += w != 1;
    } else
      most = 1;
    for (int64_t v : {(int64_t)mp, (int64_t)p.acc_groups, (int64_t)p.panels, (int64_t)p.chunk_panels, (int64_t)p.chunk_blocks, (int64_t)p.max_chunks,
                      (int64_t)p.items, (int64_t)p.max_partials, (int64_t)p.t_base, (int64_t)p.ws_doubles, items, most, ws_bad})
      plans.push_back(v);
  }

  FILE* fo = std::fopen(argv[2], "wb");
  if (!fo) return 2;
  put(fo, std::vector<int64_t>{n_pad, (int64_t)total, bad_pad, bad_value, bad_roundtrip, bad_index, nan_stored, passes});
  put(fo, plans);
  put(fo, y);
  put(fo, diag);
  put(fo, writes);
  std::fclose(fo);
  return 0;
}
