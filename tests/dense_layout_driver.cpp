// tests/dense_layout_driver.cpp -- CPU driver of tests/test_dense_operator_layout.py: the stored layout of the dense operator and the
// plan of its product (diaglib_amd/csrc/hip_plans.h: dense_pack, dense_index, dense_plan), compiled with g++ and no ROCm include.
// It packs a column-major matrix with the product's own code and multiplies by walking the STORED array the way dense_mfma_kernel and
// dense_combine_kernel do: passes of at most 48 columns; per pass the planner's chunks; per chunk and row tile the groups in
// ascending order, lane by lane (the element of lane l = 16 kk + li, half e, of group g of tile t is read at its stored position, not
// through dense_index); partial sums of a split pass into a workspace, added in ascending chunk order.
//   in : int64 n, lda, m, ncu | a (lda x n doubles, column-major) | x (n x m doubles, column-major)
//   out: int64 n_pad, row_tile, bad_pad, bad_value, bad_roundtrip, passes | per pass int64 m, acc_groups, k_chunks, chunk_groups, groups,
//        row_groups, ws_doubles | y (n x m) | diag (n) | writes (n x m int32: how often each element of y was stored) |
//        ws_writes_bad (int64: workspace elements not written exactly once)
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
  if (!get(fi, head, 4)) return 2;
  const int n = (int)head[0], lda = (int)head[1], m = (int)head[2], ncu = (int)head[3];
  std::vector<double> a, x;
  if (!get(fi, a, (size_t)lda * n) || !get(fi, x, (size_t)n * m)) return 2;
  std::fclose(fi);

  const int n_pad = dense_n_pad(n);
  std::vector<double> stored((size_t)n_pad * n_pad, -1.0), diag((size_t)n, -1.0);
  dense_pack(n, a.data(), (size_t)lda, stored.data(), diag.data());
  int64_t bad_pad = 0, bad_value = 0, bad_roundtrip = 0;
  for (size_t d = 0; d < stored.size(); ++d) {
    const int i = dense_row_of(n_pad, d), k = dense_col_of(n_pad, d);
    if (i < 0 || i >= n_pad || k < 0 || k >= n_pad || dense_index(n_pad, i, k) != d) { ++bad_roundtrip; continue; }
    uint64_t bits;
    std::memcpy(&bits, &stored[d], 8);
    if (i >= n || k >= n) bad_pad += bits != 0;                                    // +0.0, bit for bit
    else bad_value += std::memcmp(&stored[d], &a[(size_t)k * lda + i], 8) != 0;
  }

  std::vector<double> y((size_t)n * m, 0.0);
  std::vector<int32_t> writes((size_t)n * m, 0);
  std::vector<int64_t> plans;
  int64_t passes = 0, ws_writes_bad = 0;
  for (int c0 = 0; c0 < m; c0 += DENSE_MAX_COLS, ++passes) {
    const int mp = std::min(DENSE_MAX_COLS, m - c0);
    const DensePlan p = dense_plan(ncu, n, mp);
    for (int64_t v : {(int64_t)mp, (int64_t)p.acc_groups, (int64_t)p.k_chunks, (int64_t)p.chunk_groups, (int64_t)p.groups, (int64_t)p.row_groups,
                      (int64_t)p.ws_doubles})
      plans.push_back(v);
    std::vector<double> ws(p.ws_doubles, 0.0);
    std::vector<int32_t> ws_writes(p.ws_doubles, 0);
    const double* xc = x.data() + (size_t)c0 * n;
    double* yc = y.data() + (size_t)c0 * n;
    int32_t* wc = writes.data() + (size_t)c0 * n;
    for (int by = 0; by < p.k_chunks; ++by) {
      const int g0 = by * p.chunk_groups, g1 = std::min(p.groups, g0 + p.chunk_groups);
      for (int rg = 0; rg < p.row_groups; ++rg)
        for (int t = 0; t < DENSE_WAVE_TILES; ++t) {
          const int tile = rg * DENSE_WAVE_TILES + t;
          if (tile >= p.row_tiles) continue;
          std::vector<double> acc((size_t)DENSE_TILE * mp, 0.0);
          for (int g = g0; g < g1; ++g)
            for (int e = 0; e < 2; ++e)
              for (int kk = 0; kk < 4; ++kk) {
                const int k = DENSE_GROUP * g + 4 * e + kk;
                for (int li = 0; li < DENSE_TILE; ++li) {
                  const double av = stored[(((size_t)tile * p.groups + g) * 64 + (size_t)(16 * kk + li)) * 2 + e];
                  for (int c = 0; c < mp; ++c) {
                    const double xv = k < n ? xc[(size_t)c * n + k] : 0.0;
                    acc[(size_t)c * DENSE_TILE + li] = std::fma(av, xv, acc[(size_t)c * DENSE_TILE + li]);
                  }
                }
              }
          for (int li = 0; li < DENSE_TILE; ++li) {
            const int row = tile * DENSE_TILE + li;
            if (row >= n) continue;
            for (int c = 0; c < mp; ++c) {
              if (p.k_chunks == 1) { yc[(size_t)c * n + row] = acc[(size_t)c * DENSE_TILE + li]; ++wc[(size_t)c * n + row]; }
              else {
                const size_t at = ((size_t)by * mp + c) * n + row;
                ws[at] = acc[(size_t)c * DENSE_TILE + li]; ++ws_writes[at];
              }
            }
          }
        }
    }
    if (p.k_chunks > 1) {
      const size_t total = (size_t)n * mp;
      for (size_t i = 0; i < total; ++i) {
        double s = ws[i];
        for (int c = 1; c < p.k_chunks; ++c) s += ws[(size_t)c * total + i];
        yc[i] = s; ++wc[i];
      }
      for (int32_t w : ws_writes) ws_writes_bad += w != 1;
    }
  }

  FILE* fo = std::fopen(argv[2], "wb");
  if (!fo) return 2;
  put(fo, std::vector<int64_t>{n_pad, DENSE_TILE * DENSE_WAVE_TILES, bad_pad, bad_value, bad_roundtrip, passes});
  put(fo, plans);
  put(fo, y);
  put(fo, diag);
  put(fo, writes);
  put(fo, std::vector<int64_t>{ws_writes_bad});
  std::fclose(fo);
  return 0;
}
