// tests/dense_lr_layout_driver.cpp -- CPU driver of tests/test_dense_lr_layout.py: the host twin of dense_pack_pair_kernel
// (diaglib_amd/csrc/hip_plans.h: dense_pack_pair), compiled with g++ and no ROCm include.  It packs the sum and the difference of two
// column-major arrays with the product's own code, and packs two further arrays (the caller's p + q and p - q) with dense_pack;
// all output blocks start from a poison value, so that padding nobody wrote shows.
//   in : int64 n, ldp, ldq | p (ldp x n doubles, column-major) | q (ldq x n) | sum (n x n) | dif (n x n)
//   out: int64 n_pad | pair_sum (n_pad^2) | pair_dif (n_pad^2) | pair_sum_diag (n) | pair_dif_diag (n) |
//        pack_sum (n_pad^2) | pack_dif (n_pad^2) | pack_sum_diag (n) | pack_dif_diag (n)
#include <cstdint>
#include <cstdio>
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
  if (!get(fi, head, 3)) return 2;
  const int n = (int)head[0], ldp = (int)head[1], ldq = (int)head[2];
  std::vector<double> p, q, sum, dif;
  if (!get(fi, p, (size_t)ldp * n) || !get(fi, q, (size_t)ldq * n) || !get(fi, sum, (size_t)n * n) || !get(fi, dif, (size_t)n * n)) return 2;
  std::fclose(fi);

  const int n_pad = dense_n_pad(n);
  const size_t total = (size_t)n_pad * n_pad;
  const double poison = -7.25e77;
  std::vector<double> pair_sum(total, poison), pair_dif(total, poison), pair_sum_diag((size_t)n, poison), pair_dif_diag((size_t)n, poison);
  std::vector<double> pack_sum(total, poison), pack_dif(total, poison), pack_sum_diag((size_t)n, poison), pack_dif_diag((size_t)n, poison);
  dense_pack_pair(n, p.data(), (size_t)ldp, q.data(), (size_t)ldq, pair_sum.data(), pair_sum_diag.data(), pair_dif.data(), pair_dif_diag.data());
  dense_pack(n, sum.data(), (size_t)n, pack_sum.data(), pack_sum_diag.data());
  dense_pack(n, dif.data(), (size_t)n, pack_dif.data(), pack_dif_diag.data());

  FILE* fo = std::fopen(argv[2], "wb");
  if (!fo) return 2;
  put(fo, std::vector<int64_t>{n_pad});
  for (const std::vector<double>* v : {&pair_sum, &pair_dif, &pair_sum_diag, &pair_dif_diag, &pack_sum, &pack_dif, &pack_sum_diag, &pack_dif_diag}) put(fo, *v);
  std::fclose(fo);
  return 0;
}
