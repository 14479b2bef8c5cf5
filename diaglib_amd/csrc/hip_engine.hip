// diaglib_amd/csrc/hip_engine.hip -- the device engine: hand-written HIP kernels for gfx950
// (CDNA4, wave64, FP64 MFMA 16x16x4), one HIP stream, RCCL for the small cross-rank sums.
//
// Data layout: every panel is column-major float64, leading dimension n (local
// rows), columns contiguous -- the reference layout (diaglib.f90:1607), so column blocks can be
// handed to matvec/precnd callbacks unchanged.  n even => every column is 16-byte aligned and
// the kernels use 16-byte (double2) accesses (VEC=2); odd n falls back to 8-byte accesses (VEC=1).
//
// Kernels and what bounds them (all HBM-bound; arithmetic intensity k/4 flop/B):
//   gram_lds_kernel    C = X^T U          reads 8n(l+k) B     -- MFMA contracts over rows; full-line loads staged
//                      through wave-private LDS (even n); gram_kernel = direct fragment loads (odd n, tiny passes)
//   gemm_kernel        Z = XC, Z -= XC    reads 8n(l[+k]) B, writes 8nk B
//                      (also U <- U W in place for the Cholesky-QR triangular update)
//   ritz_kernel        evec = V Y, r = AV Y - theta evec, ||r||, max|r| in one sweep over V, AV
//   elementwise        axpy / sumsq / random fill / built-in operator + preconditioner
// The FP64 MFMA is used because it is the only way to contract a 16-wide column tile over
// rows held in different lanes without a shuffle storm; at k=13 it runs at ~1/3 of its peak
// when the kernel streams at HBM rate.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>
#include <cstring>
#include <ctime>
#include <map>
#include <set>
#include <vector>
#include "dla_internal.h"
#include "hip_owned.h"
#include "hip_plans.h"

using namespace dla_plans;   // the decisions (hip_plans.h); this file launches what they say

typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

// VEC doubles per lane per access: a scalar for VEC == 1, a 16-byte vector for VEC == 2
template <int V> struct VecOf;
template <> struct VecOf<1> { typedef double type; };
template <> struct VecOf<2> { typedef v2d type; };
template <int V> __device__ __forceinline__ double vget(const typename VecOf<V>::type& v, int e);
template <> __device__ __forceinline__ double vget<1>(const double& v, int) { return v; }
template <> __device__ __forceinline__ double vget<2>(const v2d& v, int e) { return e == 0 ? v.x : v.y; }
template <int V> __device__ __forceinline__ typename VecOf<V>::type vmake(double a, double b);
template <> __device__ __forceinline__ double vmake<1>(double a, double) { return a; }
template <> __device__ __forceinline__ v2d vmake<2>(double a, double b) { return (v2d){a, b}; }
template <int V> __device__ __forceinline__ typename VecOf<V>::type vzero() { return vmake<V>(0.0, 0.0); }
// streamed-once panel accesses: NT != 0 marks them non-temporal (no L2 retention wanted)
template <int V, int NT> __device__ __forceinline__ typename VecOf<V>::type pload(const double* p)
{
  typedef typename VecOf<V>::type vt;
  if constexpr (NT & 1) return __builtin_nontemporal_load((const vt*)p);
  else return *(const vt*)p;
}
// LDS images are written as 16-byte pairs and read back as single doubles by other lanes: both sides go through
// may_alias types so that type-based alias analysis cannot reorder them against each other
typedef double __attribute__((may_alias)) lds_f64;
typedef v2d __attribute__((may_alias)) lds_v2f64;
__device__ __forceinline__ void lds_store2(double* p, v2d v) { *(lds_v2f64*)p = v; }
__device__ __forceinline__ void lds_store1(double* p, double v) { *(lds_f64*)p = v; }
__device__ __forceinline__ double lds_load1(const double* p) { return *(const lds_f64*)p; }

template <int V, int NT> __device__ __forceinline__ void pstore(double* p, typename VecOf<V>::type v)
{
  typedef typename VecOf<V>::type vt;
  if constexpr (NT & 2) __builtin_nontemporal_store(v, (vt*)p);
  else *(vt*)p = v;
}

#define HIPCHK(call)                                                                  \
  do {                                                                                \
    hipError_t e_ = (call);                                                           \
    if (e_ != hipSuccess) {                                                           \
      err = std::string(#call) + ": " + hipGetErrorString(e_);                        \
      return DLA_ERR_RUNTIME;                                                         \
    }                                                                                 \
  } while (0)

// spmm_transpose_sort.hip: the stable sort of (key, value) pairs behind dla_spmm_transpose_prepare
namespace dla {
hipError_t sort_pairs_by_key(void* temp, size_t* temp_bytes, const int* key_in, int* key_out, const int* val_in, int* val_out,
                             size_t count, int key_bits, hipStream_t st);
}

namespace {

// ======================================================================================
// Gram / projection:  C(l x k) = X(n x l)^T U(n x k)
// ======================================================================================
// One wave owns a set of rows and ALL column tiles of this pass: TLW tiles (16 columns each)
// of X times KT tiles of U.  v_mfma_f64_16x16x4 computes D(16x16) += A(16x4) B(4x16) with the
// contraction index (4) spread over lane>>4; lane (c = lane&15, g = lane>>4) supplies
// A[c][g] = X[row(g)][col c] and B[g][c] = U[row(g)][col c].  Any row may sit in slot g as long
// as A and B agree, so each lane reads VEC consecutive rows (one 16-byte load for VEC=2):
// step s of a chunk covers rows  rbase + 4*VEC*s + VEC*g + e,  e < VEC.
// D layout (f64): lane holds D[(lane>>4) + 4*reg][lane&15], reg = 0..3.
struct GramArgs {
  const double* x;
  const double* u;
  double* partial;   // [pass][block][slot][256]
  long long n;
  int l, k;
  int passes_x;
  int lower;         // 1: only tile pairs on or below the block diagonal are needed (symmetric result, 'l' consumer)
  const int* phase;  // device-driven chains (ortho_chain): run only if *phase == want; nullptr = always
  int want;
  int noskip;        // A/B: issue the loads of fully padded column groups too (gram_lds_kernel)
  const double* wp;  // gram_lds_kernel WP: pending factor of the U block, packed [16][16] (wp[16 p + j] = W(p, j)); nullptr = identity
  double* uw;        // gram_lds_kernel WP: when set, the transformed tiles U W are also written back (the panel address of U)
  const double* cx;  // gram_lds_kernel WP == 2: the coefficient block C' of a projection sweep, packed [l4][16] (rows 0 .. l-1 belong to
                     // the columns of X, rows l .. l+k-1 to the columns of U, zero padded): the staged U tile is replaced by [X | U] C'
};

// A launch of a device-driven chain is speculative: the step it belongs to may not be the one the device-side state
// machine has reached (OrthoDev::phase).  Every block reads the same word, so the whole grid leaves together.
#define DLA_PREDICATED(a) do { if ((a).phase != nullptr && *(a).phase != (a).want) return; } while (0)

// (NT stays 0 here: the two 64-byte halves of a line are fetched by consecutive instructions and rely on
// the cache to merge; non-temporal loads measured -10 %)
// Quarter tiles.  v_mfma_f64_4x4x4 multiplies four independent 4x4x4 blocks in a quarter of the cycles of the 16x16x4 form
// (15 vs 60 measured, tools/mfma_probe.hip).  Lane (kk = lane>>4, blk = (lane>>2)&3, t = lane&3) supplies A[blk][t][kk] and
// B[blk][kk][t]; D[blk][i][j] comes back in lane 16 i + 4 blk + j.  With the SAME A value in all four blocks and the
// usual 16-wide fragment as B this is "4 columns of a 16x16x4 product": lane L receives D[4 qq + (L>>4)][L&15], exactly
// component qq of the 16x16x4 accumulator.  A block whose last 16-column tile holds only 4*QT live columns (37 = 32 + 5,
// 21 = 16 + 5) pays QT quarter instructions for that tile instead of a full one.
__device__ __forceinline__ double mfma_quarter(double a4, double b16, double acc)
{
  return __builtin_amdgcn_mfma_f64_4x4x4f64(a4, b16, acc, 0, 0, 0);
}

template <int TLW, int KT, int VEC, int RSTEP, int NT = 0, int PF = -1>
__global__ __launch_bounds__(256) void gram_kernel(GramArgs a)
{
  DLA_PREDICATED(a);
  constexpr int CH = 4 * VEC * RSTEP;  // rows per chunk
  constexpr bool PREFETCH = (PF < 0) ? (TLW * KT <= 12) : (PF != 0);   // A/B: also the 12-slot shapes gain (k = 37: +24 %)
  typedef typename VecOf<VEC>::type vec_t;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int xg = blockIdx.y % a.passes_x, ug = blockIdx.y / a.passes_x;
  const long long n = a.n;

  const double* xp[TLW];
  const double* up[KT];
#pragma unroll
  for (int t = 0; t < TLW; ++t) {
    int col = (xg * TLW + t) * 16 + c;
    col = col < a.l ? col : a.l - 1;           // clamp: garbage only reaches unused D rows
    xp[t] = a.x + (size_t)col * (size_t)n + VEC * g;
  }
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    int col = (ug * KT + t) * 16 + c;
    col = col < a.k ? col : a.k - 1;
    up[t] = a.u + (size_t)col * (size_t)n + VEC * g;
  }
  v4d acc[TLW][KT];
#pragma unroll
  for (int t = 0; t < TLW; ++t)
#pragma unroll
    for (int q = 0; q < KT; ++q) acc[t][q] = (v4d){0.0, 0.0, 0.0, 0.0};

  // Full chunks run through a two-stage software pipeline (the loads of the wave's next chunk are
  // in flight while the MFMAs of the current one issue); the single partial chunk at the end of the
  // panel, if any, is done by the wave it falls to with row predication.
  const long long nfull = n / CH;
  const long long stride = (long long)gridDim.x * 4;
  long long ch = (long long)blockIdx.x * 4 + wave;
  vec_t xv[TLW][RSTEP], uv[KT][RSTEP];
  auto load_chunk = [&](long long c, vec_t (&xd)[TLW][RSTEP], vec_t (&ud)[KT][RSTEP]) {
    const long long rbase = c * CH;
#pragma unroll
    for (int q = 0; q < KT; ++q)
#pragma unroll
      for (int s = 0; s < RSTEP; ++s) ud[q][s] = pload<VEC, NT>(up[q] + rbase + 4 * VEC * s);
#pragma unroll
    for (int t = 0; t < TLW; ++t)
#pragma unroll
      for (int s = 0; s < RSTEP; ++s) xd[t][s] = pload<VEC, NT>(xp[t] + rbase + 4 * VEC * s);
  };
  // tile pair (t, q) of this pass is wanted unless the caller asked for the lower block triangle only and the
  // X tile index is smaller than the U tile index (wave-uniform)
  bool want[TLW][KT];
  bool any_want = false;
#pragma unroll
  for (int t = 0; t < TLW; ++t)
#pragma unroll
    for (int q = 0; q < KT; ++q) {
      want[t][q] = !a.lower || (xg * TLW + t >= ug * KT + q);
      any_want = any_want || want[t][q];
    }
  auto mfma_chunk = [&](const vec_t (&xd)[TLW][RSTEP], const vec_t (&ud)[KT][RSTEP]) {
#pragma unroll
    for (int s = 0; s < RSTEP; ++s)
#pragma unroll
      for (int e = 0; e < VEC; ++e)
#pragma unroll
        for (int t = 0; t < TLW; ++t)
#pragma unroll
          for (int q = 0; q < KT; ++q)
            if (want[t][q])
              acc[t][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(vget<VEC>(xd[t][s], e), vget<VEC>(ud[q][s], e),
                                                               acc[t][q], 0, 0, 0);
  };
  if (!any_want) ch = (1LL << 62);   // whole pass above the diagonal: nothing to stream, zeros go out
  if constexpr (PREFETCH) {
    if (ch < nfull) {
      load_chunk(ch, xv, uv);
      for (; ch + stride < nfull; ch += stride) {
        vec_t xn[TLW][RSTEP], un[KT][RSTEP];
        load_chunk(ch + stride, xn, un);
        mfma_chunk(xv, uv);
#pragma unroll
        for (int t = 0; t < TLW; ++t)
#pragma unroll
          for (int s = 0; s < RSTEP; ++s) xv[t][s] = xn[t][s];
#pragma unroll
        for (int q = 0; q < KT; ++q)
#pragma unroll
          for (int s = 0; s < RSTEP; ++s) uv[q][s] = un[q][s];
      }
      mfma_chunk(xv, uv);
      ch += stride;
    }
  } else {
    for (; ch < nfull; ch += stride) {
      load_chunk(ch, xv, uv);
      mfma_chunk(xv, uv);
    }
  }
  if (ch == nfull && nfull * CH < n) {
    // tail chunk: rows >= n contribute zero (n even when VEC == 2, so pairs are all-in or all-out)
    const long long rbase = nfull * CH;
#pragma unroll
    for (int s = 0; s < RSTEP; ++s) {
      const bool ok = rbase + 4 * VEC * s + VEC * g < n;
#pragma unroll
      for (int q = 0; q < KT; ++q) {
        uv[q][s] = vzero<VEC>();
        if (ok) uv[q][s] = *(const vec_t*)(up[q] + rbase + 4 * VEC * s);
      }
#pragma unroll
      for (int t = 0; t < TLW; ++t) {
        xv[t][s] = vzero<VEC>();
        if (ok) xv[t][s] = *(const vec_t*)(xp[t] + rbase + 4 * VEC * s);
      }
    }
    mfma_chunk(xv, uv);
  }

  // deterministic in-block reduction over the 4 waves, one slot at a time
  __shared__ double red[4][256];
  double* pout = a.partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)(TLW * KT) * 256;
#pragma unroll
  for (int t = 0; t < TLW; ++t)
#pragma unroll
    for (int q = 0; q < KT; ++q) {
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][r * 64 + lane] = acc[t][q][r];
      __syncthreads();
      double s = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
      pout[(size_t)(t * KT + q) * 256 + threadIdx.x] = s;
      __syncthreads();
    }
}

// Same product with full-line loads: every lane loads 16 B of a 128-byte column segment (8 lanes per column,
// 8 columns per instruction), non-temporal, and the 16-row tile is staged through a wave-private LDS image
// [column][18] from which the MFMA fragments (lane (c, g): row 4s+g of column c) are read.  No block-level
// synchronisation inside the sweep; the next tile's loads are in flight while the current one is multiplied.
// Even n only (16-byte row pairs).
// SELF: U is X itself (Gram matrix of one block, TLW == KT, a single pass): the tiles are loaded and staged once and serve as
// both operands -- half the load instructions and LDS traffic of the general kernel on the same algorithmic bytes.
// QT > 0 (single U pass only): the last U tile -- for SELF the last tile of the block -- has 4*QT live columns and is multiplied
// by quarter instructions (mfma_quarter).  SELF puts the narrow tile on the A side, which lands in the standard
// accumulator layout; the general kernel has it on the B side, where lane L receives
// D[4 ((L>>2)&3) + (L>>4)][4 qq + (L&3)] -- put back in place when the accumulators go through LDS at the end.
// LOW: the whole lower block triangle of X^T U (l == k, x != u: the S^T A S of LOBPCG) in ONE pass -- the tile pairs above
// the diagonal are compiled out, so up to 7 x 7 tiles fit the accumulator registers (28 pairs) and both panels are read once.
// WP (one U tile, k <= 16): the U block in memory carries a PENDING right factor W (the triangular updates of the
// Cholesky-QR loop that have not been written back, see "pending factor" at ortho_tail16): every staged U tile is replaced
// by U W in LDS (4 MFMAs per 16 rows: D^T = W^T U^T, lane (c, g) reads U[row c][4 s + g] and writes (U W)[row c][g + 4 r]
// -- the same four LDS words, so no lane touches a word another lane reads) before the products are formed.  The values
// are those a triangular-update sweep would have stored (same instruction, same order); they are just never rounded to
// memory.  Without SELF the pass also forms (U W)^T (U W) as one extra output slot behind the TLW x KT slots of X^T (U W):
// X^T U and the Gram matrix of U in one sweep over [X | U].  With GramArgs::uw the transformed tiles are written back as well
// (full 128-byte column segments, straight from the staged image): the triangular update, the Gram matrix of its result
// and X^T of its result in ONE sweep, all three taken from the very values that reach memory.
// WP == 2 (one U tile, the whole of X in this one pass): the projection sweep of ortho_vs_x itself, U <- [X | U] C' (reference
// diaglib.f90:3544 with the pending triangular factor folded in, see OP_COMBOX).  A wave's 16 (32) rows of ALL columns of [X | U]
// sit in its staged image, so the new U tile is (l + k) / 4 MFMAs away (D^T = C'^T [X | U]^T, the coefficients C'(4 s + g, c) in
// registers for the whole sweep); it replaces the U tile in the image, goes to memory, and X^T U_new / U_new^T U_new are formed from
// the very values that were stored -- the measurement the NEXT projection (or the closing one) needs, without another pass over X.
template <int TLW, int KT, int NT = 1, int R = 16, int SELF = 0, int QT = 0, int LOW = 0, int WP = 0>
__global__ __launch_bounds__(256) void gram_lds_kernel(GramArgs a)
{
  DLA_PREDICATED(a);
  static_assert(!WP || (QT == 0 && LOW == 0 && KT <= 3 && (KT == 1 || (!SELF && R == 16))), "pending factor: up to three U tiles");
  static_assert(WP != 2 || (KT == 1 && !SELF), "projection sweep: one U tile beside the X tiles");
  constexpr int UU = (WP && !SELF) ? KT * (KT + 1) / 2 : 0;   // extra output slots: the tiles (qi >= qj) of (U W)^T (U W)
  constexpr int NSLOT = TLW * KT + UU;
  // R rows per wave tile (16 or 32): R/2 lanes cover one column segment, 128/R columns per load instruction
  constexpr int RS = R + 2;                // doubles per staged column (+2 keeps 16-byte alignment)
  constexpr int LPC = R / 2;               // lanes per column
  constexpr int CPI = 64 / LPC;            // columns per load instruction
  constexpr int NC = SELF ? 16 * TLW : 16 * (TLW + KT);      // staged columns: the pass's X tiles, then its U tiles
  constexpr int UOFF = SELF ? 0 : 16 * TLW;                   // where the U tiles sit in the staged image
  constexpr int NI = NC / CPI;             // load instructions per tile
  extern __shared__ __attribute__((aligned(16))) double glds[];   // [4][NC][RS]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* my = glds + (size_t)wave * NC * RS;
  const int c = lane & 15, g = lane >> 4;
  const int li = lane % LPC, lc = lane / LPC;
  const int xg = blockIdx.y % a.passes_x, ug = blockIdx.y / a.passes_x;
  const long long n = a.n;

  // tile pairs this pass forms: both tiles must hold columns of their block, and with `lower` the pair must lie on or
  // below the block diagonal
  v4d acc[TLW][KT];
  bool want[TLW][KT];
  bool any_want = false;
  unsigned tile_used = 0;                  // staged tiles some wanted pair reads (bit = staged tile index)
#pragma unroll
  for (int t = 0; t < TLW; ++t)
#pragma unroll
    for (int q = 0; q < KT; ++q) {
      acc[t][q] = (v4d){0.0, 0.0, 0.0, 0.0};
      const int xt = xg * TLW + t, ut = ug * KT + q;
      want[t][q] = (16 * xt < a.l) && (16 * ut < a.k) && (LOW ? (t >= q) : (!a.lower || xt >= ut));
      any_want = any_want || want[t][q];
      if (want[t][q]) tile_used |= (1u << t) | (1u << (SELF ? q : TLW + q));
    }
  // staged column j*CPI + lc of this lane -> panel column (clamped: garbage only reaches unused rows/columns of D).
  // Load instructions whose columns all lie beyond the block (40..47 of a 37-column block), or in a tile no wanted pair
  // reads (the tiles above the diagonal of a `lower` pass), fetch nothing new: all their lanes read one fixed 16-byte
  // word (a single request instead of eight 128-byte lines).  No control flow: a test per instruction splits the load
  // clause and cost the narrow passes 5-20 %.
  const double* cp[NI];
  unsigned skip = 0;
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int sc = CPI * j + lc;
    if (!(tile_used & (1u << ((CPI * j) / 16)))) skip |= 1u << j;
    if (sc < 16 * TLW) {
      int col = xg * TLW * 16 + sc;
      if (xg * TLW * 16 + CPI * j >= a.l) skip |= 1u << j;
      col = col < a.l ? col : a.l - 1;
      cp[j] = a.x + (size_t)col * (size_t)n + 2 * li;
    } else {
      int col = ug * KT * 16 + (sc - 16 * TLW);
      if (ug * KT * 16 + (CPI * j - 16 * TLW) >= a.k) skip |= 1u << j;
      col = col < a.k ? col : a.k - 1;
      cp[j] = a.u + (size_t)col * (size_t)n + 2 * li;
    }
  }
  if (a.noskip & 1) skip = 0;
  long long rmul[NI];                      // row advance of the instruction: 1, or 0 for the pinned ones
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    rmul[j] = 1;
    if (skip & (1u << j)) { rmul[j] = 0; cp[j] = a.x; }
  }
  const int i4 = lane & 3;
  // quarter tiles' accumulators, scalars of their own (see gemm_kernel): SELF [U tile][quarter], else [X tile][quarter]
  double accq[SELF ? KT : TLW][QT > 0 ? QT : 1];
#pragma unroll
  for (int t = 0; t < (SELF ? KT : TLW); ++t)
#pragma unroll
    for (int qq = 0; qq < (QT > 0 ? QT : 1); ++qq) accq[t][qq] = 0.0;
  v4d accuu[UU > 0 ? UU : 1];
#pragma unroll
  for (int e = 0; e < (UU > 0 ? UU : 1); ++e) accuu[e] = (v4d){0.0, 0.0, 0.0, 0.0};
  // A operands of the tile transform: W(16 p + 4 s + g, 16 q + c) for the tile pairs p <= q (W is upper triangular).
  // One tile: wp is the 16 x 16 image ortho_tail16 writes; more: the packed [KT][k4][16] image of ortho_tail (rows >= k4 are not there)
  double wa[WP == 1 ? KT * (KT + 1) / 2 : 1][WP == 1 ? 4 : 1];
  // WP == 2: A operands of the projection, C'(row of staged column 4 s + g, c); staged columns beyond the block get a zero
  double ca[WP == 2 ? 4 * (TLW + 1) : 1];
  if constexpr (WP == 2) {
#pragma unroll
    for (int s = 0; s < 4 * (TLW + 1); ++s) {
      const int sc = 4 * s + g;
      const int row = sc < 16 * TLW ? (sc < a.l ? sc : -1) : (sc - 16 * TLW < a.k ? a.l + sc - 16 * TLW : -1);
      ca[s] = row >= 0 ? a.cx[(size_t)row * 16 + c] : 0.0;
    }
  }
  if constexpr (WP == 1) {
    const int k4w = ((a.k + 3) / 4) * 4;
#pragma unroll
    for (int q = 0; q < KT; ++q)
#pragma unroll
      for (int p = 0; p <= q; ++p)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int pp = 16 * p + 4 * s + g;
          double v = (pp == 16 * q + c) ? 1.0 : 0.0;
          if (a.wp) v = (KT == 1) ? a.wp[pp * 16 + c] : (pp < k4w ? a.wp[((size_t)q * k4w + pp) * 16 + c] : 0.0);
          wa[q * (q + 1) / 2 + p][s] = v;
        }
  }
  typedef VecOf<2>::type vec_t;
  vec_t stg[NI];
  auto load_tile = [&](long long tile) {
    const long long r0 = tile * R;
    if constexpr (LOW) {
      // 28 load instructions per tile: their 56 address registers are recomputed instead of kept (the accumulators of the
      // 28 tile pairs need the room); l == k, one pass, nothing pinned except whole padding groups
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const int sc = CPI * j + lc;
        const bool isx = sc < 16 * TLW;
        int col = isx ? sc : sc - 16 * TLW;
        col = col < a.l ? col : a.l - 1;
        const double* base = isx ? a.x : a.u;
        const bool pin = (isx ? CPI * j : CPI * j - 16 * TLW) >= a.l;
        stg[j] = pload<2, NT>(pin ? a.x : base + (size_t)col * (size_t)n + 2 * li + r0);
      }
    } else {
#pragma unroll
      for (int j = 0; j < NI; ++j) stg[j] = pload<2, NT>(cp[j] + r0 * rmul[j]);
    }
  };
  auto stage_tile = [&]() {
#pragma unroll
    for (int j = 0; j < NI; ++j) lds_store2(my + (size_t)(CPI * j + lc) * RS + 2 * li, stg[j]);
  };
  constexpr int KF = (QT > 0 && !SELF) ? KT - 1 : KT;     // U tiles multiplied by full instructions
  constexpr int TF = (QT > 0 && SELF) ? TLW - 1 : TLW;    // X tiles ...
  // WP: staged U tile <- (U tile) W, 16 rows at a time
  auto apply_w = [&](long long r0w, bool rows_ok) {
    if constexpr (WP) {
      if (WP == 1 && a.wp == nullptr && a.uw == nullptr) return;      // nothing pending: the staged tile is the block itself
      // (all fragment reads first, then the MFMA chains of the R / 16 row groups side by side, then the stores)
      double* ut = my + (size_t)UOFF * RS + c;
      if constexpr (WP == 2) {
        // U_new[row c][g + 4 r] = sum over the staged columns j of [X | U][row c][j] C'(j, g + 4 r)
        v4d d[R / 16];
#pragma unroll
        for (int h = 0; h < R / 16; ++h) d[h] = (v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4 * (TLW + 1); ++s)
#pragma unroll
          for (int h = 0; h < R / 16; ++h)
            d[h] = __builtin_amdgcn_mfma_f64_16x16x4f64(ca[s], lds_load1(my + (size_t)(4 * s + g) * RS + c + 16 * h), d[h], 0, 0, 0);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int h = 0; h < R / 16; ++h)
#pragma unroll
          for (int r = 0; r < 4; ++r) lds_store1(ut + (size_t)(g + 4 * r) * RS + 16 * h, d[h][r]);
      } else if constexpr (KT == 1) {
        double uin[R / 16][4];
#pragma unroll
        for (int h = 0; h < R / 16; ++h)
#pragma unroll
          for (int s = 0; s < 4; ++s) uin[h][s] = lds_load1(ut + (size_t)(4 * s + g) * RS + 16 * h);
        v4d d[R / 16];
#pragma unroll
        for (int h = 0; h < R / 16; ++h) d[h] = (v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int h = 0; h < R / 16; ++h) d[h] = __builtin_amdgcn_mfma_f64_16x16x4f64(wa[0][s], uin[h][s], d[h], 0, 0, 0);
#pragma unroll
        for (int h = 0; h < R / 16; ++h)
#pragma unroll
          for (int r = 0; r < 4; ++r) lds_store1(ut + (size_t)(g + 4 * r) * RS + 16 * h, d[h][r]);
      } else {
        // several tiles (R == 16): output tile q = sum over the input tiles p <= q; every fragment is read before anything is
        // stored (an output tile overwrites an input tile other output tiles have read)
        double uin[KT][4];
#pragma unroll
        for (int p = 0; p < KT; ++p)
#pragma unroll
          for (int s = 0; s < 4; ++s) uin[p][s] = lds_load1(ut + (size_t)(16 * p + 4 * s + g) * RS);
        v4d d[KT];
#pragma unroll
        for (int q = 0; q < KT; ++q) {
          d[q] = (v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int p = 0; p <= q; ++p)
#pragma unroll
            for (int s = 0; s < 4; ++s) d[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(wa[q * (q + 1) / 2 + p][s], uin[p][s], d[q], 0, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < KT; ++q)
#pragma unroll
          for (int r = 0; r < 4; ++r) lds_store1(ut + (size_t)(16 * q + g + 4 * r) * RS, d[q][r]);
      }
      __builtin_amdgcn_wave_barrier();
      if (a.uw != nullptr && rows_ok) {
        // the wave's own rows of the block: 128-byte segments of CPI columns per instruction
#pragma unroll
        for (int j = (16 * (SELF ? 0 : TLW)) / CPI; j < NI; ++j) {
          const int uc = CPI * j + lc - UOFF;
          if (uc < a.k) pstore<2, 0>(a.uw + (size_t)uc * (size_t)n + r0w + 2 * li, *(const lds_v2f64*)(my + (size_t)(CPI * j + lc) * RS + 2 * li));
        }
      }
    }
  };
  auto mfma_tile = [&]() {
#pragma unroll
    for (int s4 = 0; s4 < R / 4; ++s4) {
      double uf[KT];
#pragma unroll
      for (int q = 0; q < (SELF ? KT : KF); ++q) uf[q] = lds_load1(my + (size_t)(UOFF + 16 * q + c) * RS + 4 * s4 + g);
      if constexpr (UU > 0) {
#pragma unroll
        for (int qi = 0; qi < KT; ++qi)
#pragma unroll
          for (int qj = 0; qj <= qi; ++qj)
            accuu[qi * (qi + 1) / 2 + qj] = __builtin_amdgcn_mfma_f64_16x16x4f64(uf[qi], uf[qj], accuu[qi * (qi + 1) / 2 + qj], 0, 0, 0);
      }
      double uq[QT > 0 ? QT : 1];
      if constexpr (QT > 0 && !SELF) {
#pragma unroll
        for (int qq = 0; qq < QT; ++qq) uq[qq] = lds_load1(my + (size_t)(UOFF + 16 * KF + 4 * qq + i4) * RS + 4 * s4 + g);
      }
#pragma unroll
      for (int t = 0; t < TF; ++t) {
        const double xf = lds_load1(my + (size_t)(16 * t + c) * RS + 4 * s4 + g);
#pragma unroll
        for (int q = 0; q < KF; ++q)
          if (want[t][q]) acc[t][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(xf, uf[q], acc[t][q], 0, 0, 0);
        if constexpr (QT > 0 && !SELF) {
#pragma unroll
          for (int qq = 0; qq < QT; ++qq)
            if (want[t][KT - 1]) accq[t][qq] = mfma_quarter(xf, uq[qq], accq[t][qq]);
        }
      }
      if constexpr (QT > 0 && SELF) {
#pragma unroll
        for (int qq = 0; qq < QT; ++qq) {
          const double xq = lds_load1(my + (size_t)(16 * TF + 4 * qq + i4) * RS + 4 * s4 + g);
#pragma unroll
          for (int q = 0; q < KT; ++q) accq[q][qq] = mfma_quarter(xq, uf[q], accq[q][qq]);
        }
      }
    }
  };
  const long long nfull = n / R;
  const long long stride = (long long)gridDim.x * 4;
  long long tile = (long long)blockIdx.x * 4 + wave;
  if (!any_want) tile = (1LL << 62);
  if (tile < nfull) {
    load_tile(tile);
    for (;;) {
      stage_tile();
      __builtin_amdgcn_wave_barrier();
      const long long next = tile + stride;
      if (next < nfull) load_tile(next);
      apply_w(tile * R, true);
      mfma_tile();
      __builtin_amdgcn_wave_barrier();
      tile = next;
      if (next >= nfull) break;
    }
  }
  if (tile == nfull && nfull * R < n) {
    // tail tile: rows >= n contribute zero (n even: a 16-byte row pair is all-in or all-out)
    const long long r0 = nfull * R;
    const bool ok = r0 + 2 * li < n;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      stg[j] = vzero<2>();
      if (ok) stg[j] = *(const vec_t*)(cp[j] + r0 * rmul[j]);
    }
    stage_tile();
    __builtin_amdgcn_wave_barrier();
    apply_w(r0, ok);
    mfma_tile();
    __builtin_amdgcn_wave_barrier();
  }

  // deterministic in-block reduction over the 4 waves, one slot at a time (the staging area is free now)
  __syncthreads();
  double* red = glds;   // [4][256]
  double* pout = a.partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)NSLOT * 256;
  if constexpr (UU > 0) {
#pragma unroll
    for (int e = 0; e < UU; ++e) {
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave * 256 + r * 64 + lane] = accuu[e][r];
      __syncthreads();
      pout[(size_t)(TLW * KT + e) * 256 + threadIdx.x] = ((red[threadIdx.x] + red[256 + threadIdx.x]) + red[512 + threadIdx.x]) + red[768 + threadIdx.x];
      __syncthreads();
    }
  }
#pragma unroll
  for (int t = 0; t < TLW; ++t)
#pragma unroll
    for (int q = 0; q < KT; ++q) {
      if (LOW && t < q) {                       // never formed: zeros go out
        pout[(size_t)(t * KT + q) * 256 + threadIdx.x] = 0.0;
        continue;
      }
      if (QT > 0 && !SELF && q == KT - 1) {
        // quarter results back to the standard layout: (row 4 blk + i', column 4 qq + j) lives in component blk of lane 16 i' + 4 qq + j
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave * 256 + r * 64 + lane] = 0.0;
#pragma unroll
        for (int qq = 0; qq < QT; ++qq) red[wave * 256 + ((lane >> 2) & 3) * 64 + 16 * g + 4 * qq + i4] = accq[t][qq];
      } else if (QT > 0 && SELF && t == TLW - 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave * 256 + r * 64 + lane] = r < QT ? accq[q][r < QT ? r : 0] : 0.0;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave * 256 + r * 64 + lane] = acc[t][q][r];
      }
      __syncthreads();
      double sum = ((red[threadIdx.x] + red[256 + threadIdx.x]) + red[512 + threadIdx.x]) + red[768 + threadIdx.x];
      pout[(size_t)(t * KT + q) * 256 + threadIdx.x] = sum;
      __syncthreads();
    }
}

// ======================================================================================
// Panel products along rows:  Z = X C  |  Z -= X C  |  U <- U W (in place)
// ======================================================================================
// Transposed formulation D^T = C^T X^T so that the 16-lane index follows ROWS (coalesced):
// lane (i = lane&15, g = lane>>4) loads rows r0 + VEC*i + e of column 4*cs + g (B operand,
// 16 B per lane, 256 B contiguous per 16 lanes); the A operand is C[4cs+g][16q + i] read from
// the LDS copy of C.  D layout: lane holds Z[row(i)][16q + g + 4*reg]; the VEC row values of
// one (q,reg) are stored with one 16-byte store.
struct GemmArgs {
  const double* x;     // n x l
  const double* cpk;   // packed C: [KT][l4][16] (zero padded), device
  double* z;           // n x k
  double* gpart;       // GRAM variants: per-block partial of Z^T Z, [nblk][256]
  long long n;
  int l, l4, k;
  const int* phase;    // see DLA_PREDICATED
  int want;
  int xpf;             // 1: the first column stage of a wave's next row tile is loaded before the epilogue of the current one
};

// small C (l <= 16, k <= 16) travels inside the kernel arguments: no staging copy, no extra launch
struct GemmArgsInl {
  const double* x;
  double* z;
  double* gpart;
  long long n;
  int l, l4, k;
  const int* phase;
  int want;
  int xpf;
  double cin[256];     // packed C: [l4 <= 16][16]
};
__device__ __forceinline__ const double* packed_c(const GemmArgs& a) { return a.cpk; }
__device__ __forceinline__ const double* packed_c(const GemmArgsInl& a) { return a.cin; }

// MODE 0: Z = XC   1: Z -= XC   2: in place U <- U W (x == z)   3: Z += XC
// GRAM: the same sweep also accumulates G = Z^T Z of the values it stores (lower block triangle) -- the next
// Gram matrix of the Cholesky-QR loop (diaglib.f90:3256) without re-reading the panel.  The stored
// rows of a 16*VEC-row group are transposed through a wave-private LDS tile (row stride 24 doubles:
// conflict-free for the fragment reads) into MFMA operands: lane (c, g) reads Z[row(g)][c].
// NT: X is read once per sweep -> non-temporal loads (+16..25 % measured on Z = XC / U -= XC, tools/tune_ab.py);
// the in-place triangular update (MODE 2) stays plain: non-temporal loads there measured +1..9 % right behind a projection
// sweep over the whole basis and -0.4..+0.7 % on whole solves, where it mostly follows a sweep over the same block.
// PIPE > 0 (used for KT >= 2, where 4*KT MFMAs follow every load and the kernel runs at 1-2 waves per SIMD; 2 steps for
// two-tile blocks -- 3 and 4 measured equal or worse there -- and for the plain three-tile products, which would lose
// their second wave per SIMD to a third step; 3 for the fused three-tile sweeps and the three-tile Ritz step, which run
// one wave per SIMD anyway: +6 % and +3 % against 2):
// column steps are processed PIPE at a time through a two-stage register pipeline -- the loads of the next
// stage are in flight while the MFMAs of the current one issue.  For KT == 1 occupancy hides the latency
// better than registers do (A/B: batching there costs 5-10 %).
// QT > 0: the last tile has only 4*QT live columns and is formed by quarter instructions (see mfma_quarter).
template <int KT, int VEC, int MODE, typename ARGS, bool GRAM = false, int NT = (MODE == 2 ? 0 : 1), int PIPE = (KT >= 2 ? 2 : 0), int ZPAD = 9,
          int QT = 0, int RTP = 2>
__global__ __launch_bounds__(256) void gemm_kernel(ARGS a)
{
  DLA_PREDICATED(a);
  constexpr int RT = RTP;                  // row groups per wave tile
  constexpr int RG = 16 * VEC;             // rows per group
  constexpr int WT = RT * RG;              // rows per wave tile (64 for VEC=2)
  extern __shared__ __attribute__((aligned(16))) double cs[];  // [KT][l4][16]
  typedef typename VecOf<VEC>::type vec_t;
  const long long n = a.n;
  const int l = a.l, l4 = a.l4;
  constexpr int KF = QT > 0 ? KT - 1 : KT;   // tiles formed by full 16x16x4 instructions
  // LDS copy of C: the full tiles as packed, [KF][l4][16]; of a quarter-tile block's last tile only the 8 leading columns,
  // [l4][8] (a 148-row C' of the [X | U] sweep at k = 37 then leaves room for two blocks per CU)
  const int csz = KF * l4 * 16 + (QT > 0 ? l4 * 8 : 0);
  {
    const double* csrc = packed_c(a);
    for (int idx = threadIdx.x; idx < KF * l4 * 16; idx += 256) cs[idx] = csrc[idx];
    if constexpr (QT > 0) {
      for (int idx = threadIdx.x; idx < l4 * 8; idx += 256) cs[KF * l4 * 16 + idx] = csrc[KF * l4 * 16 + (idx >> 3) * 16 + (idx & 7)];
    }
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int i4 = lane & 3;                  // quarter tiles: column of the 4-column group this lane's A value belongs to
  const long long ntiles = (n + WT - 1) / WT;
  const int nsteps = l4 / 4;
  // LDS row stride of the transpose tile (doubles).  The fragment reads run along a row (16 lanes, 128 contiguous
  // bytes) and are conflict-free for any stride; the tile WRITES put the 16 lanes of a group on 16 rows of one
  // column, ZS doubles apart: an odd ZS spreads them over all banks.  (The first version used 16*KT + 8 with rows
  // 2 apart: all 16 lanes on one bank, measured as 25 % LDS-issue stall in the 13-column TRMM+Gram sweep.)
  constexpr int ZS = 16 * KT + ZPAD;
  double* zs = cs + (size_t)csz + (size_t)wave * 16 * ZS;            // [16 rows][ZS] per wave (GRAM only)
  v4d gacc[KT][KT];                                        // tile (qa, qb) of Z^T Z, qa >= qb only
#pragma unroll
  for (int qa = 0; qa < KT; ++qa)
#pragma unroll
    for (int qb = 0; qb < KT; ++qb) gacc[qa][qb] = (v4d){0.0, 0.0, 0.0, 0.0};
  double gaccq[KT][QT > 0 ? QT : 1];                       // quarter rows of the last block row of G
#pragma unroll
  for (int qb = 0; qb < KT; ++qb)
#pragma unroll
    for (int qq = 0; qq < (QT > 0 ? QT : 1); ++qq) gaccq[qb][qq] = 0.0;

  // PIPE > 0: the first column stage of this wave's NEXT row tile, in flight while the epilogue of the current one
  // (stores, and for GRAM the transposes and 4..6 more MFMAs per row group) runs
  vec_t xnext[PIPE > 0 ? PIPE : 1][RT];
  bool have_next = false;
  for (long long tile = (long long)blockIdx.x * 4 + wave; tile < ntiles; tile += (long long)gridDim.x * 4) {
    const long long r0 = tile * WT;
    v4d acc[RT][VEC][KT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int e = 0; e < VEC; ++e)
#pragma unroll
        for (int q = 0; q < KT; ++q) acc[rt][e][q] = (v4d){0.0, 0.0, 0.0, 0.0};
    // the quarter tiles' accumulators are scalars of their own (as components of a v4d the compiler shuttles the whole
    // tuple between AGPRs and VGPRs around every quarter instruction)
    double accq[RT][VEC][QT > 0 ? QT : 1];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int e = 0; e < VEC; ++e)
#pragma unroll
        for (int qq = 0; qq < (QT > 0 ? QT : 1); ++qq) accq[rt][e][qq] = 0.0;
    auto accv = [&](int rt, int e, int q, int reg) -> double {
      if (QT > 0 && q == KF) return reg < QT ? accq[rt][e][reg < QT ? reg : 0] : 0.0;
      return acc[rt][e][q][reg];
    };

    long long row[RT];
    bool rok[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      row[rt] = r0 + rt * RG + VEC * i;
      rok[rt] = row[rt] < n;               // n even for VEC == 2: the pair is all-in or all-out
      if (!rok[rt]) row[rt] = 0;           // clamp to a valid address; result discarded
    }
    int cs4 = 0;
    if constexpr (PIPE > 0) {
      const int nfull4 = l / 4;                 // steps whose 4 columns all exist
      auto load_stage = [&](int c0, vec_t (&xs)[PIPE][RT]) {
#pragma unroll
        for (int u4 = 0; u4 < PIPE; ++u4) {
          const double* xc = a.x + (size_t)(4 * (c0 + u4) + g) * (size_t)n;
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) xs[u4][rt] = pload<VEC, NT>(xc + row[rt]);
        }
      };
      auto mfma_stage = [&](int c0, const vec_t (&xs)[PIPE][RT]) {
#pragma unroll
        for (int u4 = 0; u4 < PIPE; ++u4) {
          double cfu[KT];
#pragma unroll
          for (int q = 0; q < KF; ++q) cfu[q] = cs[(size_t)q * l4 * 16 + (size_t)(4 * (c0 + u4) + g) * 16 + i];
          double cfq[QT > 0 ? QT : 1];
#pragma unroll
          for (int qq = 0; qq < QT; ++qq) cfq[qq] = cs[(size_t)KF * l4 * 16 + (size_t)(4 * (c0 + u4) + g) * 8 + 4 * qq + i4];
#pragma unroll
          for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
#pragma unroll
              for (int q = 0; q < KF; ++q)
                acc[rt][e][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(cfu[q], vget<VEC>(xs[u4][rt], e), acc[rt][e][q], 0, 0, 0);
#pragma unroll
              for (int qq = 0; qq < QT; ++qq)
                accq[rt][e][qq] = mfma_quarter(cfq[qq], vget<VEC>(xs[u4][rt], e), accq[rt][e][qq]);
            }
        }
      };
      if (PIPE <= nfull4) {
        vec_t xa[PIPE][RT];
        if (have_next) {
#pragma unroll
          for (int u4 = 0; u4 < PIPE; ++u4)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) xa[u4][rt] = xnext[u4][rt];
        } else {
          load_stage(0, xa);
        }
        for (; cs4 + 2 * PIPE <= nfull4; cs4 += PIPE) {
          vec_t xb[PIPE][RT];
          load_stage(cs4 + PIPE, xb);
          mfma_stage(cs4, xa);
#pragma unroll
          for (int u4 = 0; u4 < PIPE; ++u4)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) xa[u4][rt] = xb[u4][rt];
        }
        mfma_stage(cs4, xa);
        cs4 += PIPE;
      }
    }
    for (; cs4 < nsteps; ++cs4) {
      int col = 4 * cs4 + g;
      const bool cok = col < l;
      col = cok ? col : l - 1;
      const double* xc = a.x + (size_t)col * (size_t)n;
      vec_t xv[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        vec_t v = pload<VEC, NT>(xc + row[rt]);
        xv[rt] = cok ? v : vzero<VEC>();
      }
      double cf[KT];
#pragma unroll
      for (int q = 0; q < KF; ++q) cf[q] = cs[(size_t)q * l4 * 16 + (size_t)(4 * cs4 + g) * 16 + i];
      double cfq[QT > 0 ? QT : 1];
#pragma unroll
      for (int qq = 0; qq < QT; ++qq) cfq[qq] = cs[(size_t)KF * l4 * 16 + (size_t)(4 * cs4 + g) * 8 + 4 * qq + i4];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
#pragma unroll
          for (int q = 0; q < KF; ++q)
            acc[rt][e][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(cf[q], vget<VEC>(xv[rt], e), acc[rt][e][q], 0, 0, 0);
#pragma unroll
          for (int qq = 0; qq < QT; ++qq)
            accq[rt][e][qq] = mfma_quarter(cfq[qq], vget<VEC>(xv[rt], e), accq[rt][e][qq]);
        }
    }
    if constexpr (PIPE > 0) {
      have_next = false;
      const long long ntile = tile + (long long)gridDim.x * 4;
      if (a.xpf && PIPE <= l / 4 && ntile < ntiles) {
        // (in place, MODE 2: the next tile's rows are not this tile's rows, nothing stored below is read here)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          long long nr = ntile * WT + rt * RG + VEC * i;
          if (nr >= n) nr = 0;
#pragma unroll
          for (int u4 = 0; u4 < PIPE; ++u4) xnext[u4][rt] = pload<VEC, NT>(a.x + (size_t)(4 * u4 + g) * (size_t)n + nr);
        }
        have_next = true;
      }
    }
    // epilogue
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      if (!GRAM && !rok[rt]) continue;
      vec_t vkeep[KT][4];
#pragma unroll
      for (int q = 0; q < KT; ++q)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int j = 16 * q + g + 4 * reg;
          vec_t v = vzero<VEC>();
          if (rok[rt] && j < a.k) {
            double* zp = a.z + (size_t)j * (size_t)n + row[rt];
            v = vmake<VEC>(accv(rt, 0, q, reg), accv(rt, VEC - 1, q, reg));
            // (loading the old values ahead of the sweep costs 32 VGPRs = 3 waves per SIMD and is slower)
            if constexpr (MODE == 1) { vec_t old = *(const vec_t*)zp; v = old - v; }
            if constexpr (MODE == 3) { vec_t old = *(const vec_t*)zp; v = old + v; }
            pstore<VEC, NT>(zp, v);
          }
          vkeep[q][reg] = v;
        }
      if constexpr (GRAM) {
        // 16 stored rows at a time (row e of every lane's pair) go through the wave-private tile: lane (i, g)
        // writes Z[row i][16q + g + 4 reg], lane (c, g) reads Z[row 4 s4 + g][16q + c] as MFMA operands
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
#pragma unroll
          for (int q = 0; q < KT; ++q)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) zs[i * ZS + 16 * q + g + 4 * reg] = vget<VEC>(vkeep[q][reg], e);
          __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4) {
            double zv[KT];
#pragma unroll
            for (int q = 0; q < KT; ++q) zv[q] = zs[(4 * s4 + g) * ZS + 16 * q + i];
#pragma unroll
            for (int qa = 0; qa < KF; ++qa)
#pragma unroll
              for (int qb = 0; qb <= qa; ++qb)
                gacc[qa][qb] = __builtin_amdgcn_mfma_f64_16x16x4f64(zv[qa], zv[qb], gacc[qa][qb], 0, 0, 0);
            // rows 4 qq .. 4 qq + 3 of the last block row of G: 4 columns of Z as A, the usual fragments as B
#pragma unroll
            for (int qq = 0; qq < QT; ++qq) {
              const double za = zs[(4 * s4 + g) * ZS + 16 * KF + 4 * qq + i4];
#pragma unroll
              for (int qb = 0; qb < KT; ++qb) gaccq[qb][qq] = mfma_quarter(za, zv[qb], gaccq[qb][qq]);
            }
          }
          __builtin_amdgcn_wave_barrier();
        }
      }
    }
  }
  if constexpr (GRAM) {
    // deterministic sum over the 4 waves, one tile at a time; partial layout = KT x KT slots of a 1-pass Gram
    // (slot qa*KT + qb; the upper block triangle is sent as zeros and mirrored on the host)
    double* red = cs;   // the copy of C is no longer needed: 4 x 256 doubles
    const int t = threadIdx.x;
#pragma unroll
    for (int qa = 0; qa < KT; ++qa)
#pragma unroll
      for (int qb = 0; qb < KT; ++qb) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r)
          red[wave * 256 + r * 64 + lane] = (QT > 0 && qa == KF) ? (r < QT ? gaccq[qb][r < QT ? r : 0] : 0.0) : gacc[qa][qb][r];
        __syncthreads();
        a.gpart[((size_t)blockIdx.x * (KT * KT) + (qa * KT + qb)) * 256 + t] =
            ((red[t] + red[256 + t]) + red[512 + t]) + red[768 + t];
      }
  }
}

// ======================================================================================
// Fused Ritz step: evec = V Y, r = AV Y, r_j -= theta_j evec_j (active j), sum r^2, max |r|
// (optionally also the uncorrected AV Y, which LOBPCG keeps as ax_new)
// ======================================================================================
struct RitzArgs {
  const double* v;     // n x l
  const double* av;    // n x l
  const double* cpk;   // packed Y: [KT][l4][16]
  double* evec;        // n x k
  double* r;           // n x k
  double* avy;         // n x k or nullptr
  double* red;         // block partials [nblk][16*KT][2]
  long long n;
  int l, l4, k;
  // extra products of the same sweep (LOBPCG's P block): columns k .. k+k2-1 of the packed coefficient block give
  // p2 = V C2 and ap2 = AV C2 -- no residual correction, no norms
  double* p2;
  double* ap2;
  int k2;
  double theta[48];
  int active[48];
};

// NT = 3: V / AV are read once and evec / r written once per sweep -> non-temporal loads and stores
// (+6 % measured, tools/tune_ab.py)
// XP: the coefficient block carries extra product columns behind the k Ritz columns (RitzArgs::k2); a template argument so
// that the plain Ritz step keeps its code (the same tests as run-time branches cost the one-tile kernel 37 %)
// RESERVED: always 0.  It once chose among hand-scheduled loops (none faster, profiles/r04/ritz_sched_ab.txt); it stays because the
// benchmark and profiles/pmc_traffic.json key on the seven-argument kernel names
template <int KT, int VEC, int NT = 3, int PIPE = (KT >= 3 ? 3 : KT >= 2 ? 2 : 0), int QT = 0, bool XP = false, int RESERVED = 0>
__global__ __launch_bounds__(256) void ritz_kernel(RitzArgs a)
{
  static_assert(RESERVED == 0, "ritz_kernel: the seventh template argument only keeps the kernel's name");
  constexpr int RG = 16 * VEC;             // rows per wave tile (one row group)
  extern __shared__ __attribute__((aligned(16))) double cs[];  // [KT][l4][16], later reduction scratch
  typedef typename VecOf<VEC>::type vec_t;
  const long long n = a.n;
  const int l = a.l, l4 = a.l4;
  constexpr int KF = QT > 0 ? KT - 1 : KT;   // full tiles; the last tile has 4*QT live columns (see mfma_quarter)
  for (int idx = threadIdx.x; idx < KF * l4 * 16; idx += 256) cs[idx] = a.cpk[idx];
  if constexpr (QT > 0) {                    // ... and keeps only its 8 leading columns in LDS, [l4][8] (see gemm_kernel)
    for (int idx = threadIdx.x; idx < l4 * 8; idx += 256) cs[KF * l4 * 16 + idx] = a.cpk[KF * l4 * 16 + (idx >> 3) * 16 + (idx & 7)];
  }
  __shared__ double s_theta[48];
  __shared__ int s_active[48];
  if (threadIdx.x < 48) { s_theta[threadIdx.x] = a.theta[threadIdx.x]; s_active[threadIdx.x] = a.active[threadIdx.x]; }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int i4 = lane & 3;
  const long long ntiles = (n + RG - 1) / RG;
  const int nsteps = l4 / 4;

  constexpr int KR = KT < 3 ? KT : 3;     // tiles that can hold residual columns (m <= 48); further tiles: extra products only
  constexpr bool TH_LDS = KT >= 4;
  double th[KR][4];
  int act[KR][4];
  double ssq[KR][4], smx[KR][4];
  // (four and five tiles: the norm accumulators live in LDS, one slot per lane -- 48 registers less in a kernel whose
  //  accumulators the compiler otherwise shuffles between VGPRs and AGPRs in every stage)
  __shared__ double s_nrm[TH_LDS ? 4 * 48 * 16 * 2 : 2];
  double* my_nrm = s_nrm + (TH_LDS ? (size_t)wave * 48 * 16 * 2 + i * 2 : 0);      // [col j][lane i][2], this wave
#pragma unroll
  for (int q = 0; q < KR; ++q)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int j = 16 * q + g + 4 * reg;
      th[q][reg] = s_theta[j];
      act[q][reg] = s_active[j];
      ssq[q][reg] = 0.0;
      smx[q][reg] = 0.0;
      if constexpr (TH_LDS) { my_nrm[(size_t)j * 32 + 0] = 0.0; my_nrm[(size_t)j * 32 + 1] = 0.0; }
    }

  for (long long tile = (long long)blockIdx.x * 4 + wave; tile < ntiles; tile += (long long)gridDim.x * 4) {
    long long row = tile * RG + VEC * i;
    const bool rok = row < n;
    if (!rok) row = 0;
    v4d av[VEC][KT], aav[VEC][KT];
#pragma unroll
    for (int e = 0; e < VEC; ++e)
#pragma unroll
      for (int q = 0; q < KT; ++q) { av[e][q] = (v4d){0.0, 0.0, 0.0, 0.0}; aav[e][q] = (v4d){0.0, 0.0, 0.0, 0.0}; }
    double avq[VEC][QT > 0 ? QT : 1], aavq[VEC][QT > 0 ? QT : 1];   // quarter tiles: scalars of their own (see gemm_kernel)
#pragma unroll
    for (int e = 0; e < VEC; ++e)
#pragma unroll
      for (int qq = 0; qq < (QT > 0 ? QT : 1); ++qq) { avq[e][qq] = 0.0; aavq[e][qq] = 0.0; }
    auto avv = [&](int e, int q, int reg) -> double {
      if (QT > 0 && q == KF) return reg < QT ? avq[e][reg < QT ? reg : 0] : 0.0;
      return av[e][q][reg];
    };
    auto aavv = [&](int e, int q, int reg) -> double {
      if (QT > 0 && q == KF) return reg < QT ? aavq[e][reg < QT ? reg : 0] : 0.0;
      return aav[e][q][reg];
    };
    int cs4 = 0;
    if constexpr (PIPE > 0) {
      // two-stage register pipeline over column steps (see gemm_kernel)
      const int nfull4 = l / 4;
      auto load_stage = [&](int c0, vec_t (&xs)[PIPE], vec_t (&ys)[PIPE]) {
#pragma unroll
        for (int u4 = 0; u4 < PIPE; ++u4) {
          const size_t off = (size_t)(4 * (c0 + u4) + g) * (size_t)n + row;
          xs[u4] = pload<VEC, NT>(a.v + off);
          ys[u4] = pload<VEC, NT>(a.av + off);
        }
      };
      auto mfma_stage = [&](int c0, const vec_t (&xs)[PIPE], const vec_t (&ys)[PIPE]) {
#pragma unroll
        for (int u4 = 0; u4 < PIPE; ++u4) {
          double cfu[KT];
#pragma unroll
          for (int q = 0; q < KF; ++q) cfu[q] = cs[(size_t)q * l4 * 16 + (size_t)(4 * (c0 + u4) + g) * 16 + i];
          double cfq[QT > 0 ? QT : 1];
#pragma unroll
          for (int qq = 0; qq < QT; ++qq) cfq[qq] = cs[(size_t)KF * l4 * 16 + (size_t)(4 * (c0 + u4) + g) * 8 + 4 * qq + i4];
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
#pragma unroll
            for (int q = 0; q < KF; ++q) {
              av[e][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(cfu[q], vget<VEC>(xs[u4], e), av[e][q], 0, 0, 0);
              aav[e][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(cfu[q], vget<VEC>(ys[u4], e), aav[e][q], 0, 0, 0);
            }
#pragma unroll
            for (int qq = 0; qq < QT; ++qq) {
              avq[e][qq] = mfma_quarter(cfq[qq], vget<VEC>(xs[u4], e), avq[e][qq]);
              aavq[e][qq] = mfma_quarter(cfq[qq], vget<VEC>(ys[u4], e), aavq[e][qq]);
            }
          }
        }
      };
      if (PIPE <= nfull4) {
        vec_t xa[PIPE], ya[PIPE];
        load_stage(0, xa, ya);
        for (; cs4 + 2 * PIPE <= nfull4; cs4 += PIPE) {
          vec_t xb[PIPE], yb[PIPE];
          load_stage(cs4 + PIPE, xb, yb);
          mfma_stage(cs4, xa, ya);
#pragma unroll
          for (int u4 = 0; u4 < PIPE; ++u4) { xa[u4] = xb[u4]; ya[u4] = yb[u4]; }
        }
        mfma_stage(cs4, xa, ya);
        cs4 += PIPE;
      }
    }
    for (; cs4 < nsteps; ++cs4) {
      int col = 4 * cs4 + g;
      const bool cok = col < l;
      col = cok ? col : l - 1;
      vec_t xv = pload<VEC, NT>(a.v + (size_t)col * (size_t)n + row);
      vec_t yv = pload<VEC, NT>(a.av + (size_t)col * (size_t)n + row);
      xv = cok ? xv : vzero<VEC>();
      yv = cok ? yv : vzero<VEC>();
      double cf[KT];
#pragma unroll
      for (int q = 0; q < KF; ++q) cf[q] = cs[(size_t)q * l4 * 16 + (size_t)(4 * cs4 + g) * 16 + i];
      double cfq[QT > 0 ? QT : 1];
#pragma unroll
      for (int qq = 0; qq < QT; ++qq) cfq[qq] = cs[(size_t)KF * l4 * 16 + (size_t)(4 * cs4 + g) * 8 + 4 * qq + i4];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
#pragma unroll
        for (int q = 0; q < KF; ++q) {
          av[e][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(cf[q], vget<VEC>(xv, e), av[e][q], 0, 0, 0);
          aav[e][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(cf[q], vget<VEC>(yv, e), aav[e][q], 0, 0, 0);
        }
#pragma unroll
        for (int qq = 0; qq < QT; ++qq) {
          avq[e][qq] = mfma_quarter(cfq[qq], vget<VEC>(xv, e), avq[e][qq]);
          aavq[e][qq] = mfma_quarter(cfq[qq], vget<VEC>(yv, e), aavq[e][qq]);
        }
      }
    }
    if (rok) {
#pragma unroll
      for (int q = 0; q < KT; ++q)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int j = 16 * q + g + 4 * reg;
          if (j >= a.k + (XP ? a.k2 : 0)) continue;
          const double e0 = avv(0, q, reg), e1 = avv(VEC - 1, q, reg);
          double r0 = aavv(0, q, reg), r1 = aavv(VEC - 1, q, reg);
          if constexpr (XP) {
            if (j >= a.k) {                // a column of the extra block: two plain products
              pstore<VEC, NT>(a.p2 + (size_t)(j - a.k) * (size_t)n + row, vmake<VEC>(e0, e1));
              pstore<VEC, NT>(a.ap2 + (size_t)(j - a.k) * (size_t)n + row, vmake<VEC>(r0, r1));
              continue;
            }
          }
          constexpr int KRm = KR - 1;
          const int qr = q < KR ? q : KRm;  // (j < k <= 48 implies q < 3; the clamp only keeps the unrolled indices in range)
          if (a.avy) pstore<VEC, NT>(a.avy + (size_t)j * (size_t)n + row, vmake<VEC>(r0, r1));
          // (the four- and five-tile kernels sit at the register limit: they read theta / active from LDS per tile)
          const double thv = TH_LDS ? s_theta[j] : th[qr][reg];
          const int actv = TH_LDS ? s_active[j] : act[qr][reg];
          if (actv) {
            r0 = r0 - thv * e0;            // daxpy(-eig), reference diaglib.f90:1729
            if constexpr (TH_LDS) {
              // (same order of additions as the register accumulators of the narrower kernels: same bits)
              double* slot = my_nrm + (size_t)j * 32;
              double sq = slot[0], mx = slot[1];
              sq += r0 * r0; mx = fmax(mx, fabs(r0));
              if constexpr (VEC == 2) { r1 = r1 - thv * e1; sq += r1 * r1; mx = fmax(mx, fabs(r1)); }
              slot[0] = sq;
              slot[1] = mx;
            } else {
              ssq[qr][reg] += r0 * r0;
              smx[qr][reg] = fmax(smx[qr][reg], fabs(r0));
              if constexpr (VEC == 2) {
                r1 = r1 - thv * e1;
                ssq[qr][reg] += r1 * r1;
                smx[qr][reg] = fmax(smx[qr][reg], fabs(r1));
              }
            }
          }
          if (a.evec) pstore<VEC, NT>(a.evec + (size_t)j * (size_t)n + row, vmake<VEC>(e0, e1));     // (optional: Ritz vectors nobody reads are not written)
          pstore<VEC, NT>(a.r + (size_t)j * (size_t)n + row, vmake<VEC>(r0, r1));
        }
    }
  }
  // reduce over the 16 lanes that share g (xor-shuffles stay inside 16-lane groups), then over waves
  __syncthreads();   // everyone is done with cs as the copy of Y
  double* sred = cs; // [4 waves][16*KT][2]
#pragma unroll
  for (int q = 0; q < KR; ++q)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      double s = ssq[q][reg], m = smx[q][reg];
      if constexpr (TH_LDS) { const int j = 16 * q + g + 4 * reg; s = my_nrm[(size_t)j * 32 + 0]; m = my_nrm[(size_t)j * 32 + 1]; }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) {
        s += __shfl_xor(s, off, 64);
        m = fmax(m, __shfl_xor(m, off, 64));
      }
      if (i == 0) {
        const int j = 16 * q + g + 4 * reg;
        sred[(wave * 16 * KT + j) * 2 + 0] = s;
        sred[(wave * 16 * KT + j) * 2 + 1] = m;
      }
    }
  __syncthreads();
  if (threadIdx.x < 16 * KT) {
    const int j = threadIdx.x;
    double s = 0.0, m = 0.0;
    for (int w = 0; w < 4 && j < 16 * KR; ++w) {
      s += sred[(w * 16 * KT + j) * 2 + 0];
      m = fmax(m, sred[(w * 16 * KT + j) * 2 + 1]);
    }
    a.red[((size_t)blockIdx.x * 16 * KT + j) * 2 + 0] = s;
    a.red[((size_t)blockIdx.x * 16 * KT + j) * 2 + 1] = m;
  }
}

// The same sweep with TWO coefficient blocks: e = V Y1 (stored when a.evec is given), r = AV Y2 - theta e for the active columns,
// sum r^2 and max |r| -- the residual blocks of the linear-response drivers (reference diaglib.f90:872-889, 1337-1353:
// rp = (A+B) vp u+ - w (S-D) vm u-, two panels with two different coefficient sets), which the reference forms with two dgemms and
// a daxpy / dnrm2 loop.  Packed coefficients: [2 KT][l4][16], Y1 in the leading KT tiles, Y2 behind.  Blocks of up to 48 columns,
// no register pipeline (these blocks are n_max <= 16 wide in practice: one tile, like the plain one-tile Ritz step).
template <int KT, int VEC>
__global__ __launch_bounds__(256) void ritz2_kernel(RitzArgs a)
{
  constexpr int RG = 16 * VEC;
  extern __shared__ __attribute__((aligned(16))) double cs[];  // [2 KT][l4][16], later reduction scratch
  typedef typename VecOf<VEC>::type vec_t;
  const long long n = a.n;
  const int l = a.l, l4 = a.l4;
  for (int idx = threadIdx.x; idx < 2 * KT * l4 * 16; idx += 256) cs[idx] = a.cpk[idx];
  __shared__ double s_theta[48];
  __shared__ int s_active[48];
  if (threadIdx.x < 48) { s_theta[threadIdx.x] = a.theta[threadIdx.x]; s_active[threadIdx.x] = a.active[threadIdx.x]; }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const long long ntiles = (n + RG - 1) / RG;
  const int nsteps = l4 / 4;
  double th[KT][4], ssq[KT][4], smx[KT][4];
  int act[KT][4];
#pragma unroll
  for (int q = 0; q < KT; ++q)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int j = 16 * q + g + 4 * reg;
      th[q][reg] = s_theta[j]; act[q][reg] = s_active[j]; ssq[q][reg] = 0.0; smx[q][reg] = 0.0;
    }
  const double* cs2 = cs + (size_t)KT * l4 * 16;
  for (long long tile = (long long)blockIdx.x * 4 + wave; tile < ntiles; tile += (long long)gridDim.x * 4) {
    long long row = tile * RG + VEC * i;
    const bool rok = row < n;
    if (!rok) row = 0;
    v4d av[VEC][KT], aav[VEC][KT];
#pragma unroll
    for (int e = 0; e < VEC; ++e)
#pragma unroll
      for (int q = 0; q < KT; ++q) { av[e][q] = (v4d){0.0, 0.0, 0.0, 0.0}; aav[e][q] = (v4d){0.0, 0.0, 0.0, 0.0}; }
#pragma unroll 2
    for (int cs4 = 0; cs4 < nsteps; ++cs4) {
      int col = 4 * cs4 + g;
      const bool cok = col < l;
      col = cok ? col : l - 1;
      vec_t xv = pload<VEC, 3>(a.v + (size_t)col * (size_t)n + row);
      vec_t yv = pload<VEC, 3>(a.av + (size_t)col * (size_t)n + row);
      xv = cok ? xv : vzero<VEC>();
      yv = cok ? yv : vzero<VEC>();
#pragma unroll
      for (int q = 0; q < KT; ++q) {
        const double c1 = cs[(size_t)q * l4 * 16 + (size_t)(4 * cs4 + g) * 16 + i];
        const double c2 = cs2[(size_t)q * l4 * 16 + (size_t)(4 * cs4 + g) * 16 + i];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          av[e][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(c1, vget<VEC>(xv, e), av[e][q], 0, 0, 0);
          aav[e][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(c2, vget<VEC>(yv, e), aav[e][q], 0, 0, 0);
        }
      }
    }
    if (rok) {
#pragma unroll
      for (int q = 0; q < KT; ++q)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int j = 16 * q + g + 4 * reg;
          if (j >= a.k) continue;
          const double e0 = av[0][q][reg], e1 = av[VEC - 1][q][reg];
          double r0 = aav[0][q][reg], r1 = aav[VEC - 1][q][reg];
          if (act[q][reg]) {
            r0 = r0 - th[q][reg] * e0;
            ssq[q][reg] += r0 * r0;
            smx[q][reg] = fmax(smx[q][reg], fabs(r0));
            if constexpr (VEC == 2) {
              r1 = r1 - th[q][reg] * e1;
              ssq[q][reg] += r1 * r1;
              smx[q][reg] = fmax(smx[q][reg], fabs(r1));
            }
          }
          if (a.evec) pstore<VEC, 3>(a.evec + (size_t)j * (size_t)n + row, vmake<VEC>(e0, e1));
          pstore<VEC, 3>(a.r + (size_t)j * (size_t)n + row, vmake<VEC>(r0, r1));
        }
    }
  }
  __syncthreads();
  double* sred = cs; // [4 waves][16*KT][2]
#pragma unroll
  for (int q = 0; q < KT; ++q)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      double sv = ssq[q][reg], m = smx[q][reg];
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) {
        sv += __shfl_xor(sv, off, 64);
        m = fmax(m, __shfl_xor(m, off, 64));
      }
      if (i == 0) {
        const int j = 16 * q + g + 4 * reg;
        sred[(wave * 16 * KT + j) * 2 + 0] = sv;
        sred[(wave * 16 * KT + j) * 2 + 1] = m;
      }
    }
  __syncthreads();
  if (threadIdx.x < 16 * KT) {
    const int j = threadIdx.x;
    double sv = 0.0, m = 0.0;
    for (int w = 0; w < 4; ++w) {
      sv += sred[(w * 16 * KT + j) * 2 + 0];
      m = fmax(m, sred[(w * 16 * KT + j) * 2 + 1]);
    }
    a.red[((size_t)blockIdx.x * 16 * KT + j) * 2 + 0] = sv;
    a.red[((size_t)blockIdx.x * 16 * KT + j) * 2 + 1] = m;
  }
}

// fixed-shape block reduction (shuffle tree inside each wave, then the 4 waves in order)
__device__ __forceinline__ void block_sum_max(double& s, double& m, double* sh /* >= 8 doubles */)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_down(s, off, 64);
    m = fmax(m, __shfl_down(m, off, 64));
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[w] = s; sh[4 + w] = m; }
  __syncthreads();
  s = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  m = fmax(fmax(sh[4], sh[5]), fmax(sh[6], sh[7]));
}

// out[j] = sum_b red[b][j][0]; the maxima go to the rank's own slot, out[ncol + rank * ncol + j] = max_b red[b][j][1],
// and the other ranks' slots are zeroed: ONE sum all-reduce then carries the sums and every rank's maxima
// (max |r| >= 0, so the maximum over ranks is the maximum over the slots); one block per column j
__global__ __launch_bounds__(256) void ritz_reduce_kernel(const double* red, int nblk, int ncol, double* out, double* out_host,
                                                          int nranks, int rank)
{
  const int j = blockIdx.x;
  double s = 0.0, m = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) {
    s += red[((size_t)b * ncol + j) * 2 + 0];
    m = fmax(m, red[((size_t)b * ncol + j) * 2 + 1]);
  }
  __shared__ double sh[8];
  block_sum_max(s, m, sh);
  if (threadIdx.x == 0) {
    out[j] = s; out_host[j] = s;
    for (int r = 0; r < nranks; ++r) {
      const double v = (r == rank) ? m : 0.0;
      out[ncol + r * ncol + j] = v; out_host[ncol + r * ncol + j] = v;
    }
  }
}

// ======================================================================================
// Ritz sweep that also forms and measures the next Davidson block
// ======================================================================================
// The residual block R = AV Y - (V Y) Lambda of a Davidson iteration, its norms, the preconditioned block U0 = R(:, first:) / (d + fac)
// and the two matrices the orthogonalisation chain measures first, V^T U0 and U0^T U0, in ONE sweep over V and AV -- on the data
// flow of gram_lds_kernel WP == 2: a wave stages 16 rows of ALL columns of V, then of AV, in its LDS image ([column][18]); the
// tiles of V Y and AV Y are 4 TX MFMAs each away (D^T = Y^T V^T, the coefficients in registers for the whole sweep, two independent
// chains side by side).  The two products and the correction r - theta e are ritz_kernel's, step by step: the same MFMA per four
// columns in the same order, the same expression -- R comes out bit for bit as from the plain sweep, its norms to the rounding of
// another order of summation (the one-sweep form R = [V | AV] [-Y Lambda ; Y] would save nothing and round differently: on the
// benchmark, whose tolerance sits at rounding level, a root then locked one sweep later).  Every lane then holds R[row c][g + 4 r] and
//   * adds r^2 and max |r| of the columns whose norm is wanted (RitzExpandArgs::act) to its partials -- ritz_reduce_kernel's layout,
//   * stores R (16 consecutive rows of a column per 16 lanes: full 128-byte segments),
//   * scales by the library's diagonal rule (the expression of synth_precnd_kernel / diag_precnd_kernel: a division), stores
//     columns f0 .. nb-1 as U0 and puts the stored values into the image's output tile, columns 0 .. k-1,
//   * forms V^T U0 (the AV tiles take no part) and U0^T U0 from that tile, as gram_lds_kernel WP does.
// The block partials go out as a one-pass WP sweep's: [block][TX + 1][256], slot t = V tile t, slot TX = U0^T U0 -- and they ARE that
// sweep's, bit for bit, when the grid is its grid (ritz_expand_plan takes wp_plan's): the same rows go to the same wave in the same
// order (RitzExpandArgs::pair where that sweep stages 32 rows), the same MFMAs in the same order, the same sum over the waves.  A
// solve with the fused sweep therefore differs from one without only through the order in which the norms are summed.
// Even n, 16-byte aligned panels (the callers decline everything else); rows >= n are staged as zeros and add nothing.
struct RitzExpandArgs {
  const double* v;     // n x m
  const double* av;    // n x m
  const double* cpk;   // packed coefficients Y, [16 TX][16], zero padded: both products take them
  const double* diag;  // n
  double fac;
  double* r;           // n x nb
  double* u0;          // n x k, k = nb - f0
  double* red;         // norm partials [nblk][16][2]
  double* partial;     // Gram partials [nblk][TX + 1][256]
  long long n;
  int m, nb, f0;
  int pair;            // 1: a wave takes its 16-row tiles in consecutive pairs (the 32-row tiles of the measuring sweep it stands in for)
  unsigned act;        // bit j: column j of R is an open wanted root (it is corrected and its norms are formed)
  double theta[16];    // Ritz values of the columns
};

template <int TX>
__global__ __launch_bounds__(256) void davidson_expand_kernel(RitzExpandArgs a)
{
  constexpr int RS = 18;                   // doubles per staged column (16 rows + 2: 16-byte alignment, conflict-free fragment reads)
  constexpr int NC = 16 * (2 * TX + 1);    // staged columns: V tiles, AV tiles, the output tile
  constexpr int OOFF = 32 * TX;            // where the output tile sits
  constexpr int NI = 4 * TX;               // load instructions per row tile: 8 columns of 16 rows each
  extern __shared__ __attribute__((aligned(16))) double glds[];   // [4][NC][RS]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* my = glds + (size_t)wave * NC * RS;
  const int c = lane & 15, g = lane >> 4;
  const int li = lane & 7, lc = lane >> 3;
  const long long n = a.n;
  const int k = a.nb - a.f0;

  // (the output tile's columns k .. 15 are never written by a row tile: zero once)
  for (int idx = lane; idx < 16 * RS; idx += 64) my[(size_t)OOFF * RS + idx] = 0.0;
  double ca[4 * TX];
#pragma unroll
  for (int s = 0; s < 4 * TX; ++s) ca[s] = a.cpk[(size_t)(4 * s + g) * 16 + c];
  double th[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) th[r] = a.theta[g + 4 * r];
  v4d acc[TX];
#pragma unroll
  for (int t = 0; t < TX; ++t) acc[t] = (v4d){0.0, 0.0, 0.0, 0.0};
  v4d accuu = (v4d){0.0, 0.0, 0.0, 0.0};
  double ssq[4], smx[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { ssq[r] = 0.0; smx[r] = 0.0; }

  typedef VecOf<2>::type vec_t;
  vec_t stg[NI];
  double dnext = 1.0;
  // (the 2 NI address registers are recomputed per tile, as gram_lds_kernel LOW does; instructions whose eight columns all lie
  //  beyond the basis read one fixed word, and a column beyond it inside a live instruction re-reads the last one: both meet
  //  zero coefficients and unused rows of V^T U0 only)
  auto load_tile = [&](long long tile) {
    const long long r0 = tile * 16;
    // (a tile that reaches beyond n: rows >= n are staged as zeros; n is even, so a 16-byte row pair is all-in or all-out)
    const bool rows_ok = r0 + 16 <= n || r0 + 2 * li < n;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const bool isv = j < 2 * TX;
      int col = 8 * (isv ? j : j - 2 * TX) + lc;
      col = col < a.m ? col : a.m - 1;
      const bool pin = 8 * (isv ? j : j - 2 * TX) >= a.m;
      const double* p = pin ? a.v : (isv ? a.v : a.av) + (size_t)col * (size_t)n + 2 * li + r0;
      stg[j] = vzero<2>();
      if (rows_ok) stg[j] = pload<2, 1>(p);
    }
    dnext = 1.0;
    if (r0 + c < n) dnext = a.diag[r0 + c];
  };
  auto stage_tile = [&]() {
#pragma unroll
    for (int j = 0; j < NI; ++j) lds_store2(my + (size_t)(8 * j + lc) * RS + 2 * li, stg[j]);
  };
  auto do_tile = [&](long long r0, double dg) {
    // (V Y)[row c][g + 4 r] and (AV Y)[row c][g + 4 r]: sums over the staged columns j of V / AV [row c][j] Y(j, g + 4 r)
    v4d dv = (v4d){0.0, 0.0, 0.0, 0.0}, da = (v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 4 * TX; ++s) {
      dv = __builtin_amdgcn_mfma_f64_16x16x4f64(ca[s], lds_load1(my + (size_t)(4 * s + g) * RS + c), dv, 0, 0, 0);
      da = __builtin_amdgcn_mfma_f64_16x16x4f64(ca[s], lds_load1(my + (size_t)(16 * TX + 4 * s + g) * RS + c), da, 0, 0, 0);
    }
    const long long row = r0 + c;
    const bool rok = row < n;
    const double den = dg + a.fac;
    const bool use = fabs(den) > 1.0e-5;                         // mprec, main.f90:161-169 (see synth_precnd_kernel)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = g + 4 * r;
      double val = da[r];
      if ((a.act >> j) & 1u) {
        val = val - th[r] * dv[r];       // daxpy(-eig), reference diaglib.f90:1729 (ritz_kernel's expression)
        ssq[r] += val * val;
        smx[r] = fmax(smx[r], fabs(val));
      }
      if (rok && j < a.nb) __builtin_nontemporal_store(val, a.r + (size_t)j * (size_t)n + row);
      const double u = use ? val / den : val;
      const int jj = j - a.f0;
      if (jj >= 0) {
        lds_store1(my + (size_t)(OOFF + jj) * RS + c, u);
        if (rok && jj < k) a.u0[(size_t)jj * (size_t)n + row] = u;
      }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      const double uf = lds_load1(my + (size_t)(OOFF + c) * RS + 4 * s4 + g);
      accuu = __builtin_amdgcn_mfma_f64_16x16x4f64(uf, uf, accuu, 0, 0, 0);
#pragma unroll
      for (int t = 0; t < TX; ++t) {
        const double xf = lds_load1(my + (size_t)(16 * t + c) * RS + 4 * s4 + g);
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(xf, uf, acc[t], 0, 0, 0);
      }
    }
  };
  // the wave's 16-row tiles: every (4 gridDim.x)-th, or -- pair -- every (4 gridDim.x)-th pair of consecutive ones
  const long long ntiles = (n + 15) / 16;
  const int ps = a.pair ? 1 : 0;
  const long long stride = (long long)gridDim.x * 4;
  long long tile = ((long long)blockIdx.x * 4 + wave) << ps;
  __builtin_amdgcn_wave_barrier();
  if (tile < ntiles) {
    load_tile(tile);
    for (;;) {
      stage_tile();
      const double dg = dnext;
      __builtin_amdgcn_wave_barrier();
      const long long next = (ps && !(tile & 1)) ? tile + 1 : ((tile >> ps) + stride) << ps;
      if (next < ntiles) load_tile(next);
      do_tile(tile * 16, dg);
      __builtin_amdgcn_wave_barrier();
      tile = next;
      if (next >= ntiles) break;
    }
  }

  // norms: over the 16 lanes that share g, then over the waves; Gram tiles: over the waves, one slot at a time
  __syncthreads();
  double* red = glds;   // [4][256] (the staging area is free now); the norms behind it, [4][16][2]
  double* nred = glds + 1024;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double s = ssq[r], m = smx[r];
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
      s += __shfl_xor(s, off, 64);
      m = fmax(m, __shfl_xor(m, off, 64));
    }
    if (c == 0) {
      nred[(wave * 16 + g + 4 * r) * 2 + 0] = s;
      nred[(wave * 16 + g + 4 * r) * 2 + 1] = m;
    }
  }
  double* pout = a.partial + (size_t)blockIdx.x * (size_t)(TX + 1) * 256;
#pragma unroll
  for (int t = 0; t <= TX; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave * 256 + r * 64 + lane] = t < TX ? acc[t < TX ? t : 0][r] : accuu[r];
    __syncthreads();
    pout[(size_t)t * 256 + threadIdx.x] = ((red[threadIdx.x] + red[256 + threadIdx.x]) + red[512 + threadIdx.x]) + red[768 + threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x < 16) {
    const int j = threadIdx.x;
    double s = 0.0, m = 0.0;
    for (int w = 0; w < 4; ++w) {
      s += nred[(w * 16 + j) * 2 + 0];
      m = fmax(m, nred[(w * 16 + j) * 2 + 1]);
    }
    a.red[((size_t)blockIdx.x * 16 + j) * 2 + 0] = s;
    a.red[((size_t)blockIdx.x * 16 + j) * 2 + 1] = m;
  }
}

// ======================================================================================
// Elementwise
// ======================================================================================
// small host matrix (pinned, device-mapped) -> device, 16 bytes per lane (HipEngine::stage_commit)
__global__ __launch_bounds__(256) void small_copy_kernel(double* __restrict__ dst, const double* __restrict__ src, int n)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (2 * i + 1 < n) ((v2d*)dst)[i] = ((const v2d*)src)[i];
  else if (2 * i < n) dst[2 * i] = src[2 * i];
}

__global__ void axpy_kernel(size_t len, double alpha, const double* __restrict__ x, double* __restrict__ y)
{
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < len; i += stride) y[i] += alpha * x[i];
}

// STREAM triad a = b + s c with the access shape of the sweeps (16 B per lane, non-temporal): the practical HBM
// ceiling the roofline fractions are read against (SURVEY 8d "record a measured device-triad GB/s")
template <int NT, int UNR>
__global__ __launch_bounds__(256) void triad_kernel(size_t len2, double sc, const double* __restrict__ b,
                                                    const double* __restrict__ c, double* __restrict__ a)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + (UNR - 1) * stride < len2; i += UNR * stride) {
    v2d bv[UNR], cv[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      if constexpr (NT) { bv[u] = __builtin_nontemporal_load((const v2d*)b + i + u * stride); cv[u] = __builtin_nontemporal_load((const v2d*)c + i + u * stride); }
      else { bv[u] = ((const v2d*)b)[i + u * stride]; cv[u] = ((const v2d*)c)[i + u * stride]; }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      if constexpr (NT) __builtin_nontemporal_store(bv[u] + sc * cv[u], (v2d*)a + i + u * stride);
      else ((v2d*)a)[i + u * stride] = bv[u] + sc * cv[u];
    }
  }
  for (; i < len2; i += stride) ((v2d*)a)[i] = ((const v2d*)b)[i] + sc * ((const v2d*)c)[i];
}

// block partial sums of squares; fixed grid => deterministic
__global__ __launch_bounds__(256) void sumsq_kernel(size_t len, const double* __restrict__ x, double* partial)
{
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  double s = 0.0;
  for (; i < len; i += stride) s += x[i] * x[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  __shared__ double w[4];
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ((w[0] + w[1]) + w[2]) + w[3];
}

__global__ __launch_bounds__(256) void sum_partials_kernel(const double* partial, int nblk, double* out, double* out_host)
{
  double s = 0.0, m = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) s += partial[b];
  __shared__ double sh[8];
  block_sum_max(s, m, sh);
  if (threadIdx.x == 0) { out[0] = s; out_host[0] = s; }
}

// documented counter-based generator (same as oracle/oracle.c orc_u01)
__device__ __host__ inline double u01(unsigned long long seed, unsigned long long i, unsigned long long j)
{
  unsigned long long z = seed * 0x9E3779B97F4A7C15ULL + i * 0xBF58476D1CE4E5B9ULL + j * 0x94D049BB133111EBULL;
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ULL;
  z ^= z >> 27; z *= 0x94D049BB133111EBULL;
  z ^= z >> 31;
  return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

__global__ void random_fill_kernel(long long n, int m, double* evec, long long row0, unsigned long long seed, double offset,
                                   long long support_rows)
{
  const long long total = n * (long long)m;
  long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (; idx < total; idx += stride) {
    const long long i = idx % n, j = idx / n;
    const bool in = support_rows <= 0 || row0 + i < support_rows;
    evec[idx] = in ? u01(seed, (unsigned long long)(row0 + i + 1), (unsigned long long)(j + 1)) + offset : 0.0;
  }
}

// built-in operator A = diag(i+1) + sigma W W^T, and the family of sample operators around the same W (SynthKind)
__global__ void synth_build_kernel(long long row0, int n, int rw, double sigma, double* w, double* diag, double* wsq)
{
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long gi = (unsigned long long)(row0 + i + 1);
  const double inv = 1.0 / sqrt((double)gi);
  double s = 0.0;
  for (int j = 0; j < rw; ++j) {
    const double h = 2.0 * u01(1ULL, gi, (unsigned long long)(j + 1)) - 1.0;
    const double v = h * inv;
    w[(size_t)j * n + i] = v;
    s += v * v;
  }
  diag[i] = ((double)gi + 1.0) + sigma * s;
  wsq[i] = s;
}

// Sample operators of the linear-response and generalised drivers (reference callers main.f90:403-526,
// 528-760 build dense SPD matrices A+B, A-B, S+D, S-D and a dense SPD metric): the same shape matrix-free,
//     y = d(i) x + W C W^T x,   C a 4 x 4 coupling block,  i = 1-based global row,
//   kind 0  A      d = i + 1,  C = sigma I                                (the benchmark operator)
//   kind 1  A + B  d = i + 5,  C = sigma I                                (main.f90:563: apb(i,i) = 5 + i)
//   kind 2  A - B  d = i + 2,  C = 0.2 sigma I                            (main.f90:570: amb(i,i) = 2 + i)
//   kind 3  S + D  d = s(i),   C = tau J,  J = -J^T  (D antisymmetric: W J W^T)
//   kind 4  S - D  d = s(i),   C = -tau J
//   kind 5  metric d = s(i),   C = 0.1 I   (symmetric positive definite)
// with s(i) = 1 + 0.5 / (1 + (i mod 7)) and tau = 0.05.  All of them need W^T x (4 x m, all-reduced over the shards) and one
// elementwise pass: HBM-bound at 8 n (2 m + 4) bytes like the benchmark operator.
enum { SYN_A = 0, SYN_APB = 1, SYN_AMB = 2, SYN_SPD = 3, SYN_SMD = 4, SYN_METRIC = 5 };
__device__ __host__ inline double synth_s(unsigned long long gi) { return 1.0 + 0.5 / (1.0 + (double)(gi % 7ULL)); }
__device__ __host__ inline double synth_d(int kind, unsigned long long gi)
{
  switch (kind) {
    case SYN_A: return (double)gi + 1.0;
    case SYN_APB: return (double)gi + 5.0;
    case SYN_AMB: return (double)gi + 2.0;
    default: return synth_s(gi);
  }
}
struct SynthCoupling { double c[16]; };    // column-major 4 x 4

// ax = d x + W (C t),  t = W^T x (rw x m, column-major, ld rw) already reduced
template <int RW>
__global__ __launch_bounds__(256) void synth_apply_kernel(long long row0, int n, int m, int kind, SynthCoupling cp,
                                                          const double* __restrict__ w, const double* __restrict__ t,
                                                          const double* __restrict__ x, double* __restrict__ ax)
{
  extern __shared__ double ts[];  // RW x m: C t
  for (int idx = threadIdx.x; idx < RW * m; idx += 256) {
    const int q = idx % RW, c = idx / RW;
    double v = 0.0;
#pragma unroll
    for (int p = 0; p < RW; ++p) v += cp.c[q + RW * p] * t[p + c * RW];
    ts[idx] = v;
  }
  __syncthreads();
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const double d = synth_d(kind, (unsigned long long)(row0 + i + 1));
    double wv[RW];
#pragma unroll
    for (int q = 0; q < RW; ++q) wv[q] = w[(size_t)q * n + i];
    for (int c = 0; c < m; ++c) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < RW; ++q) s += wv[q] * ts[q + c * RW];
      ax[(size_t)c * n + i] = d * x[(size_t)c * n + i] + s;
    }
  }
}

// Preconditioners of the linear-response drivers, the harness' lrprec_1 / lrprec_2 (main.f90:234-281) on the diagonals of
// the sample operators: aa = ((A+B)_ii + (A-B)_ii) / 2, sigma = S_ii (J has a zero diagonal)
//   variant 1: den = aa^2 - fac^2 sg^2,  yp = -(aa xp + fac sg xm) / den,  ym = -(aa xm + fac sg xp) / den
//   variant 2: den = fac^2 aa^2 - sg^2,  yp = (fac aa xp + sg xm) / den,   ym = (fac aa xm + sg xp) / den
__global__ void synth_lrprec_kernel(long long row0, int n, int m, int variant, double fac, double sigma, const double* __restrict__ wsq,
                                    const double* __restrict__ xp, const double* __restrict__ xm, double* __restrict__ yp,
                                    double* __restrict__ ym)
{
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const unsigned long long gi = (unsigned long long)(row0 + i + 1);
    const double aa = 0.5 * ((synth_d(SYN_APB, gi) + sigma * wsq[i]) + (synth_d(SYN_AMB, gi) + 0.2 * sigma * wsq[i]));
    const double sg = synth_s(gi);
    for (int c = 0; c < m; ++c) {
      const double a = xp[(size_t)c * n + i], b = xm[(size_t)c * n + i];
      if (variant == 1) {
        const double den = -1.0 / (aa * aa - fac * fac * sg * sg);
        yp[(size_t)c * n + i] = den * (aa * a + fac * sg * b);
        ym[(size_t)c * n + i] = den * (aa * b + fac * sg * a);
      } else {
        const double den = 1.0 / (fac * fac * aa * aa - sg * sg);
        yp[(size_t)c * n + i] = den * (fac * aa * a + sg * b);
        ym[(size_t)c * n + i] = den * (fac * aa * b + sg * a);
      }
    }
  }
}

// one thread keeps VEC rows of the diagonal in registers and walks the m columns (the diagonal is read once,
// no index arithmetic per element); panel accesses are non-temporal
template <int VEC>
__global__ void synth_precnd_kernel(int n, int m, double fac, const double* __restrict__ diag,
                                    const double* __restrict__ x, double* __restrict__ px)
{
  typedef typename VecOf<VEC>::type vec_t;
  const size_t nv = (size_t)n / VEC;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t iv = (size_t)blockIdx.x * blockDim.x + threadIdx.x; iv < nv; iv += stride) {
    const size_t i = iv * VEC;
    const vec_t dg = *(const vec_t*)(diag + i);
    double inv[VEC];
    bool use[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const double den = vget<VEC>(dg, e) + fac;
      use[e] = fabs(den) > 1.0e-5;                          // mprec, main.f90:161-169
      inv[e] = den;
    }
    for (int c = 0; c < m; ++c) {
      const vec_t xv = pload<VEC, 1>(x + (size_t)c * n + i);
      double o[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = use[e] ? vget<VEC>(xv, e) / inv[e] : vget<VEC>(xv, e);
      pstore<VEC, 2>(px + (size_t)c * n + i, vmake<VEC>(o[0], o[VEC - 1]));
    }
  }
}

// ======================================================================================
// Sample sparse operator: ax = A x for a sparse symmetric A in ELLPACK form
// ======================================================================================
// A device-resident operator with the reference's callback shape matvec(n,m,x,ax) (reference README.md:34-35,
// main.f90:72-90) for callers whose matrix is sparse: A is handed over once in CSR form (dla_spmm_setup_csr) and kept
// as column-major ELLPACK (col[w][n], val[w][n], w = widest row, shorter rows padded with a zero that points at the
// row itself) -- the row index runs along the lanes, so the two ELLPACK streams are read fully coalesced and every
// thread keeps its w (column, value) pairs in registers while it walks the m right-hand sides.  The gathers
// x[col][c] are the irregular part; for the banded / stencil matrices of the test suite neighbouring rows gather
// neighbouring entries.  HBM-bound: 12 w n bytes of matrix + 16 n m bytes of vectors per call (+ gather overfetch).
// Padding to the WIDEST row is what makes this format unusable for a matrix with a few long rows: dla_spmm_setup_csr_fmt stores
// those as sliced ELLPACK with a CSR tail (sell_spmm_kernel / csr_long_segments_kernel below) behind the same two callbacks.
// The row loop is spelled once (ell_rows) for the product, the Chebyshev step (ell_cheb_step_kernel) and the product on a row shard
// (ell_spmm_halo_kernel).  A GATHER says where entry j of column c of the gathered panel lives and which column a padding entry
// points at; an EPILOGUE says what a row does with its sum: row(i) once per row, load(o) for element o = c n + i in front of the
// gather loop -- so that panel reads it needs are in flight while the loop runs -- and store(o, held, sum) behind it.
struct GatherPlain {
  const double* x; int n;
  __device__ __forceinline__ int self(int i) const { return i; }
  __device__ __forceinline__ const double* column(int c) const { return x + (size_t)c * n; }
  __device__ __forceinline__ static double at(const double* xc, int j) { return xc[j]; }
};
// the product's epilogue: a non-temporal store of the sum
struct StoreProduct {
  double* ax;
  struct Held {};
  __device__ __forceinline__ void row(int) {}
  __device__ __forceinline__ Held load(size_t) const { return Held{}; }
  __device__ __forceinline__ void store(size_t o, Held, double s) const { __builtin_nontemporal_store(s, ax + o); }
};
template <int W, class Gather, class Epilogue>
__device__ __forceinline__ void ell_rows(int n, int m, int w, const int* __restrict__ col, const double* __restrict__ val,
                                         const Gather gather, Epilogue ep)
{
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    ep.row(i);
    if constexpr (W > 0) {
      int cj[W]; double vj[W];
#pragma unroll
      for (int q = 0; q < W; ++q) {
        const bool in = q < w;
        cj[q] = in ? col[(size_t)q * n + i] : gather.self(i);
        vj[q] = in ? val[(size_t)q * n + i] : 0.0;
      }
      for (int c = 0; c < m; ++c) {
        const size_t o = (size_t)c * n + i;
        const auto xc = gather.column(c);
        const auto held = ep.load(o);
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < W; ++q) s += vj[q] * Gather::at(xc, cj[q]);
        ep.store(o, held, s);
      }
    } else {
      for (int c = 0; c < m; ++c) {
        const size_t o = (size_t)c * n + i;
        const auto xc = gather.column(c);
        const auto held = ep.load(o);
        double s = 0.0;
        for (int q = 0; q < w; ++q) s += val[(size_t)q * n + i] * Gather::at(xc, col[(size_t)q * n + i]);
        ep.store(o, held, s);
      }
    }
  }
}
template <int W>
__global__ __launch_bounds__(256) void ell_spmm_kernel(int n, int m, int w, const int* __restrict__ col,
                                                       const double* __restrict__ val, const double* __restrict__ x,
                                                       double* __restrict__ ax)
{
  ell_rows<W>(n, m, w, col, val, GatherPlain{x, n}, StoreProduct{ax});
}

// The same product from sliced ELLPACK (dla::SellLayout, dla_spmm_setup_csr_fmt): one wavefront owns a slice of 64 slots, entry
// (q, lane) of slice s at slice_ptr[s] + 64 q + lane, so both matrix streams are read in full 256- / 512-byte rows as above
// while the width is the slice's own.  A slice can be hundreds of entries wide, so the (column, value) pairs cannot wait in
// registers for all m right-hand sides as they do above: each pair is loaded once per chunk of MC columns and feeds MC
// accumulators -- MC independent gathers in flight per entry -- and the chunk loop sits INSIDE the slice loop, where the
// slice's second read comes from cache (64 x width x 12 bytes: 196 KiB at the widest, usually a few KiB).  Per (row, column)
// the entries are accumulated in stored order, one fused multiply-add each, from 0.0: the bits of ell_spmm_kernel.
// perm[slot] is the row a slot computes; negative: the row lives in the CSR tail (csr_long_segments_kernel / long_rows_combine_kernel write it); slots past n
// in the last slice and tail slots store nothing, so every element of ax has exactly one writer.
// (This kernel and sell_cheb_step_kernel keep a slice loop each: one loop shared through the epilogues of ell_rows came out 0.6 % slower
// on skewed matrices with random gathers -- 20.54 against 20.42 ms, outside the run-to-run band, profiles/sparse_shared_loops.txt.)
template <int MC>
__global__ __launch_bounds__(256) void sell_spmm_kernel(int n, int m, int slices, const long long* __restrict__ slice_ptr,
                                                        const int* __restrict__ perm, const int* __restrict__ col,
                                                        const double* __restrict__ val, const double* __restrict__ x,
                                                        double* __restrict__ ax)
{
  const int lane = threadIdx.x & 63;
  for (int s = blockIdx.x * 4 + (threadIdx.x >> 6); s < slices; s += gridDim.x * 4) {
    const long long p0 = slice_ptr[s];
    const int width = (int)((slice_ptr[s + 1] - p0) >> 6);
    const int slot = s * 64 + lane;
    const int row = slot < n ? perm[slot] : -1;
    const int* cs = col + p0 + lane;
    const double* vs = val + p0 + lane;
    for (int c0 = 0; c0 < m; c0 += MC) {
      const double* xc = x + (size_t)c0 * n;
      double acc[MC];
#pragma unroll
      for (int k = 0; k < MC; ++k) acc[k] = 0.0;
      if (c0 + MC <= m) {
        for (int q = 0; q < width; ++q) {
          const int cj = cs[(size_t)q * 64];
          const double vj = vs[(size_t)q * 64];
#pragma unroll
          for (int k = 0; k < MC; ++k) acc[k] = fma(vj, xc[(size_t)k * n + cj], acc[k]);
        }
      } else {
        const int mc = m - c0;
        for (int q = 0; q < width; ++q) {
          const int cj = cs[(size_t)q * 64];
          const double vj = vs[(size_t)q * 64];
#pragma unroll
          for (int k = 0; k < MC; ++k) if (k < mc) acc[k] = fma(vj, xc[(size_t)k * n + cj], acc[k]);
        }
      }
      if (row >= 0) {
#pragma unroll
        for (int k = 0; k < MC; ++k) if (c0 + k < m) __builtin_nontemporal_store(acc[k], ax + (size_t)(c0 + k) * n + row);
      }
    }
  }
}

// The CSR tail of the sliced format (the contract: include/diaglib_amd.h): one wavefront per SEGMENT of a long row (at most
// dla::SELL_LONG_SEG entries, dla::sell_build), lanes striding over the segment's entries (coalesced), per-lane partial sums for MC
// columns, then a butterfly over the 64 lanes -- a fixed shape, so the result does not depend on timing -- and lane 0 stores: to
// ax where the segment is its row's only one (seg_part < 0), else to the segment's slot of the workspace, part[slot * m + column],
// which long_rows_combine_kernel adds up.  No atomics: every element of ax and of the workspace has one writer.
template <int MC>
__global__ __launch_bounds__(256) void csr_long_segments_kernel(int n, int m, int nseg, const long long* __restrict__ seg_ptr,
                                                                const int* __restrict__ seg_row, const int* __restrict__ seg_part,
                                                                const int* __restrict__ long_row, const int* __restrict__ col,
                                                                const double* __restrict__ val, const double* __restrict__ x,
                                                                double* __restrict__ ax, double* __restrict__ part)
{
  const int lane = threadIdx.x & 63;
  for (int g = blockIdx.x * 4 + (threadIdx.x >> 6); g < nseg; g += gridDim.x * 4) {
    const int row = long_row[seg_row[g]];
    const int slot = seg_part[g];
    const long long p0 = seg_ptr[g], p1 = seg_ptr[g + 1];
    for (int c0 = 0; c0 < m; c0 += MC) {
      const double* xc = x + (size_t)c0 * n;
      const int mc = min(MC, m - c0);
      double acc[MC];
#pragma unroll
      for (int k = 0; k < MC; ++k) acc[k] = 0.0;
      for (long long p = p0 + lane; p < p1; p += 64) {
        const int cj = col[p];
        const double vj = val[p];
#pragma unroll
        for (int k = 0; k < MC; ++k) if (k < mc) acc[k] = fma(vj, xc[(size_t)k * n + cj], acc[k]);
      }
#pragma unroll
      for (int k = 0; k < MC; ++k)
        for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off, 64);
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < MC; ++k)
          if (k < mc) {
            if (slot < 0) ax[(size_t)(c0 + k) * n + row] = acc[k];
            else part[(size_t)slot * m + (c0 + k)] = acc[k];
          }
      }
    }
  }
}

// ... and the rows of more than one segment: one thread per (row, column) adds the row's partial sums in segment order,
// ((part_0 + part_1) + part_2) + ..., plain double additions, and stores to ax.  Runs behind csr_long_segments_kernel on the stream.
__global__ __launch_bounds__(256) void long_rows_combine_kernel(int n, int m, int nmulti, const int* __restrict__ multi_row,
                                                                const int* __restrict__ part_ptr, const double* __restrict__ part,
                                                                double* __restrict__ ax)
{
  const long long total = (long long)nmulti * m;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const int j = (int)(t / m), c = (int)(t - (long long)j * m);
    const int s0 = part_ptr[j], s1 = part_ptr[j + 1];
    double sum = part[(size_t)s0 * m + c];
    for (int sg = s0 + 1; sg < s1; ++sg) sum += part[(size_t)sg * m + c];
    ax[(size_t)c * n + multi_row[j]] = sum;
  }
}

// ---- y = A^T x through the transposed index of the stored operator (dla::TransposeIndex; the contract: include/diaglib_amd.h,
// dla_spmm_transpose_prepare).  The three kernels above with the value fetched through a position: where they read (col, val) the
// index gives (row, pos) -- the row of x to gather, and where A's stored value array holds the entry -- so per entry 8 bytes of
// index stream coalesced and the 8 bytes of the value are a second gather (into val, beside the one into x).  pos < 0 is padding:
// it is skipped, so y_j = fma over the entries of column j in stored order from 0.0 and nothing else.  Padding only follows a
// column's entries, never precedes them.
// ELLPACK: the thread keeps its w (row, fetched value) pairs in registers across the m right-hand sides as ell_rows does, and the
// count of real entries beside them.
template <int W>
__global__ __launch_bounds__(256) void ell_spmm_t_kernel(int n, int m, int w, const int* __restrict__ trow, const int* __restrict__ tpos,
                                                         const double* __restrict__ val, const double* __restrict__ x,
                                                         double* __restrict__ y)
{
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    if constexpr (W > 0) {
      int rj[W]; double vj[W];
      int cnt = 0;
#pragma unroll
      for (int q = 0; q < W; ++q) {
        const int p = q < w ? tpos[(size_t)q * n + i] : -1;
        const bool in = p >= 0;
        rj[q] = in ? trow[(size_t)q * n + i] : i;
        vj[q] = in ? val[p] : 0.0;
        cnt += in ? 1 : 0;
      }
      for (int c = 0; c < m; ++c) {
        const double* xc = x + (size_t)c * n;
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < W; ++q) s = q < cnt ? fma(vj[q], xc[rj[q]], s) : s;
        __builtin_nontemporal_store(s, y + (size_t)c * n + i);
      }
    } else {
      for (int c = 0; c < m; ++c) {
        const double* xc = x + (size_t)c * n;
        double s = 0.0;
        for (int q = 0; q < w; ++q) {
          const int p = tpos[(size_t)q * n + i];
          if (p < 0) break;
          s = fma(val[p], xc[trow[(size_t)q * n + i]], s);
        }
        __builtin_nontemporal_store(s, y + (size_t)c * n + i);
      }
    }
  }
}
// sliced: sell_spmm_kernel<MC> with the fetch; perm[slot] is the COLUMN of A a slot computes
template <int MC>
__global__ __launch_bounds__(256) void sell_spmm_t_kernel(int n, int m, int slices, const long long* __restrict__ slice_ptr,
                                                          const int* __restrict__ perm, const int* __restrict__ trow,
                                                          const int* __restrict__ tpos, const double* __restrict__ val,
                                                          const double* __restrict__ x, double* __restrict__ y)
{
  const int lane = threadIdx.x & 63;
  for (int s = blockIdx.x * 4 + (threadIdx.x >> 6); s < slices; s += gridDim.x * 4) {
    const long long p0 = slice_ptr[s];
    const int width = (int)((slice_ptr[s + 1] - p0) >> 6);
    const int slot = s * 64 + lane;
    const int out = slot < n ? perm[slot] : -1;
    const int* rs = trow + p0 + lane;
    const int* ps = tpos + p0 + lane;
    for (int c0 = 0; c0 < m; c0 += MC) {
      const double* xc = x + (size_t)c0 * n;
      const int mc = min(MC, m - c0);
      double acc[MC];
#pragma unroll
      for (int k = 0; k < MC; ++k) acc[k] = 0.0;
      for (int q = 0; q < width; ++q) {
        const int pj = ps[(size_t)q * 64];
        if (pj < 0) continue;
        const int rj = rs[(size_t)q * 64];
        const double vj = val[pj];
#pragma unroll
        for (int k = 0; k < MC; ++k) if (k < mc) acc[k] = fma(vj, xc[(size_t)k * n + rj], acc[k]);
      }
      if (out >= 0) {
#pragma unroll
        for (int k = 0; k < MC; ++k) if (k < mc) __builtin_nontemporal_store(acc[k], y + (size_t)(c0 + k) * n + out);
      }
    }
  }
}
// the tail of the index: csr_long_segments_kernel<MC> with the fetch (a tail holds no padding); long_rows_combine_kernel adds the
// partial sums of the columns of more than one segment
template <int MC>
__global__ __launch_bounds__(256) void csr_long_segments_t_kernel(int n, int m, int nseg, const long long* __restrict__ seg_ptr,
                                                                  const int* __restrict__ seg_row, const int* __restrict__ seg_part,
                                                                  const int* __restrict__ long_row, const int* __restrict__ trow,
                                                                  const int* __restrict__ tpos, const double* __restrict__ val,
                                                                  const double* __restrict__ x, double* __restrict__ y,
                                                                  double* __restrict__ part)
{
  const int lane = threadIdx.x & 63;
  for (int g = blockIdx.x * 4 + (threadIdx.x >> 6); g < nseg; g += gridDim.x * 4) {
    const int out = long_row[seg_row[g]];
    const int slot = seg_part[g];
    const long long p0 = seg_ptr[g], p1 = seg_ptr[g + 1];
    for (int c0 = 0; c0 < m; c0 += MC) {
      const double* xc = x + (size_t)c0 * n;
      const int mc = min(MC, m - c0);
      double acc[MC];
#pragma unroll
      for (int k = 0; k < MC; ++k) acc[k] = 0.0;
      for (long long p = p0 + lane; p < p1; p += 64) {
        const int rj = trow[p];
        const double vj = val[tpos[p]];
#pragma unroll
        for (int k = 0; k < MC; ++k) if (k < mc) acc[k] = fma(vj, xc[(size_t)k * n + rj], acc[k]);
      }
#pragma unroll
      for (int k = 0; k < MC; ++k)
        for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off, 64);
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < MC; ++k)
          if (k < mc) {
            if (slot < 0) y[(size_t)(c0 + k) * n + out] = acc[k];
            else part[(size_t)slot * m + (c0 + k)] = acc[k];
          }
      }
    }
  }
}

// ---- the Chebyshev polynomial preconditioner on the stored operator (the contract: include/diaglib_amd.h, dla_spmm_precnd_cheb).
// One step is z_{k+1} = alpha u + beta v + gamma x + eta (A u) with u = z_k, v = z_{k-1} (dla::cheb_coefficients): the product
// kernels above with the combination as their epilogue, so that A u never travels to HBM.  Per step 12 w n bytes of matrix, the
// gather of u, three coalesced panel reads and one write (32 n m) instead of the 16 n m of the product plus 40 n m of a sweep
// that combines.  `out` may be the buffer of v (the same thread reads and writes the element); it is never the buffer of u, which
// other rows gather.  The combination is spelled once, with explicit fused multiply-adds: the same bits from every kernel below.
__device__ __forceinline__ double cheb_combine(const dla::ChebStep& k, double u, double v, double x, double au)
{
  return fma(k.eta, au, fma(k.gamma, x, fma(k.beta, v, k.alpha * u)));
}
// ... and the step of the diagonally scaled form (dla_spmm_precnd_cheb_jacobi): the same combination on t = r_i ((A u)_i + fac u_i),
// with y = x o r in the place of x.  fac enters here, through the product, and not through alpha.  ri is the row's 1 / den_i: the
// kernels below read it once per row and keep it in a register across the m columns.
__device__ __forceinline__ double cheb_jacobi_combine(const dla::ChebStep& k, double fac, double ri, double u, double v, double y, double au)
{
  const double t = fma(fac, u, au) * ri;
  return fma(k.eta, t, fma(k.gamma, y, fma(k.beta, v, k.alpha * u)));
}
// ... and of the pencil form (dla_spmm_precnd_cheb_pencil): t = r_i ((A u)_i + fac (B u)_i), with the metric's product in the place
// of u.  With B the identity, (B u)_i = u_i, these are the bits of cheb_jacobi_combine.
__device__ __forceinline__ double cheb_pencil_combine(const dla::ChebStep& k, double fac, double ri, double u, double v, double y, double au,
                                                      double bu)
{
  const double t = fma(fac, bu, au) * ri;
  return fma(k.eta, t, fma(k.gamma, y, fma(k.beta, v, k.alpha * u)));
}
// The forms of a step: plain (dla_spmm_precnd_cheb), scaled (dla_spmm_precnd_cheb_jacobi) and the pencil form with B u in a panel
// (dla_spmm_precnd_cheb_pencil wherever the two matrices do not share a row loop).  The gather loops of the step kernels are spelled
// once for all three.
enum ChebForm : int { CHEB_PLAIN = 0, CHEB_SCALED = 1, CHEB_PENCIL = 2 };
template <int F>
__device__ __forceinline__ double cheb_epilogue(const dla::ChebStep& k, double fac, double ri, double u, double v, double x, double au, double bu)
{
  if constexpr (F == CHEB_PENCIL) return cheb_pencil_combine(k, fac, ri, u, v, x, au, bu);
  else if constexpr (F == CHEB_SCALED) return cheb_jacobi_combine(k, fac, ri, u, v, x, au);
  else return cheb_combine(k, u, v, x, au);
}
// The step as an epilogue of ell_rows: the panel reads of an element are issued before the gather loop, so they are in flight while
// it runs.  Scaled and pencil: x is the panel y = x o r, and fac and r (n doubles) feed the epilogue -- r_i is read once per row;
// pencil: bu is the panel B u; the plain form reads none of them.
template <int F>
struct ChebStepEpilogue {
  dla::ChebStep k;
  const double *u, *v, *x;
  double* out;
  double fac;
  const double* r;
  const double* bu;
  double ri = 0.0;
  struct Held { double u = 0.0, v = 0.0, x = 0.0, bu = 0.0; };
  __device__ __forceinline__ void row(int i) { if constexpr (F != CHEB_PLAIN) ri = r[i]; }
  __device__ __forceinline__ Held load(size_t o) const
  {
    if constexpr (F == CHEB_PENCIL) return Held{u[o], v[o], x[o], bu[o]};
    else return Held{u[o], v[o], x[o], 0.0};
  }
  __device__ __forceinline__ void store(size_t o, const Held& h, double s) const
  {
    __builtin_nontemporal_store(cheb_epilogue<F>(k, fac, ri, h.u, h.v, h.x, s, h.bu), out + o);
  }
  // (the pair loop: both sums come from the row's own gather loops)
  __device__ __forceinline__ void store(size_t o, const Held& h, double sa, double sb) const
  {
    __builtin_nontemporal_store(cheb_pencil_combine(k, fac, ri, h.u, h.v, h.x, sa, sb), out + o);
  }
};
// ell_spmm_kernel<W> with that epilogue, on the same width ladder
template <int W, int F>
__global__ __launch_bounds__(256) void ell_cheb_step_kernel(int n, int m, int w, const int* __restrict__ col,
                                                            const double* __restrict__ val, dla::ChebStep k, const double* u,
                                                            const double* v, const double* x, double* out, double fac,
                                                            const double* __restrict__ r, const double* __restrict__ bu)
{
  ell_rows<W>(n, m, w, col, val, GatherPlain{u, n}, ChebStepEpilogue<F>{k, u, v, x, out, fac, r, bu});
}
// The step of the pencil form where BOTH matrices are ELLPACK: a row's (column, value) pairs of A and of B, two gather loops over the
// same u and the pencil epilogue, so that neither A u nor B u travels to HBM.  ell_rows for two matrices: each sum is accumulated
// as ell_rows accumulates it (in stored order from 0.0; padding is a zero on the row's own column), so the bits are those of the
// two products.  W: the instance holds max(wa, wb) pairs of each matrix in registers -- twice the footprint of ell_rows<W>, hence the
// shorter ladder (PAIR_WIDTHS); W = 0 streams both.
template <int W, class Gather, class Epilogue>
__device__ __forceinline__ void ell_pair_rows(int n, int m, int wa, const int* __restrict__ cola, const double* __restrict__ vala, int wb,
                                              const int* __restrict__ colb, const double* __restrict__ valb, const Gather gather, Epilogue ep)
{
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    ep.row(i);
    if constexpr (W > 0) {
      int ca[W], cb[W]; double va[W], vb[W];
#pragma unroll
      for (int q = 0; q < W; ++q) {
        const bool ina = q < wa, inb = q < wb;
        ca[q] = ina ? cola[(size_t)q * n + i] : gather.self(i);
        va[q] = ina ? vala[(size_t)q * n + i] : 0.0;
        cb[q] = inb ? colb[(size_t)q * n + i] : gather.self(i);
        vb[q] = inb ? valb[(size_t)q * n + i] : 0.0;
      }
      for (int c = 0; c < m; ++c) {
        const size_t o = (size_t)c * n + i;
        const auto xc = gather.column(c);
        const auto held = ep.load(o);
        double sa = 0.0, sb = 0.0;
#pragma unroll
        for (int q = 0; q < W; ++q) sa += va[q] * Gather::at(xc, ca[q]);
#pragma unroll
        for (int q = 0; q < W; ++q) sb += vb[q] * Gather::at(xc, cb[q]);
        ep.store(o, held, sa, sb);
      }
    } else {
      for (int c = 0; c < m; ++c) {
        const size_t o = (size_t)c * n + i;
        const auto xc = gather.column(c);
        const auto held = ep.load(o);
        double sa = 0.0, sb = 0.0;
        for (int q = 0; q < wa; ++q) sa += vala[(size_t)q * n + i] * Gather::at(xc, cola[(size_t)q * n + i]);
        for (int q = 0; q < wb; ++q) sb += valb[(size_t)q * n + i] * Gather::at(xc, colb[(size_t)q * n + i]);
        ep.store(o, held, sa, sb);
      }
    }
  }
}
template <int W>
__global__ __launch_bounds__(256) void ell_cheb_pencil_step_kernel(int n, int m, int wa, const int* __restrict__ cola,
                                                                   const double* __restrict__ vala, int wb, const int* __restrict__ colb,
                                                                   const double* __restrict__ valb, dla::ChebStep k, const double* u,
                                                                   const double* v, const double* y, double* out, double fac,
                                                                   const double* __restrict__ r)
{
  ell_pair_rows<W>(n, m, wa, cola, vala, wb, colb, valb, GatherPlain{u, n}, ChebStepEpilogue<CHEB_SCALED>{k, u, v, y, out, fac, r, nullptr});
}
// sell_spmm_kernel<MC> with the same epilogue for the rows of the slices; tail slots and slots past n store nothing
template <int MC, int F>
__global__ __launch_bounds__(256) void sell_cheb_step_kernel(int n, int m, int slices, const long long* __restrict__ slice_ptr,
                                                             const int* __restrict__ perm, const int* __restrict__ col,
                                                             const double* __restrict__ val, dla::ChebStep kc, const double* u,
                                                             const double* v, const double* x, double* out, double fac,
                                                             const double* __restrict__ r, const double* __restrict__ bu)
{
  const int lane = threadIdx.x & 63;
  for (int s = blockIdx.x * 4 + (threadIdx.x >> 6); s < slices; s += gridDim.x * 4) {
    const long long p0 = slice_ptr[s];
    const int width = (int)((slice_ptr[s + 1] - p0) >> 6);
    const int slot = s * 64 + lane;
    const int row = slot < n ? perm[slot] : -1;
    const int* cs = col + p0 + lane;
    const double* vs = val + p0 + lane;
    double ri = 0.0;
    if constexpr (F != CHEB_PLAIN) ri = row >= 0 ? r[row] : 0.0;
    for (int c0 = 0; c0 < m; c0 += MC) {
      const double* uc = u + (size_t)c0 * n;
      double acc[MC], ui[MC], vi[MC], xi[MC], bi[MC];
#pragma unroll
      for (int k = 0; k < MC; ++k) {
        acc[k] = 0.0;
        const bool live = row >= 0 && c0 + k < m;
        const size_t o = live ? (size_t)(c0 + k) * n + row : 0;
        ui[k] = live ? u[o] : 0.0; vi[k] = live ? v[o] : 0.0; xi[k] = live ? x[o] : 0.0;
        bi[k] = 0.0;
        if constexpr (F == CHEB_PENCIL) bi[k] = live ? bu[o] : 0.0;
      }
      if (c0 + MC <= m) {
        for (int q = 0; q < width; ++q) {
          const int cj = cs[(size_t)q * 64];
          const double vj = vs[(size_t)q * 64];
#pragma unroll
          for (int k = 0; k < MC; ++k) acc[k] = fma(vj, uc[(size_t)k * n + cj], acc[k]);
        }
      } else {
        const int mc = m - c0;
        for (int q = 0; q < width; ++q) {
          const int cj = cs[(size_t)q * 64];
          const double vj = vs[(size_t)q * 64];
#pragma unroll
          for (int k = 0; k < MC; ++k) if (k < mc) acc[k] = fma(vj, uc[(size_t)k * n + cj], acc[k]);
        }
      }
      if (row >= 0) {
#pragma unroll
        for (int k = 0; k < MC; ++k)
          if (c0 + k < m) __builtin_nontemporal_store(cheb_epilogue<F>(kc, fac, ri, ui[k], vi[k], xi[k], acc[k], bi[k]), out + (size_t)(c0 + k) * n + row);
      }
    }
  }
}
// the rows of the CSR tail: csr_long_segments_kernel / long_rows_combine_kernel have left (A u)[row] in the scratch panel au; one
// thread per (tail row, column) forms the combination for those rows only
template <int F>
__global__ __launch_bounds__(256) void tail_cheb_combine_kernel(int n, int m, int nlong, const int* __restrict__ long_row, dla::ChebStep k,
                                                                const double* u, const double* v, const double* x,
                                                                const double* __restrict__ au, double* out, double fac,
                                                                const double* __restrict__ r, const double* __restrict__ bu)
{
  const long long total = (long long)nlong * m;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const int j = (int)(t / m), c = (int)(t - (long long)j * m);
    const int row = long_row[j];
    const size_t o = (size_t)c * n + row;
    double ri = 0.0, bo = 0.0;
    if constexpr (F != CHEB_PLAIN) ri = r[row];
    if constexpr (F == CHEB_PENCIL) bo = bu[o];
    out[o] = cheb_epilogue<F>(k, fac, ri, u[o], v[o], x[o], au[o], bo);
  }
}
// the un-fused step (A/B comparand, Knobs::cheb_unfused): the product kernel has written A u to the panel au; one sweep combines
__global__ __launch_bounds__(256) void cheb_combine_kernel(size_t total, dla::ChebStep k, const double* u, const double* v, const double* x,
                                                           const double* __restrict__ au, double* out)
{
  for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (size_t)gridDim.x * 256)
    out[o] = cheb_combine(k, u[o], v[o], x[o], au[o]);
}
// ... of the scaled form: one thread per row, r_i in a register across the m columns
__global__ __launch_bounds__(256) void cheb_jacobi_combine_kernel(int n, int m, dla::ChebStep k, double fac, const double* __restrict__ r,
                                                                  const double* u, const double* v, const double* y,
                                                                  const double* __restrict__ au, double* out)
{
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const double ri = r[i];
    for (int c = 0; c < m; ++c) {
      const size_t o = (size_t)c * n + i;
      out[o] = cheb_jacobi_combine(k, fac, ri, u[o], v[o], y[o], au[o]);
    }
  }
}
// ... of the pencil form: A u and B u both come from panels
__global__ __launch_bounds__(256) void cheb_pencil_combine_kernel(int n, int m, dla::ChebStep k, double fac, const double* __restrict__ r,
                                                                  const double* u, const double* v, const double* y,
                                                                  const double* __restrict__ au, const double* __restrict__ bu, double* out)
{
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const double ri = r[i];
    for (int c = 0; c < m; ++c) {
      const size_t o = (size_t)c * n + i;
      out[o] = cheb_pencil_combine(k, fac, ri, u[o], v[o], y[o], au[o], bu[o]);
    }
  }
}
// the scale sweep of the scaled form and of the pencil form: y = x o r, or with one step (DIV) px = (x o r) / theta at once
template <bool DIV>
__global__ __launch_bounds__(256) void cheb_jacobi_scale_kernel(int n, int m, double theta, const double* __restrict__ r,
                                                                const double* __restrict__ x, double* __restrict__ y)
{
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const double ri = r[i];
    for (int c = 0; c < m; ++c) {
      const size_t o = (size_t)c * n + i;
      const double t = x[o] * ri;
      if constexpr (DIV) y[o] = t / theta; else y[o] = t;
    }
  }
}
// one step (d = 1): px = x / theta
__global__ __launch_bounds__(256) void cheb_scale_kernel(size_t total, double theta, const double* __restrict__ x, double* __restrict__ px)
{
  for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (size_t)gridDim.x * 256) px[o] = x[o] / theta;
}
// The Gershgorin bound of the stored matrix: g_i = diag[i] + sum of |v| over the entries of row i whose column is not i, in stored
// order from 0.0 (padding is a zero on the row's own column).  Every block leaves the maximum over its rows in partial[block]; the
// host takes the maximum of those.  A maximum does not depend on the order it is taken in, so no atomics and the same bits always.
__device__ __forceinline__ void block_max_store(double g, double* __restrict__ partial)
{
  __shared__ double wave_max[4];
  for (int off = 32; off > 0; off >>= 1) g = fmax(g, __shfl_xor(g, off, 64));
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = g;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = fmax(fmax(wave_max[0], wave_max[1]), fmax(wave_max[2], wave_max[3]));
}
// ROWS: the same sums written per row, off[row] (the scaled form's off-diagonal row sums), in place of the block maximum in `partial`
template <bool ROWS>
__global__ __launch_bounds__(256) void ell_gershgorin_kernel(int n, int w, const int* __restrict__ col, const double* __restrict__ val,
                                                             const double* __restrict__ diag, double* __restrict__ partial,
                                                             double* __restrict__ off)
{
  double g = -INFINITY;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    double s = 0.0;
    for (int q = 0; q < w; ++q) if (col[(size_t)q * n + i] != i) s += fabs(val[(size_t)q * n + i]);
    if constexpr (ROWS) off[i] = s; else g = fmax(g, diag[i] + s);
  }
  if constexpr (!ROWS) block_max_store(g, partial);
}
template <bool ROWS>
__global__ __launch_bounds__(256) void sell_gershgorin_kernel(int n, int slices, const long long* __restrict__ slice_ptr,
                                                              const int* __restrict__ perm, const int* __restrict__ col,
                                                              const double* __restrict__ val, const double* __restrict__ diag,
                                                              double* __restrict__ partial, double* __restrict__ off)
{
  const int lane = threadIdx.x & 63;
  double g = -INFINITY;
  for (int s = blockIdx.x * 4 + (threadIdx.x >> 6); s < slices; s += gridDim.x * 4) {
    const long long p0 = slice_ptr[s];
    const int width = (int)((slice_ptr[s + 1] - p0) >> 6);
    const int slot = s * 64 + lane;
    const int row = slot < n ? perm[slot] : -1;
    if (row < 0) continue;        // (a tail row: tail_gershgorin_kernel; or a slot past n)
    double sum = 0.0;
    for (int q = 0; q < width; ++q) if (col[p0 + (long long)q * 64 + lane] != row) sum += fabs(val[p0 + (long long)q * 64 + lane]);
    if constexpr (ROWS) off[row] = sum; else g = fmax(g, diag[row] + sum);
  }
  if constexpr (!ROWS) block_max_store(g, partial);
}
// ... and the rows of the tail, one wavefront per ROW whatever the number of its segments: lane l takes entries l, l + 64, ... of the
// row from 0.0, then the butterfly of the product's segments.  col / val: the tail's entries (behind the slices')
template <bool ROWS>
__global__ __launch_bounds__(256) void tail_gershgorin_kernel(int nlong, const long long* __restrict__ long_ptr, const int* __restrict__ long_row,
                                                              const int* __restrict__ col, const double* __restrict__ val,
                                                              const double* __restrict__ diag, double* __restrict__ partial,
                                                              double* __restrict__ off)
{
  const int lane = threadIdx.x & 63;
  double g = -INFINITY;
  for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < nlong; r += gridDim.x * 4) {
    const int row = long_row[r];
    double sum = 0.0;
    for (long long p = long_ptr[r] + lane; p < long_ptr[r + 1]; p += 64) if (col[p] != row) sum += fabs(val[p]);
    for (int sh = 32; sh > 0; sh >>= 1) sum += __shfl_xor(sum, sh, 64);
    if constexpr (ROWS) { if (lane == 0) off[row] = sum; } else g = fmax(g, diag[row] + sum);
  }
  if constexpr (!ROWS) block_max_store(g, partial);
}
// The bound of the scaled form for one fac (the contract: include/diaglib_amd.h, dla_spmm_precnd_cheb_jacobi): s_i = |diag[i] + fac|,
// den_i = s_i where s_i > 1e-5 and 1.0 otherwise, r[i] = 1.0 / den_i, q_i = (s_i + off[i]) / den_i; partial[block] = max q_i.
__global__ __launch_bounds__(256) void cheb_jacobi_bound_kernel(int n, double fac, const double* __restrict__ diag, const double* __restrict__ off,
                                                                double* __restrict__ r, double* __restrict__ partial)
{
  double g = -INFINITY;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const double s = fabs(diag[i] + fac);
    const double den = s > 1.0e-5 ? s : 1.0;
    r[i] = 1.0 / den;
    g = fmax(g, (s + off[i]) / den);
  }
  block_max_store(g, partial);
}
// The bound of the pencil form for one fac (the contract: include/diaglib_amd.h, dla_spmm_precnd_cheb_pencil): den0_i = a_ii + fac b_ii
// with the product rounded before the sum (no contraction: the bits pencil_precnd_kernel divides by), s_i = |den0_i|, den_i and r[i]
// as above, q_i = fma(|fac|, offB_i, s_i + offA_i) / den_i; partial[block] = max q_i.  With b_ii = 1 and offB = 0 every value has the
// bits of cheb_jacobi_bound_kernel.
__global__ __launch_bounds__(256) void cheb_pencil_bound_kernel(int n, double fac, const double* __restrict__ a_diag, const double* __restrict__ b_diag,
                                                                const double* __restrict__ off_a, const double* __restrict__ off_b,
                                                                double* __restrict__ r, double* __restrict__ partial)
{
#pragma clang fp contract(off)
  double g = -INFINITY;
  const double af = fabs(fac);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const double prod = fac * b_diag[i];
    const double s = fabs(a_diag[i] + prod);
    const double den = s > 1.0e-5 ? s : 1.0;
    r[i] = 1.0 / den;
    const double sa = s + off_a[i];
    g = fmax(g, fma(af, off_b[i], sa) / den);
  }
  block_max_store(g, partial);
}

// ---- the same two formats filled from CSR arrays that are already in DEVICE memory (dla_spmm_setup_csr_dev), and new values for a
// stored pattern (dla_spmm_refresh_values_dev).  The host keeps what depends on the row lengths alone (dla::sell_layout on the
// downloaded row pointers); everything proportional to the number of entries happens here.  Every output element has one writer; the
// only atomic is the OR into one flag word ("a column is out of range" / "the pattern differs").  Where each entry goes is spelled
// once, in the three walkers below: f(d, p, i) is called for every stored element d of the blocks with the position p of its entry
// in the caller's arrays, or p = -1 for padding, which is a zero that points at row i.  The fill kernels, their value-only
// variants and the comparison of a refresh all go through them.  Positions are rowptr[i] + shift + q: shift is 0 at set-up and, at a
// refresh, the distance between the caller's first row pointer and the stored one (the stored row pointers then index the
// caller's arrays, whose entry count has been checked, so no read leaves them whatever the caller's row pointers hold).
// ELLPACK, col[q n + i]: a wavefront on 64 consecutive rows, so the stores of one q are full rows of 256 / 512 bytes and the CSR
// reads are the strided side (each lane walks its own row; neighbouring lanes of a stencil's rows sit w entries apart).
template <class F>
__device__ __forceinline__ void ell_walk(int n, int w, const long long* __restrict__ rowptr, long long shift, F f)
{
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const long long p0 = rowptr[i] + shift, len = rowptr[i + 1] - rowptr[i];
    for (int q = 0; q < w; ++q) f((size_t)q * n + i, q < len ? p0 + q : -1LL, i);
  }
}
// sliced ELLPACK: one wavefront per slice, entry (q, lane) at slice_ptr[s] + 64 q + lane; a tail row asks nothing of its slice and
// slots past n point at row 0, exactly as dla::sell_fill pads
template <class F>
__device__ __forceinline__ void sell_walk(int n, int slices, const long long* __restrict__ slice_ptr, const int* __restrict__ perm,
                                          const long long* __restrict__ rowptr, long long shift, F f)
{
  const int lane = threadIdx.x & 63;
  for (int s = blockIdx.x * 4 + (threadIdx.x >> 6); s < slices; s += gridDim.x * 4) {
    const long long base = slice_ptr[s];
    const int width = (int)((slice_ptr[s + 1] - base) >> 6);
    const int slot = s * 64 + lane;
    const int pr = slot < n ? perm[slot] : 0;
    const int i = pr < 0 ? ~pr : pr;
    const int li = (slot < n && pr >= 0) ? (int)(rowptr[i + 1] - rowptr[i]) : 0;
    const long long p0 = rowptr[i] + shift;
    for (int q = 0; q < width; ++q) f((size_t)(base + (long long)q * 64 + lane), q < li ? p0 + q : -1LL, i);
  }
}
// the CSR tail behind the slices: one wavefront per segment, lanes striding over its entries (both sides coalesced); entry t of the
// tail is entry t - long_ptr[r] of its row
template <class F>
__device__ __forceinline__ void tail_walk(int nseg, long long stored, const long long* __restrict__ seg_ptr, const int* __restrict__ seg_row,
                                          const int* __restrict__ long_row, const long long* __restrict__ long_ptr,
                                          const long long* __restrict__ rowptr, long long shift, F f)
{
  const int lane = threadIdx.x & 63;
  for (int g = blockIdx.x * 4 + (threadIdx.x >> 6); g < nseg; g += gridDim.x * 4) {
    const int r = seg_row[g];
    const long long src0 = rowptr[long_row[r]] + shift - long_ptr[r];
    for (long long t = seg_ptr[g] + lane; t < seg_ptr[g + 1]; t += 64) f((size_t)(stored + t), src0 + t, long_row[r]);
  }
}

// every column of the caller's entries lies in [0, n): all entries, coalesced; runs (and is waited for) before any kernel indexes with them
__global__ __launch_bounds__(256) void csr_check_cols_kernel(long long nnz, const int* __restrict__ colind, int n, unsigned* __restrict__ flag)
{
  bool bad = false;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < nnz; p += (long long)gridDim.x * 256) {
    const int c = colind[p];
    bad |= c < 0 || c >= n;
  }
  if (bad) atomicOr(flag, 1u);
}
// VALS_ONLY: the columns stay as they are (refresh)
template <bool VALS_ONLY>
__global__ __launch_bounds__(256) void ell_fill_kernel(int n, int w, const long long* __restrict__ rowptr, long long shift,
                                                       const int* __restrict__ colind, const double* __restrict__ values,
                                                       int* __restrict__ col, double* __restrict__ val)
{
  ell_walk(n, w, rowptr, shift, [&](size_t d, long long p, int i) {
    if constexpr (!VALS_ONLY) col[d] = p >= 0 ? colind[p] : i;
    val[d] = p >= 0 ? values[p] : 0.0;
  });
}
template <bool VALS_ONLY>
__global__ __launch_bounds__(256) void sell_fill_kernel(int n, int slices, const long long* __restrict__ slice_ptr, const int* __restrict__ perm,
                                                        const long long* __restrict__ rowptr, long long shift, const int* __restrict__ colind,
                                                        const double* __restrict__ values, int* __restrict__ col, double* __restrict__ val)
{
  sell_walk(n, slices, slice_ptr, perm, rowptr, shift, [&](size_t d, long long p, int i) {
    if constexpr (!VALS_ONLY) col[d] = p >= 0 ? colind[p] : i;
    val[d] = p >= 0 ? values[p] : 0.0;
  });
}
template <bool VALS_ONLY>
__global__ __launch_bounds__(256) void tail_copy_kernel(int nseg, long long stored, const long long* __restrict__ seg_ptr,
                                                        const int* __restrict__ seg_row, const int* __restrict__ long_row,
                                                        const long long* __restrict__ long_ptr, const long long* __restrict__ rowptr, long long shift,
                                                        const int* __restrict__ colind, const double* __restrict__ values,
                                                        int* __restrict__ col, double* __restrict__ val)
{
  tail_walk(nseg, stored, seg_ptr, seg_row, long_row, long_ptr, rowptr, shift, [&](size_t d, long long p, int) {
    if constexpr (!VALS_ONLY) col[d] = colind[p];
    val[d] = values[p];
  });
}
// diag[i] = the sum of the (i, i) entries in the caller's order, from 0.0, plain additions: the bits of the host set-up.  A
// wavefront takes 64 consecutive rows.  Each lane walks its own row while that row has at most long_len entries; a longer one is
// never walked by one thread (a dense row of 2e6 entries took 180 ms that way in the product): the whole
// wavefront scans it 64 entries at a time, in order, and adds the matches of each scan in ascending entry order.
__global__ __launch_bounds__(256) void csr_diag_kernel(int n, int long_len, const long long* __restrict__ rowptr, long long shift,
                                                       const int* __restrict__ colind, const double* __restrict__ values,
                                                       double* __restrict__ diag)
{
  const int lane = threadIdx.x & 63;
  for (long long base = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; base < n; base += (long long)gridDim.x * 256) {
    const int i = (int)base + lane;
    const bool live = i < n;
    const long long p0 = live ? rowptr[i] + shift : 0, len = live ? rowptr[i + 1] - rowptr[i] : 0;
    const bool whole_wave = len > long_len;
    double d = 0.0;
    if (!whole_wave)
      for (long long p = p0; p < p0 + len; ++p) if (colind[p] == i) d += values[p];
    unsigned long long todo = __ballot(whole_wave);
    while (todo) {
      const int b = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const long long q0 = __shfl(p0, b, 64), q1 = q0 + __shfl(len, b, 64);
      const int row = (int)base + b;
      double sum = 0.0;
      for (long long p = q0; p < q1; p += 64) {
        const bool hit = p + lane < q1 && colind[p + lane] == row;
        const double v = hit ? values[p + lane] : 0.0;
        unsigned long long hits = __ballot(hit);
        while (hits) {
          const int h = __ffsll((long long)hits) - 1;
          hits &= hits - 1;
          sum += __shfl(v, h, 64);
        }
      }
      if (lane == b) d = sum;
    }
    if (live) diag[i] = d;
  }
}
// refresh: is the caller's pattern the stored one?  Read-only.  Bit 1 of the flag: a row of the caller's row pointers has another
// length than the stored row; bit 2: a stored column differs from the caller's, looked up through the walkers that filled it
// (stored row pointers, see above).  SELL: the slices and the tail; else ELLPACK.
template <bool SELL>
__global__ __launch_bounds__(256) void pattern_compare_kernel(int n, int w, int slices, int nseg, long long stored,
                                                              const long long* __restrict__ slice_ptr, const int* __restrict__ perm,
                                                              const long long* __restrict__ seg_ptr, const int* __restrict__ seg_row,
                                                              const int* __restrict__ long_row, const long long* __restrict__ long_ptr,
                                                              const long long* __restrict__ rowptr, long long shift,
                                                              const long long* __restrict__ rowptr_new, const int* __restrict__ colind,
                                                              const int* __restrict__ col, unsigned* __restrict__ flag)
{
  unsigned bad = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
    if (rowptr_new[i + 1] - rowptr_new[i] != rowptr[i + 1] - rowptr[i]) bad |= 1u;
  auto same = [&](size_t d, long long p, int) { if (p >= 0 && col[d] != colind[p]) bad |= 2u; };
  if constexpr (SELL) {
    sell_walk(n, slices, slice_ptr, perm, rowptr, shift, same);
    tail_walk(nseg, stored, seg_ptr, seg_row, long_row, long_ptr, rowptr, shift, same);
  } else {
    ell_walk(n, w, rowptr, shift, same);
  }
  if (bad) atomicOr(flag, bad);
}

// ---- building the transposed index of a stored matrix (dla_spmm_transpose_prepare; dla::TransposeIndex is the host twin).  The
// entries never leave the device, and no result depends on the arrival order of anything: every element below has one writer.
// Pass 1, over A's own layout through the walkers that filled it (the stored row pointers, shift 0): entry e = p - rowptr[0] of the
// caller's arrays learns its column (the sort key), its row and the position d of its value in A's blocks; ident[e] = e is the
// sort's payload.
template <bool SELL>
__global__ __launch_bounds__(256) void stored_positions_kernel(int n, int w, int slices, int nseg, long long stored,
                                                               const long long* __restrict__ slice_ptr, const int* __restrict__ perm,
                                                               const long long* __restrict__ seg_ptr, const int* __restrict__ seg_row,
                                                               const int* __restrict__ long_row, const long long* __restrict__ long_ptr,
                                                               const long long* __restrict__ rowptr, const int* __restrict__ col,
                                                               int* __restrict__ key, int* __restrict__ ident, int* __restrict__ erow,
                                                               int* __restrict__ epos)
{
  const long long first = rowptr[0];
  auto note = [&](size_t d, long long p, int i) {
    if (p < 0) return;
    const long long e = p - first;
    key[e] = col[d]; ident[e] = (int)e; erow[e] = i; epos[e] = (int)d;
  };
  if constexpr (SELL) {
    sell_walk(n, slices, slice_ptr, perm, rowptr, 0, note);
    tail_walk(nseg, stored, seg_ptr, seg_row, long_row, long_ptr, rowptr, 0, note);
  } else {
    ell_walk(n, w, rowptr, 0, note);
  }
}
// Pass 2 (behind the stable sort of (key, ident) by key): the column pointers from the sorted keys.  Entry k writes colptr[c] = k for
// every column c in (key[k - 1], key[k]] -- its own column and the empty ones in front of it -- and the last entry closes the rest.
__global__ __launch_bounds__(256) void column_pointers_kernel(long long nnz, int n, const int* __restrict__ key, long long* __restrict__ colptr)
{
  for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < nnz; k += (long long)gridDim.x * 256) {
    const int c1 = key[k];
    for (int c = k > 0 ? key[k - 1] + 1 : 0; c <= c1; ++c) colptr[c] = k;
    if (k == nnz - 1)
      for (int c = c1 + 1; c <= n; ++c) colptr[c] = nnz;
  }
}
// Pass 3, over the INDEX's layout through the same walkers, with the column pointers as its row pointers: element d takes the k-th
// entry in sorted order, or padding (position -1, the column itself as its row)
template <bool SELL>
__global__ __launch_bounds__(256) void transpose_fill_kernel(int n, int w, int slices, int nseg, long long stored,
                                                             const long long* __restrict__ slice_ptr, const int* __restrict__ perm,
                                                             const long long* __restrict__ seg_ptr, const int* __restrict__ seg_row,
                                                             const int* __restrict__ long_row, const long long* __restrict__ long_ptr,
                                                             const long long* __restrict__ colptr, const int* __restrict__ sorted,
                                                             const int* __restrict__ erow, const int* __restrict__ epos,
                                                             int* __restrict__ trow, int* __restrict__ tpos)
{
  auto place = [&](size_t d, long long k, int j) {
    const int e = k >= 0 ? sorted[k] : 0;
    trow[d] = k >= 0 ? erow[e] : j;
    tpos[d] = k >= 0 ? epos[e] : -1;
  };
  if constexpr (SELL) {
    sell_walk(n, slices, slice_ptr, perm, colptr, 0, place);
    tail_walk(nseg, stored, seg_ptr, seg_row, long_row, long_ptr, colptr, 0, place);
  } else {
    ell_walk(n, w, colptr, 0, place);
  }
}

// px = x / (d + fac) where |d + fac| > 1e-5, else x: the harness' diagonal preconditioner (main.f90:161-169) on the
// diagonal of the sparse operator
__global__ void diag_precnd_kernel(int n, int m, double fac, const double* __restrict__ diag, const double* __restrict__ x,
                                   double* __restrict__ px)
{
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const double den = diag[i] + fac;
    const bool use = fabs(den) > 1.0e-5;
    for (int c = 0; c < m; ++c) {
      const double v = x[(size_t)c * n + i];
      px[(size_t)c * n + i] = use ? v / den : v;
    }
  }
}

// px = x / (a_ii + fac b_ii) where |a_ii + fac b_ii| > 1e-5, else x: the same preconditioner on the diagonal of the pencil
// A - lambda B (fac = -lambda), for a context that holds a sparse metric beside its operator.  The product fac b_ii is rounded
// before the sum (no contraction into a fused multiply-add): den is what a host caller gets from the same expression, also where
// the two terms cancel.  16 n m bytes of vectors + 16 n bytes of the two diagonals.
__global__ void pencil_precnd_kernel(int n, int m, double fac, const double* __restrict__ a_diag, const double* __restrict__ b_diag,
                                     const double* __restrict__ x, double* __restrict__ px)
{
#pragma clang fp contract(off)
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const double den = a_diag[i] + fac * b_diag[i];
    const bool use = fabs(den) > 1.0e-5;
    for (int c = 0; c < m; ++c) {
      const double v = x[(size_t)c * n + i];
      px[(size_t)c * n + i] = use ? v / den : v;
    }
  }
}

// ---- the dense operator and metric (the contract: include/diaglib_amd.h, dla_dense_setup; layout and plan: hip_plans.h, dense_plan)
// The library's copy of a column-major a(lda, n) in device memory: one thread per STORED element, so the writes are contiguous and
// every padded element gets its 0.0; the reads walk 16 consecutive rows of a column.  The same map as dense_pack on the host.
__global__ void dense_pack_kernel(int n, int n_pad, const double* __restrict__ a, size_t lda, double* __restrict__ stored)
{
  const size_t total = (size_t)n_pad * n_pad, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t d = (size_t)blockIdx.x * blockDim.x + threadIdx.x; d < total; d += stride) {
    const int i = dense_row_of(n_pad, d), k = dense_col_of(n_pad, d);
    stored[d] = (i < n && k < n) ? a[(size_t)k * lda + i] : 0.0;
  }
}
__global__ void dense_diag_kernel(int n, const double* __restrict__ a, size_t lda, double* __restrict__ diag)
{
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) diag[i] = a[(size_t)i * lda + i];
}
// The copies of p + q and p - q of two column-major arrays p(ldp, n), q(ldq, n) at once (dla_dense_setup_lr_pair_dev): the same
// thread-to-element map as dense_pack_kernel, every source element loaded once and used for both copies, one rounded addition and
// one rounded subtraction (nothing here can contract), both writes contiguous, 0.0 in the padding.  The host twin: dense_pack_pair.
__global__ void dense_pack_pair_kernel(int n, int n_pad, const double* __restrict__ p, size_t ldp, const double* __restrict__ q, size_t ldq,
                                       double* __restrict__ sum, double* __restrict__ dif)
{
  const size_t total = (size_t)n_pad * n_pad, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t d = (size_t)blockIdx.x * blockDim.x + threadIdx.x; d < total; d += stride) {
    const int i = dense_row_of(n_pad, d), k = dense_col_of(n_pad, d);
    const bool in = i < n && k < n;
    const double pv = in ? p[(size_t)k * ldp + i] : 0.0, qv = in ? q[(size_t)k * ldq + i] : 0.0;
    sum[d] = in ? pv + qv : 0.0;
    dif[d] = in ? pv - qv : 0.0;
  }
}
__global__ void dense_diag_pair_kernel(int n, const double* __restrict__ p, size_t ldp, const double* __restrict__ q, size_t ldq,
                                       double* __restrict__ sum_diag, double* __restrict__ dif_diag)
{
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const double pv = p[(size_t)i * ldp + i], qv = q[(size_t)i * ldq + i];
    sum_diag[i] = pv + qv;
    dif_diag[i] = pv - qv;
  }
}

// One pass Y(n x m) = A X, m <= 16 G, on the stored copy, RT = DENSE_WAVE_TILES.  Block (bx, by): four wavefronts, wavefront w owns the RT row
// tiles of row group 4 bx + w and all of them contraction chunk by (groups [by chunk_groups, ...)): the four read the same
// fragments of X at about the same time.  Per group a wavefront loads RT x 1024 contiguous bytes of A (one 16-byte
// load per lane and tile, no bounds check: a row group that reaches beyond the last tile reads that tile again and stores
// nothing for it) and 2 G doubles of X per lane, and issues 2 G RT v_mfma_f64_16x16x4 with X as the A operand
// (lane: column lane & 15 of the group, contraction index lane >> 4) and the matrix as the B operand: the accumulator of lane l then
// holds matrix row l & 15 for the columns (l >> 4) + 4 r, so a store writes 16 consecutive rows of four columns.
// X has leading dimension n, which may be odd: its elements are loaded one by one (8-byte alignment is all they have), and indices
// at or beyond n -- where the stored copy holds zeros -- are not loaded at all.
// k_chunks = 1 (gridDim.y == 1): the result goes to y.  Otherwise chunk by goes to ws[by][m][n], for dense_combine_kernel.
template <int G>
__global__ __launch_bounds__(256) void dense_mfma_kernel(int n, int m, int n_pad, int chunk_groups, const double* __restrict__ a,
                                                          const double* __restrict__ x, double* __restrict__ y, double* __restrict__ ws)
{
  constexpr int RT = DENSE_WAVE_TILES;
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const int row_tiles = n_pad / DENSE_TILE, groups = n_pad / DENSE_GROUP;
  const int tile0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * RT;
  if (tile0 >= row_tiles) return;
  const int g0 = blockIdx.y * chunk_groups, g1 = min(groups, g0 + chunk_groups);
  const v2d* ap[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) ap[t] = (const v2d*)a + (size_t)min(tile0 + t, row_tiles - 1) * groups * 64 + lane;
  const double* xp[G];
  bool xin[G];
#pragma unroll
  for (int q = 0; q < G; ++q) {
    xin[q] = 16 * q + li < m;
    xp[q] = x + (size_t)(xin[q] ? 16 * q + li : 0) * n + lk;
  }
  v4d acc[RT][G];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int q = 0; q < G; ++q) acc[t][q] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
  for (int g = g0; g < g1; ++g) {
    v2d av[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) av[t] = ap[t][(size_t)g * 64];
    const int k = DENSE_GROUP * g + lk;
    double xv[G][2];
#pragma unroll
    for (int q = 0; q < G; ++q) {
      xv[q][0] = (xin[q] && k < n) ? xp[q][DENSE_GROUP * g] : 0.0;
      xv[q][1] = (xin[q] && k + 4 < n) ? xp[q][DENSE_GROUP * g + 4] : 0.0;
    }
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int q = 0; q < G; ++q)
#pragma unroll
        for (int t = 0; t < RT; ++t) acc[t][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(xv[q][e], av[t][e], acc[t][q], 0, 0, 0);
  }
  double* dst = gridDim.y == 1 ? y : ws + (size_t)blockIdx.y * m * n;
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int row = (tile0 + t) * DENSE_TILE + li;
    if (tile0 + t >= row_tiles || row >= n) continue;
#pragma unroll
    for (int q = 0; q < G; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = 16 * q + lk + 4 * r;
        if (c < m) dst[(size_t)c * n + row] = acc[t][q][r];
      }
  }
}
// One pass Y(n x m) = A^T X, m <= 16 G, on the same stored copy (plan: hip_plans.h, dense_t_plan).  The contraction now runs over the
// rows of the matrix, which are lane & 15 of a stored group -- an MFMA output index as the group is loaded -- so every 16 x 16 block
// of the matrix (two adjacent groups, 2 KB) is turned in LDS: the wavefront stores its loads lane-linearly (16 bytes per lane) into a
// region of its own and reads them back one double per lane as the B operand of v_mfma_f64_16x16x4, lane (k = lane >> 4,
// j = lane & 15) taking a(16 t + 4 s + k, 16 b + j) for step s = 0 .. 3 of row tile t.  X is the A operand as in dense_mfma_kernel
// (lane: column lane & 15 of the group, row 16 t + 4 s + (lane >> 4)), so the accumulator of lane l holds output index (matrix
// column) 16 b + (l & 15) for the columns (l >> 4) + 4 r of the group, and a store writes 16 consecutive elements of four columns.
// Block (bx, by): four wavefronts, wavefront w owns the DENSE_T_WAVE_BLOCKS column blocks of strip 4 bx + w -- 8 adjacent groups, 8 KB
// contiguous per row tile -- and all four walk the row tiles of chunk by, reading the same fragments of X at about the same time.
// No block-wide barrier: a wavefront touches its own LDS region only, and LDS operations of one wavefront complete in order.
// A strip that reaches beyond the last column block reads that block again and stores nothing for it; rows of X at or beyond n
// (where the stored copy holds zeros) and columns at or beyond m are not loaded.
// row_chunks = 1 (gridDim.y == 1): the result goes to y.  Otherwise chunk by goes to ws[by][m][n], for dense_combine_kernel.
template <int G>
__global__ __launch_bounds__(256) void dense_t_mfma_kernel(int n, int m, int n_pad, int chunk_tiles, const double* __restrict__ a,
                                                            const double* __restrict__ x, double* __restrict__ y, double* __restrict__ ws)
{
  constexpr int W = DENSE_T_WAVE_BLOCKS;
  __shared__ double turn[4][W * 256];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const int row_tiles = n_pad / DENSE_TILE, col_blocks = n_pad / 16, groups = n_pad / DENSE_GROUP;
  const int b0 = (blockIdx.x * 4 + wave) * W;
  if (b0 >= col_blocks) return;
  const int t0 = blockIdx.y * chunk_tiles, t1 = min(row_tiles, t0 + chunk_tiles);
  double* my = turn[wave];
  // the lane's 16-byte element of group 2 b + h in a row tile, and the double it reads back for step 0 of block w
  size_t aoff[W];
#pragma unroll
  for (int w = 0; w < W; ++w) aoff[w] = (size_t)(2 * min(b0 + w, col_blocks - 1)) * 64 + lane;
  const int back = (li >> 3) * 128 + (16 * (li & 3) + lk) * 2 + ((li >> 2) & 1);
  const double* xp[G];
  bool xin[G];
#pragma unroll
  for (int q = 0; q < G; ++q) {
    xin[q] = 16 * q + li < m;
    xp[q] = x + (size_t)(xin[q] ? 16 * q + li : 0) * n + lk;
  }
  v4d acc[W][G];
#pragma unroll
  for (int w = 0; w < W; ++w)
#pragma unroll
    for (int q = 0; q < G; ++q) acc[w][q] = v4d{0.0, 0.0, 0.0, 0.0};
  v2d av[W][2];
  {
    const v2d* at = (const v2d*)a + (size_t)t0 * groups * 64;
#pragma unroll
    for (int w = 0; w < W; ++w) { av[w][0] = at[aoff[w]]; av[w][1] = at[aoff[w] + 64]; }
  }
  for (int t = t0; t < t1; ++t) {
#pragma unroll
    for (int w = 0; w < W; ++w) {
      lds_store2(my + (2 * w) * 128 + 2 * lane, av[w][0]);
      lds_store2(my + (2 * w + 1) * 128 + 2 * lane, av[w][1]);
    }
    if (t + 1 < t1) {         // the next row tile's loads travel while this one is multiplied
      const v2d* at = (const v2d*)a + (size_t)(t + 1) * groups * 64;
#pragma unroll
      for (int w = 0; w < W; ++w) { av[w][0] = at[aoff[w]]; av[w][1] = at[aoff[w] + 64]; }
    }
    double xv[4][G];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int row = DENSE_TILE * t + 4 * s + lk;
#pragma unroll
      for (int q = 0; q < G; ++q) xv[s][q] = (xin[q] && row < n) ? xp[q][DENSE_TILE * t + 4 * s] : 0.0;
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const double bv = lds_load1(my + w * 256 + back + 8 * s);
#pragma unroll
        for (int q = 0; q < G; ++q) acc[w][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(xv[s][q], bv, acc[w][q], 0, 0, 0);
      }
    __builtin_amdgcn_wave_barrier();
  }
  double* dst = gridDim.y == 1 ? y : ws + (size_t)blockIdx.y * m * n;
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const int col = (b0 + w) * 16 + li;
    if (b0 + w >= col_blocks || col >= n) continue;
#pragma unroll
    for (int q = 0; q < G; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = 16 * q + lk + 4 * r;
        if (c < m) dst[(size_t)c * n + col] = acc[w][q][r];
      }
  }
}
// y = ((p_0 + p_1) + p_2) + ... over the chunks of a split pass, in ascending chunk order, one thread per element
__global__ void dense_combine_kernel(size_t total, int k_chunks, const double* __restrict__ ws, double* __restrict__ y)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    double s = ws[i];
    for (int c = 1; c < k_chunks; ++c) s += ws[(size_t)c * total + i];
    y[i] = s;
  }
}

// ---- a symmetric dense matrix stored as one triangle (the contract: include/diaglib_amd.h, dla_dense_setup_sym; layout and plan:
// hip_plans.h, dense_sym_plan)
// The triangular copy of a column-major a(lda, n) in device memory of which only the triangle `lower` (or the upper one) is
// referenced: one thread per STORED element as in dense_pack_kernel, the same map as dense_sym_pack on the host.  Elements of a
// diagonal block that lie in the other triangle are read at their mirror position; padding gets 0.0.
__global__ void dense_sym_pack_kernel(int n, int n_pad, bool lower, const double* __restrict__ a, size_t lda, double* __restrict__ stored)
{
  const size_t total = dense_sym_doubles(n_pad), stride = (size_t)gridDim.x * blockDim.x;
  for (size_t d = (size_t)blockIdx.x * blockDim.x + threadIdx.x; d < total; d += stride) {
    const int i = dense_sym_row_of(d), k = dense_sym_col_of(d);
    stored[d] = (i < n && k < n) ? a[dense_sym_source(lda, lower, i, k)] : 0.0;
  }
}
// One pass Y(n x m) = A X, m <= 16 G, on the triangular copy (plan and workspace layout: hip_plans.h, dense_sym_plan).  Block
// (bx, by): panel P = gridDim.y - 1 - by (the long panels start first), chunk bx of its column blocks; a block whose chunk the panel
// does not have leaves at once.  Wavefront w owns the RT = DENSE_WAVE_TILES row tiles 16 P + 4 w .. + 3, and all four walk the
// column blocks of the chunk together.  For a stored block (T, b), b <= T, a wavefront loads the two groups once (16 bytes per lane
// each, no bounds check; a tile beyond the matrix or above the block's diagonal is not loaded at all -- the triangle stores
// nothing there) and uses them twice:
//   forward     the MFMAs of dense_mfma_kernel -- the X fragment of block b as the A operand, the loaded pair as the B operand --
//               into acc_f[tile][q], which stays in registers across the chunk: lane l holds row 16 T + (l & 15), columns (l >> 4) + 4 r;
//   transposed  for T > b only: the pair goes lane-linearly into the wavefront's own LDS region and comes back through the `back`
//               index of dense_t_mfma_kernel as the B operand, lane (k, j) taking a(16 T + 4 s + k, 16 b + j), against the X
//               fragment of row tile T (kept in registers for the whole chunk): acc_t[q] gathers the wavefront's tiles, lane l holding
//               row 16 b + (l & 15).
// After the tiles of a column block the four acc_t go to LDS (two buffers, taken in turn: one block-wide barrier per column block)
// and every thread adds one element per column group in wavefront order ((w0 + w1) + w2) + w3; where the panel has a tile below
// block b that sum is the panel's transposed partial of block b.  The forward partial of (panel, chunk) is written at the end.
// Everything goes to the workspace for dense_sym_combine_kernel, each element by one thread -- except a matrix of one tile
// (nt = 1: one block, nothing transposed), whose workgroup writes y.  Rows of X at or beyond n and columns at or beyond m are not
// loaded; nothing is stored for rows at or beyond n, columns at or beyond m, or tiles beyond the matrix.
template <int G>
__global__ __launch_bounds__(256) void dense_sym_mfma_kernel(int n, int m, int nt, int chunk_panels, size_t t_base, const double* __restrict__ a,
                                                              const double* __restrict__ x, double* __restrict__ y, double* __restrict__ ws)
{
  constexpr int RT = DENSE_WAVE_TILES;
  __shared__ double turn[4][256];
  __shared__ double sums[2][4][G * 256];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const int P = (int)gridDim.y - 1 - (int)blockIdx.y, c = blockIdx.x;
  if (c > P / chunk_panels) return;                       // (block-uniform, before any barrier)
  const int last = min(DENSE_SYM_PANEL_TILES * P + DENSE_SYM_PANEL_TILES - 1, nt - 1);   // the panel's last tile: its last column block
  const int b0 = DENSE_SYM_PANEL_TILES * chunk_panels * c, b1 = min(last + 1, b0 + DENSE_SYM_PANEL_TILES * chunk_panels);
  const int tile0 = DENSE_SYM_PANEL_TILES * P + RT * wave;
  double* my = turn[wave];
  const int back = (li >> 3) * 128 + (16 * (li & 3) + lk) * 2 + ((li >> 2) & 1);
  const double* xp[G];
  bool xin[G];
#pragma unroll
  for (int q = 0; q < G; ++q) {
    xin[q] = 16 * q + li < m;
    xp[q] = x + (size_t)(xin[q] ? 16 * q + li : 0) * n + lk;
  }
  // the X fragments of the wavefront's own row tiles: the A operand of every transposed step
  double xt[RT][4][G];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int row = DENSE_TILE * (tile0 + t) + 4 * s;
#pragma unroll
      for (int q = 0; q < G; ++q) xt[t][s][q] = (xin[q] && row + lk < n) ? xp[q][row] : 0.0;
    }
  v4d acc_f[RT][G];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int q = 0; q < G; ++q) acc_f[t][q] = v4d{0.0, 0.0, 0.0, 0.0};
  // What column block b needs from memory -- the pairs of the wavefront's tiles and the X fragment of the block -- is loaded one
  // column block ahead, all of it together and before anything of the current block is waited for (loads return in order).  ALL: the
  // wavefront's four tiles all lie in the matrix and strictly below the blocks b and b + 1, the common case, which then runs without
  // a branch; otherwise every tile is tested on its own (wavefront-uniform).
  v2d av[RT][2], nx[RT][2];
  double xf[2][2][G], nxf[2][2][G];
#pragma unroll
  for (int t = 0; t < RT; ++t) nx[t][0] = nx[t][1] = v2d{0.0, 0.0};
  const auto fetch = [&](auto all, int b) {
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int T = tile0 + t;
      if (decltype(all)::value || (T <= last && b <= T)) {
        const v2d* p = (const v2d*)a + ((size_t)T * (size_t)(T + 1) + (size_t)(2 * b)) * 64 + lane;
        nx[t][0] = p[0];
        nx[t][1] = p[64];
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int k = DENSE_TILE * b + DENSE_GROUP * h + 4 * e;
#pragma unroll
        for (int q = 0; q < G; ++q) nxf[h][e][q] = (xin[q] && k + lk < n) ? xp[q][k] : 0.0;
      }
  };
  const auto step = [&](auto all, int b) {
    constexpr bool ALL = decltype(all)::value;
#pragma unroll
    for (int t = 0; t < RT; ++t) { av[t][0] = nx[t][0]; av[t][1] = nx[t][1]; }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int q = 0; q < G; ++q) xf[h][e][q] = nxf[h][e][q];
    // (the last column block of a chunk fetches itself again: no branch, and the lines are in the cache)
    fetch(all, min(b + 1, b1 - 1));
    v4d acc_t[G];
#pragma unroll
    for (int q = 0; q < G; ++q) acc_t[q] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int T = tile0 + t;
      if (ALL || (T <= last && b <= T)) {
        // (the turn through LDS is issued first: its latency passes behind the forward MFMAs)
        const bool turned = ALL || T > b;
        double bv[4];
        if (turned) {
          lds_store2(my + 2 * lane, av[t][0]);
          lds_store2(my + 128 + 2 * lane, av[t][1]);
          __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (int s = 0; s < 4; ++s) bv[s] = lds_load1(my + back + 8 * s);
          __builtin_amdgcn_wave_barrier();
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int q = 0; q < G; ++q) acc_f[t][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(xf[h][e][q], av[t][h][e], acc_f[t][q], 0, 0, 0);
        if (turned) {
#pragma unroll
          for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int q = 0; q < G; ++q) acc_t[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(xt[t][s][q], bv[s], acc_t[q], 0, 0, 0);
        }
      }
    }
    // the four wavefronts' sums for column block b, added in wavefront order.  The buffer alternates: this buffer is stored to again
    // two column blocks on, behind the next block's barrier, which no thread passes before its reads below have completed.
#pragma unroll
    for (int q = 0; q < G; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) sums[b & 1][wave][q * 256 + r * 64 + lane] = acc_t[q][r];
    __syncthreads();
    if (b < last) {                                       // (block-uniform: the panel has a tile below block b)
      double* dst = ws + t_base + (size_t)16 * (size_t)m * ((size_t)8 * P * P + (size_t)7 * P + (size_t)b);
#pragma unroll
      for (int q = 0; q < G; ++q) {
        const int e = q * 256 + (int)threadIdx.x;
        const double s = ((sums[b & 1][0][e] + sums[b & 1][1][e]) + sums[b & 1][2][e]) + sums[b & 1][3][e];
        const int col = 16 * q + lk + 4 * wave;
        if (col < m) dst[(size_t)col * 16 + li] = s;
      }
    }
  };
  fetch(std::false_type{}, b0);
  // every thread of the block takes the same number of steps (one block-wide barrier each), whichever path its wavefront takes
  const int b_all = tile0 + RT - 1 <= last ? min(b1, tile0) : b0;     // the blocks [b0, b_all - 1) run the branch-free path
  int b = b0;
  for (; b + 1 < b_all; ++b) step(std::true_type{}, b);
  for (; b < b1; ++b) step(std::false_type{}, b);
  const bool direct = nt == 1;
  const int rows = min(256, n - 256 * P);
  double* dst = direct ? y : ws + (size_t)m * ((size_t)256 * (size_t)dense_sym_chunks_before(P, chunk_panels) + (size_t)c * (size_t)rows);
  const size_t ld = direct ? (size_t)n : (size_t)rows;
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int row = (RT * wave + t) * DENSE_TILE + li;   // within the panel
    if (tile0 + t > last || 256 * P + row >= n) continue;
#pragma unroll
    for (int q = 0; q < G; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = 16 * q + lk + 4 * r;
        if (col < m) dst[(size_t)col * ld + row] = acc_f[t][q][r];
      }
  }
}
// y(i, col) of a pass on the triangular copy, one thread per element, in one order: the forward partials of the element's panel
// by ascending chunk, then the transposed partials of its column block by ascending panel -- ((f_0 + f_1) + ... ) + t_P + t_P+1 ...
__global__ void dense_sym_combine_kernel(int n, int m, int nt, int chunk_panels, size_t t_base, const double* __restrict__ ws, double* __restrict__ y)
{
  const size_t total = (size_t)n * m, stride = (size_t)gridDim.x * blockDim.x;
  const int panels = (nt + DENSE_SYM_PANEL_TILES - 1) / DENSE_SYM_PANEL_TILES;
  for (size_t at = (size_t)blockIdx.x * blockDim.x + threadIdx.x; at < total; at += stride) {
    const int i = (int)(at % (size_t)n), col = (int)(at / (size_t)n);
    const int P = i / 256, b = i / DENSE_TILE, rows = min(256, n - 256 * P);
    const double* f = ws + (size_t)m * (size_t)256 * (size_t)dense_sym_chunks_before(P, chunk_panels) + (size_t)col * rows + (i - 256 * P);
    double s = f[0];
    for (int c = 1; c <= P / chunk_panels; ++c) s += f[(size_t)c * m * rows];
    for (int p = dense_sym_first_panel(nt, b); p < panels; ++p)
      s += ws[t_base + (size_t)16 * (size_t)m * ((size_t)8 * p * p + (size_t)7 * p + (size_t)b) + (size_t)col * 16 + (i & 15)];
    y[at] = s;
  }
}

// The harness' lrprec_1 / lrprec_2 (main.f90:234-281; synth_lrprec_kernel restates them) on the stored diagonals of the sparse
// linear-response parts (dla_spmm_setup_lr_csr): aa = ((A+B)_ii + (A-B)_ii) / 2, sg = (S+D)_ii (D is antisymmetric: its diagonal
// is zero, so S+D carries the diagonal of S).  One thread keeps VEC rows of the three diagonals in registers -- read once -- and
// walks the m columns of the four blocks; every element of yp / ym has one writer.  Order of operations, every product, sum and
// quotient rounded on its own (no contraction into a fused multiply-add), products left to right as written:
//   aa = 0.5 * (apb_ii + amb_ii)
//   variant 1: den = -1.0 / (aa * aa - fac * fac * sg * sg),  ca = aa,        cs = fac * sg
//   variant 2: den =  1.0 / (fac * fac * aa * aa - sg * sg),  ca = fac * aa,  cs = sg
//   yp = den * (ca * xp + cs * xm),  ym = den * (ca * xm + cs * xp)
// which is what a host caller gets from the harness' expressions (ca, cs and den do not depend on the column: taking them out of
// the column loop changes no bit).  32 n m bytes of vectors + 24 n bytes of the three diagonals; panel accesses are non-temporal.
template <int VEC>
__global__ __launch_bounds__(256) void lr_precnd_kernel(int n, int m, int variant, double fac, const double* __restrict__ apb_diag,
                                                        const double* __restrict__ amb_diag, const double* __restrict__ spd_diag,
                                                        const double* __restrict__ xp, const double* __restrict__ xm,
                                                        double* __restrict__ yp, double* __restrict__ ym)
{
#pragma clang fp contract(off)
  typedef typename VecOf<VEC>::type vec_t;
  const size_t nv = (size_t)n / VEC;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t iv = (size_t)blockIdx.x * blockDim.x + threadIdx.x; iv < nv; iv += stride) {
    const size_t i = iv * VEC;
    const vec_t pv = *(const vec_t*)(apb_diag + i), mv = *(const vec_t*)(amb_diag + i), sv = *(const vec_t*)(spd_diag + i);
    double den[VEC], ca[VEC], cs[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const double aa = 0.5 * (vget<VEC>(pv, e) + vget<VEC>(mv, e)), sg = vget<VEC>(sv, e);
      if (variant == 1) {
        den[e] = -1.0 / (aa * aa - fac * fac * sg * sg);
        ca[e] = aa; cs[e] = fac * sg;
      } else {
        den[e] = 1.0 / (fac * fac * aa * aa - sg * sg);
        ca[e] = fac * aa; cs[e] = sg;
      }
    }
    for (int c = 0; c < m; ++c) {
      const size_t at = (size_t)c * n + i;
      const vec_t a = pload<VEC, 1>(xp + at), b = pload<VEC, 1>(xm + at);
      double op[VEC], om[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        op[e] = den[e] * (ca[e] * vget<VEC>(a, e) + cs[e] * vget<VEC>(b, e));
        om[e] = den[e] * (ca[e] * vget<VEC>(b, e) + cs[e] * vget<VEC>(a, e));
      }
      pstore<VEC, 2>(yp + at, vmake<VEC>(op[0], op[VEC - 1]));
      pstore<VEC, 2>(ym + at, vmake<VEC>(om[0], om[VEC - 1]));
    }
  }
}

// The same product on a ROW SHARD of A (dla_spmm_setup_csr_sharded): col[] indexes the extended local vector
// [last `halo` rows of the previous rank | the shard's n rows | first `halo` rows of the next rank]; the two halo pieces have
// arrived through the small-product all-reduce (halo_pack_kernel: every rank fills its own two slots of a zeroed buffer, the sum
// gathers).  Only the wavefronts at the two ends of the shard ever take the halo branches.
struct GatherHalo {
  const double *x, *prev, *next; int n, halo;
  struct Column { const double *pc, *xc, *nc; int n, halo; };
  __device__ __forceinline__ int self(int i) const { return i + halo; }
  __device__ __forceinline__ Column column(int c) const { return Column{prev + (size_t)c * halo, x + (size_t)c * n, next + (size_t)c * halo, n, halo}; }
  __device__ __forceinline__ static double at(const Column& k, int idx)
  {
    return idx < k.halo ? k.pc[idx] : (idx < k.halo + k.n ? k.xc[idx - k.halo] : k.nc[idx - k.halo - k.n]);
  }
};
template <int W>
__global__ __launch_bounds__(256) void ell_spmm_halo_kernel(int n, int m, int w, int halo, const int* __restrict__ col,
                                                            const double* __restrict__ val, const double* __restrict__ x,
                                                            const double* __restrict__ prev, const double* __restrict__ next,
                                                            double* __restrict__ ax)
{
  ell_rows<W>(n, m, w, col, val, GatherHalo{x, prev, next, n, halo}, StoreProduct{ax});
}

// buf[((r * 2 + side) * m + c) * halo + h]: side 0 = the first, side 1 = the last `halo` rows of rank r's x; this rank's slots
// are filled, everybody else's are zero (the all-reduce that follows is a gather)
__global__ void halo_pack_kernel(int n, int m, int halo, int nranks, int rank, const double* __restrict__ x, double* __restrict__ buf)
{
  const int total = nranks * 2 * m * halo;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const int h = idx % halo, c = (idx / halo) % m, side = (idx / (halo * m)) % 2, r = idx / (2 * halo * m);
    buf[idx] = (r == rank) ? x[(size_t)c * n + (side == 0 ? h : n - halo + h)] : 0.0;
  }
}

// ======================================================================================
// Device-resident control of the orthogonalisation loops
// ======================================================================================
// ortho_cd (reference diaglib.f90:3185-3341) and ortho_vs_x (:3481-3574) alternate n-length sweeps with k x k work
// whose outcome decides what the next sweep is (another triangular update, a projection pass, the exit).  Taking that
// decision on the host costs a stream drain per sweep (~8 per ortho_vs_x call).  Here the k x k work -- Cholesky
// factorisation with the level-shift ladder (:3261-3295), triangular inverse (:3310), norm estimates (:3314-3323,
// 3447-3479), growth / convergence tests (:3331-3332, :3562-3564) and the assembly of the coefficient block of the
// next sweep -- runs in a one-block kernel between the sweeps, and the decision is left in device memory
// (OrthoDev::phase).  The host enqueues the sequence of sweeps it expects (the one the previous call took); every
// sweep and every tail kernel checks the phase and leaves at once when it is not its turn (DLA_PREDICATED), so a
// wrong guess costs empty launches, never a wrong result.  One host wait at the end reads the state back.
// (The sweeps' names, OP_*, are shared with the host's planning: hip_plans.h.)
// the block a chain leaves pending, in pinned host memory: [row][PEND_LD] with the rows of E (the part that multiplies X: only the
// three-pass schedule has one) followed by the k rows of the triangular factor T, then the header {sequence number, rows of E}
#define PEND_LD 48
#define PEND_HDR ((size_t)PEND_ROWS * PEND_LD)
// dla_expand_project mode 4: the caller's stored basis is orthonormal to 1e-8 per block only (pending factors and projections), and a
// projection against it leaves (X_c^T X_c - I) S of what it removes -- up to m 1e-8 |S| over a basis of m columns.  A chain of that
// mode may end behind a projection only when that projection removed less than this (tools/fuzz_pending_basis.py: 1e-6 left 1.7e-12
// on a basis of 300 columns)
#define TIGHT_REMOVES 1.0e-8
enum { OST_RUNNING = 0, OST_DONE = 1, OST_CD_MAXIT = 2, OST_FACTOR_FAIL = 3, OST_VSX_MAXIT = 4 };

struct OrthoDev {
  int phase;          // the sweep the state machine waits for (OP_*)
  int status;         // OST_*
  int it_macro;       // macro-iterations of the current ortho_cd pass
  int it_outer;       // outer iterations of ortho_vs_x (0: still in the ortho_cd that precedes the loop)
  int nops;           // sweeps executed so far
  int macro_total;    // macro-iterations over all ortho_cd passes (report)
  int shifts;         // level shifts taken (report)
  int have_xu;        // pending-factor schedule: X^T U of the block in memory is known (xug) up to the factors in wst
  double growth;      // prod ||L^-1||_est of the current ortho_cd pass
  int sloppy;         // pending-factor schedule: the last projection used an X^T U carried through ill-conditioned factors
  double gdev;        // max |G - I| of the last Gram matrix that was factored (how far the pending factor is from the identity)
  int last_status;    // how the last chain ended (OST_*), kept when the machine re-arms: what runs behind a chain on the device
                      // without the host in between (bortho_tail_kernel) continues only after OST_DONE
  int log[48];        // the sweeps executed, in order
};

struct OrthoTailArgs {
  OrthoDev* st;
  OrthoDev* st_host;   // pinned mirror (device-visible address)
  const double* gsrc;  // the reduced small product: k x k (ld k, lower triangle used) or m x k (ld m)
  double* wpk;         // packed W = L^-T for the sweeps: [kt][k4][16]
  double* wfull;       // W, k x k column-major (kept for the C' assembly)
  double* cpk;         // packed C' = [-xu W ; W]: [kt][l4][16], l = m + k
  int after;           // the sweep this tail follows
  int m, k;
  int can_defer;       // 1: ortho_vs_x on the block that follows X (combined sweep available); 0: plain ortho_cd
  int maxit;           // maxit, diaglib.f90:3224,3521
  int publish;         // 1: last launch of the host's plan -- leave the state in the host mirror whatever happened
  // pending-factor schedule (ortho_tail16)
  int fold;            // 1: this chain runs it; 2: ortho_tail16 with the sweep-per-update schedule (odd n)
  int lead_once;       // 1: the ortho_cd in front of the loop (:3533) takes ONE factorisation step (see ortho_tail16)
  const double* xug;   // X^T U and U^T U of the last OP_GRAMX / OP_XW sweep: (m + k) x k, ld m + k
  double* wst;         // pending factors between launches, accumulator layout: [0,256) Wp^T, [256,512) Wd^T, [512,768) Wp
  unsigned long long* dbg;   // $DIAGLIB_AMD_CHAIN_DEBUG: time stamps of the step (100 MHz ticks), 16 per executed sweep
  int xw_ok;           // blocks of 17..48 columns (ortho_tail): the storing sweep OP_XW exists for this shape -- a triangular update
                       // inside the loop is written together with X^T U and U^T U of what it stores (one sweep instead of two)
  double* t_host;      // drop_final: pinned copy of the block that stays pending (layout: PEND_LD / PEND_HDR above; the header is
                       // written last) -- for callers that fold it into their small matrices instead (dla_expand_project modes 3, 4)
  int t_seq;
  double drop_stol;    // three-pass schedule: the closing block stays pending only when max |X^T U| of the stored block is below it
  double drop_tol;     // > 0: drop_final only when max |G - I| of the closing pass is below it (a block that STAYS in the basis may
                       // keep a pending factor only if later blocks can still be projected against it as if it were orthonormal:
                       // two passes leave (2 drop_tol)^2 of the component they remove)
  int x3;              // three-pass schedule (ortho_tail16, fold == 1): every projection is OP_COMBOX, see there
  const double* dmat;  // != nullptr: the stored columns X are not a finished basis -- the finished one is X D with this upper-triangular
  int dmat_ld;         // D (m x m, column-major, the caller's pending blocks: dla_basis_sync).  The projector onto span(X) is then
                       // X (D D^T) X^T, and the projection coefficients are -(D D^T)(xu W) instead of -(xu W) (ortho_tail16)
  int gp;              // 1: the first projection's triangular factor comes from the Gram matrix of the PROJECTED block, G - Y^T Y with
                       // Y = D^T (X^T U), both measured by OP_GRAMX -- instead of the block's own (see ortho_tail16)
  int drop_final;      // 1: the chain ends where it would ask for OP_FINAL -- the pending upper-triangular factor is NOT applied.
                       // For callers that B-orthonormalise the block by Cholesky-QR right behind the chain (dla_expand_project_metric:
                       // b_ortho, reference diaglib.f90:3094-3183): the Q factor of U W and of U is the same for any upper-triangular W
                       // with a positive diagonal, so the sweep U <- U W (16 n k bytes) buys nothing there
};
#define TSTAMP(a, nops, i) do { if ((a).dbg != nullptr && (nops) < 48) (a).dbg[(nops) * 16 + (i)] = wall_clock64(); } while (0)

// The k x k work is done by ONE wave on LDS images (row-major, row stride TLD): lane i owns row i (k <= 48 < 64).  LDS
// operations of a wave complete in order, so no workgroup barrier is needed (the routine can run at the end of a kernel
// whose other waves have already left); TSYNC keeps the compiler from moving LDS accesses across the points where
// lanes exchange data.  The code is deliberately compact (loops, not unrolled matrices): it runs once per launch, from
// a cold instruction cache, and a fully unrolled register version measured slower for that reason.  Operation order =
// the host routines (smalldense.cpp dla_potrf_lower / dla_trtri_lower): dot products in ascending index order.
#define TLD 49
#define TSYNC() __builtin_amdgcn_wave_barrier()
__device__ __forceinline__ double rlane(double v, int src)      // src: wave-uniform
{
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}

// lower Cholesky factor in place; returns 0 or the (1-based) index of the first non-positive pivot
__device__ __forceinline__ int lds_potrf(int k, double* A, int lane)
{
  const int i = lane < k ? lane : k - 1;                // idle lanes shadow the last row (no stores)
  for (int j = 0; j < k; ++j) {
    TSYNC();
    // s = a_ij - sum_{p<j} l_ip l_jp for every row i >= j at once; row j itself yields the pivot
    double sij = lds_load1(A + i * TLD + j);
#pragma unroll 4
    for (int p = 0; p < j; ++p) sij -= lds_load1(A + i * TLD + p) * lds_load1(A + j * TLD + p);
    double dj = rlane(sij, j);
    if (!(dj > 0.0) || !isfinite(dj)) return j + 1;
    dj = sqrt(dj);
    const double inv = 1.0 / dj;
    TSYNC();                                            // row j has been read by everyone
    if (lane < k && lane > j) lds_store1(A + lane * TLD + j, sij * inv);
    if (lane == j) lds_store1(A + j * TLD + j, dj);
  }
  TSYNC();
  return 0;
}

// inverse of a lower triangular matrix in place, column by column from the right
__device__ __forceinline__ void lds_trtri(int k, double* A, int lane)
{
  const int i = lane < k ? lane : k - 1;
  for (int j = k - 1; j >= 0; --j) {
    TSYNC();
    const double xj = 1.0 / lds_load1(A + j * TLD + j);
    double sacc = 0.0;
#pragma unroll 4
    for (int p = j + 1; p <= i; ++p) sacc += lds_load1(A + i * TLD + p) * lds_load1(A + p * TLD + j);
    TSYNC();
    if (lane < k && lane > j) lds_store1(A + lane * TLD + j, -sacc * xj);
    if (lane == j) lds_store1(A + j * TLD + j, xj);
  }
  TSYNC();
}

// norm_est (diaglib.f90:3447-3479): max |a_ii| + Frobenius norm of the strictly lower part; rows in parallel, then the
// row sums in row order (every lane computes the same result)
__device__ __forceinline__ double lds_norm_est(int k, const double* A, int lane)
{
  TSYNC();
  double on_i = 0.0, diag = 0.0;
  if (lane < k) {
#pragma unroll 4
    for (int j = 0; j < lane; ++j) { const double v = lds_load1(A + lane * TLD + j); on_i += v * v; }
    diag = fabs(lds_load1(A + lane * TLD + lane));
  }
  double dn = 0.0, on = 0.0;
  for (int r = 0; r < k; ++r) { dn = fmax(dn, rlane(diag, r)); on += rlane(on_i, r); }
  return dn + sqrt(on);
}

struct TailState { int it_macro, it_outer, macro_total, shifts, nops, phase, status; double growth; int have_xu, sloppy; double gdev; };
#define TAIL_LDS_DOUBLES (48 * TLD + 48 * 64)   // image A, then image S (also used as 48 x 64 scratch)

// what one lane does at the end of a step: log the sweep, report to the host when the chain ends (or the plan does), leave the
// new state -- or the initial one, ready for the next chain -- in device memory
__device__ __forceinline__ void tail_publish(const OrthoTailArgs& a, const TailState& t)
{
  OrthoDev* st = a.st;
  const int ph_out = (t.status == OST_RUNNING) ? t.phase : OP_NONE;
  const int nops = t.nops;
  if (nops < 48) st->log[nops] = a.after;
  if (t.status != OST_RUNNING || a.publish) {
    // report to the host: scalars from registers, the log from device memory
    a.st_host->phase = ph_out; a.st_host->status = t.status; a.st_host->it_macro = t.it_macro;
    a.st_host->it_outer = t.it_outer; a.st_host->nops = nops + 1; a.st_host->macro_total = t.macro_total;
    a.st_host->shifts = t.shifts; a.st_host->growth = t.growth;
    const int nl = nops + 1 < 48 ? nops + 1 : 48;
    for (int q = 0; q < nl; ++q) a.st_host->log[q] = (q == nops) ? a.after : st->log[q];
  }
  if (t.status != OST_RUNNING) {
    // finished (or failed): re-arm the machine for the next chain, so that no initial state has to be copied in
    st->it_macro = 0; st->it_outer = 0; st->nops = 0; st->macro_total = 0; st->shifts = 0; st->growth = 1.0; st->have_xu = 0; st->sloppy = 0; st->gdev = 1.0;
    st->last_status = t.status;
    st->status = OST_RUNNING;
    __hip_atomic_store(&st->phase, (int)OP_GRAM_UU, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    st->it_macro = t.it_macro; st->it_outer = t.it_outer; st->nops = nops + 1; st->macro_total = t.macro_total;
    st->shifts = t.shifts; st->growth = t.growth; st->status = t.status; st->have_xu = t.have_xu; st->sloppy = t.sloppy; st->gdev = t.gdev;
    __hip_atomic_store(&st->phase, ph_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}


// One step of the state machine, executed by the 64 lanes of one wave; lds: TAIL_LDS_DOUBLES doubles.
// pre != nullptr: the caller has checked the phase and read the state already (fused into a reduction kernel);
// g_in_lds: the caller has put the k x k Gram matrix into both LDS images (A and S) already.
__device__ __forceinline__ void ortho_tail(const OrthoTailArgs& a, double* lds, int lane, const TailState* pre = nullptr, bool g_in_lds = false)
{
  OrthoDev* st = a.st;
  if (pre == nullptr) {
    const int ph = __hip_atomic_load(&st->phase, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ph != (a.after == OP_GRAMX ? (int)OP_GRAM_UU : a.after)) {
      // not this step's turn.  The last launch of a plan still tells the host where the machine stands -- unless the
      // chain has already ended (a terminal step reported it and re-armed the machine: nops == 0)
      if (a.publish && lane == 0 && st->nops > 0) *a.st_host = *st;
      return;
    }
  }
  const int k = a.k, m = a.m;
  const int kt = (k + 15) / 16, k4 = ((k + 3) / 4) * 4;
  const double eps = 2.220446049250313e-16, tol = 2.0 * eps;   // epsilon(one), tol_ortho (diaglib.f90:151)
  const int maxit = a.maxit, can_defer = a.can_defer;
  TailState t = pre ? *pre : TailState{st->it_macro, st->it_outer, st->macro_total, st->shifts, st->nops, OP_NONE, OST_RUNNING, st->growth, 0, st->sloppy, st->gdev};
  const int force_defer = can_defer && t.it_outer == 0;   // the ortho_cd that precedes the loop always leaves W pending
  double* A = lds;
  double* S = lds + 48 * TLD;
  // C' = [-(xu W) ; W ; 0] packed for the combined sweep, W(pp, j) in the LDS image A (row pp), xu m x k with leading dimension ldx
  // (to_host: the block stays pending -- the same rows also go to the caller's pinned buffer, the header last)
  auto assemble = [&](const double* xu, int ldx, bool to_host) {
    const int l = m + k, l4 = ((l + 3) / 4) * 4;
    // rows that are not products: the W block, the zero padding of rows and columns
    for (int idx = lane; idx < kt * l4 * 16; idx += 64) {
      const int q = idx / (l4 * 16), p = (idx / 16) % l4, j = 16 * q + (idx % 16);
      if (p >= m || j >= k) {
        const double v = (p < l && j < k) ? lds_load1(A + (p - m) * TLD + j) : 0.0;
        a.cpk[idx] = v;
        if (to_host && p >= m && p < l && j < k) a.t_host[(size_t)p * PEND_LD + j] = v;
      }
    }
    for (int p = lane; p < m; p += 64) {
      // row p of xu into the lane's own LDS row (the S image is free here), then the k dot products
      for (int pp = 0; pp < k; ++pp) lds_store1(S + pp * 64 + lane, xu[(size_t)p + (size_t)pp * ldx]);
      for (int j = 0; j < k; ++j) {
        double sacc = 0.0;
#pragma unroll 4
        for (int pp = 0; pp <= j; ++pp) sacc += lds_load1(S + pp * 64 + lane) * lds_load1(A + pp * TLD + j);
        a.cpk[((size_t)(j / 16) * l4 + p) * 16 + (j % 16)] = -sacc;
        if (to_host) a.t_host[(size_t)p * PEND_LD + j] = -sacc;
      }
    }
    if (to_host) {
      __threadfence_system();
      if (lane == 0) { a.t_host[PEND_HDR + 1] = (double)m; a.t_host[PEND_HDR + 2] = 0.0; __threadfence_system(); a.t_host[PEND_HDR] = (double)a.t_seq; }
    }
  };
  // A caller that folds pending blocks into its small matrices (drop_final + t_host) lets the chain END wherever X^T U has been
  // measured on the stored block and the factor of that block's Gram matrix has converged: the closing pass of the reference
  // (:3543-3544, then one macro-iteration with a near-identity factor) is then the block [-(xu W) ; W], which the caller applies
  // to its coefficients exactly (dla_basis_admit) -- as long as xu is small enough for that algebra to be benign (drop_stol).
  const bool may_pend = a.drop_final && a.t_host != nullptr && m > 0;
  // (wn: norm estimate of the factor that is pending on the measured block -- what has to be small is xu W.  A block of LOBPCG
  //  residuals of norm 1e-8 measured in front of its first projection has a tiny X^T U and a factor of 1e8: found by
  //  tools/fuzz_multirank.py, seed 78)
  auto xu_max = [&](const double* xu, int ldx, double wn) {
    double sm = 0.0;
    for (int idx = lane; idx < m * k; idx += 64) sm = fmax(sm, fabs(xu[(size_t)(idx % m) + (size_t)(idx / m) * ldx]));
    for (int off = 32; off > 0; off >>= 1) sm = fmax(sm, __shfl_xor(sm, off, 64));
    return sm * fmax(wn, 1.0);
  };
  auto small_xu = [&](const double* xu, int ldx, double wn) { return xu_max(xu, ldx, wn) < a.drop_stol; };
  // (the caller's stored basis is orthonormal to drop_tol only, dla_expand_project mode 4: a projection against it leaves that share
  //  of what it removes, so no chain may end behind a projection that removed more than TIGHT_REMOVES -- see ortho_tail16)
  const bool tight = a.drop_tol > 0.0 && m > 0;

  if (a.after == OP_FINAL) {
    t.status = OST_DONE;
  } else if (a.after == OP_XU) {
    // C' = [-(xu W) ; W]  (host_logic.cpp ortho_vs_x_impl, X^T (U W) = (X^T U) W), packed for the combined sweep
    for (int idx = lane; idx < k * k; idx += 64) lds_store1(A + (idx % k) * TLD + idx / k, a.wfull[idx]);   // A[pp][j] = W(pp, j)
    TSYNC();
    const bool pend = may_pend && t.gdev < (a.drop_tol > 0.0 ? a.drop_tol : 1.0) && small_xu(a.gsrc, m, t.growth);
    if (!pend && tight && xu_max(a.gsrc, m, t.growth) >= TIGHT_REMOVES) t.sloppy = 1;
    assemble(a.gsrc, m, pend);
    t.it_macro = 0;           // the ortho_cd that follows the combined sweep starts afresh (*growth = 1, it = 0)
    t.growth = 1.0;
    if (pend) t.status = OST_DONE;
    else t.phase = OP_COMBO;
  } else {
    // one macro-iteration of ortho_cd on the Gram matrix the sweep left in gsrc
    ++t.it_macro;
    if (t.it_macro > maxit) {
      t.status = OST_CD_MAXIT;                                  // :3252-3254, the host prints and reports ok = .false.
    } else {
      ++t.macro_total;
      if (!g_in_lds) {
        // (OP_GRAMX / OP_XW: [X | U]^T U in one sweep, (m + k) x k: the Gram matrix of U sits under X^T U)
        const bool xu_above = a.after == OP_GRAMX || a.after == OP_XW;
        const int roff = xu_above ? m : 0, ldg = xu_above ? m + k : k;
        for (int idx = lane; idx < k * k; idx += 64) {
          const int i = idx % k, j = idx / k;
          if (i >= j) { const double v = a.gsrc[(size_t)(roff + i) + (size_t)j * ldg]; lds_store1(A + i * TLD + j, v); lds_store1(S + i * TLD + j, v); }
        }
      }
      {
        double dv = 0.0;                  // max |G - I| of the Gram matrix about to be factored
        for (int idx = lane; idx < k * k; idx += 64) {
          const int i = idx % k, j = idx / k;
          if (i >= j) dv = fmax(dv, fabs(lds_load1(S + i * TLD + j) - (i == j ? 1.0 : 0.0)));
        }
        for (int off = 32; off > 0; off >>= 1) dv = fmax(dv, __shfl_xor(dv, off, 64));
        t.gdev = dv;
      }
      int info = lds_potrf(k, A, lane);
      int it_micro = 0;
      if (info != 0) {
        // level-shift ladder (:3265-3295): shift = max(eps alpha ||U||_F, 2 eps), alpha = 100, 1000, ...
        double tr = 0.0;
        for (int i = 0; i < k; ++i) tr += lds_load1(S + i * TLD + i);
        const double unorm = sqrt(tr > 0.0 ? tr : 0.0);
        double alpha = 100.0;
        while (info != 0) {
          if (++it_micro > maxit) break;
          const double shift = fmax(eps * alpha * unorm, tol);
          TSYNC();
          for (int idx = lane; idx < k * k; idx += 64) {
            const int i = idx % k, j = idx / k;
            if (i >= j) lds_store1(A + i * TLD + j, lds_load1(S + i * TLD + j) + (i == j ? shift : 0.0));
          }
          info = lds_potrf(k, A, lane);
          alpha *= 10.0;
          ++t.shifts;
        }
      }
      // (a factor that needed a level shift is not one a block may stay pending with: a zero block -- Davidson on a multiple of the
      //  identity, residuals exactly zero -- "converges" with any shift, and the reference stops on it in ortho_vs_x after maxit
      //  passes; the pending endings behind OP_XU look at gdev, tools/fuzz_degenerate_drivers.py)
      if (it_micro > 0) t.gdev = fmax(t.gdev, 2.0);
      if (info != 0) {
        t.status = OST_FACTOR_FAIL;                             // reference: stop (:3283)
      } else {
        const double l_norm = lds_norm_est(k, A, lane);
        lds_trtri(k, A, lane);
        const double linv_norm = lds_norm_est(k, A, lane);
        // W = L^-T (upper triangular): W(p, j) = Linv(j, p), p <= j
        for (int idx = lane; idx < k * k; idx += 64) {
          const int pp = idx % k, j = idx / k;
          a.wfull[idx] = (pp <= j) ? lds_load1(A + j * TLD + pp) : 0.0;
        }
        for (int idx = lane; idx < kt * k4 * 16; idx += 64) {
          const int q = idx / (k4 * 16), pp = (idx / 16) % k4, j = 16 * q + (idx % 16);
          a.wpk[idx] = (j < k && pp <= j) ? lds_load1(A + j * TLD + pp) : 0.0;
        }
        const double rcond = l_norm * linv_norm;
        t.growth *= linv_norm;
        // (lead_once: the ortho_cd in front of the loop takes one factorisation step, see ortho_tail16; with a first
        //  projection of that quality the closing pass is mandatory -- here it always is: the pass decision below looks at
        //  growth eps, and a block that needed more than this one step has growth >= 2)
        // (a block that needed a level shift is numerically rank deficient: its weakest columns come out as amplified
        //  rounding noise, WHICH noise depends on the order of the operations, and the solvers' convergence history can
        //  depend on it -- the reference's dense test matrix with unit guesses does, tests/test_trace_text.py.  There the
        //  reference's order is kept: ortho_cd in front of the loop runs to convergence before the first projection)
        const bool lead = force_defer && a.lead_once && it_micro == 0 && (a.after == OP_GRAM_UU || a.after == OP_GRAMX);
        const bool macro_done = (eps * rcond * rcond < tol) || lead;      // :3331-3332
        // OP_XW measured X^T U and U^T U on the block it stored.  When this factor ends the ortho_cd pass and ortho_vs_x goes on
        // (growth eps >= tol, :3562-3564), the next projection has its coefficients already: C' = [-(xu W) ; W] with the
        // factor of this step pending -- exactly what the separate X^T U sweep (OP_XU) would have produced
        const bool xw_project = a.after == OP_XW && macro_done && can_defer && (t.sloppy || t.growth * eps >= tol || may_pend) && t.it_outer <= maxit;
        if ((a.after == OP_GRAMX && lead) || xw_project) {
          // X^T U came with the Gram matrix: the first projection follows at once, C' = [-(xu W) ; W] (one factorisation step
          // in front of the loop, closing pass mandatory after a factor that is not near the identity: see lead_once above)
          TSYNC();
          for (int idx = lane; idx < k * k; idx += 64) {       // W image: S2[pp][j] = W(pp, j) = Linv(j, pp), through the free S image
            const int pp = idx / k, j = idx % k;
            lds_store1(S + pp * TLD + j, pp <= j ? lds_load1(A + j * TLD + pp) : 0.0);
          }
          TSYNC();
          for (int idx = lane; idx < k * k; idx += 64) lds_store1(A + (idx / k) * TLD + idx % k, lds_load1(S + (idx / k) * TLD + idx % k));
          TSYNC();
          const bool pend = xw_project && may_pend && (a.drop_tol <= 0.0 || t.gdev < a.drop_tol) && small_xu(a.gsrc, m + k, linv_norm);
          assemble(a.gsrc, m + k, pend);
          t.sloppy = (!xw_project && t.growth * eps >= tol) ? 1 : 0;      // (a measured X^T U of the stored block is not sloppy)
          if (!pend && tight && xu_max(a.gsrc, m + k, xw_project ? linv_norm : t.growth) >= TIGHT_REMOVES) t.sloppy = 1;
          ++t.it_outer;
          t.it_macro = 0; t.growth = 1.0;
          if (pend) t.status = OST_DONE;
          else t.phase = OP_COMBO;
        } else if (!macro_done) {
          // inside the loop, without a level shift: the update is stored together with X^T U and U^T U of what it stores
          t.phase = (a.xw_ok && can_defer && !force_defer && it_micro == 0) ? OP_XW : OP_TRMMG;
        } else if (can_defer && (force_defer || t.sloppy || t.growth * eps >= tol || (a.drop_tol > 0.0 && t.it_outer < 2))) {
          // the pass ends with W pending; ortho_vs_x goes on with a projection pass (xu_norm = growth eps >= tol)
          // (drop_tol > 0: the caller's stored basis may carry pending blocks -- it is orthonormal to drop_tol only, and ONE
          //  projection against it leaves that share of the component it removes (round-4 advisor): there are always two, the
          //  second one on a measured X^T U)
          if (!force_defer && t.it_outer > maxit) t.status = OST_VSX_MAXIT;     // :3568
          else {
            // (a first projection whose pending factor is not the near-identity one of a converged macro-iteration leaves
            //  an X component of order eps cond(U): the closing pass is then mandatory)
            t.sloppy = (force_defer && t.growth * eps >= tol) ? 1 : 0;
            ++t.it_outer; t.phase = OP_XU;
          }
        } else {
          if (can_defer && t.it_outer > maxit) t.status = OST_VSX_MAXIT;
          else if (a.drop_final && (a.drop_tol <= 0.0 || [&]() {
                     // max |G - I| of this pass (the S image keeps the Gram matrix the factorisation started from)
                     double dev = 0.0;
                     for (int idx = lane; idx < k * k; idx += 64) {
                       const int i = idx % k, j = idx / k;
                       if (i >= j) dev = fmax(dev, fabs(lds_load1(S + i * TLD + j) - (i == j ? 1.0 : 0.0)));
                     }
                     for (int off = 32; off > 0; off >>= 1) dev = fmax(dev, __shfl_xor(dev, off, 64));
                     return dev < a.drop_tol; }())) {
            t.status = OST_DONE;
            if (a.t_host != nullptr) {
              // the factor that stays pending: W of this step (everything before it has been written by the sweeps)
              for (int idx = lane; idx < k * k; idx += 64) {
                const int pp = idx % k, j = idx / k;
                a.t_host[(size_t)pp * PEND_LD + j] = (pp <= j) ? lds_load1(A + j * TLD + pp) : 0.0;
              }
              __threadfence_system();
              if (lane == 0) { a.t_host[PEND_HDR + 1] = 0.0; a.t_host[PEND_HDR + 2] = 0.0; a.t_host[PEND_HDR] = (double)a.t_seq; }
            }
          }
          else t.phase = OP_FINAL;
        }
      }
    }
  }
  if (lane == 0) tail_publish(a, t);
}


// ======================================================================================
// k <= 16: the k x k step on the matrix cores, and the pending-factor schedule
// ======================================================================================
// Pending factor.  A macro-iteration of ortho_cd (reference diaglib.f90:3246-3332) ends with U <- U W, W = L^-T, and the next
// one starts with the Gram matrix of the result.  The update need not reach memory in between: a sweep can form U W tile by
// tile on the fly (gram_lds_kernel WP: same instruction sequence as the update sweep, so the same values -- just not rounded to
// memory), and the projection sweep applies the pending factors together with its own coefficients (the identity the
// pending-W folding already used: X^T (U W) = (X^T U) W).  The chain carries Wp, the product of the factors not yet applied to
// the block in memory U_mem, and Wd, the product of the factors since X^T U was last formed (X^T of the current block is
// xu Wd).  What may stay pending is decided by what the RESULT's accuracy rests on.  The reference ends every call with a
// pass in which X^T U and U^T U are measured on the stored block and only a near-identity factor (the one of the converged
// macro-iteration) is still to be applied: that pass is kept exactly.  Everything before it -- the ortho_cd in front of the
// loop and the first projection -- only has to hand a well-conditioned block with a small X component to that pass, so there
// products are carried on the small side:
//     OP_GRAMX  X^T U and U^T U in one sweep over [X | U]                                  (dgemm :3256 and dgemm :3543)
//     OP_GRAMW  Gram matrix of U Wp on the fly, reads U, writes nothing                    (dtrmm :3327 + dgemm :3256)
//               (after a level shift, :3265-3295, the block is numerically rank deficient and the next Gram matrix would see a
//                fresh realisation of the rounding noise every time: there the update is written, OP_TRMMG)
//     OP_COMBO  U <- [X | U] [-xu Wd ; Wp] + Gram matrix of the result                     (dgemm :3544 + the pending dtrmm + :3256)
//     OP_XW     U <- U W written back, X^T U and U^T U of the stored result, one sweep     (dtrmm + dgemm :3256 + dgemm :3543)
//     OP_COMBO  with the measured xu and the converged factor, OP_FINAL
// = 4 L + 10 k columns of traffic and 5 k x k steps per ortho_vs_x call with the usual decisions, against
// 4 L + 13 k and 7 for the sweep-per-update schedule above.  When the first projection used an X^T U carried through
// ill-conditioned factors (growth of the leading ortho_cd times eps above tol_ortho) the closing pass is run even where the
// reference would stop after one (:3562-3564 decide on the growth of the last ortho_cd only): never less orthogonal than the
// reference.  Plain ortho_cd calls write every update (the result's accuracy rests on each of them).
// Wp and Wd live in device memory between launches in the accumulator layout of v_mfma_f64_16x16x4 ("C-layout": lane
// (c = lane & 15, g = lane >> 4) keeps M[g + 4 r][c] in register r), transposed, because a C-layout register quadruple is
// directly the B operand of M and the A operand of M^T.
//
// The k x k work itself (diaglib.f90:3261-3332) runs on ONE wave with the matrices in registers:
//   * Cholesky factorisation G = R^T R, right-looking, one row per step: the pivot comes from a readlane, the row is scaled,
//     and the rank-1 update of the trailing matrix is ONE v_mfma_f64_16x16x4 whose A and B operands are the same register
//     (row j of R sits in the 16 lanes g = j & 3 of register j >> 2, which is where both operand layouts want it);
//   * L^-1 (L = R^T) by forward substitution on the identity, row operations X[i] -= L[i][j] X[j]: the same A operand, one
//     more MFMA per step, interleaved with the factorisation (two independent dependency chains);
//   * products of 16 x 16 matrices: 4 MFMAs each; one transpose of X through LDS gives W = X^T in C-layout.
// 13 steps of ~0.1 us replace the ~7.4 us of LDS-latency-bound loops of ortho_tail.  Operation order differs from the host
// routines (outer-product instead of dot-product form); results agree to rounding, decisions are taken on all-reduced
// numbers and are identical on every rank.
__device__ __forceinline__ double sel4(const v4d& m, int r) { return r == 0 ? m[0] : (r == 1 ? m[1] : (r == 2 ? m[2] : m[3])); }
__device__ __forceinline__ v4d mfma16(double a, double b, v4d c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// a: Gram matrix in C-layout (identity beyond k).  Out: R (upper triangle of a), X = L^-1 (lower), the largest diagonal
// entries of both.  Returns 0 or the 1-based index of the first non-positive pivot.
// The loop is pure issue latency for one wave, so it is written to the instruction: the factorisation runs in its
// square-root-free form G = Lu D Lu^T (unit lower Lu), where a step needs NO write to the matrix registers besides the MFMA
// itself -- row j of the working matrix is the unscaled row u_j = d_j Lu(:, j)^T, the trailing update is A -= (u_j / d_j) u_j^T
// (one MFMA, A operand u_j / d_j, B operand u_j, both masked to the 16 lanes that hold row j), and Lu^-1 grows beside it by
// X[i] -= (u_j[i] / d_j) X[j] (one more MFMA with the same A operand; its diagonal is 1, nothing to scale).  R = D^-1/2 U and
// L^-1 = D^-1/2 Lu^-1 are two row scalings at the end, the square roots of all pivots taken at once.  A step is: two readlanes
// (pivot), a reciprocal (hardware estimate + two Newton steps), three selects, one multiply, two MFMAs.
// One step, row j = 4 RR + gj: the register index RR is a template argument (the loop branches to one of four copies of the step;
// a register picked by a run-time index costs a dozen selects per access).
#ifndef CHOL_BLOCKED
#define CHOL_BLOCKED 1
#endif
template <int RR>
__device__ __forceinline__ void ldl_inv_step(int j, double d, v4d& a, v4d& x, v4d& drow, int c, int g)
{
  const int gj = j & 3;
  double inv = __builtin_amdgcn_rcp(d);
  inv = fma(fma(-d, inv, 1.0), inv, inv);
  inv = fma(fma(-d, inv, 1.0), inv, inv);
  const bool rowj = (g == gj);
  const double u = (rowj && c > j) ? a[RR] : 0.0;            // u_j[c], c > j
  const double xb = rowj ? x[RR] : 0.0;                       // X[j][c] (unit diagonal: final as it stands)
  if (rowj) drow[RR] = d;                                     // the pivot of this lane's row g + 4 RR
  const double ua = -u * inv;
  a = mfma16(ua, u, a);       // A[i][c'] -= u_j[i] u_j[c'] / d_j,  i, c' > j
  x = mfma16(ua, xb, x);      // X[i][c'] -= Lu[i][j] X[j][c'],     i > j
}

// The same factorisation four rows at a time.  The rows 4B .. 4B+3 of the working matrix are the four 16-lane groups of register
// B, so the 4 x 4 diagonal block is ten readlanes away from every lane; its LDL^T factors are computed by all lanes alike
// (uniform values), the four rows are gathered per column with three cross-group shuffles and eliminated against each other in
// registers, and the trailing matrix gets ONE rank-4 update: v_mfma_f64_16x16x4 with A(i, q) = -u_q[i] / d_q and B(q, c) = u_q[c]
// is exactly that (operand index q = lane >> 4 = the row's group).  L^-1 follows with the same A operand, as before.  Four block
// steps of a few hundred cycles each replace sixteen dependent row steps (13 k cycles at k = 13).
__device__ __forceinline__ double rcp_nr(double d)
{
  double inv = __builtin_amdgcn_rcp(d);
  inv = fma(fma(-d, inv, 1.0), inv, inv);
  return fma(fma(-d, inv, 1.0), inv, inv);
}
template <int B>
__device__ __forceinline__ int ldl_inv_block(int k, v4d& a, v4d& x, v4d& drow, int c, int g, double& dlo, double& dhi)
{
  constexpr int j0 = 4 * B;
  const double ab = a[B], xb = x[B];
  // upper triangle of the diagonal block: D[p][q] = A[j0 + p][j0 + q] sits in lane 16 p + j0 + q
  const double d00 = rlane(ab, j0), d01 = rlane(ab, j0 + 1), d02 = rlane(ab, j0 + 2), d03 = rlane(ab, j0 + 3);
  const double d11 = rlane(ab, 16 + j0 + 1), d12 = rlane(ab, 16 + j0 + 2), d13 = rlane(ab, 16 + j0 + 3);
  const double d22 = rlane(ab, 32 + j0 + 2), d23 = rlane(ab, 32 + j0 + 3);
  const double d33 = rlane(ab, 48 + j0 + 3);
  // the rows of the block at this lane's column, and the rows of X (independent of the scalar chain below)
  const double a0 = __shfl(ab, c, 64), a1 = __shfl(ab, 16 + c, 64), a2 = __shfl(ab, 32 + c, 64), a3 = __shfl(ab, 48 + c, 64);
  const double x0 = __shfl(xb, c, 64), x1 = __shfl(xb, 16 + c, 64), x2 = __shfl(xb, 32 + c, 64), x3 = __shfl(xb, 48 + c, 64);
  const double p0 = d00;
  if (!(p0 > 0.0) || !isfinite(p0)) return j0 + 1;
  const double i0 = rcp_nr(p0);
  const double l10 = d01 * i0, l20 = d02 * i0, l30 = d03 * i0;
  const double p1 = fma(-l10, d01, d11), e12 = fma(-l10, d02, d12), e13 = fma(-l10, d03, d13);
  if (!(p1 > 0.0) || !isfinite(p1)) return j0 + 2;
  const double i1 = rcp_nr(p1);
  const double l21 = e12 * i1, l31 = e13 * i1;
  const double p2 = fma(-l21, e12, fma(-l20, d02, d22)), e23 = fma(-l21, e13, fma(-l20, d03, d23));
  if (!(p2 > 0.0) || !isfinite(p2)) return j0 + 3;
  const double i2 = rcp_nr(p2);
  const double l32 = e23 * i2;
  const double p3 = fma(-l32, e23, fma(-l31, e13, fma(-l30, d03, d33)));
  if (!(p3 > 0.0) || !isfinite(p3)) return j0 + 4;
  const double i3 = rcp_nr(p3);
  // (pivots of the padding rows beyond k are 1 and do not count)
  dlo = fmin(dlo, fmin(fmin(p0, j0 + 1 < k ? p1 : p0), fmin(j0 + 2 < k ? p2 : p0, j0 + 3 < k ? p3 : p0)));
  dhi = fmax(dhi, fmax(fmax(p0, j0 + 1 < k ? p1 : p0), fmax(j0 + 2 < k ? p2 : p0, j0 + 3 < k ? p3 : p0)));
  // eliminated rows u_q = row q - sum_{s<q} l_qs u_s, the same for X
  const double u0 = a0;
  const double u1 = fma(-l10, u0, a1);
  const double u2 = fma(-l21, u1, fma(-l20, u0, a2));
  const double u3 = fma(-l32, u2, fma(-l31, u1, fma(-l30, u0, a3)));
  const double y0 = x0;
  const double y1 = fma(-l10, y0, x1);
  const double y2 = fma(-l21, y1, fma(-l20, y0, x2));
  const double y3 = fma(-l32, y2, fma(-l31, y1, fma(-l30, y0, x3)));
  const double um = g == 0 ? u0 : (g == 1 ? u1 : (g == 2 ? u2 : u3));
  const double ym = g == 0 ? y0 : (g == 1 ? y1 : (g == 2 ? y2 : y3));
  const double im = g == 0 ? i0 : (g == 1 ? i1 : (g == 2 ? i2 : i3));
  a[B] = um; x[B] = ym;
  drow[B] = g == 0 ? p0 : (g == 1 ? p1 : (g == 2 ? p2 : p3));
  const bool trail = c > j0 + 3;
  const double ua = trail ? -um * im : 0.0;
  const double ub = trail ? um : 0.0;
  a = mfma16(ua, ub, a);      // A[i][c'] -= sum_q u_q[i] u_q[c'] / d_q,  i, c' > j0 + 3
  x = mfma16(ua, ym, x);      // X[i][c'] -= sum_q Lu[i][j0 + q] X[j0 + q][c'],  i > j0 + 3
  return 0;
}

__device__ __forceinline__ int chol_inv16(int k, v4d& a, v4d& x, double& dmax, double& xmax, int lane)
{
  const int c = lane & 15, g = lane >> 4;
  v4d drow;
#pragma unroll
  for (int r = 0; r < 4; ++r) { x[r] = (g + 4 * r == c) ? 1.0 : 0.0; drow[r] = 1.0; }
  double dlo = 1.0e300, dhi = 0.0;
  int info = 0;
  if (CHOL_BLOCKED) {
    // (the matrix is the identity beyond k: a partly filled last block factors like any other)
    info = ldl_inv_block<0>(k, a, x, drow, c, g, dlo, dhi);
    if (!info && k > 4) info = ldl_inv_block<1>(k, a, x, drow, c, g, dlo, dhi);
    if (!info && k > 8) info = ldl_inv_block<2>(k, a, x, drow, c, g, dlo, dhi);
    if (!info && k > 12) info = ldl_inv_block<3>(k, a, x, drow, c, g, dlo, dhi);
    if (info > k) info = 0;                  // (cannot happen: the padding rows are unit vectors)
  } else
#pragma unroll 1
  for (int j = 0; j < k; ++j) {
    const int src = 16 * (j & 3) + j;                        // the lane that holds A[j][j], in register j >> 2
    double d;
    switch (j >> 2) {
      case 0: d = rlane(a[0], src); break;
      case 1: d = rlane(a[1], src); break;
      case 2: d = rlane(a[2], src); break;
      default: d = rlane(a[3], src); break;
    }
    if (!(d > 0.0) || !isfinite(d)) { info = j + 1; break; }
    dlo = fmin(dlo, d); dhi = fmax(dhi, d);
    switch (j >> 2) {
      case 0: ldl_inv_step<0>(j, d, a, x, drow, c, g); break;
      case 1: ldl_inv_step<1>(j, d, a, x, drow, c, g); break;
      case 2: ldl_inv_step<2>(j, d, a, x, drow, c, g); break;
      default: ldl_inv_step<3>(j, d, a, x, drow, c, g); break;
    }
  }
  if (info) return info;
  // R = D^-1/2 U, L^-1 = D^-1/2 Lu^-1: every lane scales its four rows (1 / sqrt: hardware estimate + two Newton steps)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double d = drow[r];
    double s = __builtin_amdgcn_rsq(d);
    s = s * fma(-0.5 * d * s, s, 1.5);
    s = s * fma(-0.5 * d * s, s, 1.5);
    a[r] *= s; x[r] *= s;
  }
  dmax = sqrt(dhi);                  // max R[j][j] = sqrt(max d_j)
  xmax = 1.0 / sqrt(dlo);            // max X[j][j] = 1 / sqrt(min d_j)
  return 0;
}

// sums of two per-lane values over the wave: shifts inside the 16-lane rows (DPP row_shr, no LDS traffic), then the four row
// totals through readlanes; every lane gets both sums
__device__ __forceinline__ double dpp_row_shr(double v, int sh)     // sh: compile-time 1, 2, 4, 8
{
  int lo = __double2loint(v), hi = __double2hiint(v);
  switch (sh) {
    case 1: lo = __builtin_amdgcn_update_dpp(0, lo, 0x111, 0xf, 0xf, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0x111, 0xf, 0xf, true); break;
    case 2: lo = __builtin_amdgcn_update_dpp(0, lo, 0x112, 0xf, 0xf, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0x112, 0xf, 0xf, true); break;
    case 4: lo = __builtin_amdgcn_update_dpp(0, lo, 0x114, 0xf, 0xf, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0x114, 0xf, 0xf, true); break;
    default: lo = __builtin_amdgcn_update_dpp(0, lo, 0x118, 0xf, 0xf, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0x118, 0xf, 0xf, true); break;
  }
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ void wave_sum2(double& p, double& q)
{
#pragma unroll
  for (int sh = 1; sh < 16; sh <<= 1) { p += dpp_row_shr(p, sh); q += dpp_row_shr(q, sh); }     // lane 15 of each row: the row's sum
  p = ((rlane(p, 15) + rlane(p, 31)) + rlane(p, 47)) + rlane(p, 63);
  q = ((rlane(q, 15) + rlane(q, 31)) + rlane(q, 47)) + rlane(q, 63);
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// LDS use of ortho_tail16 (doubles): [0,256) G hand-over / transpose scratch (16 x 17), [272,528) Wd for the assembly,
// [528,784) Wp for the assembly
#define T16_LDS_DOUBLES 784
#define T16_ZS_ROWS DMAT_LD                // rows of the coefficient block the exact projection (OrthoTailArgs::dmat) keeps in LDS behind them

// One step of the state machine for k <= 16, called by ALL 256 threads of a block (wave 0 does the serial part, all four
// waves assemble the coefficient block of a projection sweep).  g_in_lds: lds[64 r + lane] already holds the Gram matrix
// in C-layout (a single-tile reduction hands it over from its registers).
__device__ __forceinline__ void ortho_tail16(const OrthoTailArgs& a, double* lds, const TailState* pre, bool g_in_lds, unsigned long long t_entry = 0)
{
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  OrthoDev* st = a.st;
  __shared__ int s_go;
  if (pre == nullptr) {
    const int ph = __hip_atomic_load(&st->phase, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // (the first sweep of any chain answers the start phase; a plain projection sweep in a three-pass chain would answer the
    //  measuring one's -- no plan contains one any more, see ortho_chain_begin)
    const int need = a.after == OP_GRAMX ? (int)OP_GRAM_UU : (a.x3 && a.after == OP_COMBO) ? (int)OP_COMBOX : a.after;
    if (ph != need) {
      if (a.publish && tid == 0 && st->nops > 0) *a.st_host = *st;
      return;
    }
  }
  const int k = a.k, m = a.m;
  const double eps = 2.220446049250313e-16, tol = 2.0 * eps;
  const int maxit = a.maxit, can_defer = a.can_defer;
  const int after = a.after;
  const bool sweep_xu = (after == OP_GRAMX || after == OP_XW || after == OP_COMBOX);   // this sweep formed xu (and G) in xug, on the stored block
  const int op_project = a.x3 ? (int)OP_COMBOX : (int)OP_COMBO;       // the projection sweep of this chain
  // coefficient source of a possible assembly: rows of xu, prefetched by every wave (tiles wave, wave + 4, ...)
  const double* xsrc = (after == OP_XU || sweep_xu) ? a.gsrc : a.xug;
  const int ldx = (after == OP_XU) ? m : m + k;
  const bool may_assemble = m > 0 && (after == OP_XU || sweep_xu || after == OP_GRAMW || after == OP_TRMMG || after == OP_TRMMC);
  double xa[4][4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int row = 16 * (wave + 4 * q) + c, col = 4 * s + g;
      xa[q][s] = 0.0;
      if (may_assemble && row < m && col < k)
        xa[q][s] = __hip_atomic_load(xsrc + (size_t)row + (size_t)col * ldx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  double* lds_d = lds + 272;
  double* lds_p = lds + 528;
  // max |X^T U| of the stored block (three-pass schedule: what a closing projection on the small side has to be small against)
  __shared__ double s_smax[4];
  __shared__ double s_colsq[4][16];            // sum over this wave's rows of S(row, col)^2
  const bool meas_sweep = a.x3 && (after == OP_COMBOX || after == OP_XW);    // S = X^T U and G = U^T U measured on the block the sweep stored
  // a caller that folds pending blocks into its small matrices: the chain ends wherever X^T U has been measured on the stored block
  // and the factor of that block has converged (see ortho_tail) -- for the sweep-per-update schedule that is the step behind OP_XU
  const bool may_pend = a.drop_final && a.t_host != nullptr && m > 0;
  // (tight: the caller's stored basis is orthonormal to drop_tol only -- dla_expand_project mode 4 -- and a projection against it
  //  leaves that share of what it removes: no chain may END behind a projection that removed more than TIGHT_REMOVES)
  const bool tight = a.drop_tol > 0.0 && may_assemble;
  if (meas_sweep || (may_pend && after == OP_XU) || tight) {
    double sm = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int s = 0; s < 4; ++s) sm = fmax(sm, fabs(xa[q][s]));
    double sq_far[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t0 = 16 * (wave + 16); t0 < m; t0 += 64)          // (m > 256: the rows beyond the prefetched ones)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int row = t0 + c, col = 4 * s + g;
        if (row < m && col < k) {
          const double v = __hip_atomic_load(xsrc + (size_t)row + (size_t)col * ldx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          sm = fmax(sm, fabs(v));
          sq_far[s] += v * v;
        }
      }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sm = fmax(sm, __shfl_xor(sm, off, 64));
    if (lane == 0) s_smax[wave] = sm;
    // column 4 s + g: the 16 lanes of row group g hold its rows
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      double sq = sq_far[s];
#pragma unroll
      for (int q = 0; q < 4; ++q) sq += xa[q][s] * xa[q][s];
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);
      if (c == 0) s_colsq[wave][4 * s + g] = sq;
    }
    __syncthreads();
  }
  // zs <- D^T zs for the caller's upper-triangular D (a.dmat), 16 x 16 tiles on the matrix cores: D(Q, R) = 0 for Q > R.  A wave owns
  // the row tiles R = wave, wave + 4, ...; products with the contraction index p = g + 4 s: A[c][p], B[p][c] (see mfma16).
  // Called by all 256 threads; zs holds [16 nt][16] doubles.
  double* zs = lds + T16_LDS_DOUBLES;
  auto dt_times_zs = [&](int nt) {
    const int ld = a.dmat_ld;
    __syncthreads();
    v4d y1[5];
#pragma unroll
    for (int qq = 0; qq < 5; ++qq) {
      const int R = wave + 4 * qq;
      y1[qq] = (v4d){0.0, 0.0, 0.0, 0.0};
      if (R < nt)
        for (int Q0 = 0; Q0 <= R; Q0 += 4) {
          // (four tiles of D per round: sixteen loads in flight, then sixteen MFMAs)
          double av[4][4];
#pragma unroll
          for (int dq = 0; dq < 4; ++dq)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
              const int rowd = 16 * (Q0 + dq) + g + 4 * s, cold = 16 * R + c;        // A[c][p] = D(16 Q + p, 16 R + c)
              av[dq][s] = (Q0 + dq <= R && rowd < m && cold < m) ? a.dmat[(size_t)rowd + (size_t)cold * ld] : 0.0;
            }
#pragma unroll
          for (int dq = 0; dq < 4; ++dq)
            if (Q0 + dq <= R)
#pragma unroll
              for (int s = 0; s < 4; ++s)
                y1[qq] = mfma16(av[dq][s], lds_load1(zs + (size_t)(16 * (Q0 + dq) + g + 4 * s) * 16 + c), y1[qq]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int qq = 0; qq < 5; ++qq) {
      const int R = wave + 4 * qq;
      if (R < nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) lds_store1(zs + (size_t)(16 * R + g + 4 * r) * 16 + c, y1[qq][r]);
    }
    __syncthreads();
  };
  // The first projection (the step behind OP_GRAMX in a three-pass chain) takes its triangular factor from the Gram matrix of the
  // block it is about to STORE: (U - X (D D^T) S)^T (U - X (D D^T) S) = G - Y^T Y with Y = D^T S, all of it measured by the sweep in
  // front of this step.  The reference factors U^T U there (its ortho_cd in front of the loop, :3533) and finds, behind the
  // projection, a block whose columns have lost most of their norm and some of their independence -- on the benchmark a Gram
  // matrix 1.0 off the identity, a second projection with its factor, a third factor.  With the projected block's own factor the
  // stored block comes out near orthonormal (to eps cond^2 of the PROJECTED block), and its measured S and G usually end the chain:
  // two passes over X instead of three.  Same Q factor as the reference's in exact arithmetic (every factor is upper triangular
  // with a positive diagonal); a Gram matrix that is not positive definite, or has lost 13 digits to the subtraction, leaves the
  // reference's order in place (level shifts included).
  const int it_outer_in = pre ? pre->it_outer : st->it_outer;
  const bool gp_step = a.gp && a.x3 && a.fold == 1 && after == OP_GRAMX && m > 0 && m <= 256 && a.lead_once && can_defer && it_outer_in == 0;
  v4d gp_p = (v4d){0.0, 0.0, 0.0, 0.0};
  if (gp_step) {
    const int nt = (m + 15) / 16;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int t0 = 16 * (wave + 4 * q);
      if (t0 < 16 * nt) {
#pragma unroll
        for (int s = 0; s < 4; ++s) lds_store1(zs + (size_t)(t0 + c) * 16 + 4 * s + g, xa[q][s]);      // (zero beyond m and k)
      }
    }
    if (a.dmat != nullptr) dt_times_zs(nt);
    else __syncthreads();
    if (wave == 0) {
      for (int R = 0; R < nt; ++R)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const double v = lds_load1(zs + (size_t)(16 * R + 4 * s + g) * 16 + c);     // A[c][p] = B[p][c] = Y(16 R + p, c)
          gp_p = mfma16(v, v, gp_p);
        }
    }
    __syncthreads();     // (the assembly below reuses zs)
  }
  // max_j sum_i S_ij^2 >= |(S^T S)_ij|: what the Gram matrix of the projected block differs from G by (wave 0, every lane)
  auto colsq_max = [&]() {
    double cs = lane < 16 ? ((s_colsq[0][lane] + s_colsq[1][lane]) + s_colsq[2][lane]) + s_colsq[3][lane] : 0.0;
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) cs = fmax(cs, __shfl_xor(cs, off, 64));
    return rlane(cs, 0);
  };
  // (a pending block's projection is closed on the caller's k x k matrices through the Cholesky factor of I - F^T F, F = D^T S T:
  //  that stays well conditioned while the columns' sums of squares do)
  const double CS_CAP = 0.02;
  if (wave == 0) {
    TailState t = pre ? *pre : TailState{st->it_macro, st->it_outer, st->macro_total, st->shifts, st->nops, OP_NONE, OST_RUNNING, st->growth, st->have_xu, st->sloppy, st->gdev};
    t.phase = OP_NONE; t.status = OST_RUNNING;
    const int force_defer = can_defer && t.it_outer == 0;
    int go = 0;
    v4d pnew, dnew;
    const int dslot = t.nops;
    if (lane == 0 && a.dbg != nullptr && dslot < 48) { a.dbg[dslot * 16 + 8] = t_entry; a.dbg[dslot * 16 + 9] = (unsigned long long)after; }
    if (lane == 0) TSTAMP(a, dslot, 0);
    if (after == OP_FINAL || after == OP_CLOSE) {
      t.status = OST_DONE;
    } else if (after == OP_XU) {
      // the block in memory is U_mem with Wp pending: C' = [-(X^T U_mem) Wp ; Wp]
#pragma unroll
      for (int r = 0; r < 4; ++r) { pnew[r] = a.wst[512 + 64 * r + lane]; dnew[r] = pnew[r]; }
      const double wn = fmax(t.growth, 1.0);     // norm estimate of Wp: what has to be small is (X^T U_mem) Wp
      t.it_macro = 0; t.growth = 1.0; t.have_xu = 0; t.sloppy = 0;
      // a projection against stored columns that are orthonormal to drop_tol = 1e-8 only leaves m 1e-8 of what it removes: when that
      // is more than TIGHT_REMOVES the block needs another measured projection behind this one (fuzz_pending_basis.py: a block that lies in
      // span(X) to 1e-9 came out orthogonal to the finished basis to 1.7e-10 only)
      if (tight && fmax(fmax(s_smax[0], s_smax[1]), fmax(s_smax[2], s_smax[3])) * wn >= TIGHT_REMOVES) t.sloppy = 1;
      // (the block stays pending when the caller takes pending blocks and both X^T U, just measured, and the distance of the
      //  pending factor from the identity -- the Gram matrix it came from -- are within the caller's bounds)
      if (may_pend && fmax(fmax(s_smax[0], s_smax[1]), fmax(s_smax[2], s_smax[3])) * wn < a.drop_stol && t.gdev < (a.drop_tol > 0.0 ? a.drop_tol : 1.0) &&
          colsq_max() * wn * wn < CS_CAP) { t.status = OST_DONE; go = 2; }
      else { t.phase = op_project; go = 1; }
    } else {
      ++t.it_macro;
      if (t.it_macro > maxit) {
        t.status = OST_CD_MAXIT;
      } else {
        ++t.macro_total;
        // the sweep left the block itself in memory (nothing pending), or its Gram matrix belongs to U_mem Wp formed on the fly
        const bool fresh = (after != OP_GRAMW);
        const bool stage0 = can_defer && t.it_outer == 0;       // the ortho_cd in front of the loop (:3533)
        if (after == OP_TRMMG && !stage0) t.have_xu = 0;        // (closing passes use a measured X^T U only)
        v4d ptold, dtold;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double id = (g + 4 * r == c) ? 1.0 : 0.0;
          ptold[r] = fresh ? id : a.wst[64 * r + lane];
          dtold[r] = (sweep_xu || !t.have_xu) ? id : a.wst[256 + 64 * r + lane];
        }
        // Gram matrix, lower triangle mirrored, identity beyond k
        v4d g0;
        const int roff = sweep_xu ? m : 0, ldg = sweep_xu ? m + k : k;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = g + 4 * r, hi = i > c ? i : c, lo = i > c ? c : i;
          double v = (i == c) ? 1.0 : 0.0;
          if (i < k && c < k) {
            if (g_in_lds) v = lds_load1(lds + 64 * (hi >> 2) + 16 * (hi & 3) + lo);     // register hi >> 2, lane 16 (hi & 3) + lo
            else v = __hip_atomic_load(a.gsrc + (size_t)(roff + hi) + (size_t)lo * ldg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          g0[r] = v;
        }
        {
          double dv = 0.0;                // max |G - I| (identity beyond k)
#pragma unroll
          for (int r = 0; r < 4; ++r) dv = fmax(dv, fabs(g0[r] - ((g + 4 * r == c) ? 1.0 : 0.0)));
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) dv = fmax(dv, __shfl_xor(dv, off, 64));
          t.gdev = dv;
        }
        v4d am = g0, x;
        double dmax, xmax;
        if (lane == 0 && g0[0] == g0[0]) TSTAMP(a, dslot, 1);
        const unsigned long long cyc0 = a.dbg ? __builtin_readcyclecounter() : 0ULL;
        // factorisation; on a non-positive pivot the level-shift ladder (:3265-3295): shift = max(eps alpha ||U||_F, 2 eps),
        // alpha = 100, 1000, ...  (one call site: the factorisation loop exists once in the code)
        int info = 1, it_micro = 0;
        double alpha = 100.0, unorm = -1.0;
        bool used_gp = false;
        if (gp_step) {
          v4d amp;
          double lost = 1.0;           // smallest ratio of a projected column's squared norm to the column's own
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool in = (g + 4 * r < k && c < k);
            amp[r] = in ? g0[r] - gp_p[r] : g0[r];
            if (in && g + 4 * r == c) lost = fmin(lost, g0[r] > 0.0 ? amp[r] / g0[r] : 0.0);
          }
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) lost = fmin(lost, __shfl_xor(lost, off, 64));
          if (lost > 1.0e-13) {
            // (a projected block that is numerically rank deficient gets the reference's level shifts, :3265-3295, on ITS Gram
            //  matrix: the factor is then only approximate, and everything behind it is measured on what it stored)
            const v4d amp0 = amp;
            double trp = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) if (g + 4 * r == c && c < k) trp += amp0[r];
            const double tr = wave_sum(trp), un = sqrt(tr > 0.0 ? tr : 0.0);
            double al = 100.0;
            int itm = 0;
            for (;;) {
              info = chol_inv16(k, amp, x, dmax, xmax, lane);
              if (info == 0 || ++itm > maxit || a.gp < 2) break;
              const double shift = fmax(eps * al * un, tol);
#pragma unroll
              for (int r = 0; r < 4; ++r) amp[r] = amp0[r] + ((g + 4 * r == c && c < k) ? shift : 0.0);
              al *= 10.0;
            }
            if (info == 0) { used_gp = true; am = amp; t.shifts += itm; }
          }
        }
        if (!used_gp) for (;;) {
          info = chol_inv16(k, am, x, dmax, xmax, lane);
          if (info == 0) break;
          if (unorm < 0.0) {
            double trp = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) if (g + 4 * r == c && c < k) trp += g0[r];
            const double tr = wave_sum(trp);
            unorm = sqrt(tr > 0.0 ? tr : 0.0);       // ||U||_F = sqrt(trace(U^T U)), dnrm2 at :3268
          }
          if (++it_micro > maxit) break;
          const double shift = fmax(eps * alpha * unorm, tol);
#pragma unroll
          for (int r = 0; r < 4; ++r) am[r] = g0[r] + ((g + 4 * r == c && c < k) ? shift : 0.0);
          alpha *= 10.0;
          ++t.shifts;
        }
        if (it_micro > 0) t.gdev = fmax(t.gdev, 2.0);       // (no pending ending behind a shifted factor: see ortho_tail)
        if (info != 0) {
          t.status = OST_FACTOR_FAIL;
        } else {
          // norm_est (:3447-3479) of L = R^T and of L^-1: largest diagonal entry + Frobenius norm of the strict triangle
          double fr = 0.0, fx = 0.0;
          if (lane == 0 && x[0] == x[0]) TSTAMP(a, dslot, 2);
          if (lane == 0 && a.dbg != nullptr && dslot < 48) a.dbg[dslot * 16 + 11] = __builtin_readcyclecounter() - cyc0;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = g + 4 * r;
            if (i < k && c < k) { if (c > i) fr += am[r] * am[r]; if (c < i) fx += x[r] * x[r]; }
          }
          wave_sum2(fr, fx);
          const double l_norm = dmax + sqrt(fr), linv_norm = xmax + sqrt(fx);
          if (lane == 0 && l_norm == l_norm) TSTAMP(a, dslot, 3);
          // W = X^T in C-layout (transpose through LDS; the wave's LDS operations complete in order)
          TSYNC();
#pragma unroll
          for (int r = 0; r < 4; ++r) lds_store1(lds + (g + 4 * r) * 17 + c, x[r]);
          TSYNC();
          v4d w;
#pragma unroll
          for (int r = 0; r < 4; ++r) w[r] = lds_load1(lds + c * 17 + (g + 4 * r));
          TSYNC();
          // Wp <- Wp W, Wd <- Wd W and their transposes (X M^T = (M W)^T)
          v4d ptnew = (v4d){0.0, 0.0, 0.0, 0.0}, dtnew = ptnew;
          pnew = ptnew; dnew = ptnew;
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            pnew = mfma16(ptold[s], w[s], pnew);
            ptnew = mfma16(w[s], ptold[s], ptnew);
            dnew = mfma16(dtold[s], w[s], dnew);
            dtnew = mfma16(w[s], dtold[s], dtnew);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            a.wst[64 * r + lane] = ptnew[r];
            a.wst[256 + 64 * r + lane] = dtnew[r];
            a.wst[512 + 64 * r + lane] = pnew[r];
            const int pp = g + 4 * r;
            a.wpk[pp * 16 + c] = (pp < k && c < k) ? pnew[r] : 0.0;      // packed for the sweeps: [16][16], zero padded
          }
          if (lane == 0 && pnew[0] == pnew[0]) TSTAMP(a, dslot, 4);
          if (sweep_xu) t.have_xu = 1;
          const double rcond = l_norm * linv_norm;
          if (lane == 0 && a.dbg != nullptr && dslot < 48) a.dbg[dslot * 16 + 10] = (unsigned long long)__double_as_longlong(rcond);
          if (a.dbg != nullptr && dslot < 48) {
            // (debug) how far the Gram matrix of this step is from the identity: max |G - I|
            double dev = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) dev = fmax(dev, fabs(g0[r] - ((g + 4 * r == c) ? 1.0 : 0.0)));
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) dev = fmax(dev, __shfl_xor(dev, off, 64));
            if (lane == 0) a.dbg[dslot * 16 + 12] = (unsigned long long)__double_as_longlong(dev);
          }
          t.growth *= linv_norm;
          // The ortho_cd in front of the loop is not iterated (lead_once): its result feeds the first projection, which is
          // linear in the block and does not care how orthonormal it is, and every later decision is taken on Gram matrices
          // measured after that projection.  The reference's second macro-iteration there (its first one leaves condition
          // 1 + O(eps c^2), the second one confirms it) costs a sweep and a k x k step per call and changes nothing the closing
          // passes do not re-measure; with a carried X^T U of that quality (growth eps >= tol_ortho) the closing pass is
          // mandatory (sloppy), as for every carried product.  Not after a level shift: a numerically rank-deficient block
          // keeps the reference's order of operations (see ortho_tail), because its weakest columns are amplified rounding
          // noise whose realisation depends on that order and the solvers' convergence history on the noise.
          const bool macro_done = (eps * rcond * rcond < tol) || (stage0 && a.lead_once && a.fold == 1 && after == OP_GRAMX && it_micro == 0);      // :3331-3332
          // Three-pass schedule (x3).  OP_COMBOX (and OP_XW) have measured S = X^T U and G = U^T U on the block they stored, so their
          // step never needs a sweep that only measures:
          //   * factor not converged (the block that comes out of the first projection is as ill-conditioned as the expansion
          //     vectors are dependent -- 1e7 on the benchmark): the next projection follows at once, C' = [-(S W) ; W].  It removes
          //     what the last one left (S is measured, not carried) and applies W in the same sweep -- the reference's second pass
          //     over X (:3543-3544) moved in front of the second macro-iteration of ortho_cd instead of behind it.  Its result
          //     carries an X component of order eps ||W||: the closing projection is mandatory (sloppy).  (After a level shift the
          //     reference's order is kept, as everywhere: written update, then OP_XW.)
          //   * factor converged: the reference's closing pass is  S = X^T U (:3543), U -= X S (:3544), one macro-iteration of
          //     ortho_cd with a near-identity factor (:3256-3327).  S and G are already here, measured on the stored block.
          //       - a caller that folds pending blocks into its small matrices (drop_final + t_host) gets [-(S W) ; W] and the chain
          //         ENDS: no sweep at all.  The caller finishes the algebra exactly (dla_basis_admit: the Gram matrix of the
          //         projected block is G - S^T S, which it corrects with a k x k factor of its own), so S only has to be small
          //         enough for that correction to be well conditioned and for the stored basis to stay a good one for the
          //         projections of later blocks: max |S| below drop_stol, max |G - I| below drop_tol;
          //       - otherwise the pass is the single sweep U <- [X | U] [-(S W) ; W] (OP_CLOSE, nothing measured behind it -- the
          //         reference does not measure behind its last update either), when it is due (sloppy, growth eps >= tol_ortho,
          //         :3562-3564).  G was measured before the projection instead of after it: the two differ by S^T S, so this
          //         takes place only for max |S| < 1e-9 (m |S|^2 below eps); a larger S gets one more measured projection.
          const bool cx_step = meas_sweep && !stage0 && it_micro == 0;
          // (behind OP_TRMMC: the carried product is good for a pending block when this step's factor has converged without a
          //  level shift; otherwise the chain goes on as behind any written update, on measured products only)
          const bool carried_pend = after == OP_TRMMC && macro_done && it_micro == 0 && may_pend && t.have_xu;
          if (after == OP_TRMMC && !carried_pend) t.have_xu = 0;
          const double smax = cx_step ? fmax(fmax(s_smax[0], s_smax[1]), fmax(s_smax[2], s_smax[3])) : 0.0;
          bool pend = false, pend_e = false, pend_r = false;
          // (X^T U too large to stay on the small side of a basis that has to remain orthonormal in memory, but small enough for the
          //  Gram matrix of the projected block, I - (S W)^T (S W), to be factored by the caller: the closing sweep runs without
          //  measuring anything and the caller gets [-(S W) ; W] marked APPLIED -- it owes the block only the k x k factor)
          if (cx_step && macro_done && may_pend && smax >= a.drop_stol && t.it_outer <= maxit && a.dmat == nullptr) {
            // |(S^T S)_ij| <= max_j sum_i S_ij^2: what the block's Gram matrix in memory will be off the identity by
            const double cs = colsq_max();
            pend_r = 2.0 * cs < (a.drop_tol > 0.0 ? a.drop_tol : 1.0e-8);
            if (lane == 0 && a.dbg != nullptr && dslot < 48) a.dbg[dslot * 16 + 14] = (unsigned long long)__double_as_longlong(cs);
          }
          if (cx_step && macro_done && may_pend && smax < a.drop_stol) {
            double dev = 0.0;              // max |G - I| of this pass (g0: the Gram matrix, identity beyond k)
#pragma unroll
            for (int r = 0; r < 4; ++r) dev = fmax(dev, fabs(g0[r] - ((g + 4 * r == c) ? 1.0 : 0.0)));
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) dev = fmax(dev, __shfl_xor(dev, off, 64));
            pend = a.drop_tol <= 0.0 || dev < a.drop_tol;
            pend_e = !pend;
            if (pend && colsq_max() >= CS_CAP) pend = false;      // (one more measured projection: the branch for a large S below)
          }
          if (lane == 0 && a.dbg != nullptr && dslot < 48) a.dbg[dslot * 16 + 13] = (unsigned long long)__double_as_longlong(smax);
          if (pend) {
            t.status = OST_DONE; go = 2;                          // the closing block stays pending
          } else if (pend_e) {
            // X^T U is small enough to stay on the small side, the factor is not (a block that stays in the caller's basis has to
            // be orthonormal to drop_tol in memory): the projection stays pending, [-(S W) ; I], and the factor is applied by the
            // cheapest sweep there is (U <- U W, nothing of X is read)
            t.phase = OP_FINAL; go = 3;
          } else if (pend_r) {
            t.phase = OP_CLOSE; go = 4;
          } else if (carried_pend) {
            // (the update behind a measured X^T U has been written and its Gram matrix measured: S W was carried, see below)
            double dev = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) dev = fmax(dev, fabs(g0[r] - ((g + 4 * r == c) ? 1.0 : 0.0)));
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) dev = fmax(dev, __shfl_xor(dev, off, 64));
            if (a.drop_tol <= 0.0 || dev < a.drop_tol) { t.status = OST_DONE; go = 2; }
            else { t.phase = OP_FINAL; go = 3; }
          } else if (cx_step && (!macro_done || smax >= 1.0e-9 || (may_pend && smax < a.drop_stol && macro_done && !pend_e))) {
            // A caller with pending blocks, a factor that has not converged but is close (eps rcond^2 < 1e-10: W is within a few
            // hundred of the identity) and an X^T U so small that S W stays far inside the caller's bound: the next macro-iteration
            // of ortho_cd does not need X.  U <- U W is written with the Gram matrix of what it stores (OP_TRMMC), X^T (U W) = S W
            // is carried exactly as the first projection's product is (Wd), and when that Gram matrix's factor has converged the
            // block stays pending as [-(S W) T ; T].  What the written update adds to X^T U is its rounding, eps ||W|| at most --
            // the reference's own last update (dtrsm behind its last projection, :3327) leaves the same.
            const bool carry = may_pend && !macro_done && eps * rcond * rcond < 1.0e-10 && 4.0 * smax * linv_norm < a.drop_stol;
            if (t.it_outer > maxit) t.status = OST_VSX_MAXIT;     // :3568
            else if (carry) { t.sloppy = 1; t.phase = OP_TRMMC; }
            else {
              ++t.it_outer;
              t.sloppy = macro_done ? 0 : 1;
              t.it_macro = 0; t.growth = 1.0; t.have_xu = 0; t.phase = OP_COMBOX; go = 1;
            }
          } else if (cx_step) {
            const bool need_proj = t.sloppy || t.growth * eps >= tol || may_pend;
            if (t.it_outer > maxit && need_proj) t.status = OST_VSX_MAXIT;
            else if (need_proj || smax >= 64.0 * eps) { t.phase = OP_CLOSE; go = 1; }
            else t.phase = OP_FINAL;
          } else if (!macro_done) {
            // another macro-iteration.  In front of the loop its Gram matrix comes from U_mem Wp on the fly -- unless the
            // factorisation needed a level shift (rank-deficient block: the update is written); inside the loop the update is
            // written, together with X^T U and U^T U of what is stored (OP_XW) when it is expected to be the last one
            if (!can_defer || a.fold != 1) t.phase = OP_TRMMG;           // (fold == 2: odd n, no on-the-fly sweeps)
            else if (stage0) t.phase = (it_micro > 0) ? OP_TRMMG : OP_GRAMW;
            // (a Cholesky-QR step without a level shift almost always leaves a block that passes the test -- measured on the
            //  benchmark: every time -- while a shifted one never does: without a shift the update sweep measures X^T U of
            //  what it stores on its way, a wrong guess costs one more sweep over X)
            else if (it_micro == 0) t.phase = OP_XW;
            else { t.phase = OP_TRMMG; t.have_xu = 0; }
          } else if (can_defer && (force_defer || t.sloppy || t.growth * eps >= tol || (a.drop_tol > 0.0 && t.it_outer < 2))) {
            // ortho_vs_x goes on with a projection pass (xu_norm = growth eps >= tol, :3562-3564)
            // (drop_tol > 0: always two projections against a basis that may carry pending blocks, see ortho_tail)
            if (!force_defer && t.it_outer > maxit) t.status = OST_VSX_MAXIT;     // :3568
            else {
              ++t.it_outer;
              if (t.have_xu) {
                t.sloppy = (stage0 && t.growth * eps >= tol) ? 1 : 0;
                if (tight && fmax(fmax(s_smax[0], s_smax[1]), fmax(s_smax[2], s_smax[3])) * fmax(t.growth, 1.0) >= TIGHT_REMOVES) t.sloppy = 1;    // (see OP_XU above)
                t.it_macro = 0; t.growth = 1.0; t.have_xu = 0; t.phase = op_project; go = 1;
              }
              else t.phase = OP_XU;
            }
          } else {
            if (can_defer && t.it_outer > maxit) t.status = OST_VSX_MAXIT;
            else if (a.drop_final && (a.drop_tol <= 0.0 || [&]() {
                       double dev = 0.0;              // max |G - I| of this pass (g0: the Gram matrix, identity beyond k)
#pragma unroll
                       for (int r = 0; r < 4; ++r) dev = fmax(dev, fabs(g0[r] - ((g + 4 * r == c) ? 1.0 : 0.0)));
                       for (int off = 32; off > 0; off >>= 1) dev = fmax(dev, __shfl_xor(dev, off, 64));
                       return dev < a.drop_tol; }())) {
              t.status = OST_DONE;
              if (a.t_host != nullptr) {
                // the factor that stays pending: Wp (accumulator layout: lane (c, g) holds Wp(g + 4 r, c))
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  const int pp = g + 4 * r;
                  if (pp < k && c < k) a.t_host[(size_t)pp * PEND_LD + c] = pnew[r];
                }
                __threadfence_system();
                if (lane == 0) { a.t_host[PEND_HDR + 1] = 0.0; a.t_host[PEND_HDR + 2] = 0.0; a.t_host[PEND_HDR] = (double)a.t_seq; }
              }
            }
            else t.phase = OP_FINAL;
          }
        }
      }
    }
    if (go) {
#pragma unroll
      for (int r = 0; r < 4; ++r) { lds_store1(lds_d + 64 * r + lane, dnew[r]); lds_store1(lds_p + 64 * r + lane, pnew[r]); }
    }
    if (lane == 0) { TSTAMP(a, dslot, 5); s_go = go; tail_publish(a, t); TSTAMP(a, dslot, 6); }
  }
  __syncthreads();
  if (!s_go) return;
  // C' = [-(xu Wd) ; Wp ; 0], packed [l4][16] for the projection sweep; 16 rows of xu per MFMA quadruple
  // (s_go >= 2: the block stays pending -- it also goes to the caller's pinned buffer, the header last; 3: only its projection
  //  part does, the factor is applied in memory by the OP_FINAL sweep that follows)
  const bool to_host = s_go >= 2;
  const bool t_ident = s_go == 3;
  const double applied = s_go == 4 ? 1.0 : 0.0;     // 4: the whole block is applied in memory by the OP_CLOSE sweep that follows
  const int l = m + k, l4 = ((l + 3) / 4) * 4;
  // Exact projection against an unfinished basis (a.dmat): Z = xu Wd goes to LDS first, the coefficients become -(D D^T) Z.  The
  // block that goes to the HOST stays -Z: the caller applies D D^T itself (dla_basis_admit).
  // (the coefficients are only read by a sweep that follows: a block that stays pending needs none -- s_go 2, 3)
  const bool dfix = a.dmat != nullptr && m <= T16_ZS_ROWS && (s_go == 1 || s_go == 4);          // (zs: [16 ceil(m / 16)][16])
  // behind OP_GRAMX zs still holds Y = D^T S of the step's first phase: D^T (S Wd) = Y Wd, one product with D saved
  const bool have_y = dfix && gp_step;
  double db[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) db[s] = lds_load1(lds_d + 64 * s + lane);
  if (have_y) {
    const int nt = (m + 15) / 16;
#pragma unroll
    for (int qq = 0; qq < 5; ++qq) {
      const int R = wave + 4 * qq;
      if (R >= nt) continue;
      v4d acc = (v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = mfma16(lds_load1(zs + (size_t)(16 * R + c) * 16 + 4 * s + g), db[s], acc);    // A[c][p] = Y(16 R + c, p)
#pragma unroll
      for (int r = 0; r < 4; ++r) lds_store1(zs + (size_t)(16 * R + g + 4 * r) * 16 + c, acc[r]);      // (the wave's own tile rows)
    }
  } else {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int t0 = 16 * (wave + 4 * q);
    if (t0 >= m) break;
    v4d acc = (v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = mfma16(xa[q][s], db[s], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p_ = t0 + g + 4 * r;
      if (dfix) lds_store1(zs + (size_t)p_ * 16 + c, (p_ < m && c < k) ? acc[r] : 0.0);
      else if (p_ < m) a.cpk[(size_t)p_ * 16 + c] = (c < k) ? -acc[r] : 0.0;
      if (to_host && p_ < m && c < k) a.t_host[(size_t)p_ * PEND_LD + c] = -acc[r];
    }
  }
  // (m > 256: the tiles beyond the prefetched ones)
  for (int t0 = 16 * (wave + 16); t0 < m; t0 += 64) {
    v4d acc = (v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int row = t0 + c, col = 4 * s + g;
      const double v = (row < m && col < k) ? __hip_atomic_load(xsrc + (size_t)row + (size_t)col * ldx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
      acc = mfma16(v, db[s], acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p_ = t0 + g + 4 * r;
      if (dfix) lds_store1(zs + (size_t)p_ * 16 + c, (p_ < m && c < k) ? acc[r] : 0.0);
      else if (p_ < m) a.cpk[(size_t)p_ * 16 + c] = (c < k) ? -acc[r] : 0.0;
      if (to_host && p_ < m && c < k) a.t_host[(size_t)p_ * PEND_LD + c] = -acc[r];
    }
  }
  }
  if (dfix) {
    // Z' = D (D^T Z): the first product through dt_times_zs (or Y Wd above), the second one the same way with D's rows
    const int nt = (m + 15) / 16, ld = a.dmat_ld;
    if (have_y) __syncthreads();
    else dt_times_zs(nt);
#pragma unroll
    for (int qq = 0; qq < 5; ++qq) {
      const int R = wave + 4 * qq;
      if (R >= nt) continue;
      v4d acc = (v4d){0.0, 0.0, 0.0, 0.0};
      for (int Q0 = R; Q0 < nt; Q0 += 4) {
        double av[4][4];
#pragma unroll
        for (int dq = 0; dq < 4; ++dq)
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const int rowd = 16 * R + c, cold = 16 * (Q0 + dq) + g + 4 * s;          // A[c][p] = D(16 R + c, 16 Q + p)
            av[dq][s] = (Q0 + dq < nt && rowd < m && cold < m) ? a.dmat[(size_t)rowd + (size_t)cold * ld] : 0.0;
          }
#pragma unroll
        for (int dq = 0; dq < 4; ++dq)
          if (Q0 + dq < nt)
#pragma unroll
            for (int s = 0; s < 4; ++s)
              acc = mfma16(av[dq][s], lds_load1(zs + (size_t)(16 * (Q0 + dq) + g + 4 * s) * 16 + c), acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p_ = 16 * R + g + 4 * r;
        if (p_ < m) a.cpk[(size_t)p_ * 16 + c] = (c < k) ? -acc[r] : 0.0;
      }
    }
  }
  if (wave == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int pp = g + 4 * r;
      if (pp < k) a.cpk[(size_t)(m + pp) * 16 + c] = (c < k) ? lds_load1(lds_p + 64 * r + lane) : 0.0;
      if (to_host && pp < k && c < k) a.t_host[(size_t)(m + pp) * PEND_LD + c] = t_ident ? (pp == c ? 1.0 : 0.0) : lds_load1(lds_p + 64 * r + lane);
    }
    for (int idx = lane; idx < (l4 - l) * 16; idx += 64) a.cpk[(size_t)l * 16 + idx] = 0.0;
    if (lane == 0 && pre != nullptr) TSTAMP(a, pre->nops, 7);
  }
  if (to_host) {
    __threadfence_system();
    __syncthreads();
    if (tid == 0) { a.t_host[PEND_HDR + 1] = (double)m; a.t_host[PEND_HDR + 2] = applied; __threadfence_system(); a.t_host[PEND_HDR] = (double)a.t_seq; }
  }
}

// b_ortho (reference diaglib.f90:3094-3183) behind a device-driven chain, without the host in between: M = U^T B U has been reduced
// into g (k x k, ld k); this one-wave kernel factors it (dpotrf 'l', :3173 -- no level shift, no refinement: the reference has
// none here), inverts the factor and leaves W = L^-T packed for the two triangular updates U <- U W, BU <- BU W (:3177-3178) that
// follow on the stream, predicated on *go == seq.  It only goes on when the chain in front of it has ENDED WELL (the state machine
// is re-armed and its last status is OST_DONE): after a chain that stopped half way the block is not orthogonal to X yet and
// must not be touched.  status (pinned host word): seq = done, -seq = the metric is not positive definite, 0 = did not run.
struct BOrthoTailArgs {
  const OrthoDev* st;
  const double* g;     // k x k, ld k (lower triangle used)
  double* wpk;         // [kt][k4][16]
  int k;
  int need_chain;      // 1: only behind a chain that ended with OST_DONE
  int seq;
  int* go;             // device word the updates are predicated on
  int* status_host;
};
__global__ __launch_bounds__(64) void bortho_tail_kernel(BOrthoTailArgs a)
{
  __shared__ __attribute__((aligned(16))) double lds[48 * TLD];
  const int lane = threadIdx.x, k = a.k;
  if (a.need_chain) {
    const bool ended_well = __hip_atomic_load(&a.st->phase, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)OP_GRAM_UU && a.st->nops == 0 &&
                            a.st->last_status == (int)OST_DONE;
    if (!ended_well) { if (lane == 0) { *a.go = 0; *a.status_host = 0; } return; }
  }
  double* A = lds;
  for (int idx = lane; idx < k * k; idx += 64) {
    const int i = idx % k, j = idx / k;
    if (i >= j) lds_store1(A + i * TLD + j, a.g[(size_t)i + (size_t)j * k]);
  }
  const int info = lds_potrf(k, A, lane);
  if (info != 0) { if (lane == 0) { *a.go = 0; *a.status_host = -a.seq; } return; }
  lds_trtri(k, A, lane);
  const int kt = (k + 15) / 16, k4 = ((k + 3) / 4) * 4;
  for (int idx = lane; idx < kt * k4 * 16; idx += 64) {
    const int q = idx / (k4 * 16), pp = (idx / 16) % k4, j = 16 * q + (idx % 16);
    a.wpk[idx] = (j < k && pp <= j) ? lds_load1(A + j * TLD + pp) : 0.0;
  }
  __threadfence();
  if (lane == 0) { *a.go = a.seq; *a.status_host = a.seq; }
}

__global__ __launch_bounds__(64) void ortho_tail_kernel(OrthoTailArgs a)
{
  __shared__ __attribute__((aligned(16))) double lds[TAIL_LDS_DOUBLES];
  ortho_tail(a, lds, threadIdx.x);
}

__global__ __launch_bounds__(256) void ortho_tail16_kernel(OrthoTailArgs a)
{
  __shared__ __attribute__((aligned(16))) double lds[T16_LDS_DOUBLES + T16_ZS_ROWS * 16];
  ortho_tail16(a, lds, nullptr, false);
}

// ======================================================================================
// One-shot all-reduce of a small buffer over peer mailboxes
// ======================================================================================
// Every reduction of this library is latency-bound (<= 64 KB: a k x k Gram matrix, an L x k projection block, a handful of
// norms).  Instead of a ring collective every rank writes its contribution straight into a slot of every peer's
// mailbox (one xGMI hop), raises a flag there, waits until all flags of its OWN mailbox are up and adds the slots in
// RANK ORDER -- the same sum, bit for bit, on every rank, whatever the arrival order.
//   * mailboxes are fine-grained device allocations shared through hipIpc handles (dla_p2p_export / dla_p2p_attach);
//   * two mailbox sets alternate (parity of the sequence number): a peer can write for call s+2 only after it has seen
//     this rank's flag for call s+1, which this rank raises only after it has finished reading call s;
//   * the wait is bounded (DLA_OPT_P2P_TIMEOUT_MS, default 5 s of the 100 MHz wall clock; 0 = no limit): a rank that gives up
//     writes the sequence number into the ERROR WORD of every mailbox (its own included), sets its status word and ends --
//     the grid always drains.  Every exchange looks at its own error word first and while it waits, so a peer that arrives
//     late -- it would find flag and data of the abandoned exchange in place and succeed alone -- fails the SAME exchange, and
//     so does every later one: all ranks report DLA_ERR_COMM at their next host wait, the transport stays down until it is
//     detached and exported again.  Ranks whose skew can exceed the limit (host-mode callbacks of unequal length, a paused
//     process) raise it or use the RCCL / hook transports, which have none;
//   * a launch belongs to the device-driven chains like any other: when it is not its turn (DLA_PREDICATED) it returns
//     before touching a mailbox, on every rank alike (all ranks hold the same phase).
#define P2P_MAX_RANKS 8
#define P2P_FLAG_STRIDE 16                 // one flag per 128-byte line
#define P2P_ERR_WORD(nr) ((size_t)2 * (nr) * P2P_FLAG_STRIDE)   // index of the error word behind a mailbox's flags
struct P2PArgs {
  double* buf;                             // in: this rank's contribution, out: the reduced values
  double* buf_host;                        // optional pinned mirror of the result
  int count, op;                           // op 0 sum, 1 max
  int nranks, rank;
  unsigned long long* executed;            // device word: exchanges this rank has completed.  The sequence number of a call
                                           // is taken from it, not from the host: launches of a device-driven chain that find
                                           // it is not their turn must not consume a number, or two consecutive exchanges
                                           // could fall on the same mailbox set (all ranks execute the same exchanges, so
                                           // the counters agree)
  double* data[P2P_MAX_RANKS];             // mailbox of rank r: [2][nranks][P2P_MAX_DOUBLES]
  unsigned long long* flags[P2P_MAX_RANKS];//                    [2][nranks][P2P_FLAG_STRIDE]
  int* status;                             // device word: != 0 after a timeout
  const int* phase; int want;
  unsigned long long timeout_ticks;        // 100 MHz ticks a rank waits for its peers; 0 = no limit
};

// the exchange itself, executed by the 256 threads of ONE block (ends with a block barrier); false: a peer timed out
__device__ __forceinline__ bool p2p_exchange(const P2PArgs& a)
{
  const unsigned long long seq = *a.executed + 1;
  const int tid = threadIdx.x, par = (int)(seq & 1ULL);
  const size_t slot = ((size_t)par * a.nranks + a.rank) * P2P_MAX_DOUBLES;
  // 1. my contribution into every mailbox (my own included)
  for (int r = 0; r < a.nranks; ++r) {
    double* dst = a.data[r] + slot;
    for (int i = tid; i < a.count; i += 256) __hip_atomic_store(dst + i, a.buf[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  __threadfence_system();
  __syncthreads();
  // 2. raise my flag everywhere, 3. wait for everyone's flag in my mailbox
  __shared__ int s_bad;
  unsigned long long* my_err = a.flags[a.rank] + P2P_ERR_WORD(a.nranks);
  if (tid == 0) s_bad = __hip_atomic_load(my_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0ULL;     // an earlier exchange was abandoned
  __syncthreads();
  if (!s_bad && tid < a.nranks) {
    __hip_atomic_store(a.flags[tid] + ((size_t)par * a.nranks + a.rank) * P2P_FLAG_STRIDE, seq, __ATOMIC_RELEASE,
                       __HIP_MEMORY_SCOPE_SYSTEM);
    const unsigned long long* mine = a.flags[a.rank] + ((size_t)par * a.nranks + tid) * P2P_FLAG_STRIDE;
    const unsigned long long t0 = wall_clock64();
    while (__hip_atomic_load(mine, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < seq) {
      if (__hip_atomic_load(my_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0ULL) { s_bad = 1; break; }   // a peer gave up
      if (a.timeout_ticks != 0ULL && wall_clock64() - t0 > a.timeout_ticks) { s_bad = 2; break; }
      __builtin_amdgcn_s_sleep(8);
    }
  }
  __syncthreads();
  if (s_bad) {
    // tell everyone (a peer that is late for this exchange must fail it too), then the host
    if (tid < a.nranks) __hip_atomic_store(a.flags[tid] + P2P_ERR_WORD(a.nranks), seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (tid == 0) __hip_atomic_store(a.status, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
    return false;
  }
  // 4. combine the slots of my mailbox in rank order
  const double* mine = a.data[a.rank] + (size_t)par * a.nranks * P2P_MAX_DOUBLES;
  for (int i = tid; i < a.count; i += 256) {
    double v = __hip_atomic_load(mine + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    for (int r = 1; r < a.nranks; ++r) {
      const double x = __hip_atomic_load(mine + (size_t)r * P2P_MAX_DOUBLES + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      v = a.op == 0 ? v + x : fmax(v, x);
    }
    a.buf[i] = v;
    if (a.buf_host) a.buf_host[i] = v;
  }
  if (tid == 0) *a.executed = seq;         // (every thread read the old value before the first barrier above)
  __syncthreads();
  return true;
}

__global__ __launch_bounds__(256) void p2p_allreduce_kernel(P2PArgs a)
{
  DLA_PREDICATED(a);
  (void)p2p_exchange(a);
}

struct GramReduceArgs {
  const double* partial;
  double* lvl2;        // [output tiles][groups][256]
  unsigned* ticket;    // [output tiles], zero between launches
  double* c;           // l x k, ld = ldc (device)
  double* c_host;      // same, pinned host mirror (device-visible address)
  int nblk, l, k, tlw, kt, passes_x;
  const int* phase;
  int want;
  // device-driven chains on one rank: the block that completes the LAST output tile also runs the state machine's
  // step (ortho_tail / ortho_tail16) on the reduced matrix, so that no further launch stands between two sweeps
  int do_tail;
  int n_ps;            // number of output tiles = passes * tlw * kt + extra
  unsigned* gticket;   // zero between launches
  OrthoTailArgs tail;
  // ... and with several ranks on the peer-to-peer transport the same block first exchanges the reduced matrix with
  // its peers (p2p.nranks > 1), so that sweep -> [reduce, cross-rank sum, k x k step] is still one launch
  P2PArgs p2p;
  int extra;           // more output tiles behind the tlw * kt slots of pass 0 (gram_lds_kernel WP: the tiles qi >= qj of the Gram
                       // matrix of the U block, 1 / 3 / 6 for one / two / three column tiles); they land in rows l .. l + k - 1 of c
  int ldc;             // leading dimension of c: l, or l + k with the extra tile
  int fenced;          // 1: hand the level-2 rows and C over behind agent-scope release / acquire fences (the portable form: what
                       // the HIP memory model guarantees) instead of write-through stores + drained store counter + sc1 loads
                       // (what gfx942 / gfx950 make of relaxed agent-scope atomics: 3.4 us per launch less).  Knobs::fenced_reduce;
                       // tests/test_ortho_chain_gpu.py runs both and requires identical bits, tests/test_abi.py checks the
                       // sc1 bits in the code object.
};

// Second stage of every reduction: sum the block partials in a fixed order and scatter into column-major C.
// One launch, two levels: block (tile, grp) sums its share of the partials into lvl2[tile][grp]; the block that draws the last
// ticket of the tile adds the `groups` level-2 rows in index order (so the result does not depend on arrival order) and
// writes C to the device buffer and to its pinned host mirror.  The level-2 rows are handed over WITHOUT cache
// maintenance: write-through (sc1) stores, drained, then one agent-scope ticket per block; the last arriver reads them
// with sc1 loads (MI355X_MICROARCH.md, "Valid forms": one signalling lane per storing workgroup, one workgroup per CU --
// this grid has at most a few dozen blocks).  An agent-scope release + acquire pair in their place costs 3.4 us per launch.
// TAIL: the block that completes the last output tile also runs the state machine's step
template <bool TAIL>
__global__ __launch_bounds__(256) void gram_reduce_kernel(GramReduceArgs a)
{
  // (the predicate of a device-driven chain is looked at AFTER the first level's loads and sums: the word and the partials are
  //  independent latencies, and nothing before the test has a side effect)
  const int turn = (a.phase != nullptr) ? *a.phase : a.want;
  const unsigned long long t_entry = (TAIL && a.tail.dbg != nullptr) ? wall_clock64() : 0ULL;
  const int nsl = a.tlw * a.kt;              // output tiles of one pass
  const int slots = nsl + a.extra;           // partial slots per (pass, block)
  const int ps = blockIdx.x, grp = blockIdx.y, G = gridDim.y;
  const bool is_extra = ps >= a.n_ps - a.extra;
  const int pass = is_extra ? 0 : ps / nsl, slot = is_extra ? nsl + (ps - (a.n_ps - a.extra)) : ps % nsl;
  const int e = threadIdx.x;
  const double* p = a.partial + ((size_t)pass * a.nblk) * (size_t)slots * 256 + (size_t)slot * 256 + e;
  const int per = (a.nblk + G - 1) / G;
  const int b0 = grp * per, b1 = min(a.nblk, b0 + per);
  // what the fused tail will need from the state machine: read now, hidden behind the reduction (this launch is the
  // only writer of the state until its own tail runs)
  TailState pre{};
  if constexpr (TAIL) {
    if (threadIdx.x < 64)
      pre = TailState{a.tail.st->it_macro, a.tail.st->it_outer, a.tail.st->macro_total, a.tail.st->shifts, a.tail.st->nops,
                      OP_NONE, OST_RUNNING, a.tail.st->growth, a.tail.st->have_xu, a.tail.st->sloppy, a.tail.st->gdev};
  }
  // loads are issued in batches of 32 / 8 (independent), the adds stay in index order
  double s = 0.0;
  int b = b0;
  for (; b + 32 <= b1; b += 32) {
    double v[32];
#pragma unroll
    for (int q = 0; q < 32; ++q) v[q] = p[(size_t)(b + q) * slots * 256];
#pragma unroll
    for (int q = 0; q < 32; ++q) s += v[q];
  }
  for (; b + 8 <= b1; b += 8) {
    double v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = p[(size_t)(b + q) * slots * 256];
#pragma unroll
    for (int q = 0; q < 8; ++q) s += v[q];
  }
  for (; b < b1; ++b) s += p[(size_t)b * slots * 256];
  if (turn != a.want) {
    // not this launch's turn.  The last launch of a plan still tells the host where the machine stands (unless the chain has ended:
    // a terminal step reported it and re-armed the machine, nops == 0) -- so that a plan need not end with a launch whose only
    // purpose is to report
    if constexpr (TAIL) {
      if (a.do_tail && a.tail.publish && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && a.tail.st->nops > 0) *a.tail.st_host = *a.tail.st;
    }
    return;
  }
  __shared__ int s_last;
  double tot = s;
  if (G > 1) {
    __hip_atomic_store(&a.lvl2[((size_t)ps * G + grp) * 256 + e], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      if (a.fenced) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      const unsigned t = __hip_atomic_fetch_add(&a.ticket[ps], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = (t == (unsigned)(G - 1));
      if (last) __hip_atomic_store(&a.ticket[ps], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (last && a.fenced) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    tot = 0.0;
    double v[32];
#pragma unroll
    for (int q = 0; q < 32; ++q)
      v[q] = (q < G) ? __hip_atomic_load(&a.lvl2[((size_t)ps * G + q) * 256 + e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
#pragma unroll
    for (int q = 0; q < 32; ++q) tot += v[q];   // G <= 32; padding zeros do not change the sum
  }
  const int xg = pass % a.passes_x, ug = pass / a.passes_x;
  const int t = slot / a.kt, q = slot % a.kt;
  const int reg = e >> 6, lane = e & 63;
  // extra tile e = ps - (n_ps - extra): the tile (qi >= qj) of the Gram matrix of the U block, e = qi (qi + 1) / 2 + qj
  int eqi = 0, eqj = 0;
  if (is_extra) {
    const int ei = ps - (a.n_ps - a.extra);
    while ((eqi + 1) * (eqi + 2) / 2 <= ei) ++eqi;
    eqj = ei - eqi * (eqi + 1) / 2;
  }
  const int xcol = is_extra ? a.l + 16 * eqi + (lane >> 4) + 4 * reg : (xg * a.tlw + t) * 16 + (lane >> 4) + 4 * reg;
  const int ucol = is_extra ? 16 * eqj + (lane & 15) : (ug * a.kt + q) * 16 + (lane & 15);
  const bool live = (is_extra ? xcol < a.l + a.k : xcol < a.l) && ucol < a.k;
  const bool exchange = TAIL && a.p2p.nranks > 1;
  // the chain's tail reads C in this same launch: for ortho_tail16 (sc1 loads) write-through stores, drained, and a ticket
  // are the whole hand-over; the LDS-loop tail and the peer-to-peer exchange read with plain loads behind an acquire
  const bool wt = TAIL && a.tail.fold && !exchange && !a.fenced;
  if (live) {
    double* dst = a.c + (size_t)xcol + (size_t)ucol * a.ldc;
    if (wt) __hip_atomic_store(dst, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *dst = tot;
    if (a.c_host) a.c_host[(size_t)xcol + (size_t)ucol * a.ldc] = tot;
  }
  if constexpr (!TAIL) return;
  __shared__ __attribute__((aligned(16))) double tail_lds[TAIL ? (TAIL_LDS_DOUBLES > T16_LDS_DOUBLES + T16_ZS_ROWS * 16 ? TAIL_LDS_DOUBLES : T16_LDS_DOUBLES + T16_ZS_ROWS * 16) : 1];
  if (!exchange && a.n_ps == 1 && a.tail.after != OP_XU) {
    // a single 16 x 16 tile, complete in this block's registers: it reaches the tail through LDS, no hand-over
    if (a.tail.fold) {
      tail_lds[e] = tot;                     // wave w holds register w of the C-layout
      __syncthreads();
      ortho_tail16(a.tail, tail_lds, &pre, true, t_entry);
      return;
    }
    const int gi = (lane >> 4) + 4 * reg, gj = lane & 15;
    tail_lds[gi * TLD + gj] = tot;
    tail_lds[48 * TLD + gi * TLD + gj] = tot;
    __syncthreads();
    if (threadIdx.x < 64) ortho_tail(a.tail, tail_lds, threadIdx.x, &pre, true);
    return;
  }
  // hand the finished tile(s) over to the block that runs the tail
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    if (!wt) { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
    int last = 1;
    if (a.n_ps > 1) {
      const unsigned t2 = __hip_atomic_fetch_add(a.gticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last = (t2 == (unsigned)(a.n_ps - 1));
      if (last) __hip_atomic_store(a.gticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (last && !wt) { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
    s_last = last;
  }
  __syncthreads();
  if (!s_last) return;
  if (exchange) {
    // the whole reduced matrix is in a.c now (acquired above); sum it over the ranks in place, then run the step on it
    if (!p2p_exchange(a.p2p)) return;      // a peer timed out: the status word tells the host
    __threadfence();
    __syncthreads();
  }
  if (a.tail.fold) { ortho_tail16(a.tail, tail_lds, &pre, false, t_entry); return; }
  if (threadIdx.x >= 64) return;
  ortho_tail(a.tail, tail_lds, threadIdx.x, &pre);
}

// ======================================================================================
// host side of the engine
// ======================================================================================
struct TimedLaunch { hipEvent_t a, b; int cls; std::string kname; };
// every launch of the engine goes through here: a dry run (HipEngine::LaunchCtx::dry) walks the launch paths -- shape decisions,
// workspace growth, requests for more than 64 KiB of LDS -- without launching anything
#define DLA_LAUNCH(...) do { if (!lc.dry) hipLaunchKernelGGL(__VA_ARGS__); } while (0)
// A dispatch ladder over an instance list of hip_plans.h: f(std::integral_constant<size_t, I>) for I = 0 .. N - 1 until one call
// returns true (false: no row took the plan).  Inside f, `constexpr auto s = LIST[decltype(i)::value]` has the row's fields as
// compile-time values, so every listed row is instantiated and nothing else is.
template <typename F, size_t... I>
bool first_instance(std::index_sequence<I...>, F&& f) { return (f(std::integral_constant<size_t, I>{}) || ...); }
template <size_t N, typename F>
bool first_instance(F&& f) { return first_instance(std::make_index_sequence<N>{}, f); }
struct HipEngine : dla::Engine {
  int device = 0;
  int ncu = 256;
  hipStream_t st = nullptr;
  std::string nm;
  // workspaces (hip_owned.h: each owner releases itself, reserve() is the one regrow primitive)
  DeviceBuffer<double> d_partial;
  DeviceBuffer<double> d_small;         // reduced results (device)
  MappedHostBuffer<double> h_small;     // pinned, device-mapped host mirror
  DeviceBuffer<double> d_lvl2;          // second-level partials of the Gram reduction
  DeviceBuffer<unsigned> d_ticket;
  static const int RING = 8;
  MappedHostBuffer<double> h_ring[RING]; Event ring_ev[RING]; int ring_pos = 0;
  DeviceBuffer<double> d_cpk;
    // built-in operator
  DeviceBuffer<double> d_w, d_diag, d_t, d_wsq;
  long long syn_row0 = 0; int syn_n = 0, syn_rw = 0; double syn_sigma = 0.0;
  // rccl
  ncclComm_t comm = nullptr;
  void set_tune(int i, int v) override { knobs.set(i, v); }
  int get_tune(int i) override { return knobs.get(i); }
  void begin_solve() override { x3_cooldown = X3_COOLDOWN_START; drop_measured(); }
  // per-kernel statistics (names as rocprofv3 prints them, without namespace / argument list)
  struct KStat { long long launches = 0; double alg_bytes = 0.0, ms = 0.0, flops = 0.0; };
  std::map<std::string, KStat> kstats;
  int kernel_stats(dla_kernel_stat* out, int cap) override
  {
    collect_times();
    int i = 0;
    for (auto& kv : kstats) {
      if (i >= cap) break;
      std::memset(&out[i], 0, sizeof(out[i]));
      std::strncpy(out[i].name, kv.first.c_str(), sizeof(out[i].name) - 1);
      out[i].launches = kv.second.launches; out[i].alg_bytes = kv.second.alg_bytes; out[i].ms = kv.second.ms;
      out[i].flops = kv.second.flops;
      ++i;
    }
    return i;
  }
  void reset_kernel_stats() override { kstats.clear(); }
  // timing / tracing ($DIAGLIB_AMD_TRACE=1: print and synchronise around every launch)
  bool trace = false;
  // where the HOST waits ($DIAGLIB_AMD_HOSTTIME=1 prints the totals at destruction)
  double t_sync = 0.0, t_evsync = 0.0, t_alloc = 0.0, t_free = 0.0;
  long n_sync = 0;
  static double now() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }
  std::vector<TimedLaunch> timed;
  std::vector<hipEvent_t> ev_pool;
  struct SpecRec { int tag, cls; std::string kname; double bytes, flops; };
  std::vector<SpecRec> ahead_log;

  const char* name() const override { return nm.c_str(); }
  void* stream() override { return (void*)st; }

  Knobs knobs;                       // the experiment knobs (hip_plans.h)
  PlanEnv env() const { return PlanEnv{ncu, lds_limit, knobs}; }     // what the planners read of this engine

  // What the launches of the current step are enqueued under.  Nothing a launch depends on is a bare engine member: a caller
  // installs a modified copy with CtxScope, which puts back what was there before on every way out.  Outside any scope the
  // context is this default: unpredicated, not dry, nothing fused.
  struct LaunchCtx {
    const int* phase = nullptr;      // predicate of the launches (device-driven chains): run only if *phase == want; nullptr = always
    int want = 0;
    std::vector<SpecRec>* rec = nullptr;   // speculative launches are booked here under `tag` instead of the statistics (Scope)
    int tag = 0;
    bool dry = false;                // see DLA_LAUNCH
    bool fuse_tail = false;          // the reduction of this step may run `tail` in its last block (launch_reduce)
    OrthoTailArgs tail{};
    bool xw = false;                 // the chain may use the storing sweep OP_XW for its wide block (ortho_tail)
    bool x3 = false;                 // the chain runs the three-pass schedule (OP_COMBOX / OP_CLOSE, ortho_tail16)
    size_t small_off = 0;            // element offset of a Gram's result inside d_small / h_small ...
    bool in_chunk = false;           // ... which is a column chunk of a larger result: one rank only (gram_chunk)
  } lc;
  struct CtxScope {
    HipEngine* e; LaunchCtx saved;
    CtxScope(HipEngine* e_, const LaunchCtx& c) : e(e_), saved(e_->lc) { e->lc = c; }
    ~CtxScope() { e->lc = saved; }
    CtxScope(const CtxScope&) = delete;
    CtxScope& operator=(const CtxScope&) = delete;
  };
  // What an enqueued step reports back; it lives in the frame of whoever asked for the step.
  struct StepOut {
    bool tail_fused = false;         // the reduction ran the chain's tail in its last block
    double* summed_at = nullptr;     // the cross-rank sum went out of place, to this buffer (RCCL inside a chain); nullptr: in place
    bool mirror_fresh = false;       // the cross-rank sum already wrote the pinned mirror h_small (peer-to-peer exchange)
    bool lower_only = false;         // a Gram formed only the lower block triangle of its result
  };

  ~HipEngine() override
  {
    if (std::getenv("DIAGLIB_AMD_HOSTTIME"))
      std::fprintf(stderr, "[dla] host waits: stream sync %.3f s (%ld), ring event sync %.3f s, alloc %.3f s, free %.3f s\n",
                   t_sync, n_sync, t_evsync, t_alloc, t_free);
    // Everything queued is waited for here, so nothing below can pull memory from under a running kernel; the buffers and
    // events are members that release themselves after this body, and once the streams are idle their order does not matter.
    if (st) (void)hipStreamSynchronize(st);
    if (st_down) (void)hipStreamSynchronize(st_down);
    if (st_up) (void)hipStreamSynchronize(st_up);
    p2p_release();
    if (comm) ncclCommDestroy(comm);
    for (auto& b : cache) (void)hipFree(b.ptr);
    for (auto& b : live) (void)hipFree(b.ptr);
    for (auto& t : timed) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
    for (auto e : ev_pool) (void)hipEventDestroy(e);
    if (st_down) (void)hipStreamDestroy(st_down);
    if (st_up) (void)hipStreamDestroy(st_up);
    if (st) (void)hipStreamDestroy(st);
  }

  int init(int dev)
  {
    int cnt = 0;
    HIPCHK(hipGetDeviceCount(&cnt));
    if (cnt <= 0) { err = "no HIP device"; return DLA_ERR_NO_DEVICE; }
    if (dev >= cnt) {
      // a wrong LOCAL_RANK must not silently put two ranks on one GPU (RCCL would fail later with an obscure error);
      // sharing a device is an explicit rehearsal mode
      if (!std::getenv("DIAGLIB_AMD_SHARE_DEVICES")) {
        err = "device index " + std::to_string(dev) + " out of range (" + std::to_string(cnt) +
              " visible); set DIAGLIB_AMD_SHARE_DEVICES=1 to let ranks share devices (rehearsal only)";
        return DLA_ERR_NO_DEVICE;
      }
      dev = dev % cnt;
    }
    device = dev;
    trace = std::getenv("DIAGLIB_AMD_TRACE") != nullptr;
    force_lds_refusal = std::getenv("DIAGLIB_AMD_FORCE_LDS_REFUSAL") ? 1 : 0;
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t p;
    HIPCHK(hipGetDeviceProperties(&p, device));
    ncu = p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
    nm = std::string("hip:") + p.gcnArchName;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    HIPCHK(d_small.reserve(512 * 512));
    HIPCHK(h_small.reserve(512 * 512));
    HIPCHK(d_ticket.reserve(4100));                                         // [4096] per output tile + 1 global
    HIPCHK(hipMemsetAsync(d_ticket, 0, sizeof(unsigned) * 4100, st));       // (on the engine's stream: see RowShard::d_halo)
    return DLA_OK;
  }

  // ---- timing helpers
  // The engine's allocations, events and launches belong to `device`; a host application that switches the calling thread's
  // current device between calls (torch does) must not redirect them: every allocating or launching path starts here.
  void bind()
  {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != device) (void)hipSetDevice(device);
  }
  struct Scope {
    HipEngine* e; int cls; hipEvent_t a = nullptr, b = nullptr; std::string kname;
    Scope(HipEngine* e_, int cls_, double bytes, double flops, const std::string& kname_ = std::string()) : e(e_), cls(cls_), kname(kname_)
    {
      e->bind();
      if (e->lc.dry) return;
      e->drop_measured();              // (whatever is launched now may rewrite the block a fused Ritz sweep measured: see ritz_expand)
      if (e->lc.rec) {
        // speculative launch of a device-driven chain: counted after the read-back, if the device executed it
        e->lc.rec->push_back({e->lc.tag, cls_, kname_, bytes, flops});
        if (e->profile) { a = e->get_event(); b = e->get_event(); (void)hipEventRecord(a, e->st); }
        return;
      }
      if (!kname.empty()) { auto& ks = e->kstats[kname]; ks.launches += 1; ks.alg_bytes += bytes; ks.flops += flops; }
      if (e->ahead_log_on) e->ahead_log.push_back({0, cls_, kname_, bytes, flops});
      if (e->trace) {
        timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts);
        std::fprintf(stderr, "[dla] %ld.%06ld launch class %d, %.3e alg bytes\n", (long)ts.tv_sec, ts.tv_nsec / 1000, cls_, bytes);
        std::fflush(stderr);
      }
      e->stats.launches[cls] += 1;
      e->stats.alg_bytes[cls] += bytes;
      e->stats.flops[cls] += flops;
      if (e->profile) {
        a = e->get_event(); b = e->get_event();
        (void)hipEventRecord(a, e->st);
      }
    }
    ~Scope()
    {
      if (e->lc.dry) return;
      if (e->trace) {
        hipError_t er = hipStreamSynchronize(e->st);
        timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts);
        std::fprintf(stderr, "[dla] %ld.%06ld   done: %s\n", (long)ts.tv_sec, ts.tv_nsec / 1000, hipGetErrorString(er)); std::fflush(stderr);
      }
      if (e->profile) {
        (void)hipEventRecord(b, e->st);
        e->timed.push_back({a, b, cls, kname});
        if (e->timed.size() > 4096) e->collect_times();
      }
    }
  };
  // launches booked while dla_expand_project runs ahead of a chain's report (see dla_internal.h)
  bool ahead_log_on = false;
  size_t ahead_timed0 = 0, ahead_timed1 = 0;
  void spec_stats_begin() override { ahead_log.clear(); ahead_log_on = true; ahead_timed0 = ahead_timed1 = timed.size(); }
  // first call: stop logging; a call with discard = true (the same or a later one) takes the logged launches out again
  void spec_stats_end(bool discard) override
  {
    if (ahead_log_on) { ahead_log_on = false; ahead_timed1 = timed.size(); }
    if (!discard) return;
    for (auto& r : ahead_log) {
      stats.launches[r.cls] -= 1; stats.alg_bytes[r.cls] -= r.bytes; stats.flops[r.cls] -= r.flops;
      if (!r.kname.empty()) { auto& ks = kstats[r.kname]; ks.launches -= 1; ks.alg_bytes -= r.bytes; ks.flops -= r.flops; }
    }
    ahead_log.clear();
    // their event pairs (a collection in between has emptied the list: then there is nothing left to drop)
    if (ahead_timed0 < ahead_timed1 && ahead_timed1 <= timed.size()) {
      for (size_t i = ahead_timed0; i < ahead_timed1; ++i) { ev_pool.push_back(timed[i].a); ev_pool.push_back(timed[i].b); }
      timed.erase(timed.begin() + ahead_timed0, timed.begin() + ahead_timed1);
    }
    ahead_timed0 = ahead_timed1 = 0;
  }
  hipEvent_t get_event()
  {
    if (!ev_pool.empty()) { hipEvent_t e = ev_pool.back(); ev_pool.pop_back(); return e; }
    // timing events without the system-scope fence: a default event makes the kernel before it write its output back
    // and the kernel after it start from cold caches, which slows the bracketed kernels by 5-15 % (measured against
    // rocprofv3's dispatch times of an event-free run)
    hipEvent_t e;
    if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) { (void)hipGetLastError(); (void)hipEventCreate(&e); }
    return e;
  }
  void collect_times() override
  {
    account_chains();
    if (timed.empty()) return;
    (void)hipStreamSynchronize(st);
    for (auto& t : timed) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) {
        stats.ms[t.cls] += ms;
        if (!t.kname.empty()) kstats[t.kname].ms += ms;
      }
      ev_pool.push_back(t.a); ev_pool.push_back(t.b);
    }
    timed.clear();
    ahead_timed0 = ahead_timed1 = 0;       // (a run-ahead's event pairs went with the rest)
  }

  // ---- memory
  // Panels are GiB-sized and a driver call allocates/frees the same sizes every solve; hipMalloc/hipFree of
  // such blocks can take tens of milliseconds each (measured 39 ms per 4 GiB hipMalloc on some boxes, versus
  // ~3 ms of device work per iteration), so freed blocks are kept and handed out again (exact size class,
  // 2 MiB granules).  dla_destroy releases everything; the cache is capped at cache_limit bytes.
  struct Block { size_t bytes; void* ptr; };
  std::vector<Block> cache;
  std::vector<Block> live;
  size_t cached_bytes = 0, cache_limit = (size_t)96 << 30;
  int alloc(size_t bytes, void** dev) override
  {
    *dev = nullptr;
    bind();
    const size_t gran = (size_t)2 << 20;
    bytes = ((std::max(bytes, (size_t)8) + gran - 1) / gran) * gran;
    for (size_t i = 0; i < cache.size(); ++i)
      if (cache[i].bytes == bytes) {
        *dev = cache[i].ptr;
        cached_bytes -= bytes;
        cache.erase(cache.begin() + i);
        live.push_back({bytes, *dev});
        return DLA_OK;
      }
    const double t0 = now();
    hipError_t e = hipMalloc(dev, bytes);
    if (e != hipSuccess && !cache.empty()) {       // out of memory: drop the cache and retry once
      release_cache();
      e = hipMalloc(dev, bytes);
    }
    t_alloc += now() - t0;
    if (e != hipSuccess) { err = std::string("hipMalloc: ") + hipGetErrorString(e); return DLA_ERR_ALLOC; }
    live.push_back({bytes, *dev});
    return DLA_OK;
  }
  void release_cache()
  {
    (void)hipStreamSynchronize(st);
    for (auto& b : cache) (void)hipFree(b.ptr);
    cache.clear();
    cached_bytes = 0;
  }
  int free_(void* dev) override
  {
    if (!dev) return DLA_OK;
    const double t0 = now();
    (void)hipStreamSynchronize(st);      // nothing queued may still touch the block
    size_t bytes = 0;
    for (size_t i = 0; i < live.size(); ++i)
      if (live[i].ptr == dev) { bytes = live[i].bytes; live.erase(live.begin() + i); break; }
    if (bytes == 0) {                    // not ours (should not happen): plain free
      HIPCHK(hipFree(dev));
    } else if (cached_bytes + bytes > cache_limit) {
      HIPCHK(hipFree(dev));
    } else {
      cache.push_back({bytes, dev});
      cached_bytes += bytes;
    }
    t_free += now() - t0;
    return DLA_OK;
  }
  // hand the cached (freed) blocks back to the runtime; live blocks are untouched
  int trim(size_t* released) override
  {
    (void)hipStreamSynchronize(st);
    size_t rel = 0;
    for (auto& b : cache) { HIPCHK(hipFree(b.ptr)); rel += b.bytes; }
    cache.clear();
    cached_bytes = 0;
    if (released) *released = rel;
    return DLA_OK;
  }
  int zero(void* dev, size_t bytes) override
  {
    Scope s(this, DLA_OP_ELEM, (double)bytes, 0.0);
    HIPCHK(hipMemsetAsync(dev, 0, bytes, st));
    return DLA_OK;
  }
  int h2d(void* dev, const void* host, size_t bytes) override
  {
    drop_measured();
    HIPCHK(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return DLA_OK;
  }
  int d2h(void* host, const void* dev, size_t bytes) override
  {
    HIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    stats.host_syncs++;
    return DLA_OK;
  }
  int d2d(void* dst, const void* src, size_t bytes) override
  {
    Scope s(this, DLA_OP_ELEM, 2.0 * (double)bytes, 0.0);
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
    return DLA_OK;
  }
  int sync() override { HIPCHK(hipStreamSynchronize(st)); return DLA_OK; }
  // device-mode callbacks (dla_internal.h): order the user's stream(s) against ours
  Event ev_cb, ev_cb2;
  int callback_begin(int mode) override
  {
    if (mode != 2) drop_measured();    // (a caller's own routine may write anywhere)
    if (mode == 2) return DLA_OK;
    if (mode == 1) { int stw = wait_stream(); if (stw) return stw; stats.host_syncs++; return DLA_OK; }
    HIPCHK(ev_cb.ensure(hipEventDisableTiming));
    HIPCHK(ev_cb2.ensure(hipEventDisableTiming));
    HIPCHK(hipEventRecord(ev_cb, st));
    HIPCHK(hipStreamWaitEvent(nullptr, ev_cb, 0));     // legacy null stream: every blocking stream follows it
    return DLA_OK;
  }
  int callback_end(int mode) override
  {
    if (mode == 2) return DLA_OK;
    if (mode == 1) { HIPCHK(hipDeviceSynchronize()); return DLA_OK; }
    HIPCHK(hipEventRecord(ev_cb2, nullptr));
    HIPCHK(hipStreamWaitEvent(st, ev_cb2, 0));
    return DLA_OK;
  }
  // ---- staging pipeline of host-mode callbacks (dla_internal.h)
  hipStream_t st_down = nullptr, st_up = nullptr;
  bool stage_pending = false, stage_ready = false;
  Event ev_stage_ready, ev_stage_done, ev_down[16];
  int stage_init()
  {
    if (stage_ready) return DLA_OK;
    if (!st_down) HIPCHK(hipStreamCreateWithFlags(&st_down, hipStreamNonBlocking));
    if (!st_up) HIPCHK(hipStreamCreateWithFlags(&st_up, hipStreamNonBlocking));
    HIPCHK(ev_stage_ready.ensure(hipEventDisableTiming));
    HIPCHK(ev_stage_done.ensure(hipEventDisableTiming));
    for (int i = 0; i < 16; ++i) HIPCHK(ev_down[i].ensure(hipEventDisableTiming));
    stage_ready = true;
    return DLA_OK;
  }
  int stage_begin() override
  {
    int stc = stage_init();
    if (stc) return stc;
    // the previous callback's uploads read the pinned buffers this one is about to overwrite
    if (stage_pending) { HIPCHK(hipEventSynchronize(ev_stage_done)); stage_pending = false; }
    HIPCHK(hipEventRecord(ev_stage_ready, st));
    HIPCHK(hipStreamWaitEvent(st_down, ev_stage_ready, 0));
    HIPCHK(hipStreamWaitEvent(st_up, ev_stage_ready, 0));      // the output block may still be read by queued kernels
    return DLA_OK;
  }
  int stage_d2h(void* host, const void* dev, size_t bytes, int slot) override
  {
    HIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st_down));
    HIPCHK(hipEventRecord(ev_down[slot & 15], st_down));
    return DLA_OK;
  }
  int stage_wait(int slot) override
  {
    const double t0 = now();
    HIPCHK(hipEventSynchronize(ev_down[slot & 15]));
    t_sync += now() - t0; n_sync++;
    stats.host_syncs++;
    return DLA_OK;
  }
  int stage_h2d(void* dev, const void* host, size_t bytes) override
  {
    HIPCHK(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, st_up));
    return DLA_OK;
  }
  int stage_end() override
  {
    HIPCHK(hipEventRecord(ev_stage_done, st_up));
    HIPCHK(hipStreamWaitEvent(st, ev_stage_done, 0));
    stage_pending = true;
    return DLA_OK;
  }
  int host_alloc(size_t bytes, void** p) override { bind(); HIPCHK(hipHostMalloc(p, bytes, hipHostMallocDefault)); return DLA_OK; }
  int host_free(void* p) override { if (p) HIPCHK(hipHostFree(p)); return DLA_OK; }

  // the workspaces hold doubles; their callers think in bytes
  static size_t doubles(size_t bytes) { return (bytes + sizeof(double) - 1) / sizeof(double); }
  int ensure_partial(size_t bytes)
  {
    if (doubles(bytes) <= d_partial.capacity()) return DLA_OK;
    bind();
    if (d_partial) HIPCHK(hipStreamSynchronize(st));
    HIPCHK(d_partial.reserve(doubles(bytes)));
    return DLA_OK;
  }
  int ensure_small(size_t bytes)
  {
    if (doubles(bytes) <= std::min(d_small.capacity(), h_small.capacity())) return DLA_OK;
    bind();
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(d_small.reserve(doubles(bytes)));
    HIPCHK(h_small.reserve(doubles(bytes)));
    return DLA_OK;
  }
  // the 16-byte path of a sweep over n rows: every rank's row count is even and every panel starts on 16 bytes (null pointers are
  // aligned).  (gram_dev_once goes by peers_even alone, on purpose: gram_plan tests n itself.)
  template <typename... P> bool on_16_bytes(long long n, const P*... p) const { return even_rows(n) && (((uintptr_t)p | ...) % 16 == 0); }
  // first allocation of a buffer that starts zeroed (on the engine's stream): both or nothing, so that a later call retries
  template <class T> int reserve_zeroed(DeviceBuffer<T>& b, size_t count)
  {
    if (b) return DLA_OK;
    HIPCHK(b.reserve(count));
    const hipError_t e = hipMemsetAsync(b, 0, sizeof(T) * count, st);
    if (e != hipSuccess) b.reset();
    HIPCHK(e);
    return DLA_OK;
  }
  int ensure_lvl2(size_t bytes)
  {
    if (doubles(bytes) <= d_lvl2.capacity()) return DLA_OK;
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(d_lvl2.reserve(doubles(std::max(bytes, (size_t)1 << 20))));
    return DLA_OK;
  }
  // Host wait for the stream: poll an event instead of blocking in the driver.  A blocking
  // hipStreamSynchronize sleeps on an interrupt and pays a scheduler wake-up per call (tens of
  // microseconds on an idle host, milliseconds on a busy one); a solve makes ~90 such waits.
  Event ev_wait;
  int wait_stream()
  {
    const double t0 = now();
    hipError_t q;
    if (knobs.poll_stream()) {               // A/B: poll the stream itself, no event packet
      while ((q = hipStreamQuery(st)) == hipErrorNotReady) {
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
      }
      t_sync += now() - t0; n_sync++;
      if (q != hipSuccess) { err = std::string("hipStreamQuery: ") + hipGetErrorString(q); return DLA_ERR_RUNTIME; }
      return DLA_OK;
    }
    HIPCHK(ev_wait.ensure(hipEventDisableTiming));
    HIPCHK(hipEventRecord(ev_wait, st));
    while ((q = hipEventQuery(ev_wait)) == hipErrorNotReady) {
#if defined(__x86_64__)
      __builtin_ia32_pause();
#endif
    }
    t_sync += now() - t0; n_sync++;
    if (q != hipSuccess) { err = std::string("hipEventQuery: ") + hipGetErrorString(q); return DLA_ERR_RUNTIME; }
    return p2p_check();
  }

  // reduced small result -> host: single rank reads the pinned mirror the kernel wrote,
  // multi-rank copies the all-reduced device buffer, unless the cross-rank sum already wrote the mirror (StepOut::mirror_fresh)
  int small_to_host(size_t count, bool mirror_fresh)
  {
    DLA_T("  wait for a small result");
    if (!local_only && (nranks > 1 || comm || p2p.on) && !mirror_fresh)
      HIPCHK(hipMemcpyAsync(h_small, d_small, sizeof(double) * count, hipMemcpyDeviceToHost, st));
    int stw = wait_stream();
    if (stw) return stw;
    stats.host_syncs++;
    return DLA_OK;
  }
  // ... and on into the caller's matrix: the l x k result stands densely in h_small (leading dimension l).  lower_only: a symmetric
  // matrix of which only the lower triangle of 16 x 16 blocks was formed; the rest is mirrored from it
  int small_result_home(int l, int k, bool mirror_fresh, double* c_host, int ldc, bool lower_only = false)
  {
    const int stc = small_to_host((size_t)l * k, mirror_fresh);
    if (stc) return stc;
    for (int j = 0; j < k; ++j) {
      double* cj = c_host + (size_t)j * ldc;
      if (!lower_only) { std::memcpy(cj, h_small + (size_t)j * l, sizeof(double) * l); continue; }
      for (int i2 = 0; i2 < l; ++i2) cj[i2] = (i2 / 16) >= (j / 16) ? h_small[(size_t)i2 + (size_t)j * l] : h_small[(size_t)j + (size_t)i2 * l];
    }
    return DLA_OK;
  }

  // Stage a small host matrix to the device through a ring of pinned, device-mapped buffers (no host sync): the caller packs
  // straight into the slot (stage_slot), stage_commit enqueues the copy.
  // (The runtime's copy shows up as __amd_rocclr_copyBuffer, 16 us of stream time per 30 KB in a solve's trace, and in isolation
  // a copy kernel of the engine's own is faster -- tools/upload_probe.hip: 26 us host-to-consumer against 20 us -- but inside a
  // solve it buys nothing: interleaved A/B, Knobs::own_copy_kernel, 16.88 / 16.90 ms against 16.90 / 16.88 at n = 2e6 and 3.90 / 3.90 against
  // 3.86 / 3.87 at 250 k rows.  The runtime's copy stays.)
  int stage_slot(size_t bytes, double** host, int* slot_out)
  {
    bind();
    size_t have = h_ring[0].capacity();        // of the smallest slot: one that failed to regrow is empty, the others are not
    for (int i = 1; i < RING; ++i) have = std::min(have, h_ring[i].capacity());
    if (doubles(bytes) > have) {
      HIPCHK(hipStreamSynchronize(st));
      for (int i = 0; i < RING; ++i) {
        HIPCHK(ring_ev[i].ensure(hipEventDisableTiming));
        HIPCHK(h_ring[i].reserve(doubles(std::max(bytes, (size_t)1 << 16))));
      }
    }
    const int slot = ring_pos;
    ring_pos = (ring_pos + 1) % RING;
    const double t0 = now();
    HIPCHK(hipEventSynchronize(ring_ev[slot]));
    t_evsync += now() - t0;
    *host = h_ring[slot];
    *slot_out = slot;
    return DLA_OK;
  }
  int stage_commit(int slot, size_t bytes, double* dev)
  {
    if (!knobs.own_copy_kernel()) {
      HIPCHK(hipMemcpyAsync(dev, h_ring[slot], bytes, hipMemcpyHostToDevice, st));
    } else {                                 // A/B: a copy kernel of the engine's own reading the mapped slot
      const int cnt = (int)(bytes / sizeof(double));
      hipLaunchKernelGGL(small_copy_kernel, dim3((cnt / 2 + 255) / 256 > 0 ? (cnt / 2 + 255) / 256 : 1), dim3(256), 0, st, dev,
                         (const double*)h_ring[slot].dev(), cnt);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(ring_ev[slot], st));
    return DLA_OK;
  }
  int stage_to_device(const double* host_packed, size_t bytes, double* dev)
  {
    double* h = nullptr;
    int slot = 0;
    const int stc = stage_slot(bytes, &h, &slot);
    if (stc) return stc;
    std::memcpy(h, host_packed, bytes);
    return stage_commit(slot, bytes, dev);
  }

  // ---- collectives on small device buffers
  // exchanged: the reduction kernel that produced `dev` carried the cross-rank sum already (launch_reduce)
  int allreduce_dev(double* dev, int count, int op /*0 sum, 1 max*/, double* host_mirror, StepOut& out, bool exchanged = false)
  {
    out.summed_at = nullptr; out.mirror_fresh = false;
    if (local_only || (nranks <= 1 && !comm && !p2p.on)) return DLA_OK;
    if (lc.dry) return DLA_OK;
    stats.allreduces++;
    if (p2p.on && count <= P2P_MAX_DOUBLES) {
      if (exchanged) return DLA_OK;
      P2PArgs pa = p2p_args(dev, count, op);
      // outside the device-driven chains the host reads the result next: the exchange writes the pinned mirror itself
      if (!lc.phase && dev == d_small && host_mirror == h_small) { pa.buf_host = h_small.dev(); out.mirror_fresh = true; }
      Scope s(this, DLA_OP_ELEM, 0.0, 0.0, "p2p_allreduce_kernel");
      DLA_LAUNCH(p2p_allreduce_kernel, dim3(1), dim3(256), 0, st, pa);
      HIPCHK(hipGetLastError());
      return DLA_OK;
    }
    if (comm) {
      // inside a chain: out of place (see d_red_small), the tail reads the destination
      double* dst = dev;
      if (lc.phase && d_red_small && count <= RED_DOUBLES && (dev == d_small || dev == d_xug)) dst = (dev == d_xug) ? d_red_xug : d_red_small;
      if (dst != dev) out.summed_at = dst;
      ncclResult_t r = ncclAllReduce(dev, dst, (size_t)count, ncclDouble, op == 0 ? ncclSum : ncclMax, comm, st);
      if (r != ncclSuccess) { err = std::string("ncclAllReduce: ") + ncclGetErrorString(r); return DLA_ERR_COMM; }
      return DLA_OK;
    }
    if (hook) {
      HIPCHK(hipMemcpyAsync(host_mirror, dev, sizeof(double) * count, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      hook(hook_user, host_mirror, count, op);
      HIPCHK(hipMemcpyAsync(dev, host_mirror, sizeof(double) * count, hipMemcpyHostToDevice, st));
      HIPCHK(hipStreamSynchronize(st));
      return DLA_OK;
    }
    err = "nranks > 1 but neither an RCCL communicator nor a reduction hook is attached";
    return DLA_ERR_COMM;
  }
  // the cross-rank sum of d_small and its copy to the host
  int sum_to_host(int count, int op)
  {
    StepOut out;
    const int stc = allreduce_dev(d_small, count, op, h_small, out);
    return stc ? stc : small_to_host((size_t)count, out.mirror_fresh);
  }
  P2PArgs p2p_args(double* dev, int count, int op)
  {
    P2PArgs pa{};
    pa.buf = dev; pa.buf_host = nullptr; pa.count = count; pa.op = op; pa.nranks = nranks; pa.rank = rank;
    pa.executed = p2p.d_executed;
    for (int r = 0; r < nranks; ++r) { pa.data[r] = p2p.data[r]; pa.flags[r] = p2p.flags[r]; }
    pa.status = p2p.h_status.dev(); pa.phase = lc.phase; pa.want = lc.want;
    pa.timeout_ticks = (unsigned long long)std::max(0, p2p_timeout_ms) * 100000ULL;
    return pa;
  }
  static const int X3_COOLDOWN_START = 2;
  int x3_cooldown = X3_COOLDOWN_START;   // > 0: a recent chain needed a level shift (or the solve is new: no evidence yet) -- that many
                                     // chains run the five-sweep schedule.  Reset at every driver call (begin_solve): the schedule of
                                     // a solve depends on that solve alone, repeated solves give identical bits
  // ---- one-shot peer-to-peer all-reduce (p2p_allreduce_kernel)
  struct P2P {
    bool on = false;
    DeviceBuffer<double> my_data; DeviceBuffer<unsigned long long> my_flags;     // fine-grained
    double* data[P2P_MAX_RANKS] = {nullptr}; unsigned long long* flags[P2P_MAX_RANKS] = {nullptr};
    MappedHostBuffer<int> h_status;      // pinned, device-mapped: a timed-out kernel sets it, the host reads it at its waits
    DeviceBuffer<unsigned long long> d_executed;   // see P2PArgs::executed
    int slots = 0;                       // ranks the local mailbox was sized for
  } p2p;
  static size_t p2p_data_bytes(int nr) { return sizeof(double) * 2 * (size_t)nr * P2P_MAX_DOUBLES; }
  static size_t p2p_flag_bytes(int nr) { return sizeof(unsigned long long) * (2 * (size_t)nr + 1) * P2P_FLAG_STRIDE; }   // flags + error word
  int p2p_timeout_ms = 5000;           // DLA_OPT_P2P_TIMEOUT_MS

  // allocate this rank's mailbox (fine-grained: peers write into it while kernels of this rank poll it) and export it
  int p2p_export(int nr, void* handles /* 2 x hipIpcMemHandle_t */) override
  {
    if (nr < 1 || nr > P2P_MAX_RANKS) { err = "p2p: 1..8 ranks"; return DLA_ERR_ARG; }
    HIPCHK(hipSetDevice(device));
    p2p_release();
    // (everything below is a first allocation: p2p_release left the mailbox empty)
    HIPCHK(p2p.my_data.reserve(p2p_data_bytes(nr) / sizeof(double), hipDeviceMallocFinegrained));
    HIPCHK(p2p.my_flags.reserve(p2p_flag_bytes(nr) / sizeof(unsigned long long), hipDeviceMallocFinegrained));
    HIPCHK(hipMemset(p2p.my_data, 0, p2p_data_bytes(nr)));
    HIPCHK(hipMemset(p2p.my_flags, 0, p2p_flag_bytes(nr)));
    HIPCHK(p2p.h_status.reserve(1));
    *p2p.h_status = 0;
    HIPCHK(p2p.d_executed.reserve(1));
    HIPCHK(hipMemset(p2p.d_executed, 0, sizeof(unsigned long long)));
    HIPCHK(hipDeviceSynchronize());
    p2p.slots = nr;
    hipIpcMemHandle_t* h = (hipIpcMemHandle_t*)handles;
    HIPCHK(hipIpcGetMemHandle(&h[0], p2p.my_data));
    HIPCHK(hipIpcGetMemHandle(&h[1], p2p.my_flags));
    return DLA_OK;
  }
  // open every peer's mailbox; handles = nr entries of (data handle, flag handle) in rank order
  int p2p_attach(int nr, int rk, const void* handles) override
  {
    if (nr != p2p.slots || rk < 0 || rk >= nr) { err = "p2p_attach: export first, with the same rank count"; return DLA_ERR_ARG; }
    // a second attach on the same export would start the sequence numbers at 1 again while the mailboxes still hold larger
    // ones (every wait would pass at once, stale slots would be summed): a re-formed group exports again on every rank
    if (p2p.on) { err = "p2p_attach: already attached; detach and export again on every rank"; return DLA_ERR_ARG; }
    HIPCHK(hipSetDevice(device));
    const hipIpcMemHandle_t* h = (const hipIpcMemHandle_t*)handles;
    for (int r = 0; r < P2P_MAX_RANKS; ++r) { p2p.data[r] = nullptr; p2p.flags[r] = nullptr; }
    hipError_t e1 = hipSuccess;
    for (int r = 0; r < nr && e1 == hipSuccess; ++r) {
      if (r == rk) { p2p.data[r] = p2p.my_data; p2p.flags[r] = p2p.my_flags; continue; }
      e1 = hipIpcOpenMemHandle((void**)&p2p.data[r], h[2 * r], hipIpcMemLazyEnablePeerAccess);
      if (e1 == hipSuccess) e1 = hipIpcOpenMemHandle((void**)&p2p.flags[r], h[2 * r + 1], hipIpcMemLazyEnablePeerAccess);
    }
    if (e1 != hipSuccess) {
      // close what was opened so far: the mailbox set is all or nothing
      for (int r = 0; r < nr; ++r) {
        if (r == rk) continue;
        if (p2p.data[r]) (void)hipIpcCloseMemHandle(p2p.data[r]);
        if (p2p.flags[r]) (void)hipIpcCloseMemHandle(p2p.flags[r]);
        p2p.data[r] = nullptr; p2p.flags[r] = nullptr;
      }
      err = std::string("hipIpcOpenMemHandle: ") + hipGetErrorString(e1);
      return DLA_ERR_RUNTIME;
    }
    nranks = nr; rank = rk;
    HIPCHK(hipMemset(p2p.d_executed, 0, sizeof(unsigned long long)));
    HIPCHK(hipDeviceSynchronize());
    p2p.on = true;
    return DLA_OK;
  }
  void p2p_release()
  {
    if (p2p.on) {
      (void)hipStreamSynchronize(st);
      for (int r = 0; r < nranks && r < P2P_MAX_RANKS; ++r)
        if (r != rank) { if (p2p.data[r]) (void)hipIpcCloseMemHandle(p2p.data[r]); if (p2p.flags[r]) (void)hipIpcCloseMemHandle(p2p.flags[r]); }
    }
    p2p = P2P{};      // (after the peers' handles were closed: this releases the local mailbox)
  }
  int p2p_detach() override { p2p_release(); return DLA_OK; }
  int set_p2p_timeout(int ms) override { p2p_timeout_ms = ms; return DLA_OK; }
  int p2p_check()
  {
    if (p2p.on && *(volatile int*)p2p.h_status) {
      err = "p2p all-reduce: a peer did not arrive within " + std::to_string(p2p_timeout_ms) + " ms (DLA_OPT_P2P_TIMEOUT_MS); the transport is down on every rank";
      return DLA_ERR_COMM;
    }
    return DLA_OK;
  }

  int comm_finalize() override
  {
    p2p_release();
    if (comm) { (void)hipStreamSynchronize(st); ncclCommDestroy(comm); comm = nullptr; }
    nranks = 1; rank = 0;
    return DLA_OK;
  }
  int comm_init(int nr, int rk, const char id[128]) override
  {
    ncclUniqueId uid;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    std::memcpy(&uid, id, 128);
    HIPCHK(hipSetDevice(device));
    ncclResult_t r = ncclCommInitRank(&comm, nr, uid, rk);
    if (r != ncclSuccess) { err = std::string("ncclCommInitRank: ") + ncclGetErrorString(r); comm = nullptr; return DLA_ERR_COMM; }
    nranks = nr; rank = rk;
    return DLA_OK;
  }

  // more than 64 KiB of dynamic LDS has to be enabled per kernel function and device (gfx950 has 160 KiB per CU);
  // remembered per engine, i.e. per device
  std::vector<std::pair<const void*, size_t>> lds_raised;
  // More than 64 KiB of dynamic LDS has to be enabled per kernel function.  A refusal is NOT swallowed: the launch
  // is not made, lds_limit drops to 64 KiB (every shape decision below honours it: narrower Gram passes, chunked
  // contraction, unfused epilogues) and the operation is redone once under that limit.
  size_t lds_limit = (size_t)160 * 1024;
  bool lds_retry = false;
  int force_lds_refusal = 0;   // $DIAGLIB_AMD_FORCE_LDS_REFUSAL=1 (tests): treat the first > 64 KiB request as refused
  // static_lds: what the kernel declares itself (__shared__ arrays); the 64 KiB a launch gets without asking cover both
  bool raise_lds(const void* kfn, size_t lds, size_t static_lds = 0)
  {
    if (lds + static_lds <= (size_t)64 * 1024) return true;
    bool refused = false;
    if (force_lds_refusal > 0) { force_lds_refusal = 0; refused = true; }
    if (!refused)
      for (auto& e : lds_raised)
        if (e.first == kfn) {
          if (e.second >= lds) return true;
          if (hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess) { e.second = lds; return true; }
          refused = true;
          break;
        }
    // (kernels with static LDS of their own cannot take the full 160 KiB: ask for what the launch needs)
    if (!refused) {
      if (hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess) {
        lds_raised.push_back({kfn, lds});
        return true;
      }
    }
    (void)hipGetLastError();
    lds_limit = (size_t)64 * 1024;
    lds_retry = true;
    err = "hipFuncSetAttribute refused " + std::to_string(lds) + " bytes of dynamic LDS";
    return false;
  }
  // run op(); when it stopped at a refused LDS request, run it once more under the 64 KiB limit
  template <typename F> int with_lds_retry(F&& op)
  {
    lds_retry = false;
    int st = op();
    if (st != DLA_OK && lds_retry) { lds_retry = false; st = op(); }
    return st;
  }

  // ---- device-driven orthogonalisation chain (see ortho_tail_kernel)
  DeviceBuffer<OrthoDev> d_ost;             // state machine (device)
  MappedHostBuffer<OrthoDev> h_ost;         // pinned mirror the tail kernels write
  MappedHostBuffer<OrthoDev> h_ost_init;    // pinned (not mapped) source of the initial state
  DeviceBuffer<double> d_wpk, d_wfull, d_cpk2;
  DeviceBuffer<unsigned long long> d_dbg;   // $DIAGLIB_AMD_CHAIN_DEBUG: time stamps of the chain's steps (empty otherwise)
  DeviceBuffer<double> d_wst;               // pending factors of ortho_tail16 (3 x 256 doubles)
  DeviceBuffer<double> d_xug;               // X^T U | U^T U of the last OP_GRAMX / OP_XW sweep: (m + k) x k
  // RCCL inside a device-driven chain: the collective itself cannot be predicated (it is enqueued by the host), so a launch
  // whose turn it is not still all-reduces whatever its source buffer holds.  Out of place, into these buffers, that is harmless:
  // the source is never scaled, and the tail that would read the result is predicated off like its sweep.
  DeviceBuffer<double> d_red_small, d_red_xug;
  static const int RED_DOUBLES = 640 * 48;
  MappedHostBuffer<double> h_tpend;  // the factor a drop_final chain left pending (OrthoTailArgs::t_host)
  int t_seq = 0;                     // sequence number of the chain being enqueued
  int t_pending_k = 0;               // > 0: the last chain ended with a k x k factor pending and nobody has fetched it yet
  std::map<ChainShape, std::vector<int>> plan_of_shape;   // the sweeps the last chain of that shape executed
  std::map<ChainShape, std::vector<int>> plan_of_kind;    // ... the most recent chain of that kind() and width, whatever its m
  std::set<ChainShape> chain_verified;                    // shapes whose launch paths have been walked (see ortho_chain)

  bool chain_armed = false;          // the device state machine stands at its initial state
  const bool chain_debug = std::getenv("DIAGLIB_AMD_CHAIN_DEBUG") != nullptr;   // print every chain's plan and outcome

  bool chain_buffers_ready = false;
  int ensure_chain_buffers()
  {
    if (chain_buffers_ready) return DLA_OK;
    bind();
    HIPCHK(d_ost.reserve(1));
    HIPCHK(h_ost.reserve(1));
    HIPCHK(h_ost_init.reserve(1, false));
    HIPCHK(d_wpk.reserve(3 * 48 * 16));
    HIPCHK(d_wfull.reserve(48 * 48));
    HIPCHK(d_cpk2.reserve((size_t)80 * 1024 / sizeof(double)));
    HIPCHK(d_wst.reserve(768));
    if (chain_debug) { const int stz = reserve_zeroed(d_dbg, 48 * 16); if (stz) return stz; }
    HIPCHK(d_xug.reserve(XUG_DOUBLES));
    if (!h_tpend) {
      HIPCHK(h_tpend.reserve(PEND_HDR + 8));
      h_tpend[PEND_HDR] = 0.0; h_tpend[PEND_HDR + 1] = 0.0; h_tpend[PEND_HDR + 2] = 0.0;
    }
    HIPCHK(d_red_small.reserve(RED_DOUBLES));
    HIPCHK(d_red_xug.reserve(RED_DOUBLES));
    chain_buffers_ready = true;
    return DLA_OK;
  }

  // groups of the reduction's first level: one per 32 block partials, at most 32 (the second level adds them in one pass of 32 loads).
  int reduce_groups(int nblk) const
  {
    const int per = knobs.reduce_group_size();
    return std::max(1, std::min(32, (nblk + per - 1) / per));
  }
  struct Rode { bool tail = false, exchange = false; };   // what went along in a reduction kernel: the chain's tail, the cross-rank sum
  Rode launch_reduce(GramReduceArgs& ra, dim3 grid)
  {
    Rode rode;
    if (ra.ldc == 0) ra.ldc = ra.l;
    ra.fenced = knobs.fenced_reduce() ? 1 : 0;
    rode.tail = lc.fuse_tail && !(p2p.on && ra.ldc * ra.k > P2P_MAX_DOUBLES);   // beyond a mailbox slot: separate launches
    if (rode.tail) {
      ra.do_tail = 1; ra.tail = lc.tail;
      ra.p2p = P2PArgs{};
      if (p2p.on) { ra.p2p = p2p_args(ra.c, ra.ldc * ra.k, 0); rode.exchange = true; }
      DLA_LAUNCH(gram_reduce_kernel<true>, grid, dim3(256), 0, st, ra);
    } else {
      DLA_LAUNCH(gram_reduce_kernel<false>, grid, dim3(256), 0, st, ra);
    }
    return rode;
  }
  // Second stage of every Gram: the per-block partials in d_partial -> c (l x k, leading dimension ldc, 0 = l; `extra`: see
  // GramReduceArgs), then the cross-rank sum of c unless the kernel carried it or the result is a column chunk of one rank.
  // (partial: the block partials of a sweep that left them elsewhere -- the fused Ritz sweep, ritz_expand -- nullptr: d_partial)
  int reduce_and_sum(int cls, double* c, double* c_host, int nblk, int l, int k, int tlw, int kt, int px, int n_out, int extra, int ldc,
                     StepOut& out, const double* partial = nullptr)
  {
    Rode rode;
    {
      Scope s2(this, cls, 0.0, 0.0, "gram_reduce_kernel");
      const int groups = reduce_groups(nblk);
      { const int stl = ensure_lvl2(sizeof(double) * (size_t)n_out * groups * 256); if (stl) return stl; }
      if (n_out > 4096) { err = "gram: too many output tiles"; return DLA_ERR_ARG; }     // (d_ticket holds one word per output tile)
      GramReduceArgs ra{partial ? partial : (const double*)d_partial, d_lvl2, d_ticket, c, c_host, nblk, l, k, tlw, kt, px,
                        lc.phase, lc.want, 0, n_out, d_ticket + 4096, OrthoTailArgs{}, P2PArgs{}, extra, ldc};
      rode = launch_reduce(ra, dim3(n_out, groups));
    }
    HIPCHK(hipGetLastError());
    out.tail_fused = rode.tail;
    if (lc.in_chunk) return DLA_OK;
    return allreduce_dev(c, (ldc ? ldc : l) * k, 0, h_small, out, rode.exchange);
  }
  void launch_tail_kernel(const OrthoTailArgs& ta)
  {
    if (ta.fold) DLA_LAUNCH(ortho_tail16_kernel, dim3(1), dim3(256), 0, st, ta);
    else DLA_LAUNCH(ortho_tail_kernel, dim3(1), dim3(64), 0, st, ta);
  }

  // one speculative step: the sweep, its reduction (+ cross-rank sum) and the tail that takes the next decision.
  // On one rank the tail rides in the last block of the reduction kernel; with a communicator the all-reduce has to
  // come between the two, so the tail is a launch of its own.
  int launch_op(int op, int n, int m, int k, const double* x, const double* bx, double* u, bool publish, int fold)
  {
    OrthoTailArgs tail{d_ost, h_ost.dev(), d_small, d_wpk, d_wfull, d_cpk2, op, m, k, m > 0 ? 1 : 0, ortho_maxit, publish ? 1 : 0,
                       fold, knobs.lead_full() ? 0 : 1, d_xug, d_wst, d_dbg, lc.xw ? 1 : 0};
    if ((fold == 1 && op == OP_GRAMX) || op == OP_XW || op == OP_COMBOX) tail.gsrc = d_xug;
    tail.x3 = lc.x3 ? 1 : 0;
    // (A/B, Knobs::first_factor_source: 0 = the first factor from U^T U as the reference's; 2 = level shifts on the projected block's Gram matrix
    //  instead of the reference's order for a numerically rank-deficient block -- 14.2-14.36 against 14.37-14.46 ms on the benchmark,
    //  but such a block's weakest columns then depend on the schedule, and the reference's dense test matrix with unit guesses takes
    //  another history (tests/test_trace_text.py::dav_n1000_unit fails with it, also when only the drivers' chains use it): not shipped)
    tail.gp = knobs.first_factor_source();
    tail.dmat = (policy.basis_exact && fold && m > 0 && dmat_nontrivial && dmat_cols == m && m <= DMAT_LD) ? d_dmat : nullptr;
    tail.dmat_ld = DMAT_LD;
    tail.drop_final = (policy.drop_final && m > 0) ? 1 : 0;
    tail.t_host = (tail.drop_final && policy.publish_pending && m + k <= PEND_ROWS) ? h_tpend.dev() : nullptr;
    tail.t_seq = t_seq;
    tail.drop_tol = policy.drop_tol;
    tail.drop_stol = policy.drop_stol;
    StepOut out;
    int stc = DLA_OK;
    {
      LaunchCtx step = lc;
      step.fuse_tail = p2p.on ? !knobs.exchange_own_launch() : (nranks <= 1 && !comm);
      step.tail = tail;
      step.phase = &d_ost->phase;
      step.want = (op == OP_GRAMX) ? (int)OP_GRAM_UU : (lc.x3 && op == OP_COMBO) ? (int)OP_COMBOX : op;   // the first sweep answers the start phase
      CtxScope scope(this, step);
      int blocks = 0;
      switch (op) {
        case OP_GRAM_UU: stc = gram_dev_once(n, k, u, k, u, DLA_OP_GRAM, false, out); break;
        case OP_XU:      stc = gram_dev_once(n, m, bx, k, u, DLA_OP_GRAM, false, out); break;
        case OP_GRAMX:
          // one-tile blocks: the WP kernel family; wider blocks: the plain product with [X | U] as the left panel (U follows X)
          stc = fold == 1 ? gram_wp_once(n, m, bx, k, u, nullptr, nullptr, out) : gram_dev_once(n, m + k, x, k, u, DLA_OP_GRAM, false, out);
          break;
        case OP_XW:      stc = gram_wp_once(n, m, bx, k, u, d_wpk, u, out); break;
        case OP_GRAMW:   stc = gram_wp_once(n, 0, nullptr, k, u, d_wpk, nullptr, out); break;
        case OP_TRMMG:
        case OP_TRMMC:
          stc = gemm_chunk(n, 0, k, u, k, nullptr, 0, u, 2, DLA_OP_TRMM, &blocks, d_wpk);
          if (!stc) stc = fused_reduce(k, blocks, out);
          break;
        case OP_COMBO:
          stc = gemm_chunk(n, 0, m + k, x, k, nullptr, 0, u, 0, DLA_OP_GEMM, &blocks, d_cpk2);
          if (!stc) stc = fused_reduce(k, blocks, out);
          break;
        case OP_FINAL:   stc = gemm_chunk(n, 0, k, u, k, nullptr, 0, u, 2, DLA_OP_TRMM, nullptr, d_wpk); break;
        // three-pass schedule: the projection that measures what it stores, and the closing one that measures nothing
        case OP_COMBOX:  stc = gram_wp_once(n, m, bx, k, u, nullptr, u, out, d_cpk2); break;
        case OP_CLOSE:   stc = gemm_chunk(n, 0, m + k, x, k, nullptr, 0, u, 0, DLA_OP_GEMM, nullptr, d_cpk2); break;
        default: err = "ortho_chain: bad op"; stc = DLA_ERR_ARG;
      }
    }
    if (stc || out.tail_fused) return stc;
    if (comm && !p2p.on && d_red_small) {
      // RCCL: the reduced matrices live in the out-of-place destinations of the all-reduce
      if (out.summed_at) tail.gsrc = out.summed_at;
      tail.xug = d_red_xug;
    }
    Scope s(this, DLA_OP_GRAM, 0.0, 0.0, fold ? "ortho_tail16_kernel" : "ortho_tail_kernel");
    launch_tail_kernel(tail);
    HIPCHK(hipGetLastError());
    return DLA_OK;
  }

  // Sweeps of the pending-factor schedule (gram_lds_kernel WP; k <= 16, even n):
  //   m > 0:  X^T (U W) and (U W)^T (U W) in one pass over [X | U] -> d_xug ((m + k) x k, the Gram matrix in rows m..);
  //   m == 0: (U W)^T (U W) -> d_small (k x k).   wp == nullptr: W = identity.
  template <int TLW, int KT, int R>
  int launch_gram_wp(const GramArgs& a, dim3 grid, bool self)
  {
    if (a.cx != nullptr) {
      // the projection sweep (WP == 2): one U tile
      if constexpr (KT == 1) {
        auto kfn = gram_lds_kernel<TLW, 1, 1, R, 0, 0, 0, 2>;
        const size_t lds = gram_lds_bytes(TLW, 1, R, false, false);
        if (!raise_lds((const void*)kfn, lds)) return DLA_ERR_RUNTIME;
        DLA_LAUNCH(kfn, grid, dim3(256), lds, st, a);
        return DLA_OK;
      }
      err = "gram_wp: the projection sweep takes one-tile blocks"; return DLA_ERR_ARG;
    }
    if (self) {
      if constexpr (TLW == 1 && KT == 1) {
        auto kfn = gram_lds_kernel<1, 1, 1, 32, 1, 0, 0, 1>;
        const size_t lds = gram_lds_bytes(1, 1, 32, true, false);
        DLA_LAUNCH(kfn, grid, dim3(256), lds, st, a);
      }
      return DLA_OK;
    }
    auto kfn = gram_lds_kernel<TLW, KT, 1, R, 0, 0, 0, 1>;
    const size_t lds = gram_lds_bytes(TLW, KT, R, false, false);
    if (!raise_lds((const void*)kfn, lds)) return DLA_ERR_RUNTIME;
    DLA_LAUNCH(kfn, grid, dim3(256), lds, st, a);
    return DLA_OK;
  }
  //   cx != nullptr (m > 0, uw = u, one pass): U <- [X | U] C' stored, X^T U and U^T U of the stored result (OP_COMBOX)
  int gram_wp_once(int n, int m, const double* x, int k, const double* u, const double* wp, double* uw, StepOut& out, const double* cx = nullptr)
  {
    out = StepOut{};
    const bool self = (m == 0);
    if (cx != nullptr && (self || uw == nullptr || wp != nullptr || k > 16)) { err = "gram_wp: bad projection sweep"; return DLA_ERR_ARG; }
    if (k > 48 || (self && k > 16)) { err = "gram_wp: block too wide"; return DLA_ERR_ARG; }
    if (!lc.dry && rx_keep && measured.valid && !self && wp == nullptr && uw == nullptr && cx == nullptr && x == measured.x && u == measured.u &&
        n == measured.n && m == measured.m && k == measured.k) {
      // the measuring sweep of this block has run already, inside the Ritz sweep that formed it (ritz_expand): its partials are reduced
      // in the sweep's place -- same layout, same reduction, same tail
      measured.valid = false;
      if (m * k + k * k > XUG_DOUBLES) { err = "gram_wp: basis too wide for the chain's buffer"; return DLA_ERR_ARG; }
      int stm = ensure_small(sizeof(double) * (size_t)k * k);
      if (stm) return stm;
      return reduce_and_sum(DLA_OP_GRAM, d_xug, nullptr, measured.blocks, m, k, measured.tx, 1, 1, measured.tx + 1, 1, m + k, out, d_rxpart);
    }
    const WpPlan p = wp_plan(env(), n, m, k, cx != nullptr);
    const int tlw = p.tlw, kt = p.kt, passes = p.passes, blocks = p.blocks, extra = p.extra, slots = p.slots;
    int stc = ensure_partial(sizeof(double) * (size_t)passes * blocks * slots * 256);
    if (stc) return stc;
    stc = ensure_small(sizeof(double) * (size_t)k * k);
    if (stc) return stc;
    if (!self && (m + k) * k > XUG_DOUBLES) { err = "gram_wp: basis too wide for the chain's buffer"; return DLA_ERR_ARG; }
    // (written-back tiles: every pass would transform the block again, and passes run side by side)
    if (uw != nullptr && passes != 1) { err = "gram_wp: the storing sweep takes one pass"; return DLA_ERR_ARG; }
    GramArgs a{self ? u : x, u, d_partial, (long long)n, self ? k : m, k, passes, 0, lc.phase, lc.want, 0, wp, uw, cx};
    dim3 grid(blocks, passes);
    {
      // reference-schedule flops: the Gram matrix (2 n k^2), X^T U (2 n m k), and the triangular update the sweep applies on the fly
      // (n k^2) -- or, for the projection sweep, the update U -= X (X^T U) (2 n m k) with the pending factor (n k^2)
      Scope s(this, cx ? DLA_OP_GEMM : DLA_OP_GRAM, 8.0 * (double)n * (double)(m + k + (uw ? k : 0)),
              2.0 * (double)n * (m + k) * k + ((wp || cx) ? 1.0 * (double)n * k * k : 0.0) + (cx ? 2.0 * (double)n * m * k : 0.0), p.name());
      int r_ = DLA_ERR_RUNTIME;
      if (!first_instance<std::size(WP_TILES)>([&](auto i) {
            constexpr WpTile s = WP_TILES[decltype(i)::value];
            if (tlw != s.tlw || kt != s.kt || p.R != s.R) return false;
            r_ = launch_gram_wp<s.tlw, s.kt, s.R>(a, grid, self);
            return true;
          }))
        err = "gram_wp: no kernel instance";
      if (r_) return r_;
    }
    const int n_out = self ? 1 : passes * tlw * kt + extra;
    return reduce_and_sum(DLA_OP_GRAM, self ? d_small : d_xug, nullptr, blocks, self ? k : m, k, tlw, kt, passes, n_out, extra, self ? k : m + k, out);
  }

  // A chain runs in two halves: ortho_chain_begin enqueues the planned launches, ortho_chain_finish waits, reads what the
  // device reports and continues from there when it went another way than planned.  ortho_chain is the two back to back;
  // dla_expand_project (host_logic.cpp) puts the operator and the projection sweep of the new block between them, so that
  // the chain's report is read at THEIR wait (one host wait per expansion instead of two; the speculated launches are
  // simply repeated when the report is not the expected one).
  struct ChainRun {
    bool active = false;
    int n = 0, m = 0, k = 0, fold = 0;
    bool vsx = false;
    const double *x = nullptr, *bx = nullptr;
    double* u = nullptr;
    ChainShape shape;                // of the plan: plan_of_shape[shape], plan_of_kind[shape.kind()]
    bool xw = false;                 // wide block with the storing sweep OP_XW (see ortho_chain_begin)
    bool x3 = false;                 // three-pass schedule
    bool lean = false;               // the plan carries no closing / final sweep (the machine will not ask for them: see ortho_chain_begin)
    std::vector<int> plan, launched;
    std::vector<SpecRec> recs;
  } run;

  // ---- the caller's pending blocks on the device (dla_basis_sync): D, upper triangular, column-major with leading dimension
  // DMAT_LD -- what the exact projection of ortho_tail16 multiplies with.  Columns arrive in order, block by block.
  DeviceBuffer<double> d_dmat;
  // the same on the host, column by column (column j: rows 0 .. j) -- what the host-driven loop multiplies with (basis_dd).  The host
  // copy has no width limit: a basis that outgrows the device copy (DMAT_LD columns) goes on with blocks finished in memory by the
  // host-driven loop, exactly, instead of being refused or -- before round 6 -- silently projected against unfinished columns
  std::vector<std::vector<double>> h_dcols;
  int dmat_cols = 0;                 // columns described so far
  bool dmat_nontrivial = false;      // some entry differs from the identity at all (exact comparison: a rounding-level pending factor
                                     // already switches the chains to the D D^T assembly -- two more k x k x m products per step --
                                     // because a threshold would make the projections inexact by that threshold)
  int basis_state(int m) const override { return m <= 0 ? 0 : dmat_cols != m ? -1 : dmat_nontrivial ? 1 : 0; }
  int basis_capacity() const override { return DMAT_LD; }
  bool basis_exact_ok() const override { return !hook && !local_only && !knobs.no_exact_basis() && lds_limit > (size_t)128 * 1024; }
  int basis_dd(int m, int k, double* xu, int ld) override
  {
    if (!policy.basis_exact || m <= 0) return DLA_OK;
    if (dmat_cols != m) { err = "ortho_vs_x: the copy of the caller's pending blocks does not describe this basis (dla_basis_sync after every block)"; return DLA_ERR_ARG; }
    if (!dmat_nontrivial) return DLA_OK;
    std::vector<double> y(m);
    for (int j = 0; j < k; ++j) {
      double* s = xu + (size_t)j * ld;
      for (int r = 0; r < m; ++r) {                      // y = D^T s: column r of D, rows 0 .. r
        const double* dr = h_dcols[r].data();
        double acc = 0.0;
        for (int i = 0; i <= r; ++i) acc += dr[i] * s[i];
        y[r] = acc;
      }
      for (int i = 0; i < m; ++i) s[i] = 0.0;
      for (int q = 0; q < m; ++q) {                      // s = D y
        const double* dq = h_dcols[q].data();
        const double yq = y[q];
        for (int i = 0; i <= q; ++i) s[i] += dq[i] * yq;
      }
    }
    return DLA_OK;
  }
  int basis_sync(int m, int k, const double* dmat, int ld) override
  {
    if (k <= 0) { dmat_cols = 0; dmat_nontrivial = false; h_dcols.clear(); return DLA_OK; }
    if (m != dmat_cols) { err = "basis_sync: the blocks of D arrive in order (" + std::to_string(dmat_cols) + " columns known, block starts at " + std::to_string(m) + ")"; return DLA_ERR_ARG; }
    h_dcols.resize((size_t)m + k);
    for (int j = 0; j < k; ++j) {
      std::vector<double>& col = h_dcols[(size_t)m + j];
      col.resize((size_t)m + j + 1);
      for (int i = 0; i <= m + j; ++i) {
        const double v = dmat[(size_t)i + (size_t)(m + j) * ld];
        col[i] = v;
        if (v != (i == m + j ? 1.0 : 0.0)) dmat_nontrivial = true;
      }
    }
    dmat_cols = m + k;
    // the device copy takes the first DMAT_LD columns (what the exact projection of ortho_tail16 keeps in LDS); a block that reaches
    // beyond them stays on the host only -- dla_expand_project sends such a basis through the host-driven loop (round-5 advisor)
    if (m + k > DMAT_LD) return DLA_OK;
    bind();
    { const int stz = reserve_zeroed(d_dmat, (size_t)DMAT_LD * DMAT_LD); if (stz) return stz; }
    double* h = nullptr;
    int slot = 0;
    const size_t bytes = sizeof(double) * (size_t)k * DMAT_LD;
    const int stc = stage_slot(bytes, &h, &slot);
    if (stc) return stc;
    std::memset(h, 0, bytes);
    for (int j = 0; j < k; ++j) std::memcpy(h + (size_t)j * DMAT_LD, h_dcols[(size_t)m + j].data(), sizeof(double) * (size_t)(m + j + 1));
    return stage_commit(slot, bytes, d_dmat + (size_t)m * DMAT_LD);
  }

  // the block the last chain left pending (policy.publishes()): p = [E ; T], (m + k) x k -- the finished block is
  // [X | U_stored] p -- or [0 ; I] when nothing is pending; fetching it clears it
  int pending_block(int m, int k, double* p, int ldp, int* applied) override
  {
    for (int j = 0; j < k; ++j)
      for (int i = 0; i < m + k; ++i) p[(size_t)i + (size_t)j * ldp] = (i == m + j) ? 1.0 : 0.0;
    if (applied) *applied = 0;
    if (t_pending_k == k && h_tpend) {
      if (applied) *applied = h_tpend[PEND_HDR + 2] != 0.0 ? 1 : 0;
      const int er = (int)h_tpend[PEND_HDR + 1];
      if (er != 0 && er != m) { t_pending_k = 0; err = "pending_block: the chain's basis width is not the caller's"; return DLA_ERR_ARG; }
      for (int j = 0; j < k; ++j) {
        for (int i = 0; i < er; ++i) p[(size_t)i + (size_t)j * ldp] = h_tpend[(size_t)i * PEND_LD + j];
        for (int i = 0; i <= j; ++i) p[(size_t)(m + i) + (size_t)j * ldp] = h_tpend[(size_t)(er + i) * PEND_LD + j];
      }
    }
    t_pending_k = 0;
    return DLA_OK;
  }
  int ortho_chain(int n, int m, int k, const double* x, const double* bx, double* u, dla::OrthoReport* rep) override
  {
    int stc = ortho_chain_begin(n, m, k, x, bx, u, rep);
    if (stc || !rep->handled) return stc;
    return ortho_chain_finish(rep, false);
  }

  int ortho_chain_begin(int n, int m, int k, const double* x, const double* bx, double* u, dla::OrthoReport* rep) override
  {
    rep->handled = 0;
    t_pending_k = 0;                 // (whatever an earlier chain left: nobody fetched it, it belongs to no later call)
    // A block that the Ritz sweep in front of this call formed and measured (ritz_expand): the record is kept while this call's own
    // launches go out -- the first of them, the planned OP_GRAMX, takes it (gram_wp_once) -- and dropped on every way out that did not
    struct TakeMeasured {
      HipEngine* e;
      TakeMeasured(HipEngine* e_, bool match) : e(e_) { e->rx_keep = match; if (!match) e->drop_measured(); }
      ~TakeMeasured() { e->rx_keep = false; e->drop_measured(); }
    } take_measured(this, measured.valid && x == measured.x && bx == x && u == measured.u && n == measured.n && m == measured.m && k == measured.k);
    if (run.active) { err = "ortho_chain: a chain is already in flight"; return DLA_ERR_RUNTIME; }
    // (policy.basis_exact: the stored columns are not orthonormal, only the device chain projects with the caller's D -- the host-driven
    //  loop, which ends on the reference's growth test, must not take such a block)
    auto not_handled = [&]() {
      if (!(policy.basis_exact && m > 0) || dmat_cols == m) return (int)DLA_OK;     // (the host-driven loop projects with D as well: basis_dd)
      err = "ortho_chain: dla_expand_project mode 5 needs the caller's pending blocks (dla_basis_sync after every block of the basis)";
      return (int)DLA_ERR_ARG;
    };
    // which schedule, if any: chain_choice (hip_plans.h) reads these facts and the policy, and nothing else
    const bool vsx = m > 0;
    ChainIn in{};
    in.m = m; in.k = k;
    in.vec2 = on_16_bytes(n, u, x, bx);
    in.bx_is_x = bx == x;
    in.combo_ok = vsx && u == x + (size_t)n * m && can_combo(m, k);
    in.host_between = hook || local_only;
    in.x3_cooldown = x3_cooldown; in.dmat_cols = dmat_cols; in.dmat_nontrivial = dmat_nontrivial;
    in.fused_lds_kk = k > 0 ? fused_lds(k, k) : 0;
    const ChainChoice choice = chain_choice(env(), policy, in);
    if (choice.take == ChainChoice::host_loop) return not_handled();
    if (choice.take == ChainChoice::nothing) return DLA_OK;
    const int fold = choice.fold;
    const bool x3 = choice.x3, wide_gramx = choice.wide_gramx, wide_xw = choice.wide_xw;
    int stc = ensure_chain_buffers();
    if (stc) return stc;
    // First chain of a shape: walk every launch path it may take WITHOUT launching (workspaces grow now, not half way; a
    // refused request for more than 64 KiB of LDS shows up before anything has touched U).  After a refusal the engine's LDS
    // limit is down and the host-driven loop, which redoes single operations under it, takes the call.
    {
      ChainShape walked;
      walked.k = k; walked.m = m; walked.fold = fold; walked.vsx = vsx; walked.wide_xw = wide_xw; walked.x3 = x3;
      if (!chain_verified.count(walked)) {
        static const int every_op[] = {OP_GRAM_UU, OP_GRAMX, OP_GRAMW, OP_XW, OP_XU, OP_TRMMG, OP_COMBO, OP_FINAL, OP_COMBOX, OP_CLOSE, OP_TRMMC};
        lds_retry = false;
        int std_ = DLA_OK;
        {
          LaunchCtx walk = lc;
          walk.dry = true; walk.xw = wide_xw; walk.x3 = x3;
          CtxScope scope(this, walk);
          for (int op : every_op) {
            if (!vsx && (op == OP_GRAMX || op == OP_XW || op == OP_XU || op == OP_COMBO || op == OP_GRAMW)) continue;
            if ((op == OP_COMBOX || op == OP_CLOSE || op == OP_TRMMC) && !x3) continue;
            if (fold != 1 && (op == OP_GRAMW || (op == OP_XW && !wide_xw))) continue;
            if (fold != 1 && op == OP_GRAMX && !wide_gramx) continue;
            std_ = launch_op(op, n, m, k, x, bx, u, false, fold);
            if (std_) break;
          }
        }
        if (std_) {
          if (lds_retry) { lds_retry = false; return not_handled(); }        // rep->handled stays 0: host-driven loop
          return std_;
        }
        chain_verified.insert(walked);
      }
    }
    // the widest reductions of the chain: make sure nothing reallocates (and drains the stream) half way
    stc = ensure_small(sizeof(double) * (size_t)(m + k) * k);
    if (stc) return stc;

    if (!chain_armed) {
      // first chain (or the previous one was abandoned on an error): copy the initial state in.  Afterwards the
      // tail that ends a chain re-arms the machine itself.
      OrthoDev init{};
      init.phase = OP_GRAM_UU; init.status = OST_RUNNING; init.growth = 1.0; init.gdev = 1.0;
      *h_ost_init = init;
      HIPCHK(hipMemcpyAsync(d_ost, h_ost_init, sizeof(OrthoDev), hipMemcpyHostToDevice, st));
    }
    chain_armed = false;
    h_ost->status = -1;              // nothing reported yet (the tails write this mirror)
    h_ost->nops = 0;

    // the schedule depends on how much of the new block already lies in span(X): remembered per basis width
    const bool dropf = policy.drop_final && vsx;
    t_pending_k = 0;
    t_seq = t_seq >= 1000000 ? 1 : t_seq + 1;
    ChainShape shape;
    shape.k = k; shape.m = m; shape.fold = fold; shape.vsx = vsx; shape.wide_gramx = wide_gramx; shape.wide_xw = wide_xw; shape.dropf = dropf; shape.x3 = x3;
    std::vector<int> plan = plan_of_shape[shape];
    if (plan.empty()) plan = plan_of_kind[shape.kind()];   // most recent call of this kind and width
    if (plan.empty()) plan = default_plan(shape);
    const bool lean = chain_lean(env(), policy, m, k, Transport{p2p.on, nranks, comm != nullptr});
    plan = close_plan(plan, lean, x3);
    // (The plain projection sweep never stands in for the measuring one, although it is faster -- 4 m / 16 fewer MFMAs per 16 rows,
    //  5.7 against 5.0-5.4 TB/s -- and its measurement is thrown away whenever the block it stored needs a level shift: which
    //  sweep ran would decide what the step behind it knows, the chain's path would depend on the plan, the plan on the chains
    //  this context has seen before, and two identical solves would differ in their last bits.  r05: tried, 0.02 ms per shifted
    //  chain of the benchmark; tests/test_solver_gpu.py compares repeated solves bit for bit.)
    run.n = n; run.m = m; run.k = k; run.fold = fold; run.vsx = vsx; run.x = x; run.bx = bx; run.u = u;
    run.shape = shape;
    run.xw = wide_xw;
    run.x3 = x3;
    run.lean = lean;
    run.plan = plan; run.launched.clear(); run.recs.clear();
    stc = chain_enqueue();
    if (stc) return stc;
    account_chains();                // (the device has work now)
    run.active = true;
    rep->handled = 1;
    rep->status = 0;                 // in flight
    return DLA_OK;
  }

  // statistics of finished chains: the launches the device executed are the greedy match of its log inside the launch
  // sequence.  Called with the device busy (behind the next chain's launches) or when somebody reads the statistics.
  struct ChainDone { std::vector<int> launched; std::vector<SpecRec> recs; int log[48]; int nlog = 0, n = 0, k = 0; };
  std::vector<ChainDone> unaccounted;
  void account_chains()
  {
    for (auto& cd : unaccounted) {
      std::vector<char> ran(cd.launched.size(), 0);
      int j = 0;
      for (size_t i = 0; i < cd.launched.size() && j < cd.nlog; ++i)
        if (cd.launched[i] == cd.log[j]) { ran[i] = 1; ++j; }
      for (auto& r : cd.recs) {
        if (!ran[r.tag]) continue;
        stats.launches[r.cls] += 1; stats.alg_bytes[r.cls] += r.bytes; stats.flops[r.cls] += r.flops;
        if (!r.kname.empty()) { auto& ks = kstats[r.kname]; ks.launches += 1; ks.alg_bytes += r.bytes; ks.flops += r.flops; }
      }
      // reference-schedule flops of what the fused sweeps fold in (same bookkeeping as trmm_gram / combo_gram)
      for (size_t i = 0; i < cd.launched.size(); ++i) {
        if (!ran[i]) continue;
        if (cd.launched[i] == OP_TRMMG || cd.launched[i] == OP_TRMMC) stats.flops[DLA_OP_GRAM] += 2.0 * (double)cd.n * cd.k * cd.k;
        if (cd.launched[i] == OP_COMBO) { stats.flops[DLA_OP_GRAM] += 2.0 * (double)cd.n * cd.k * cd.k; stats.flops[DLA_OP_GEMM] -= 1.0 * (double)cd.n * cd.k * cd.k; }
      }
    }
    unaccounted.clear();
  }

  // enqueue run.plan (every launch predicated on the device state machine standing where the plan expects it)
  int chain_enqueue()
  {
    int stc = DLA_OK;
    for (size_t pi = 0; pi < run.plan.size() && !stc; ++pi) {
      LaunchCtx spec = lc;
      spec.rec = &run.recs; spec.tag = (int)run.launched.size(); spec.xw = run.xw; spec.x3 = run.x3;
      CtxScope scope(this, spec);
      run.launched.push_back(run.plan[pi]);
      stc = launch_op(run.plan[pi], run.n, run.m, run.k, run.x, run.bx, run.u, pi + 1 == run.plan.size(), run.fold);
    }
    if (stc) { (void)hipStreamSynchronize(st); chain_armed = false; return stc; }
    return DLA_OK;
  }

  // `waited`: the caller has waited for the stream since ortho_chain_begin (its own result came through the same wait).
  // rep->clean = 1 when the planned launches were the whole chain (nothing was enqueued here).
  int ortho_chain_finish(dla::OrthoReport* rep, bool waited) override
  {
    if (!run.active) { err = "ortho_chain_finish: no chain in flight"; return DLA_ERR_RUNTIME; }
    run.active = false;
    const int n = run.n, m = run.m, k = run.k, fold = run.fold;
    const bool vsx = run.vsx;
    std::vector<int>& plan = run.plan;
    std::vector<int>& launched = run.launched;
    std::vector<SpecRec>& recs = run.recs;
    std::vector<int>& hist = plan_of_shape[run.shape];
    std::vector<int>& last_k = plan_of_kind[run.shape.kind()];
    int stc = DLA_OK;
    rep->clean = 1;
    OrthoDev sres{};
    for (int round = 0; round < 256; ++round) {
      if (round > 0) {
        rep->clean = 0;
        stc = chain_enqueue();
        if (stc) return stc;
      }
      if (round > 0 || !waited) {
        stc = wait_stream();
        if (stc) { chain_armed = false; return stc; }
        stats.host_syncs++;
      }
      sres = *h_ost;
      if (sres.status < 0) { err = "ortho_chain: the device reported nothing"; return DLA_ERR_RUNTIME; }
      if (sres.status != OST_RUNNING) break;
      // the device went another way than expected: continue from where it stands with the most likely tail
      // (a launch whose turn it is not costs ~2 us, a host round trip ~25: the continuation lists what may follow, in order)
      if (run.x3) {
        switch (sres.phase) {
          case OP_TRMMG: plan = sres.it_outer == 0 ? std::vector<int>{OP_TRMMG, OP_GRAMW, OP_COMBOX, OP_COMBOX, OP_CLOSE, OP_FINAL}
                                                   : std::vector<int>{OP_TRMMG, OP_XW, OP_XU, OP_COMBOX, OP_CLOSE, OP_FINAL}; break;
          case OP_TRMMC:  plan = {OP_TRMMC, OP_XW, OP_XU, OP_COMBOX, OP_CLOSE, OP_FINAL}; break;
          case OP_GRAMW:  plan = {OP_GRAMW, OP_GRAMW, OP_COMBOX, OP_COMBOX, OP_CLOSE, OP_FINAL}; break;
          case OP_COMBOX: plan = {OP_COMBOX, OP_COMBOX, OP_CLOSE, OP_FINAL}; break;
          case OP_XW:     plan = {OP_XW, OP_COMBOX, OP_CLOSE, OP_FINAL}; break;
          case OP_XU:     plan = {OP_XU, OP_COMBOX, OP_COMBOX, OP_CLOSE, OP_FINAL}; break;
          case OP_CLOSE:  plan = {OP_CLOSE, OP_FINAL}; break;
          case OP_FINAL:  plan = {OP_FINAL}; break;
          default: err = "ortho_chain: device state machine in an unexpected phase"; return DLA_ERR_RUNTIME;
        }
      } else if (fold == 1) {
        switch (sres.phase) {
          case OP_TRMMG: plan = sres.it_outer == 0 ? std::vector<int>{OP_TRMMG, OP_GRAMW, OP_COMBO, OP_XW, OP_COMBO, OP_FINAL}
                                                   : std::vector<int>{OP_TRMMG, OP_XU, OP_COMBO, OP_FINAL}; break;
          case OP_GRAMW: plan = {OP_GRAMW, OP_GRAMW, OP_COMBO, OP_XW, OP_COMBO, OP_FINAL}; break;
          case OP_COMBO: plan = sres.it_outer <= 1 ? std::vector<int>{OP_COMBO, OP_XW, OP_COMBO, OP_FINAL}
                                                   : std::vector<int>{OP_COMBO, OP_XW, OP_XU, OP_COMBO, OP_FINAL}; break;
          case OP_XW:    plan = {OP_XW, OP_TRMMG, OP_XU, OP_COMBO, OP_FINAL}; break;
          case OP_XU:    plan = {OP_XU, OP_COMBO, OP_FINAL}; break;
          case OP_FINAL: plan = {OP_FINAL}; break;
          default: err = "ortho_chain: device state machine in an unexpected phase"; return DLA_ERR_RUNTIME;
        }
      } else {
        switch (sres.phase) {
          case OP_TRMMG: plan = vsx ? std::vector<int>{OP_TRMMG, OP_XU, OP_COMBO, OP_FINAL} : std::vector<int>{OP_TRMMG, OP_FINAL}; break;
          case OP_XW:    plan = {OP_XW, OP_COMBO, OP_FINAL}; break;
          case OP_XU:    plan = {OP_XU, OP_COMBO, OP_FINAL}; break;
          case OP_COMBO: plan = {OP_COMBO, OP_FINAL}; break;
          case OP_FINAL: plan = {OP_FINAL}; break;
          default: err = "ortho_chain: device state machine in an unexpected phase"; return DLA_ERR_RUNTIME;
        }
      }
      if (run.lean && sres.phase != OP_CLOSE && sres.phase != OP_FINAL) trim_closing(plan);
      h_ost->status = -1;
    }
    if (sres.status == OST_RUNNING) { err = "ortho_chain: no progress"; return DLA_ERR_RUNTIME; }
    chain_armed = true;              // a terminal tail has put the machine back to its initial state
    if (vsx && fold == 1) { if (sres.shifts > 0) x3_cooldown = 16; else if (x3_cooldown > 0) --x3_cooldown; }
    if (chain_debug) {
      std::printf("  [dla] chain k=%d m=%d: %zu launches enqueued, executed:", k, m, launched.size());
      for (int i = 0; i < std::min(sres.nops, 48); ++i) std::printf(" %d", sres.log[i]);
      std::printf("  (host waits so far %lld)\n", (long long)stats.host_syncs);
      if (d_dbg && fold) {
        std::vector<unsigned long long> hs(48 * 16);
        (void)hipMemcpy(hs.data(), d_dbg, sizeof(unsigned long long) * 48 * 16, hipMemcpyDeviceToHost);
        for (int i = 0; i < std::min(sres.nops, 48); ++i) {
          const unsigned long long* q = &hs[i * 16];
          auto us = [&](int a_, int b_) { return (q[a_] && q[b_]) ? (double)(long long)(q[b_] - q[a_]) * 0.01 : -1.0; };
          double rc, gdev, sdev, csq; std::memcpy(&rc, &q[10], 8); std::memcpy(&gdev, &q[12], 8); std::memcpy(&sdev, &q[13], 8); std::memcpy(&csq, &q[14], 8);
          std::printf("    op %llu (err est %.2e, max|G-I| %.2e, max|X^T U| %.2e (col sq %.2e), chol %llu cycles = %.2f GHz): kernel entry->tail %.2f us | G load %.2f | chol+inv %.2f | norms %.2f | products+stores %.2f | decide %.2f | publish %.2f | assemble %.2f\n",
                      q[9], 2.2e-16 * rc * rc, gdev, sdev, csq, q[11], us(1, 2) > 0 ? (double)q[11] / (us(1, 2) * 1e3) : 0.0, us(8, 0), us(0, 1), us(1, 2), us(2, 3), us(3, 4), us(4, 5), us(5, 6), us(6, 7));
        }
        (void)hipMemset(d_dbg, 0, sizeof(unsigned long long) * 48 * 16);
      }
    }
    // the launches the device executed are accounted for later, off the critical path (account_chains): the caller is
    // waiting for this report with the device idle
    {
      const int nlog = std::min(sres.nops, 48);
      ChainDone cd;
      cd.launched.swap(launched); cd.recs.swap(recs);
      std::copy(sres.log, sres.log + nlog, cd.log);
      cd.nlog = nlog; cd.n = n; cd.k = k;
      unaccounted.push_back(std::move(cd));
      if (sres.status == OST_DONE && sres.nops <= 48) { hist.assign(sres.log, sres.log + nlog); last_k = hist; }
    }
    // a chain that ended with its last factor pending has left it in the pinned buffer (the tail wrote the sequence number last)
    if (sres.status == OST_DONE && policy.publishes() && vsx && h_tpend[PEND_HDR] == (double)t_seq) t_pending_k = k;
    rep->handled = 1;
    rep->status = sres.status;
    rep->growth = sres.growth;
    rep->outer_its = sres.it_outer;
    rep->macro_its = sres.macro_total;
    rep->shifts = sres.shifts;
    return DLA_OK;
  }

  // ---- b_ortho behind a chain (dla_expand_project_metric): Gram sweep U^T BU, k x k step on the device, the two updates
  // predicated on its outcome; nothing waits.  b_ortho_ahead_status() after the caller's next host wait: 1 done, 0 did not run
  // (the chain in front of it had not ended well: the caller repeats everything behind the chain), -1 metric not positive definite.
  DeviceBuffer<int> d_bgo; MappedHostBuffer<int> h_bstat; DeviceBuffer<double> d_wpk_b;
  int b_seq = 0;
  int b_ortho_ahead(int n, int k, double* u, double* bu, bool behind_chain, int* handled) override
  {
    *handled = 0;
    if (k <= 0 || k > 48 || hook || local_only || knobs.no_b_ortho_ahead()) return DLA_OK;
    bind();
    { const int stz = reserve_zeroed(d_bgo, 1); if (stz) return stz; }
    HIPCHK(h_bstat.reserve(1));
    HIPCHK(d_wpk_b.reserve(3 * 48 * 16));
    int stc = ensure_chain_buffers();
    if (stc) return stc;
    // M = U^T (B U): every rank's share summed like any other small product
    StepOut gram_out;
    stc = gram_dev(n, k, u, k, bu, gram_out);
    if (stc) return stc;
    b_seq = b_seq >= 1000000 ? 1 : b_seq + 1;
    *h_bstat = 0;
    {
      Scope s(this, DLA_OP_GRAM, 0.0, 0.0, "bortho_tail_kernel");
      BOrthoTailArgs ta{d_ost, d_small, d_wpk_b, k, behind_chain ? 1 : 0, b_seq, d_bgo, h_bstat.dev()};
      DLA_LAUNCH(bortho_tail_kernel, dim3(1), dim3(64), 0, st, ta);
      HIPCHK(hipGetLastError());
    }
    {
      LaunchCtx behind = lc;
      behind.phase = d_bgo; behind.want = b_seq;
      CtxScope scope(this, behind);
      stc = gemm_chunk(n, 0, k, u, k, nullptr, 0, u, 2, DLA_OP_TRMM, nullptr, d_wpk_b);
      if (!stc) stc = gemm_chunk(n, 0, k, bu, k, nullptr, 0, bu, 2, DLA_OP_TRMM, nullptr, d_wpk_b);
    }
    if (stc) return stc;
    *handled = 1;
    return DLA_OK;
  }
  int b_ortho_ahead_status() override
  {
    const int v = *(volatile int*)h_bstat;
    return v == b_seq ? 1 : (v == -b_seq ? -1 : 0);
  }

  // ---- Gram
  template <int TLW, int KT, int R>
  int launch_gram_lds(const GramArgs& a, dim3 grid, const GramPlan& p)
  {
    int r_ = DLA_OK;
    const bool hit = first_instance<std::size(GRAM_LDS_FORMS)>([&](auto i) {
      constexpr GramLdsForm f = GRAM_LDS_FORMS[decltype(i)::value];
      if constexpr (!gram_lds_form(TLW, KT, f)) return false;
      else {
        if ((p.self ? 1 : 0) != f.self || p.qt != f.qt) return false;
        auto kfn = gram_lds_kernel<TLW, KT, 1, R, f.self, f.qt>;
        const size_t lds = gram_lds_bytes(TLW, KT, R, f.self, false);
        if (!raise_lds((const void*)kfn, lds)) r_ = DLA_ERR_RUNTIME;
        else DLA_LAUNCH(kfn, grid, dim3(256), lds, st, a);
        return true;
      }
    });
    if (!hit) { err = "gram: no kernel instance"; return DLA_ERR_RUNTIME; }
    return r_;
  }
  // single-pass lower triangle (gram_lds_kernel LOW): T x T tiles, 16-row wave tiles
  template <int T>
  int launch_gram_low(const GramArgs& a, dim3 grid, const GramPlan& p)
  {
    auto kfn = gram_lds_kernel<T, T, 1, 16, 0, 0, 1>;
    const size_t lds = gram_lds_bytes(T, T, 16, false, true);
    if (!raise_lds((const void*)kfn, lds)) return DLA_ERR_RUNTIME;
    DLA_LAUNCH(kfn, grid, dim3(256), lds, st, a);
    return DLA_OK;
  }
  template <int TLW, int KT>
  int launch_gram(const GramArgs& a, dim3 grid, const GramPlan& p)
  {
    if constexpr (KT <= 3) {
      if (p.lds) {
        if constexpr (gram_can32(TLW, KT)) { if (p.rows == 32) return launch_gram_lds<TLW, KT, 32>(a, grid, p); }
        return launch_gram_lds<TLW, KT, 16>(a, grid, p);
      }
    }
    if constexpr (!gram_direct_instance(TLW, KT)) {
      err = "gram: width without a direct-load instance";
      return DLA_ERR_RUNTIME;
    } else {
      constexpr int RS = gram_rs(TLW, KT);
      if (p.vec2) DLA_LAUNCH((gram_kernel<TLW, KT, 2, RS>), grid, dim3(256), 0, st, a);
      else      DLA_LAUNCH((gram_kernel<TLW, KT, 1, RS>), grid, dim3(256), 0, st, a);
      return DLA_OK;
    }
  }

  // result stays on the device in d_small (l x k, ld = l), reduced over ranks
  // out.lower_only: only the lower block triangle was formed (whoever copies the result out mirrors it, see gram())
  int gram_dev(int n, int l, const double* x, int k, const double* u, StepOut& out, int cls = DLA_OP_GRAM, bool lower = false)
  {
    return with_lds_retry([&]() { return gram_dev_once(n, l, x, k, u, cls, lower, out); });
  }
  int gram_dev_once(int n, int l, const double* x, int k, const double* u, int cls, bool lower, StepOut& out)
  {
    out = StepOut{};
    const GramPlan p = gram_plan(env(), n, l, k, x == u, peers_even && ((uintptr_t)x | (uintptr_t)u) % 16 == 0, lower);
    const int tlw = p.tlw, kt = p.kt, passes = p.passes, blocks_per_pass = p.blocks_per_pass;
    out.lower_only = p.self;
    const int slots = tlw * kt;
    int stc = ensure_partial(sizeof(double) * (size_t)passes * blocks_per_pass * slots * 256);
    if (stc) return stc;
    stc = ensure_small(sizeof(double) * (size_t)l * k);
    if (stc) return stc;
    GramArgs a{x, u, d_partial, (long long)n, l, k, p.px, p.lower ? 1 : 0, lc.phase, lc.want, knobs.gram_load_pads() ? 1 : 0};
    dim3 grid(blocks_per_pass, passes);
    {
      const bool same = (x == u) && (l == k);
      Scope s(this, cls, 8.0 * (double)n * (same ? (double)k : (double)(l + k)), 2.0 * (double)n * l * k, p.name());
      int r_ = DLA_ERR_RUNTIME;
      const bool hit = p.low_single ? first_instance<std::size(GRAM_LOW_TILES)>([&](auto i) {
                                        constexpr int T = GRAM_LOW_TILES[decltype(i)::value];
                                        if (tlw != T) return false;
                                        r_ = launch_gram_low<T>(a, grid, p);
                                        return true;
                                      })
                                    : first_instance<std::size(GRAM_TILES)>([&](auto i) {
                                        constexpr GramTile s = GRAM_TILES[decltype(i)::value];
                                        if (tlw != s.tlw || kt != s.kt) return false;
                                        r_ = launch_gram<s.tlw, s.kt>(a, grid, p);
                                        return true;
                                      });
      if (!hit) err = "gram: no kernel instance";
      if (r_) return r_;
    }
    return reduce_and_sum(cls, d_small + lc.small_off, lc.phase ? nullptr : h_small.dev() + lc.small_off, blocks_per_pass, l, k, tlw, kt, p.px,
                          passes * slots, 0, 0, out);
  }

  // ---- projection of a block that arrives in column chunks (host-mode callbacks: SURVEY 8f row 4, reference README.md:34-35).
  // C(:, c0 : c0 + kc) = X^T U_chunk is enqueued behind the uploads issued so far and lands in its columns of the l x k result;
  // the sweep runs while the caller's routine works on the next chunk.  gram_chunks_collect waits once for all of them.
  Event ev_chunk;
  bool gram_chunks_ok(int n, int l, int k) override
  {
    (void)n;
    return !hook && !comm && !p2p.on && (local_only || nranks <= 1) && l > 0 && k > 0 && lc.phase == nullptr;
  }
  int gram_chunk(int n, int l, const double* x, int k_total, int c0, int kc, const double* u_chunk) override
  {
    if (c0 == 0) { int stc = ensure_small(sizeof(double) * (size_t)l * k_total); if (stc) return stc; }
    HIPCHK(ev_chunk.ensure(hipEventDisableTiming));
    HIPCHK(hipEventRecord(ev_chunk, st_up));
    HIPCHK(hipStreamWaitEvent(st, ev_chunk, 0));
    LaunchCtx chunk = lc;
    chunk.small_off = (size_t)c0 * l; chunk.in_chunk = true;
    CtxScope scope(this, chunk);
    StepOut out;
    return gram_dev(n, l, x, kc, u_chunk, out);
  }
  int gram_chunks_collect(int l, int k, double* c_host, int ldc) override
  {
    return small_result_home(l, k, false, c_host, ldc);   // (one rank: no cross-rank sum has written the mirror)
  }

  int gram_lower(int n, int l, const double* x, const double* u, double* c_host, int ldc) override
  {
    StepOut out;
    const int stc = gram_dev(n, l, x, l, u, out, DLA_OP_GRAM, true);
    return stc ? stc : small_result_home(l, l, out.mirror_fresh, c_host, ldc);
  }

  int gram(int n, int l, const double* x, int k, const double* u, double* c_host, int ldc) override
  {
    StepOut out;
    const int stc = gram_dev(n, l, x, k, u, out);
    // (lower_only: a block against itself, l == k -- the Gram matrix of a block is symmetric)
    return stc ? stc : small_result_home(l, k, out.mirror_fresh, c_host, ldc, out.lower_only);
  }

  // second stage of a Gram whose per-block partials a fused kernel left in d_partial (`blocks` of them: gemm_chunk): result in
  // d_small (k x k, lower block triangle), summed over ranks
  int fused_reduce(int k, int blocks, StepOut& out)
  {
    out = StepOut{};
    int stc = ensure_small(sizeof(double) * (size_t)k * k);
    if (stc) return stc;
    const int kt = (k + 15) / 16;
    return reduce_and_sum(DLA_OP_GRAM, d_small, lc.phase ? nullptr : h_small.dev(), blocks, k, k, kt, kt, 1, kt * kt, 0, 0, out);
  }

  // ... and its copy to the host
  int finish_fused_gram(int k, int blocks, double* g_host, int ldg)
  {
    StepOut out;
    const int stc = fused_reduce(k, blocks, out);
    // (the kernel formed the lower block triangle; G is symmetric)
    return stc ? stc : small_result_home(k, k, out.mirror_fresh, g_host, ldg, true);
  }

  // U <- U W and G = U^T U of the result, one sweep (k <= 48); otherwise two sweeps
  int trmm_gram(int n, int k, double* u, const double* w_host, int ld, double* g_host, int ldg) override
  {
    return with_lds_retry([&]() { return trmm_gram_once(n, k, u, w_host, ld, g_host, ldg); });
  }
  int trmm_gram_once(int n, int k, double* u, const double* w_host, int ld, double* g_host, int ldg)
  {
    if (k > 48 || fused_lds(k, k) > lds_limit) return Engine::trmm_gram(n, k, u, w_host, ld, g_host, ldg);
    int blocks = 0;
    {
      // accounted as TRMM traffic (16nk) -- the Gram rides along
      int stc = gemm_chunk(n, 0, k, u, k, w_host, ld, u, 2, DLA_OP_TRMM, &blocks);
      if (stc) return stc;
    }
    stats.flops[DLA_OP_GRAM] += 2.0 * (double)n * k * k;   // reference-schedule flops of the Gram it replaces
    return finish_fused_gram(k, blocks, g_host, ldg);
  }

  // U <- [X | U] C' and G = U^T U of the result in one sweep; U is the last k columns of the same
  // contiguous panel (each wave reads all m+k columns of its rows before it stores, so in place is safe)
  bool can_combo(int m, int k) override
  {
    const int kt = (k + 15) / 16;
    return k <= 48 && m > 0 && (size_t)(m + k + 3) * 16 * kt * sizeof(double) <= (size_t)64 * 1024 &&   // C' in one LDS chunk
           fused_lds(m + k, k) <= lds_limit;
  }
  int combo_gram(int n, int m, const double* x, int k, const double* c_host, int ldc, double* u, double* g_host, int ldg) override
  {
    int st = with_lds_retry([&]() { return combo_gram_once(n, m, x, k, c_host, ldc, u, g_host, ldg); });
    if (st != DLA_OK && lds_limit <= (size_t)64 * 1024 && !can_combo(m, k) && u == x + (size_t)n * m && k <= 48) {
      // the fused sweep was refused its LDS and nothing was launched: same result in separate sweeps
      // (U <- [X | U] C' through a scratch panel, then the Gram)
      void* tmp = nullptr;
      st = alloc(sizeof(double) * (size_t)n * k, &tmp);
      if (!st) st = gemm(n, m + k, x, k, c_host, ldc, (double*)tmp, 0);
      if (!st) st = d2d(u, tmp, sizeof(double) * (size_t)n * k);
      if (!st) st = gram(n, k, u, k, u, g_host, ldg);
      int stf = free_(tmp);
      return st ? st : stf;
    }
    return st;
  }
  int combo_gram_once(int n, int m, const double* x, int k, const double* c_host, int ldc, double* u, double* g_host, int ldg)
  {
    if (!can_combo(m, k) || u != x + (size_t)n * m) { err = "combo_gram: unsupported shape"; return DLA_ERR_ARG; }
    int blocks = 0;
    int stc = gemm_chunk(n, 0, m + k, x, k, c_host, ldc, u, 0, DLA_OP_GEMM, &blocks);
    if (stc) return stc;
    // reference-schedule flops of what was folded in: dtrmm (n k^2) + the Gram (2 n k^2); the 2 n m k of the
    // update itself were counted by gemm_chunk (it counted 2 n (m+k) k)
    stats.flops[DLA_OP_GRAM] += 2.0 * (double)n * k * k;
    stats.flops[DLA_OP_GEMM] -= 1.0 * (double)n * k * k;
    return finish_fused_gram(k, blocks, g_host, ldg);
  }

  // U -= X C and G = U^T U of the result, one sweep (k <= 48, C fits one LDS chunk)
  int update_gram(int n, int l, const double* x, int k, const double* c_host, int ldc, double* u, double* g_host, int ldg) override
  {
    return with_lds_retry([&]() { return update_gram_once(n, l, x, k, c_host, ldc, u, g_host, ldg); });
  }
  int update_gram_once(int n, int l, const double* x, int k, const double* c_host, int ldc, double* u, double* g_host, int ldg)
  {
    if (k > 48 || l == 0 || (size_t)(l + 3) * 16 * ((k + 15) / 16) * sizeof(double) > (size_t)64 * 1024 ||
        fused_lds(l, k) > lds_limit)
      return Engine::update_gram(n, l, x, k, c_host, ldc, u, g_host, ldg);
    int blocks = 0;
    int stc = gemm_chunk(n, 0, l, x, k, c_host, ldc, u, 1, DLA_OP_GEMM, &blocks);
    if (stc) return stc;
    stats.flops[DLA_OP_GRAM] += 2.0 * (double)n * k * k;
    return finish_fused_gram(k, blocks, g_host, ldg);
  }

  // ---- packed C upload: [KT][l4][16], zero padded
  int upload_packed(const double* c_host, int ldc, int l0, int l, int k, int kt, int l4)
  {
    bind();
    const size_t cnt = (size_t)kt * l4 * 16;
    if (cnt > d_cpk.capacity()) {
      HIPCHK(hipStreamSynchronize(st));
      HIPCHK(d_cpk.reserve(std::max(cnt, doubles((size_t)1 << 16))));
    }
    double* pk = nullptr;                    // packed straight into the pinned slot
    int slot = 0;
    const int stc = stage_slot(sizeof(double) * cnt, &pk, &slot);
    if (stc) return stc;
    std::memset(pk, 0, sizeof(double) * cnt);
    for (int j = 0; j < k; ++j) {
      const int q = j / 16, jj = j % 16;
      double* dst = pk + (size_t)q * l4 * 16 + jj;
      const double* src = c_host + (size_t)l0 + (size_t)j * ldc;
      for (int p = 0; p < l; ++p) dst[(size_t)p * 16] = src[p];
    }
    return stage_commit(slot, sizeof(double) * cnt, d_cpk);
  }

  // The one launch of gemm_kernel: the row of GEMM_INSTANCES (hip_plans.h) whose template arguments equal the plan's fields, and nothing
  // else selects an instance.  The rows are what a predicate admits of the product argument type x KT x VEC x MODE x fuse x depth x
  // quarter tiles x row groups, and exactly they are instantiated; a plan that names none launches nothing.  ARGS is the plan's `inl`.
  template <typename ARGS>
  int launch_gemm(const GemmPlan& p, const ARGS& a)
  {
    int r_ = DLA_OK;
    const bool hit = first_instance<std::size(GEMM_INSTANCES.row)>([&](auto i) {
      constexpr GemmInstance s = GEMM_INSTANCES.row[decltype(i)::value];
      if constexpr (s.inl != std::is_same_v<ARGS, GemmArgsInl>) return false;
      else {
        if (!p.names(s)) return false;
        auto kfn = gemm_kernel<s.kt, s.vec, s.mode, ARGS, s.fuse, (s.mode == 2 ? 0 : 1), s.pipe, 9, s.qt, s.rtp>;
        if (s.fuse && !raise_lds((const void*)kfn, p.lds)) r_ = DLA_ERR_RUNTIME;
        else DLA_LAUNCH(kfn, dim3(p.blocks), dim3(256), p.lds, st, a);
        return true;
      }
    });
    if (!hit) { err = "gemm: no kernel instance"; return DLA_ERR_RUNTIME; }
    return r_;
  }

  // cpk_dev != nullptr: the coefficient block is already packed in device memory (ortho_tail_kernel wrote it)
  // fused_blocks != nullptr: the fused variant, which also leaves the partials of the result's Gram matrix in d_partial -- one set per
  // block, and their number here for fused_reduce
  int gemm_chunk(int n, int l0, int l, const double* x, int k, const double* c_host, int ldc, double* z, int mode, int cls,
                 int* fused_blocks = nullptr, const double* cpk_dev = nullptr)
  {
    const bool fuse = fused_blocks != nullptr;
    const bool vec2 = on_16_bytes(n, x, z);
    const GemmPlan p = gemm_plan(env(), n, l, k, mode, fuse, cpk_dev != nullptr, vec2);
    const int kt = p.kt, l4 = p.l4, blocks = p.blocks;
    if (!p.inl && cpk_dev == nullptr) {
      int stc = upload_packed(c_host, ldc, l0, l, k, kt, l4);
      if (stc) return stc;
    }
    if (fuse) {
      int stp = ensure_partial(sizeof(double) * (size_t)blocks * kt * kt * 256);
      if (stp) return stp;
      *fused_blocks = blocks;
    }
    GemmArgs a{};
    a.x = x + (size_t)l0 * n; a.cpk = cpk_dev ? cpk_dev : d_cpk; a.z = z; a.n = n; a.l = l; a.l4 = l4; a.k = k; a.gpart = d_partial;
    a.phase = lc.phase; a.want = lc.want; a.xpf = knobs.no_next_tile_prefetch() ? 0 : 1;
    const double rd = (mode == 0) ? 8.0 * n * (double)l : (mode == 2 ? 8.0 * n * (double)k : 8.0 * n * (double)(l + k));
    Scope s(this, cls, rd + 8.0 * n * (double)k, (cls == DLA_OP_TRMM ? 1.0 : 2.0) * (double)n * l * k, p.name());
    int stl;
    if (p.inl) {
      GemmArgsInl ai{};
      ai.x = a.x; ai.z = z; ai.n = n; ai.l = l; ai.l4 = l4; ai.k = k; ai.gpart = d_partial;
      for (int j = 0; j < k; ++j)
        for (int r = 0; r < l; ++r) ai.cin[r * 16 + j] = c_host[(size_t)(l0 + r) + (size_t)j * ldc];
      stl = launch_gemm(p, ai);
    } else {
      stl = launch_gemm(p, a);
    }
    if (stl) return stl;
    HIPCHK(hipGetLastError());
    return DLA_OK;
  }

  int gemm_cols(int n, int l, const double* x, int k, const double* c_host, int ldc, double* z, int mode, int cls)
  {
    // split the contraction so that the LDS copy of C stays <= 64 KiB (two blocks per CU)
    const int kt = (k + 15) / 16;
    int lmax = (int)((64 * 1024) / (sizeof(double) * 16 * kt));
    lmax = std::max(4, (lmax / 4) * 4);
    if (mode == 2 && l > lmax) { err = "trmm: k too large"; return DLA_ERR_ARG; }
    if (mode != 2 && l > lmax && z >= x && z < x + (size_t)n * l) {
      err = "panel_gemm: output aliases the input panel but the contraction needs several LDS chunks";
      return DLA_ERR_ARG;
    }
    if (l == 0) {
      if (mode == 0) return zero(z, sizeof(double) * (size_t)n * k);
      return DLA_OK;
    }
    int l0 = 0, m = mode;
    while (l0 < l) {
      const int lc = std::min(lmax, l - l0);
      int stc = gemm_chunk(n, l0, lc, x, k, c_host, ldc, z, m, cls);
      if (stc) return stc;
      l0 += lc;
      if (m == 0) m = 3;   // later chunks accumulate
    }
    return DLA_OK;
  }

  int gemm(int n, int l, const double* x, int k, const double* c_host, int ldc, double* z, int mode) override
  {
    // wide outputs are processed 48 columns at a time: a later block would read columns of X that an earlier
    // block has already overwritten, so the output must not alias the input panel then
    if (k > 48 && z >= x && z < x + (size_t)n * l) {
      err = "panel_gemm: output aliases the input panel and has more than 48 columns";
      return DLA_ERR_ARG;
    }
    for (int k0 = 0; k0 < k; k0 += 48) {
      const int kc = std::min(48, k - k0);
      int stc = gemm_cols(n, l, x, kc, c_host + (size_t)k0 * ldc, ldc, z + (size_t)k0 * n, mode, DLA_OP_GEMM);
      if (stc) return stc;
    }
    return DLA_OK;
  }

  int trmm(int n, int k, double* u, const double* w_host, int ld) override
  {
    if (k <= 48) return gemm_cols(n, k, u, k, w_host, ld, u, 2, DLA_OP_TRMM);
    // wide block (cold path: the drivers never exceed n_max columns): W is upper triangular, so column
    // block J of U W needs columns <= max(J) only; go right to left through a scratch panel
    DeviceBuffer<double> tmp;
    bind();
    HIPCHK(tmp.reserve((size_t)n * 48));
    int stc = DLA_OK;
    for (int j1 = k; j1 > 0 && stc == DLA_OK; j1 -= 48) {
      const int j0 = std::max(0, j1 - 48), kc = j1 - j0;
      stc = gemm_cols(n, j1, u, kc, w_host + (size_t)j0 * ld, ld, tmp, 0, DLA_OP_TRMM);
      if (stc == DLA_OK) stc = d2d(u + (size_t)j0 * n, tmp, sizeof(double) * (size_t)n * kc);
    }
    (void)hipStreamSynchronize(st);          // before tmp goes out of scope
    return stc;
  }

  // ---- what the three Ritz sweeps (ritz_kernel, ritz2_kernel, davidson_expand_kernel) share on the host
  // the open wanted roots: f(j) for every j < min(n_res, cap) that `skip` does not close; returns their number
  template <typename F> static int for_open_roots(int n_res, int cap, const int* skip, F&& f)
  {
    int nact = 0;
    for (int j = 0; j < n_res && j < cap; ++j)
      if (!(skip && skip[j])) { f(j); ++nact; }
    return nact;
  }
  // Everything behind the pack step.  p: the sweep's plan (blocks, ncol, nslots, small_doubles(), name()); a: its arguments, which
  // get their block partials here; bytes, flops: what the sweep is booked with; ladder: launches the plan's instance of a (under the
  // sweep's Scope) and returns a status.  out[2 j], out[2 j + 1]: sum and maximum over the rows of column j < n_res -- the sums and
  // all ranks' maxima come home in one collective (reference :1730-1731 are two reductions).
  template <typename PLAN, typename ARGS, typename LADDER>
  int ritz_sweep_tail(const PLAN& p, ARGS& a, double bytes, double flops, int n_res, double* out, LADDER&& ladder)
  {
    int stc = ensure_partial(sizeof(double) * (size_t)p.blocks * p.ncol * 2);
    if (stc) return stc;
    stc = ensure_small(sizeof(double) * p.small_doubles());
    if (stc) return stc;
    a.red = d_partial;
    {
      Scope s(this, DLA_OP_RITZ, bytes, flops, p.name());
      stc = ladder();
      if (stc) return stc;
    }
    {
      Scope s2(this, DLA_OP_RITZ, 0.0, 0.0, "ritz_reduce_kernel");
      DLA_LAUNCH(ritz_reduce_kernel, dim3(p.ncol), dim3(256), 0, st, (const double*)d_partial, p.blocks, p.ncol, d_small,
                         h_small.dev(), p.nslots, local_only ? 0 : rank);
    }
    HIPCHK(hipGetLastError());
    stc = sum_to_host((int)p.small_doubles(), 0);
    if (stc) return stc;
    for (int j = 0; j < n_res; ++j) {
      double mx = 0.0;
      for (int s = 0; s < p.nslots; ++s) mx = std::max(mx, h_small[p.ncol + s * p.ncol + j]);
      out[2 * j] = h_small[j]; out[2 * j + 1] = mx;
    }
    return DLA_OK;
  }

  int ritz_residual(int n, int l, int m, const double* v, const double* av, const double* y_host, int ldy,
                    const double* eig, int n_res, const int* skip, double* evec, double* r, double* avy,
                    double* out) override
  {
    return with_lds_retry([&]() { return ritz_residual_once(n, l, m, v, av, y_host, ldy, eig, n_res, skip, evec, r, avy, out); });
  }
  bool ritz_p_declined = false;
  // the sweep with k2 extra products (Engine::ritz_residual_p): one pass when [Y | C2] fits five column tiles and the LDS copy,
  // otherwise the Ritz step and two panel products
  int ritz_residual_p(int n, int l, int m, const double* v, const double* av, const double* y_host, int ldy,
                      const double* eig, int n_res, const int* skip, double* evec, double* r, double* avy,
                      double* out, int k2, const double* c2_host, int ldc2, double* p2, double* ap2) override
  {
    if (k2 <= 0) return ritz_residual(n, l, m, v, av, y_host, ldy, eig, n_res, skip, evec, r, avy, out);
    const int ktot = (m + k2 + 15) / 16, l4 = ((l + 3) / 4) * 4;
    const bool one_pass = on_16_bytes(n, v, av, evec, r, avy, p2, ap2) && m <= 48 && ktot <= 5 && !knobs.ritz_p_separate() &&
                          sizeof(double) * (size_t)l4 * 16 * ktot <= ritz_dyn_limit(env(), ktot);
    if (!one_pass) return Engine::ritz_residual_p(n, l, m, v, av, y_host, ldy, eig, n_res, skip, evec, r, avy, out, k2, c2_host, ldc2, p2, ap2);
    // [Y | C2] as one coefficient block
    std::vector<double> yc((size_t)l * (m + k2));
    for (int j = 0; j < m; ++j) std::memcpy(&yc[(size_t)j * l], y_host + (size_t)j * ldy, sizeof(double) * l);
    for (int j = 0; j < k2; ++j) std::memcpy(&yc[(size_t)(m + j) * l], c2_host + (size_t)j * ldc2, sizeof(double) * l);
    ritz_p_declined = false;
    int st = with_lds_retry([&]() { return ritz_residual_once(n, l, m, v, av, yc.data(), l, eig, n_res, skip, evec, r, avy, out, k2, p2, ap2); });
    if (st != DLA_OK && ritz_p_declined)      // (the LDS request was refused and the retry found the block too large: nothing ran)
      return Engine::ritz_residual_p(n, l, m, v, av, y_host, ldy, eig, n_res, skip, evec, r, avy, out, k2, c2_host, ldc2, p2, ap2);
    return st;
  }
  int ritz_residual_once(int n, int l, int m, const double* v, const double* av, const double* y_host, int ldy,
                         const double* eig, int n_res, const int* skip, double* evec, double* r, double* avy,
                         double* out, int k2 = 0, double* p2 = nullptr, double* ap2 = nullptr)
  {
    if (m > 48) {
      // more than three 16-column tiles: blocks of 48 columns, each a sweep of its own over V and AV
      for (int j0 = 0; j0 < m; j0 += 48) {
        const int mc = std::min(48, m - j0);
        const int nr = std::max(0, std::min(n_res - j0, mc));
        std::vector<double> o2((size_t)2 * std::max(nr, 1), 0.0);
        int stq = ritz_residual(n, l, mc, v, av, y_host + (size_t)j0 * ldy, ldy, eig + j0, nr, skip ? skip + j0 : nullptr,
                                evec ? evec + (size_t)j0 * n : nullptr, r + (size_t)j0 * n, avy ? avy + (size_t)j0 * n : nullptr, o2.data());
        if (stq) return stq;
        for (int j = 0; j < nr; ++j) { out[2 * (j0 + j)] = o2[2 * j]; out[2 * (j0 + j) + 1] = o2[2 * j + 1]; }
      }
      return DLA_OK;
    }
    const int nslots = (local_only || nranks < 1) ? 1 : nranks;
    const RitzPlan p = ritz_plan(env(), n, l, m, k2, on_16_bytes(n, v, av, evec, r, avy, p2, ap2), nslots);
    if (!p.fits) {
      if (k2 > 0) { ritz_p_declined = true; err = "ritz sweep with extra products: coefficient block beyond the LDS limit"; return DLA_ERR_RUNTIME; }
      // Y does not fit the LDS copy in one piece (wide block times deep subspace, e.g. 37 columns x 20 blocks): form the
      // two products with the chunked panel GEMM, then run the fused sweep on the n x m results with Y = identity
      // for the residual correction and the norms (same arithmetic for r; evec and AV Y are plain products)
      void* tmp = nullptr;
      void* ev_tmp = nullptr;
      int stf = alloc(sizeof(double) * (size_t)n * m, &tmp);
      if (stf) return stf;
      if (!evec) {                         // (the caller does not want the vectors, this path needs them as an operand)
        stf = alloc(sizeof(double) * (size_t)n * m, &ev_tmp);
        if (stf) { (void)free_(tmp); return stf; }
        evec = (double*)ev_tmp;
      }
      stf = gemm(n, l, av, m, y_host, ldy, (double*)tmp, 0);
      if (!stf) stf = gemm(n, l, v, m, y_host, ldy, evec, 0);
      if (!stf && avy) stf = d2d(avy, tmp, sizeof(double) * (size_t)n * m);
      if (!stf) {
        std::vector<double> ident((size_t)m * m, 0.0);
        for (int j = 0; j < m; ++j) ident[(size_t)j * m + j] = 1.0;
        stf = ritz_residual(n, m, m, evec, (const double*)tmp, ident.data(), m, eig, n_res, skip, evec, r, nullptr, out);
      }
      int stq = free_(tmp);
      if (ev_tmp) { const int stq2 = free_(ev_tmp); if (!stq) stq = stq2; }
      return stf ? stf : stq;
    }
    const int stc = upload_packed(y_host, ldy, 0, l, m + k2, p.kt, p.l4);
    if (stc) return stc;
    RitzArgs a{};
    a.v = v; a.av = av; a.cpk = d_cpk; a.evec = evec; a.r = r; a.avy = avy; a.p2 = p2; a.ap2 = ap2; a.k2 = k2;
    a.n = n; a.l = l; a.l4 = p.l4; a.k = m;
    const int nact = for_open_roots(n_res, 48, skip, [&](int j) { a.theta[j] = eig[j]; a.active[j] = 1; });
    // (flops: the two Ritz products and, with extra columns, the two panel products they replace)
    return ritz_sweep_tail(p, a, 8.0 * n * (2.0 * l + ((avy ? 2.0 : 1.0) + (evec ? 1.0 : 0.0)) * m + 2.0 * k2),
                           4.0 * (double)n * l * (m + k2) + 5.0 * (double)n * nact, n_res, out, [&]() {
      // (with extra products the 16-byte path is guaranteed by the caller, ritz_residual_p)
      int r_ = DLA_OK;
      if (!first_instance<std::size(RITZ_INSTANCES)>([&](auto i) {
            constexpr RitzInstance s = RITZ_INSTANCES[decltype(i)::value];
            if (p.kt != s.kt || (p.vec2 ? 2 : 1) != s.vec || p.pipe != s.pipe || p.qt != s.qt || p.xp != s.xp) return false;
            auto kfn = ritz_kernel<s.kt, s.vec, 3, s.pipe, s.qt, s.xp>;
            if (!raise_lds((const void*)kfn, p.lds, ritz_static_lds(p.kt))) r_ = DLA_ERR_RUNTIME;
            else DLA_LAUNCH(kfn, dim3(p.blocks), dim3(256), p.lds, st, a);
            return true;
          })) {
        err = "ritz: no kernel instance";
        return (int)DLA_ERR_RUNTIME;
      }
      return r_;
    });
  }

  // ---- the Ritz sweep that also forms and measures the next block (davidson_expand_kernel, Engine::ritz_expand)
  // What it measured is remembered until the chain that orthogonalises the block starts: ortho_chain_begin on the same panel, block
  // and widths takes the partials in d_rxpart in the place of its OP_GRAMX sweep (gram_wp_once).  Any launch in between -- another
  // Ritz sweep, a preconditioner, a product, a copy -- drops the record (Scope, zero, d2d, h2d): the block may have been rewritten.
  DeviceBuffer<double> d_rxpart;     // the Gram partials of the last fused sweep: nothing else writes here
  struct Measured {
    bool valid = false;
    const double *x = nullptr, *u = nullptr;
    int n = 0, m = 0, k = 0, blocks = 0, tx = 0;
    double fac = 0.0;
  } measured;
  bool rx_keep = false;              // the launches of the moment belong to the fused sweep itself or to the chain that takes the record
  struct KeepMeasured {              // ... for the life of this guard
    bool& f;
    explicit KeepMeasured(bool& f_) : f(f_) { f = true; }
    ~KeepMeasured() { f = false; }
  };
  long long rx_run = 0, rx_discarded = 0;
  void drop_measured() { if (measured.valid && !rx_keep) { measured.valid = false; ++rx_discarded; } }
  void ritz_expand_counts(long long* run, long long* discarded) override { *run = rx_run; *discarded = rx_discarded; }
  // what the record holds, reduced as the chain would reduce it: [V | U0]^T U0, (m + k) x k; the record stays (tests)
  int ritz_expand_measured(int m, int k, double* c_host, int ldc) override
  {
    if (!measured.valid || m != measured.m || k != measured.k) { err = "ritz_expand_measured: no fused sweep of this shape is on record"; return DLA_ERR_ARG; }
    int stc = ensure_small(sizeof(double) * (size_t)(m + k) * k);
    if (stc) return stc;
    KeepMeasured keep{rx_keep};
    StepOut out;
    stc = reduce_and_sum(DLA_OP_GRAM, d_small, h_small.dev(), measured.blocks, m, k, measured.tx, 1, 1, measured.tx + 1, 1, m + k, out, d_rxpart);
    return stc ? stc : small_result_home(m + k, k, out.mirror_fresh, c_host, ldc);
  }
  // the device-resident diagonal of one of the library's diagonal preconditioners (kind 0 / 1 / 2: the sample operator, the stored
  // sparse operator, the stored dense operator); nullptr: none of n rows has been set up
  const double* precnd_diagonal(int kind, int n)
  {
    if (kind == 0) return (n == syn_n && d_diag) ? (const double*)d_diag : nullptr;
    if (kind == 1) return (n == ops[dla::SPMM_A].n && ops[dla::SPMM_A].diag) ? ops[dla::SPMM_A].diagonal() : nullptr;
    if (kind == 2) return (dense[dla::DENSE_A].n == n && dense[dla::DENSE_A].diag) ? (const double*)dense[dla::DENSE_A].diag : nullptr;
    return nullptr;
  }
  int ritz_expand(int n, int l, int m, const double* v, const double* av, const double* y_host, int ldy, const double* eig, int n_res,
                  const int* skip, double* r, double* out, int precnd_kind, double fac, int first0, int k, double* u0, int* ran) override
  {
    *ran = 0;
    drop_measured();
    if (nranks > 1 || comm || local_only || hook || p2p.on) return DLA_OK;        // (sharded runs keep the plain sweep)
    const double* dg = precnd_diagonal(precnd_kind, n);
    if (!dg || !u0 || !r || k <= 0 || k != m - first0) return DLA_OK;
    const RitzExpandPlan p = ritz_expand_plan(env(), n, l, m, first0, on_16_bytes(n, v, av, r, u0));
    if (!p.fits || (size_t)p.blocks * p.gram_slots * 256 == 0) return DLA_OK;
    const int tx = p.tx;
    bind();
    // (a refused request for LDS lowers the engine's limit, like everywhere; nothing has run, the caller takes the plain sweep)
    bool raised = false;
    first_instance<std::size(RITZ_EXPAND_TILES)>([&](auto i) {
      constexpr int TX = RITZ_EXPAND_TILES[decltype(i)::value];
      if (tx != TX) return false;
      raised = raise_lds((const void*)davidson_expand_kernel<TX>, p.lds);
      return true;
    });
    if (!raised) { lds_retry = false; return DLA_OK; }
    const size_t gp = (size_t)p.blocks * p.gram_slots * 256;
    if (gp > d_rxpart.capacity()) {
      HIPCHK(hipStreamSynchronize(st));
      HIPCHK(d_rxpart.reserve(gp));
    }
    // coefficients Y, [16 tx][16] (one column tile: the plan fits no block beyond 16 columns)
    int stc = upload_packed(y_host, ldy, 0, l, m, 1, 16 * tx);
    if (stc) return stc;
    RitzExpandArgs a{v, av, d_cpk, dg, fac, r, u0, nullptr, d_rxpart, (long long)n, l, m, first0, p.rows == 32 ? 1 : 0, 0u, {}};
    // (open wanted roots only are corrected and measured, as by dla_ritz_residual)
    const int nact = for_open_roots(n_res, m, skip, [&](int j) { a.act |= 1u << j; a.theta[j] = eig[j]; });
    KeepMeasured keep{rx_keep};
    // what the sweep moves and what it stands for: the two Ritz products with the correction and the norms, the diagonal scaling,
    // and X^T U, U^T U of the new block
    stc = ritz_sweep_tail(p, a, 8.0 * n * (2.0 * l + m + k + 1.0),
                          4.0 * (double)n * l * m + 5.0 * (double)n * nact + (double)n * k + 2.0 * (double)n * (l + k) * k, n_res, out, [&]() {
      first_instance<std::size(RITZ_EXPAND_TILES)>([&](auto i) {
        constexpr int TX = RITZ_EXPAND_TILES[decltype(i)::value];
        if (tx != TX) return false;
        DLA_LAUNCH(davidson_expand_kernel<TX>, dim3(p.blocks), dim3(256), p.lds, st, a);
        return true;
      });
      return (int)DLA_OK;
    });
    if (stc) return stc;
    measured = Measured{true, v, u0, n, l, k, p.blocks, tx, fac};
    ++rx_run;
    *ran = 1;
    return DLA_OK;
  }

  // the Ritz sweep with two coefficient blocks (ritz2_kernel); shapes it does not take go through the three-sweep default
  int ritz_residual2(int n, int l, int m, const double* v, const double* av, const double* y1_host, int ldy1,
                     const double* y2_host, int ldy2, const double* eig, int n_res, const int* skip,
                     double* e, double* r, double* t_work, double* junk, double* out) override
  {
    const int nslots = (local_only || nranks < 1) ? 1 : nranks;
    const Ritz2Plan p = ritz2_plan(env(), n, l, m, on_16_bytes(n, v, av, e, r), nslots);
    const int kt = p.kt;
    if (!p.fits)
      return Engine::ritz_residual2(n, l, m, v, av, y1_host, ldy1, y2_host, ldy2, eig, n_res, skip, e, r, t_work, junk, out);
    // [Y1 | Y2] packed as 2 kt tiles: Y2 starts at tile kt
    std::vector<double> yy((size_t)l * (16 * kt + m), 0.0);
    for (int j = 0; j < m; ++j) {
      std::memcpy(&yy[(size_t)j * l], y1_host + (size_t)j * ldy1, sizeof(double) * l);
      std::memcpy(&yy[(size_t)(16 * kt + j) * l], y2_host + (size_t)j * ldy2, sizeof(double) * l);
    }
    const int stc = upload_packed(yy.data(), l, 0, l, 16 * kt + m, 2 * kt, p.l4);
    if (stc) return stc;
    RitzArgs a{};
    a.v = v; a.av = av; a.cpk = d_cpk; a.evec = e; a.r = r;
    a.n = n; a.l = l; a.l4 = p.l4; a.k = m;
    const int nact = for_open_roots(n_res, 48, skip, [&](int j) { a.theta[j] = eig[j]; a.active[j] = 1; });
    // (flops: the two products and the residual correction, as the reference's dgemm pair + daxpy / dnrm2 loop)
    return ritz_sweep_tail(p, a, 8.0 * n * (2.0 * l + 2.0 * m), 4.0 * (double)n * l * m + 5.0 * (double)n * nact, n_res, out, [&]() {
      int r_ = DLA_OK;
      if (!first_instance<std::size(RITZ2_INSTANCES)>([&](auto i) {
            constexpr Ritz2Instance s = RITZ2_INSTANCES[decltype(i)::value];
            if (kt != s.kt || (p.vec2 ? 2 : 1) != s.vec) return false;
            auto kfn = ritz2_kernel<s.kt, s.vec>;
            if (!raise_lds((const void*)kfn, p.lds, 1024)) r_ = DLA_ERR_RUNTIME;
            else DLA_LAUNCH(kfn, dim3(p.blocks), dim3(256), p.lds, st, a);
            return true;
          })) {
        err = "ritz2: no kernel instance";
        return (int)DLA_ERR_RUNTIME;
      }
      return r_;
    });
  }

  int axpy(size_t len, double alpha, const double* x, double* y) override
  {
    Scope s(this, DLA_OP_ELEM, 24.0 * (double)len, 2.0 * (double)len);
    const int blocks = grid_blocks(env(), (long long)len, 256);
    DLA_LAUNCH(axpy_kernel, dim3(blocks), dim3(256), 0, st, len, alpha, x, y);
    HIPCHK(hipGetLastError());
    return DLA_OK;
  }

  // a = b + s c over len doubles (len even), reps times; returns the best GB/s of the repetitions (24 B per element)
  int stream_triad(size_t len, int reps, double* gbps) override
  {
    *gbps = 0.0;
    len &= ~(size_t)1;
    void *pa = nullptr, *pb = nullptr, *pc = nullptr;
    int stc = alloc(sizeof(double) * len, &pa);
    if (!stc) stc = alloc(sizeof(double) * len, &pb);
    if (!stc) stc = alloc(sizeof(double) * len, &pc);
    if (!stc) {
      HIPCHK(hipMemsetAsync(pb, 0, sizeof(double) * len, st));
      HIPCHK(hipMemsetAsync(pc, 0, sizeof(double) * len, st));
      hipEvent_t e0 = get_event(), e1 = get_event();
      // a few launch shapes; the best one is the ceiling quoted
      const int shapes[4][3] = {{1, 4, 8}, {0, 4, 8}, {1, 1, 16}, {1, 2, 4}};     // {non-temporal, unroll, blocks per CU}
      for (int r = 0; r < 4 * (reps + 1); ++r) {    // the first repetition of every shape warms up
        const int* sh = shapes[r / (reps + 1)];
        const int blocks = (int)std::min((size_t)ncu * sh[2], (len / 2 + 255) / 256);
        HIPCHK(hipEventRecord(e0, st));
#define TRIAD(NT, U) DLA_LAUNCH((triad_kernel<NT, U>), dim3(blocks), dim3(256), 0, st, len / 2, 0.5, (const double*)pb, (const double*)pc, (double*)pa)
        if (sh[0] == 1 && sh[1] == 4) TRIAD(1, 4); else if (sh[0] == 0) TRIAD(0, 4); else if (sh[1] == 1) TRIAD(1, 1); else TRIAD(1, 2);
#undef TRIAD
        HIPCHK(hipEventRecord(e1, st));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        if (r % (reps + 1) > 0 && ms > 0.f) *gbps = std::max(*gbps, 24.0 * (double)len / (ms * 1e6));
      }
      ev_pool.push_back(e0); ev_pool.push_back(e1);
    }
    int s1 = free_(pa), s2 = free_(pb), s3 = free_(pc);
    return stc ? stc : (s1 ? s1 : (s2 ? s2 : s3));
  }

  int sumsq(size_t len, const double* x, double* out) override
  {
    const int blocks = (int)std::max((size_t)1, std::min((size_t)ncu * 4, (len + 1023) / 1024));
    int stc = ensure_partial(sizeof(double) * blocks);
    if (stc) return stc;
    {
      Scope s(this, DLA_OP_ELEM, 8.0 * (double)len, 2.0 * (double)len);
      DLA_LAUNCH(sumsq_kernel, dim3(blocks), dim3(256), 0, st, len, x, d_partial);
      DLA_LAUNCH(sum_partials_kernel, dim3(1), dim3(256), 0, st, (const double*)d_partial, blocks, d_small, h_small.dev());
    }
    HIPCHK(hipGetLastError());
    stc = sum_to_host(1, 0);
    if (stc) return stc;
    *out = h_small[0];
    return DLA_OK;
  }

  int random_fill(int n, int m, double* evec, long long row0, unsigned long long seed, double offset, long long support_rows) override
  {
    Scope s(this, DLA_OP_ELEM, 8.0 * (double)n * m, 0.0);
    const size_t total = (size_t)n * m;
    const int blocks = grid_blocks(env(), (long long)total, 256);
    DLA_LAUNCH(random_fill_kernel, dim3(blocks), dim3(256), 0, st, (long long)n, m, evec, row0, seed, offset, support_rows);
    HIPCHK(hipGetLastError());
    return DLA_OK;
  }

  // ---- the stored sparse matrices (ELLPACK; sliced ELLPACK below)
  // Everything ONE stored sparse matrix consists of.  The context holds six, ops[SPMM_A .. SPMM_SMD] (dla_internal.h says what they
  // are and what ties them together); the set-up, refresh, info and launch functions below take the one they act on, so all have
  // independent storage and independent formats and every product comes from the code that forms A's.
  struct SparseOp {
    DeviceBuffer<int> col; DeviceBuffer<double> val, diag;   // ELLPACK blocks, or the slices followed by the CSR tail; diag[n]
    int n = 0, w = 0;                  // w: ELLPACK width (0 for the sliced format)
    int fmt = -1;                      // DLA_SPMM_ELL / DLA_SPMM_SELL: what the blocks hold; -1 while nothing is stored
    long long nnz = 0, sell_stored = 0, sell_long_entries = 0;
    int sell_slices = 0, sell_long_rows = 0;
    int sell_long_segments = 0, sell_multi_rows = 0, sell_multi_segments = 0;   // the tail's segments (dla::SellLayout)
    DeviceBuffer<long long> sell_ptr, seg_ptr;
    DeviceBuffer<int> sell_perm, long_row, seg_row, seg_part, multi_row, part_ptr;
    DeviceBuffer<double> long_part;    // partial sums of the rows of more than one segment: multi_segments x m, grown by the product
    // what only a refresh of the values reads (refresh_dev): the caller's row pointers [n + 1] and the tail rows' offsets [long_rows + 1]
    DeviceBuffer<long long> rowptr, long_ptr;
    // The device view: the typed const pointers the product kernels read, with their counts.  The tail's entries follow the slices' in
    // the shared blocks: that offset is formed here and nowhere else.
    struct Ell { int w; const int* col; const double* val; };
    struct Slices { int count; const long long* ptr; const int *perm, *col; const double* val; };
    struct Tail {
      int rows, segments, multi_rows;
      const long long *long_ptr, *seg_ptr;
      const int *long_row, *seg_row, *seg_part, *multi_row, *part_ptr, *col;
      const double* val;
    };
    Ell ell() const { return {w, col, val}; }
    Slices slices() const { return {sell_slices, sell_ptr, sell_perm, col, val}; }
    Tail tail() const
    {
      return {sell_long_rows, sell_long_segments, sell_multi_rows, long_ptr, seg_ptr, long_row, seg_row, seg_part, multi_row, part_ptr,
              col + sell_stored, val + sell_stored};
    }
    const double* diagonal() const { return diag; }
    // give the device blocks back (the caller has waited for the stream)
    void drop()
    {
      col.reset(); val.reset(); diag.reset(); sell_ptr.reset(); seg_ptr.reset(); sell_perm.reset(); long_row.reset();
      seg_row.reset(); seg_part.reset(); multi_row.reset(); part_ptr.reset(); long_part.reset(); rowptr.reset(); long_ptr.reset();
      n = w = 0; fmt = -1; nnz = sell_stored = sell_long_entries = 0; sell_slices = sell_long_rows = 0;
      sell_long_segments = sell_multi_rows = sell_multi_segments = 0;
    }
  };
  SparseOp ops[dla::SPMM_SLOTS];
  // The words a message about a slot needs: what the slot is called, what is said while it is empty and beside a row-sharded A, and
  // the name of each public entry that reaches it.  quoted_*: a refusal of the shared set-up / refresh code is passed on behind the
  // entry's (and a part's) name; whole: the calls that are refused while A is row-sharded.  The differences between the rows are
  // what callers have read since each family of entries was added.
  enum SlotCall : unsigned { CALL_SETUP = 1, CALL_REFRESH = 2, CALL_SHARD = 4, NEED_STORED = 8 };
  struct SlotWords {
    const char *noun, *missing, *sharded;
    const char *setup, *setup_dev, *refresh, *info, *mul;
    bool quoted_host, quoted_dev;
    unsigned whole;
  };
  static const SlotWords& words(int slot)
  {
#define LR_WORDS(P, SUM) {"part " P " (" SUM ")", "part " P " (" SUM ") has not been set up", "row-sharded linear-response parts are", "spmm_setup_lr_csr", \
                          "spmm_setup_lr_csr_dev", "spmm_refresh_lr_values_dev", "spmm_lr_info", "spmm_" P "mul", true, true, CALL_SETUP | CALL_REFRESH}
    static const SlotWords table[dla::SPMM_SLOTS] = {
      {"operator", "no operator has been set up", "", "spmm_setup_csr_fmt", "spmm_setup_csr_dev", "spmm_refresh_values_dev", "spmm_info",
       "spmm_matvec", false, false, CALL_REFRESH},
      {"metric", "no metric has been set up", "a row-sharded metric is", "spmm_setup_metric_csr", "spmm_setup_csr_dev", "spmm_refresh_values_dev",
       "spmm_metric_info", "spmm_bvec", true, false, CALL_SETUP},
      LR_WORDS("apb", "A+B"), LR_WORDS("amb", "A-B"), LR_WORDS("spd", "S+D"), LR_WORDS("smd", "S-D")};
#undef LR_WORDS
    // (a number out of range is refused in the words of the entries that take such a number)
    return table[slot == dla::SPMM_NO_PART ? dla::SPMM_APB : (slot < 0 || slot >= dla::SPMM_SLOTS) ? dla::SPMM_A : slot];
  }
  // "<entry>: " or "<entry>, part apb (A+B): " in front of a quoted refusal
  static std::string quote(int slot, const char* entry)
  {
    return std::string(entry) + (slot >= dla::SPMM_APB ? std::string(", ") + words(slot).noun : std::string()) + ": ";
  }
  // The one place that decides whether a call on a slot is admitted (call: one SlotCall, with NEED_STORED where the slot must hold a
  // matrix): the slot exists; while A is row-sharded B and the parts are refused, and so is a refresh of A; the sharded set-up
  // (CALL_SHARD, slot SPMM_A) is refused while B or a part is stored.  Leaves the refusal in err.
  int admit(int slot, const char* entry, unsigned call)
  {
    const std::string who = std::string(entry) + ": ";
    if (slot < 0 || slot >= dla::SPMM_SLOTS) {
      err = who + (slot == dla::SPMM_NO_PART ? "part must be 0 (A+B), 1 (A-B), 2 (S+D) or 3 (S-D)" : "which must be 0 (the operator) or 1 (the metric)");
      return DLA_ERR_ARG;
    }
    const SlotWords& w = words(slot);
    if (call & CALL_SHARD) {
      for (int s = dla::SPMM_SLOTS - 1; s > dla::SPMM_A; --s) {
        if (ops[s].fmt < 0) continue;
        err = who + (s == dla::SPMM_B ? "this context holds a metric (dla_spmm_setup_metric_csr), and a row-sharded metric is not supported; drop it first"
                                      : "this context holds linear-response parts (dla_spmm_setup_lr_csr), and row-sharded parts are not supported; drop them first (dla_spmm_drop_lr)");
        return DLA_ERR_ARG;
      }
    }
    if (shard.on && (call & w.whole) && slot != dla::SPMM_A) {
      err = who + "the operator of this context is row-sharded, and " + w.sharded + " not supported";
      return DLA_ERR_ARG;
    }
    if ((call & NEED_STORED) && ops[slot].fmt < 0) { err = who + w.missing; return DLA_ERR_ARG; }
    if (shard.on && (call & w.whole)) { err = who + "the operator of this context is row-sharded"; return DLA_ERR_ARG; }
    return DLA_OK;
  }
  // A on a row shard (spmm_setup_sharded; A only): whether it is, and the exchange with the neighbouring ranks.  The one place that
  // answers "is A sharded" (admit above goes by it).
  struct RowShard {
    bool on = false;
    int halo = 0;                      // rows exchanged with each neighbour
    DeviceBuffer<double> d_halo;
    std::vector<double> h_halo;        // host mirror for the hook transport
    // A is whole again; the exchange buffers only grow, like the operator's blocks (upload_ell)
    void drop() { on = false; halo = 0; }
  } shard;
  // replace a matrix on the device (both ELLPACK set-up routines end here); the caller has bound the device.  The arrays only grow:
  // a smaller matrix after a larger one keeps the larger blocks (the kernels go by n / w); the same holds for synth_setup
  int upload_ell(SparseOp& op, const std::vector<int>& col, const std::vector<double>& val, const std::vector<double>& diag)
  {
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(op.col.reserve(col.size()));
    HIPCHK(op.val.reserve(val.size()));
    HIPCHK(op.diag.reserve(diag.size()));
    HIPCHK(hipMemcpy(op.col, col.data(), sizeof(int) * col.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(op.val, val.data(), sizeof(double) * val.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(op.diag, diag.data(), sizeof(double) * diag.size(), hipMemcpyHostToDevice));
    return DLA_OK;
  }
  // (the matrix has passed dla::spmm_csr_check; w: its widest row)
  int setup_ell(SparseOp& op, int n, int w, const long long* rowptr, const int* colind, const double* values)
  {
    std::vector<int> col((size_t)w * n);
    std::vector<double> val((size_t)w * n, 0.0), diag((size_t)n, 0.0);
    for (int i = 0; i < n; ++i) {
      const long long p0 = rowptr[i], p1 = rowptr[i + 1];
      for (int q = 0; q < w; ++q) {
        const bool in = p0 + q < p1;
        const int cj = in ? colind[p0 + q] : i;
        col[(size_t)q * n + i] = cj;
        val[(size_t)q * n + i] = in ? values[p0 + q] : 0.0;
        if (in && cj == i) diag[i] += values[p0 + q];
      }
    }
    HIPCHK(hipSetDevice(device));
    { const int stc = upload_ell(op, col, val, diag); if (stc) return stc; }
    HIPCHK(op.rowptr.reserve((size_t)n + 1));
    HIPCHK(hipMemcpy(op.rowptr, rowptr, sizeof(long long) * ((size_t)n + 1), hipMemcpyHostToDevice));
    op.n = n; op.w = w;
    op.fmt = DLA_SPMM_ELL; op.nnz = rowptr[n] - rowptr[0];
    return DLA_OK;
  }
  // ---- ... as sliced ELLPACK with a CSR tail (dla::sell_build).  The slices and the tail share the ELLPACK blocks -- columns and
  // values of the tail follow the `stored` padded entries of the slices -- so either format replaces the other in place.
  static constexpr int SELL_MC = 8, LONG_MC = 4;   // right-hand sides per load of a matrix entry (sell_spmm_kernel / csr_long_segments_kernel)
  // room for a sliced layout in op's blocks and the layout's small tables (everything but the entries and the diagonal); rowptr: host.
  // The caller has bound the device and waited for the stream.
  static hipError_t up(void* dst, const void* src, size_t bytes) { return bytes ? hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) : hipSuccess; }
  int place_sell(SparseOp& op, int n, const dla::SellLayout& L, const long long* rowptr)
  {
    const size_t tot = (size_t)(L.stored + L.long_entries);
    HIPCHK(op.col.reserve(tot));
    HIPCHK(op.val.reserve(tot));
    HIPCHK(op.diag.reserve((size_t)n));
    HIPCHK(op.rowptr.reserve((size_t)n + 1));
    { const int stc = place_sell_tables(op, n, L); if (stc) return stc; }
    HIPCHK(up(op.rowptr, rowptr, sizeof(long long) * ((size_t)n + 1)));
    return DLA_OK;
  }
  // ... the tables alone: what a layout consists of besides its entries (the transposed index has a layout and other entries)
  int place_sell_tables(SparseOp& op, int n, const dla::SellLayout& L)
  {
    const size_t nl = L.long_row.size(), ns = L.seg_row.size(), nm = L.multi_row.size();
    HIPCHK(op.sell_ptr.reserve(L.slice_ptr.size()));
    HIPCHK(op.sell_perm.reserve((size_t)n));
    HIPCHK(op.long_row.reserve(std::max<size_t>(1, nl)));
    HIPCHK(op.seg_ptr.reserve(ns + 1));
    HIPCHK(op.seg_row.reserve(std::max<size_t>(1, ns)));
    HIPCHK(op.seg_part.reserve(std::max<size_t>(1, ns)));
    HIPCHK(op.multi_row.reserve(std::max<size_t>(1, nm)));
    HIPCHK(op.part_ptr.reserve(nm + 1));
    HIPCHK(op.long_ptr.reserve(nl + 1));
    HIPCHK(up(op.sell_ptr, L.slice_ptr.data(), sizeof(long long) * L.slice_ptr.size()));
    HIPCHK(up(op.sell_perm, L.perm.data(), sizeof(int) * (size_t)n));
    HIPCHK(up(op.long_row, L.long_row.data(), sizeof(int) * nl));
    HIPCHK(up(op.seg_ptr, L.seg_ptr.data(), sizeof(long long) * (ns + 1)));
    HIPCHK(up(op.seg_row, L.seg_row.data(), sizeof(int) * ns));
    HIPCHK(up(op.seg_part, L.seg_part.data(), sizeof(int) * ns));
    HIPCHK(up(op.multi_row, L.multi_row.data(), sizeof(int) * nm));
    HIPCHK(up(op.part_ptr, L.part_ptr.data(), sizeof(int) * (nm + 1)));
    HIPCHK(up(op.long_ptr, L.long_ptr.data(), sizeof(long long) * (nl + 1)));
    return DLA_OK;
  }
  // op holds the sliced layout L from now on
  static void hold_sell(SparseOp& op, int n, const dla::SellLayout& L)
  {
    op.n = n; op.w = 0;
    op.fmt = DLA_SPMM_SELL; op.nnz = L.nnz; op.sell_stored = L.stored; op.sell_long_entries = L.long_entries;
    op.sell_slices = L.slices; op.sell_long_rows = (int)L.long_row.size();
    op.sell_long_segments = L.long_segments; op.sell_multi_rows = (int)L.multi_row.size(); op.sell_multi_segments = L.multi_segments;
  }
  // entry: the name the checks speak under
  int setup_fmt(SparseOp& op, int n, const long long* rowptr, const int* colind, const double* values, int format, const char* entry)
  {
    int w = 0; long long nnz = 0;
    { const int stc = dla::spmm_csr_check(n, rowptr, colind, values, format, &w, &nnz, err, entry); if (stc) return stc; }
    if (dla::spmm_pick_format(format, w, n, nnz) == DLA_SPMM_ELL) return setup_ell(op, n, w, rowptr, colind, values);
    dla::SellLayout L;
    dla::sell_build(n, rowptr, colind, values, L);
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamSynchronize(st));
    { const int stc = place_sell(op, n, L, rowptr); if (stc) return stc; }
    HIPCHK(up(op.col, L.col.data(), sizeof(int) * L.col.size()));
    HIPCHK(up(op.val, L.val.data(), sizeof(double) * L.val.size()));
    HIPCHK(up(op.col + L.stored, L.long_col.data(), sizeof(int) * L.long_col.size()));
    HIPCHK(up(op.val + L.stored, L.long_val.data(), sizeof(double) * L.long_val.size()));
    HIPCHK(up(op.diag, L.diag.data(), sizeof(double) * (size_t)n));
    hold_sell(op, n, L);
    return DLA_OK;
  }
  // ---- ... and from CSR arrays in DEVICE memory (dla_spmm_setup_csr_dev), with the result of setup_fmt for the same arrays: the row
  // pointers come to the host (8 (n + 1) bytes, the only transfer that grows with n), where the checks on them, the choice of the
  // format and dla::sell_layout run as they do above; the entries never leave the device (the kernels beside ell_spmm_kernel).
  // Order of the launches: csr_check_cols_kernel runs alone and is waited for; while a column is out of range nothing else is
  // launched, so no kernel ever indexes with an unchecked column (the fill kernels only copy columns, the product gathers with
  // them) and nothing of the slot has been touched -- not even grown, which would discard its blocks.  Synchronous: the call
  // returns after the stream has been waited for.  The set-up kernels are not booked into the statistics (the host set-up is not).
  DeviceBuffer<unsigned> d_setup_flag;
  // flag word <- 0 / flag word -> host, behind what is queued on the stream
  int flag_clear()
  {
    HIPCHK(d_setup_flag.reserve(1));
    HIPCHK(hipMemsetAsync(d_setup_flag, 0, sizeof(unsigned), st));
    return DLA_OK;
  }
  int flag_read(unsigned* out)
  {
    HIPCHK(hipMemcpyAsync(out, d_setup_flag, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return DLA_OK;
  }
  // the entries of the caller's arrays into op's blocks (VALS_ONLY: the values alone) and the diagonal, in the format op holds;
  // rowptr (device) and shift as the walkers take them
  template <bool VALS_ONLY>
  int fill_from_device(SparseOp& op, const long long* rowptr, long long shift, const int* colind, const double* values)
  {
    const bool sell = op.fmt == DLA_SPMM_SELL;
    const SpmmSetupPlan p = spmm_setup_plan(env(), op.n, op.nnz, sell ? op.sell_slices : 0, sell ? op.sell_long_segments : 0);
    if (sell) {
      DLA_LAUNCH((sell_fill_kernel<VALS_ONLY>), dim3(p.slice_blocks), dim3(256), 0, st, op.n, op.sell_slices, (const long long*)op.sell_ptr,
                 (const int*)op.sell_perm, rowptr, shift, colind, values, (int*)op.col, (double*)op.val);
      HIPCHK(hipGetLastError());
      if (p.seg_blocks > 0) {
        DLA_LAUNCH((tail_copy_kernel<VALS_ONLY>), dim3(p.seg_blocks), dim3(256), 0, st, op.sell_long_segments, op.sell_stored,
                   (const long long*)op.seg_ptr, (const int*)op.seg_row, (const int*)op.long_row, (const long long*)op.long_ptr, rowptr, shift,
                   colind, values, (int*)op.col, (double*)op.val);
        HIPCHK(hipGetLastError());
      }
    } else {
      DLA_LAUNCH((ell_fill_kernel<VALS_ONLY>), dim3(p.row_blocks), dim3(256), 0, st, op.n, op.w, rowptr, shift, colind, values, (int*)op.col,
                 (double*)op.val);
      HIPCHK(hipGetLastError());
    }
    DLA_LAUNCH(csr_diag_kernel, dim3(p.row_blocks), dim3(256), 0, st, op.n, dla::SELL_LONG_ROW, rowptr, shift, colind, values, (double*)op.diag);
    HIPCHK(hipGetLastError());
    return DLA_OK;
  }
  int setup_dev(SparseOp& op, int n, const long long* rowptr_dev, const int* colind_dev, const double* values_dev, int format)
  {
    if (format != DLA_SPMM_ELL && format != DLA_SPMM_SELL && format != DLA_SPMM_AUTO) { err = "spmm_setup_csr_dev: unknown format"; return DLA_ERR_ARG; }
    if (n <= 0 || !rowptr_dev || !colind_dev || !values_dev) { err = "spmm_setup_csr_dev: bad arguments"; return DLA_ERR_ARG; }
    bind();
    const double t_host = dla::ApiTimer::on() ? dla::ApiTimer::now() : 0.0;
    std::vector<long long> rp((size_t)n + 1);
    HIPCHK(hipMemcpyAsync(rp.data(), rowptr_dev, sizeof(long long) * rp.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));       // (queued products of the slot's previous matrix are done as well)
    int w = 0;
    for (int i = 0; i < n; ++i) {
      if (rp[i + 1] < rp[i]) { err = "spmm_setup_csr_dev: row pointers not ascending"; return DLA_ERR_ARG; }
      if (rp[i + 1] - rp[i] > w) w = (int)std::min<long long>(rp[i + 1] - rp[i], 2147483647LL);
    }
    if (w <= 0) { err = "spmm_setup_csr_dev: empty matrix"; return DLA_ERR_ARG; }
    if (rp[0] < 0) { err = "spmm_setup_csr_dev: bad arguments"; return DLA_ERR_ARG; }      // (the host entry would read in front of its arrays)
    const long long nnz = rp[n] - rp[0];
    const bool sell = dla::spmm_pick_format(format, w, n, nnz) == DLA_SPMM_SELL;
    dla::SellLayout L;
    if (sell) dla::sell_layout(n, rp.data(), L);
    // ($DIAGLIB_AMD_HOSTTIME: what of this call is still host work, for tools/time_spmm_setup.py)
    if (dla::ApiTimer::on()) dla::ApiTimer::add(sell ? "  spmm_setup_csr_dev host part, sell" : "  spmm_setup_csr_dev host part, ell", dla::ApiTimer::now() - t_host);
    // every check that reads the entries, before the first write into the slot (see above)
    {
      const SpmmSetupPlan p = spmm_setup_plan(env(), n, nnz, 0, 0);
      unsigned bad = 0;
      { const int stc = flag_clear(); if (stc) return stc; }
      DLA_LAUNCH(csr_check_cols_kernel, dim3(p.entry_blocks), dim3(256), 0, st, nnz, colind_dev + rp[0], n, (unsigned*)d_setup_flag);
      HIPCHK(hipGetLastError());
      { const int stc = flag_read(&bad); if (stc) return stc; }
      if (bad) { err = "spmm_setup_csr_dev: column index out of range"; return DLA_ERR_ARG; }
    }
    if (sell) {
      { const int stc = place_sell(op, n, L, rp.data()); if (stc) return stc; }
      hold_sell(op, n, L);
    } else {
      HIPCHK(op.col.reserve((size_t)w * n));
      HIPCHK(op.val.reserve((size_t)w * n));
      HIPCHK(op.diag.reserve((size_t)n));
      HIPCHK(op.rowptr.reserve((size_t)n + 1));
      HIPCHK(hipMemcpy(op.rowptr, rp.data(), sizeof(long long) * rp.size(), hipMemcpyHostToDevice));
      op.n = n; op.w = w;
      op.fmt = DLA_SPMM_ELL; op.nnz = nnz;
    }
    { const int stc = fill_from_device<false>(op, rowptr_dev, 0, colind_dev, values_dev); if (stc) return stc; }
    HIPCHK(hipStreamSynchronize(st));       // (the caller may free or overwrite its arrays from here on)
    return DLA_OK;
  }
  // new values for the pattern a slot holds: everything is compared in a read-only pass (pattern_compare_kernel) that is waited
  // for before the first value is written; the stored format stays (AUTO is not decided again).  Synchronous like the set-up.
  int spmm_refresh_dev(int slot, int n, const long long* rowptr_dev, const int* colind_dev, const double* values_dev) override
  {
    const SlotWords& w = words(slot);
    { const int stc = admit(slot, w.refresh, CALL_REFRESH | NEED_STORED); if (stc) return stc; }
    const int stc = refresh_dev(ops[slot], n, rowptr_dev, colind_dev, values_dev);
    if (slot == dla::SPMM_A) cheb.upper_valid = cheb.off_valid = false;
    if (slot == dla::SPMM_B) cheb.offb_valid = false;
    if (stc == DLA_ERR_ARG && w.quoted_dev) err = quote(slot, w.refresh) + err;
    return stc;
  }
  // (op holds a matrix and is not row-sharded)
  int refresh_dev(SparseOp& op, int n, const long long* rowptr_dev, const int* colind_dev, const double* values_dev)
  {
    if (n <= 0 || !rowptr_dev || !colind_dev || !values_dev) { err = "spmm_refresh_values_dev: bad arguments"; return DLA_ERR_ARG; }
    if (n != op.n) { err = "spmm_refresh_values_dev: n = " + std::to_string(n) + " differs from the stored " + std::to_string(op.n); return DLA_ERR_ARG; }
    bind();
    long long ends[2] = {0, 0}, first_stored = 0;
    HIPCHK(hipMemcpyAsync(&ends[0], rowptr_dev, sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&ends[1], rowptr_dev + n, sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&first_stored, (const long long*)op.rowptr, sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ends[0] < 0 || ends[1] - ends[0] != op.nnz) {
      err = "spmm_refresh_values_dev: " + std::to_string(ends[1] - ends[0]) + " entries, the stored matrix has " + std::to_string(op.nnz);
      return DLA_ERR_ARG;
    }
    // (the stored row pointers index the caller's arrays from here on: rowptr[i] + shift, all inside the nnz entries just checked)
    const long long shift = ends[0] - first_stored;
    const bool sell = op.fmt == DLA_SPMM_SELL;
    const SpmmSetupPlan p = spmm_setup_plan(env(), n, op.nnz, sell ? op.sell_slices : 0, sell ? op.sell_long_segments : 0);
    const int blocks = std::max(p.row_blocks, std::max(p.slice_blocks, p.seg_blocks));
    unsigned bad = 0;
    { const int stc = flag_clear(); if (stc) return stc; }
#define CMP(S) DLA_LAUNCH((pattern_compare_kernel<S>), dim3(blocks), dim3(256), 0, st, n, op.w, op.sell_slices, op.sell_long_segments, op.sell_stored, \
                          (const long long*)op.sell_ptr, (const int*)op.sell_perm, (const long long*)op.seg_ptr, (const int*)op.seg_row,              \
                          (const int*)op.long_row, (const long long*)op.long_ptr, (const long long*)op.rowptr, shift, rowptr_dev, colind_dev,       \
                          (const int*)op.col, (unsigned*)d_setup_flag)
    if (sell) CMP(true); else CMP(false);
#undef CMP
    HIPCHK(hipGetLastError());
    { const int stc = flag_read(&bad); if (stc) return stc; }
    if (bad) {
      err = (bad & 1u) ? "spmm_refresh_values_dev: the row pointers are not the stored pattern's" : "spmm_refresh_values_dev: the columns are not the stored pattern's";
      return DLA_ERR_ARG;
    }
    { const int stc = fill_from_device<true>(op, (const long long*)op.rowptr, shift, colind_dev, values_dev); if (stc) return stc; }
    HIPCHK(hipStreamSynchronize(st));
    return DLA_OK;
  }
  // from CSR arrays in host or device memory (via: dla::SpmmVia; PLAIN stores ELLPACK and speaks under its own name)
  int spmm_setup(int slot, int via, int n, const long long* rowptr, const int* colind, const double* values, int format) override
  {
    const SlotWords& w = words(slot);
    const bool dev = via == dla::SPMM_VIA_DEVICE, plain = via == dla::SPMM_VIA_PLAIN, quoted = dev ? w.quoted_dev : w.quoted_host;
    const char* entry = plain ? "spmm_setup_csr" : dev ? w.setup_dev : w.setup;
    { const int stc = admit(slot, entry, CALL_SETUP); if (stc) return stc; }
    const int stc = dev ? setup_dev(ops[slot], n, rowptr, colind, values, format)
                        : setup_fmt(ops[slot], n, rowptr, colind, values, plain ? (int)DLA_SPMM_ELL : format, quoted ? "spmm_setup_csr_fmt" : entry);
    if (stc == DLA_ERR_ARG && quoted) err = quote(slot, entry) + err;
    if (slot == dla::SPMM_A) cheb.upper_valid = cheb.off_valid = false;
    if (slot == dla::SPMM_B) cheb.offb_valid = false;
    if (!stc && slot == dla::SPMM_A) { shard.drop(); tidx.drop(); }     // (a new pattern: the transposed index of the old one goes)
    return stc;
  }
  int op_info(const SparseOp& op, struct dla_spmm_info* out) const
  {
    const bool sell = op.fmt == DLA_SPMM_SELL;
    struct dla_spmm_info zero{};    // (elaborated: the function of the same name hides the struct)
    *out = zero;
    out->format = op.fmt; out->n = op.n; out->nnz = op.nnz;
    out->stored = sell ? op.sell_stored : (long long)op.w * op.n;
    out->device_bytes = 12 * out->stored + 8 * (long long)op.n;
    if (sell) {
      out->slice_rows = dla::SELL_C; out->sort_window = dla::SELL_SIGMA; out->long_row_threshold = dla::SELL_LONG_ROW;
      out->slices = op.sell_slices; out->long_rows = op.sell_long_rows; out->long_entries = op.sell_long_entries;
      out->long_segment_entries = dla::SELL_LONG_SEG; out->long_segments = op.sell_long_segments; out->multi_segments = op.sell_multi_segments;
      // (the tail's tables: long_row; seg_ptr, seg_row, seg_part; multi_row, part_ptr)
      out->device_bytes += 12 * op.sell_long_entries + 4 * (long long)op.n + 8 * ((long long)op.sell_slices + 1) + 4 * (long long)op.sell_long_rows +
                           16 * (long long)op.sell_long_segments + 8 + 8 * (long long)op.sell_multi_rows + 4;
    }
    return DLA_OK;
  }
  int spmm_info(int slot, struct dla_spmm_info* out) override
  {
    { const int stc = admit(slot, words(slot).info, NEED_STORED); if (stc) return stc; }
    return op_info(ops[slot], out);
  }
  // (nothing stored: neither the device nor the stream is touched)
  int spmm_drop(int first, int last) override
  {
    bool any = false;
    for (int s = first; s <= last; ++s) any = any || ops[s].fmt >= 0 || ops[s].col;
    if (!any) return DLA_OK;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamSynchronize(st));     // (products of these slots may still be queued)
    for (int s = first; s <= last; ++s) ops[s].drop();
    if (first <= dla::SPMM_A && dla::SPMM_A <= last) tidx.drop();
    if (first <= dla::SPMM_A && dla::SPMM_A <= last) cheb.upper_valid = cheb.off_valid = false;
    if (first <= dla::SPMM_B && dla::SPMM_B <= last) cheb.offb_valid = false;
    return DLA_OK;
  }
  // The ELLPACK width ladder, spelled once for the product, the Chebyshev step and the product on a row shard: launch(W) for the
  // narrowest instance that keeps w (column, value) pairs in registers; W = 0 loops over any width.
  static constexpr int ELL_WIDTHS[] = {4, 8, 16, 32, 0};
  template <class F>
  static void ell_width(int w, F&& launch)
  {
    first_instance<std::size(ELL_WIDTHS)>([&](auto i) {
      constexpr int W = ELL_WIDTHS[decltype(i)::value];
      if (W > 0 && w > W) return false;
      launch(std::integral_constant<int, W>{});
      return true;
    });
  }
  // The tail of a sliced product, dst[tail rows] = (the tail of op) x: the segments kernel and, for the rows of more than one segment,
  // the combine kernel; p: their launch shapes and workspace (long_rows_plan).  Runs behind the slices' kernel on the stream.
  int tail_product(SparseOp& op, const LongRowsPlan& p, int n, int m, const double* x, double* dst)
  {
    if (p.part_doubles > op.long_part.capacity()) {
      HIPCHK(hipStreamSynchronize(st));       // (queued products may still use the old block)
      HIPCHK(op.long_part.reserve(p.part_doubles));
    }
    const SparseOp::Tail t = op.tail();
    double* part = op.long_part;
    if (t.segments > 0) {
      DLA_LAUNCH((csr_long_segments_kernel<LONG_MC>), dim3(p.seg_blocks), dim3(256), 0, st, n, m, t.segments, t.seg_ptr, t.seg_row, t.seg_part,
                 t.long_row, t.col, t.val, x, dst, part);
      HIPCHK(hipGetLastError());
    }
    if (p.combine_blocks > 0) {
      DLA_LAUNCH(long_rows_combine_kernel, dim3(p.combine_blocks), dim3(256), 0, st, n, m, t.multi_rows, t.multi_row, t.part_ptr, (const double*)part, dst);
      HIPCHK(hipGetLastError());
    }
    return DLA_OK;
  }
  // ax = (the matrix of op) x on one rank, in the format op holds (n == op.n has been checked)
  int op_matvec(SparseOp& op, int n, int m, const double* x, double* ax)
  {
    if (op.fmt == DLA_SPMM_SELL) {
      const LongRowsPlan p = long_rows_plan(env(), op.sell_long_segments, op.sell_multi_rows, op.sell_multi_segments, m, LONG_MC);
      // (the partial sums are written once and read once)
      Scope s(this, DLA_OP_MATVEC, 12.0 * (double)(op.sell_stored + op.sell_long_entries) + 4.0 * n + 16.0 * (double)n * m + 16.0 * (double)p.part_doubles,
              2.0 * (double)op.nnz * m, op.sell_long_segments > 0 ? p.name() : std::string());
      const SparseOp::Slices sl = op.slices();
      DLA_LAUNCH((sell_spmm_kernel<SELL_MC>), dim3(grid_blocks(env(), sl.count, 4)), dim3(256), 0, st, n, m, sl.count, sl.ptr, sl.perm, sl.col, sl.val, x, ax);
      HIPCHK(hipGetLastError());
      return tail_product(op, p, n, m, x, ax);
    }
    Scope s(this, DLA_OP_MATVEC, 12.0 * (double)op.w * n + 16.0 * (double)n * m, 2.0 * (double)op.w * n * m);
    const SparseOp::Ell e = op.ell();
    const dim3 grid(grid_blocks(env(), n, 256));
    ell_width(e.w, [&](auto W) { DLA_LAUNCH((ell_spmm_kernel<decltype(W)::value>), grid, dim3(256), 0, st, n, m, e.w, e.col, e.val, x, ax); });
    HIPCHK(hipGetLastError());
    return DLA_OK;
  }
  // ---- y = A^T x through the transposed index of slot A (the contract: include/diaglib_amd.h, dla_spmm_transpose_prepare; the
  // kernels: beside ell_spmm_t_kernel and stored_positions_kernel).  The index is a layout of its own over the COLUMN lengths of A --
  // the tables of a SparseOp without its entries -- plus (row, pos) per stored entry and its own workspace of partial sums.  It
  // belongs to A's stored pattern: spmm_setup, spmm_setup_csr_sharded and spmm_drop give it up, a refresh of the values keeps it.
  struct TransposeIdx {
    // the index's own layout over the column lengths of A: the tables and counts of a stored matrix, with the source rows where a matrix
    // has its columns (lay.col) and the workspace of partial sums; lay.val, lay.diag and lay.rowptr stay empty
    SparseOp lay;
    DeviceBuffer<int> pos;             // [entries], beside lay.col: where A's stored values hold the entry; -1: padding
    bool held() const { return lay.fmt >= 0; }
    // (the caller has waited for the stream)
    void drop() { lay.drop(); pos.reset(); }
  };
  TransposeIdx tidx;
  int spmm_transpose_prepare(int format) override
  {
    const char* who = "spmm_transpose_prepare: ";
    SparseOp& op = ops[dla::SPMM_A];
    if (op.fmt < 0) { err = std::string(who) + "no operator has been set up"; return DLA_ERR_ARG; }
    if (shard.on) { err = std::string(who) + "the operator of this context is row-sharded, and a transposed index of a row shard is not supported"; return DLA_ERR_ARG; }
    if (format != DLA_SPMM_ELL && format != DLA_SPMM_SELL && format != DLA_SPMM_AUTO) { err = std::string(who) + "unknown format"; return DLA_ERR_ARG; }
    const bool a_sell = op.fmt == DLA_SPMM_SELL;
    const int n = op.n;
    const long long nnz = op.nnz, a_entries = a_sell ? op.sell_stored + op.sell_long_entries : (long long)op.w * n;
    if (a_entries > 2147483647LL) {
      err = std::string(who) + "the operator stores " + std::to_string(a_entries) + " entries, and positions beyond 2147483647 do not fit the index";
      return DLA_ERR_ARG;
    }
    bind();
    HIPCHK(hipStreamSynchronize(st));
    // the temporaries, 24 bytes per entry and the sort's own: released when this function returns
    DeviceBuffer<int> key, ident, erow, epos, key_sorted, sorted;
    DeviceBuffer<long long> colptr;
    DeviceBuffer<char> sort_temp;
    for (DeviceBuffer<int>* b : {&key, &ident, &erow, &epos, &key_sorted, &sorted}) HIPCHK(b->reserve((size_t)nnz));
    HIPCHK(colptr.reserve((size_t)n + 1));
    int key_bits = 1;
    while (key_bits < 31 && (1LL << key_bits) < (long long)n) ++key_bits;
    size_t temp_bytes = 0;
    HIPCHK(dla::sort_pairs_by_key(nullptr, &temp_bytes, key, key_sorted, ident, sorted, (size_t)nnz, key_bits, st));
    HIPCHK(sort_temp.reserve(std::max<size_t>(1, temp_bytes)));
    // one launch over a layout's rows, slices and tail segments at once
    auto walk_blocks = [&](const SparseOp& o) {
      const bool sell = o.fmt == DLA_SPMM_SELL;
      const SpmmSetupPlan p = spmm_setup_plan(env(), n, nnz, sell ? o.sell_slices : 0, sell ? o.sell_long_segments : 0);
      return dim3(std::max(p.row_blocks, std::max(p.slice_blocks, p.seg_blocks)));
    };
#define LAYOUT_OF(O) n, (O).w, (O).sell_slices, (O).sell_long_segments, (O).sell_stored, (const long long*)(O).sell_ptr, (const int*)(O).sell_perm, \
                     (const long long*)(O).seg_ptr, (const int*)(O).seg_row, (const int*)(O).long_row, (const long long*)(O).long_ptr
    if (a_sell) DLA_LAUNCH((stored_positions_kernel<true>), walk_blocks(op), dim3(256), 0, st, LAYOUT_OF(op), (const long long*)op.rowptr, (const int*)op.col,
                           (int*)key, (int*)ident, (int*)erow, (int*)epos);
    else DLA_LAUNCH((stored_positions_kernel<false>), walk_blocks(op), dim3(256), 0, st, LAYOUT_OF(op), (const long long*)op.rowptr, (const int*)op.col,
                    (int*)key, (int*)ident, (int*)erow, (int*)epos);
    HIPCHK(hipGetLastError());
    HIPCHK(dla::sort_pairs_by_key((char*)sort_temp, &temp_bytes, key, key_sorted, ident, sorted, (size_t)nnz, key_bits, st));
    DLA_LAUNCH(column_pointers_kernel, dim3(grid_blocks(env(), nnz, 256)), dim3(256), 0, st, nnz, n, (const int*)key_sorted, (long long*)colptr);
    HIPCHK(hipGetLastError());
    std::vector<long long> cp((size_t)n + 1);
    HIPCHK(hipMemcpyAsync(cp.data(), (const long long*)colptr, sizeof(long long) * cp.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // the host lays the index out (dla::spmm_transpose_layout: the format rule and dla::sell_layout on the column lengths)
    dla::TransposeIndex T;
    { const int stc = dla::spmm_transpose_layout(n, cp.data(), format, a_entries, T, err); if (stc) return stc; }
    // everything is allocated in a fresh index; the one in use is given up only when the new one is complete
    TransposeIdx fresh;
    SparseOp& lay = fresh.lay;
    HIPCHK(lay.col.reserve((size_t)T.entries()));
    HIPCHK(fresh.pos.reserve((size_t)T.entries()));
    if (T.fmt == DLA_SPMM_SELL) {
      { const int stc = place_sell_tables(lay, n, T.lay); if (stc) return stc; }
      hold_sell(lay, n, T.lay);
    } else {
      lay.n = n; lay.w = T.w; lay.fmt = DLA_SPMM_ELL; lay.nnz = nnz;
    }
    if (T.fmt == DLA_SPMM_SELL) DLA_LAUNCH((transpose_fill_kernel<true>), walk_blocks(lay), dim3(256), 0, st, LAYOUT_OF(lay), (const long long*)colptr,
                                           (const int*)sorted, (const int*)erow, (const int*)epos, (int*)lay.col, (int*)fresh.pos);
    else DLA_LAUNCH((transpose_fill_kernel<false>), walk_blocks(lay), dim3(256), 0, st, LAYOUT_OF(lay), (const long long*)colptr, (const int*)sorted,
                    (const int*)erow, (const int*)epos, (int*)lay.col, (int*)fresh.pos);
#undef LAYOUT_OF
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    tidx = std::move(fresh);
    return DLA_OK;
  }
  int spmm_transpose_info(struct dla_spmm_info* out) override
  {
    if (!tidx.held()) { err = "spmm_transpose_info: no transposed index has been prepared (dla_spmm_transpose_prepare)"; return DLA_ERR_ARG; }
    const int stc = op_info(tidx.lay, out);
    // (the index arrays only: 8 bytes per entry where a matrix has 12, and no diagonal)
    out->device_bytes -= 4 * (out->stored + out->long_entries) + 8 * (long long)out->n;
    return stc;
  }
  // (no index: neither the device nor the stream is touched)
  int spmm_transpose_drop() override
  {
    if (!tidx.held()) return DLA_OK;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamSynchronize(st));     // (products may still be queued)
    tidx.drop();
    return DLA_OK;
  }
  int spmm_mul_t(int n, int m, const double* x, double* y) override
  {
    const SparseOp& op = ops[dla::SPMM_A];
    SparseOp& t = tidx.lay;
    if (op.fmt < 0) { err = "spmm_matvec_t: no operator has been set up"; return DLA_ERR_ARG; }
    if (!tidx.held()) { err = "spmm_matvec_t: no transposed index (dla_spmm_matvec_t before dla_spmm_transpose_prepare)"; return DLA_ERR_ARG; }
    if (n != op.n) { err = "spmm_matvec_t: n differs from setup"; return DLA_ERR_ARG; }
    const double* val = op.val;
    const int *row = t.col, *pos = tidx.pos;
    const double flops = 2.0 * (double)t.nnz * m;
    if (t.fmt == DLA_SPMM_SELL) {
      const LongRowsPlan p = long_rows_plan(env(), t.sell_long_segments, t.sell_multi_rows, t.sell_multi_segments, m, LONG_MC);
      if (p.part_doubles > t.long_part.capacity()) {
        bind();
        HIPCHK(hipStreamSynchronize(st));       // (queued products may still use the old block)
        HIPCHK(t.long_part.reserve(p.part_doubles));
      }
      {
        Scope s(this, DLA_OP_MATVEC, 8.0 * (double)(t.sell_stored + t.sell_long_entries) + 8.0 * (double)t.nnz + 4.0 * n + 16.0 * (double)n * m + 16.0 * (double)p.part_doubles,
                flops, plan_name("sell_spmm_t_kernel<%d>", SELL_MC));
        DLA_LAUNCH((sell_spmm_t_kernel<SELL_MC>), dim3(grid_blocks(env(), t.sell_slices, 4)), dim3(256), 0, st, n, m, t.sell_slices, (const long long*)t.sell_ptr,
                   (const int*)t.sell_perm, row, pos, val, x, y);
        HIPCHK(hipGetLastError());
      }
      if (t.sell_long_segments > 0) {
        Scope s(this, DLA_OP_MATVEC, 0.0, 0.0, plan_name("csr_long_segments_t_kernel<%d>", LONG_MC));
        DLA_LAUNCH((csr_long_segments_t_kernel<LONG_MC>), dim3(p.seg_blocks), dim3(256), 0, st, n, m, t.sell_long_segments, (const long long*)t.seg_ptr,
                   (const int*)t.seg_row, (const int*)t.seg_part, (const int*)t.long_row, row + t.sell_stored, pos + t.sell_stored, val, x, y, (double*)t.long_part);
        HIPCHK(hipGetLastError());
      }
      if (p.combine_blocks > 0) {
        Scope s(this, DLA_OP_MATVEC, 0.0, 0.0, "long_rows_combine_kernel");
        DLA_LAUNCH(long_rows_combine_kernel, dim3(p.combine_blocks), dim3(256), 0, st, n, m, t.sell_multi_rows, (const int*)t.multi_row, (const int*)t.part_ptr,
                   (const double*)t.long_part, y);
        HIPCHK(hipGetLastError());
      }
      return DLA_OK;
    }
    const dim3 grid(grid_blocks(env(), n, 256));
    ell_width(t.w, [&](auto W) {
      Scope s(this, DLA_OP_MATVEC, 8.0 * (double)t.w * n + 8.0 * (double)t.nnz + 16.0 * (double)n * m, flops, plan_name("ell_spmm_t_kernel<%d>", decltype(W)::value));
      DLA_LAUNCH((ell_spmm_t_kernel<decltype(W)::value>), grid, dim3(256), 0, st, n, m, t.w, row, pos, val, x, y);
    });
    HIPCHK(hipGetLastError());
    return DLA_OK;
  }

  // ---- ... on a row shard (banded matrices: the columns of a shard reach at most `halo` rows into its neighbours); A only
  // all-reduce of a few host values through the engine's small-product transport (setup-time agreement between the ranks)
  bool has_transport() const override { return hook != nullptr || comm != nullptr || p2p.on; }
  int allreduce_host(double* v, int count, int op) override
  {
    std::vector<double> t(v, v + count);
    const int stc = host_allreduce(t, op);
    if (stc) return stc;
    std::memcpy(v, t.data(), sizeof(double) * (size_t)count);
    return DLA_OK;
  }
  int host_allreduce(std::vector<double>& v, int op)
  {
    if (local_only || (nranks <= 1 && !comm && !p2p.on)) return DLA_OK;
    bind();
    int stc = ensure_small(sizeof(double) * v.size());
    if (stc) return stc;
    HIPCHK(hipMemcpyAsync(d_small, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice, st));
    stc = sum_to_host((int)v.size(), op);
    if (stc) return stc;
    std::memcpy(v.data(), h_small, sizeof(double) * v.size());
    return DLA_OK;
  }
  int spmm_setup_csr_sharded(int n, long long row0, long long n_global, const long long* rowptr, const long long* colind,
                             const double* values) override
  {
    int w = 0; long long need = 0;
    std::string lerr;
    // (a metric or a part beside a sharded operator would have to be sharded as well: refused like a bad shard, so that every rank agrees)
    const bool held = admit(dla::SPMM_A, "spmm_setup_csr_sharded", CALL_SHARD) != DLA_OK;
    if (held) lerr = err;
    const int bad = (held || values == nullptr) ? DLA_ERR_ARG : dla::sharded_ell_need(n, row0, n_global, rowptr, colind, &w, &need, lerr);
    const int nr = std::max(1, nranks);
    // agree on the halo width and check the layout, collectively: [max need | any failure | row0 and n of every rank (slots)]
    std::vector<double> mx{(double)need, bad ? 1.0 : 0.0};
    int stc = host_allreduce(mx, 1);
    if (stc) return stc;
    if (mx[1] != 0.0) { err = bad ? (lerr.empty() ? std::string("spmm_setup_csr_sharded: bad arguments") : lerr) : std::string("spmm_setup_csr_sharded: another rank rejected its shard"); return DLA_ERR_ARG; }
    std::vector<double> lay((size_t)2 * nr, 0.0);
    lay[2 * rank] = (double)row0; lay[2 * rank + 1] = (double)n;
    stc = host_allreduce(lay, 0);
    if (stc) return stc;
    const long long halo = (long long)mx[0];
    long long expect = 0;
    for (int r = 0; r < nr; ++r) {
      if ((long long)lay[2 * r] != expect) { err = "spmm_setup_csr_sharded: the shards are not contiguous in rank order"; return DLA_ERR_ARG; }
      if (halo > (long long)lay[2 * r + 1]) { err = "spmm_setup_csr_sharded: a shard reaches beyond its neighbour (halo wider than a shard)"; return DLA_ERR_ARG; }
      expect += (long long)lay[2 * r + 1];
    }
    if (expect != n_global) { err = "spmm_setup_csr_sharded: the shards do not cover n_global rows"; return DLA_ERR_ARG; }
    if (halo > 4096) { err = "spmm_setup_csr_sharded: halo wider than 4096 rows (not a banded matrix)"; return DLA_ERR_ARG; }
    // one right-hand side of the halo exchange is nranks x 2 x halo doubles and has to fit a mailbox slot when the mailboxes are the
    // only transport (round-4 advisor: beyond it the product had nowhere to go, and its abort left the peers in their exchange
    // until the timeout).  Same numbers on every rank: refused by all of them, here.
    if (p2p.on && !comm && !hook && (long long)nr * 2 * halo > (long long)P2P_MAX_DOUBLES) {
      err = "spmm_setup_csr_sharded: nranks x 2 x halo = " + std::to_string((long long)nr * 2 * halo) + " doubles per column exceed a peer-to-peer mailbox slot (" +
            std::to_string(P2P_MAX_DOUBLES) + "); attach RCCL (dla_comm_init) or a reduction hook beside the mailboxes";
      return DLA_ERR_ARG;
    }
    dla::ShardedEll e;
    dla::sharded_ell_build(n, row0, rowptr, colind, values, (int)halo, e);
    bind();
    cheb.upper_valid = cheb.off_valid = false;
    stc = upload_ell(ops[dla::SPMM_A], e.col, e.val, e.diag);
    if (stc) return stc;
    tidx.drop();
    ops[dla::SPMM_A].n = n; ops[dla::SPMM_A].w = e.w; shard.halo = (int)halo; shard.on = true;
    ops[dla::SPMM_A].fmt = DLA_SPMM_ELL; ops[dla::SPMM_A].nnz = rowptr[n] - rowptr[0];
    return DLA_OK;
  }
  int spmm_matvec_sharded(int n, int m, const double* x, double* ax)
  {
    const int nr = std::max(1, nranks), H = shard.halo;
    const SparseOp::Ell e = ops[dla::SPMM_A].ell();
    const dim3 grid(grid_blocks(env(), n, 256));
    // columns per exchange: a mailbox slot of the peer-to-peer transport holds P2P_MAX_DOUBLES
    int mc = m;
    if (H > 0 && nr > 1) mc = std::max(1, std::min(m, P2P_MAX_DOUBLES / (nr * 2 * H)));
    const size_t need = (size_t)std::max(1, nr * 2 * mc * std::max(1, H));
    if (need > shard.d_halo.capacity()) {
      HIPCHK(hipStreamSynchronize(st));
      HIPCHK(shard.d_halo.reserve(need));
      // (on the engine's stream: hipMemset runs on the null stream, which this non-blocking stream does not wait for -- the
      //  zeros would land in the middle of the first exchange)
      HIPCHK(hipMemsetAsync(shard.d_halo, 0, sizeof(double) * need, st));
      shard.h_halo.assign(need, 0.0);
    }
    for (int c0 = 0; c0 < m; c0 += mc) {
      const int mcur = std::min(mc, m - c0);
      const double* xc = x + (size_t)c0 * n;
      if (H > 0 && nr > 1) {
        const int total = nr * 2 * mcur * H;
        DLA_LAUNCH(halo_pack_kernel, dim3(std::max(1, std::min(64, (total + 255) / 256))), dim3(256), 0, st, n, mcur, H, nr, rank, xc, shard.d_halo);
        HIPCHK(hipGetLastError());
        StepOut halo_out;
        const int stc = allreduce_dev(shard.d_halo, total, 0, shard.h_halo.data(), halo_out);
        if (stc) return stc;
      }
      // (the first / last rank never index their missing neighbour: any valid address serves)
      const double* prev = shard.d_halo + (size_t)((rank > 0 ? (rank - 1) * 2 + 1 : 0) * mcur) * H;
      const double* next = shard.d_halo + (size_t)((rank + 1 < nr ? (rank + 1) * 2 : 0) * mcur) * H;
      ell_width(e.w, [&](auto W) {
        DLA_LAUNCH((ell_spmm_halo_kernel<decltype(W)::value>), grid, dim3(256), 0, st, n, mcur, e.w, H, e.col, e.val, xc, prev, next, ax + (size_t)c0 * n);
      });
      HIPCHK(hipGetLastError());
    }
    return DLA_OK;
  }
  // y = (slot) x; the words of a refusal are the callback's (SlotWords::mul)
  int spmm_mul(int slot, int n, int m, const double* x, double* y) override
  {
    { const int stc = admit(slot, words(slot).mul, 0); if (stc) return stc; }
    const SlotWords& w = words(slot);
    SparseOp& op = ops[slot];
    const std::string who = std::string(w.mul) + ": ";
    if (slot == dla::SPMM_A) {
      if (n != op.n || !op.col) { err = who + "n differs from setup"; return DLA_ERR_ARG; }
    } else {
      if (op.fmt < 0) { err = who + w.missing + " (dla_" + w.setup + ")"; return DLA_ERR_ARG; }
      if (n != op.n && slot == dla::SPMM_B) { err = who + "n differs from the metric's"; return DLA_ERR_ARG; }
      if (n != op.n) { err = who + "n = " + std::to_string(n) + " differs from the " + std::to_string(op.n) + " rows of " + w.noun; return DLA_ERR_ARG; }
    }
    if (shard.on && slot == dla::SPMM_A) {
      Scope s(this, DLA_OP_MATVEC, 12.0 * (double)op.w * n + 16.0 * (double)n * m, 2.0 * (double)op.w * n * m);
      return spmm_matvec_sharded(n, m, x, y);
    }
    return op_matvec(op, n, m, x, y);
  }
  // The three elementwise preconditioner launches, on the stored diagonals of the sparse or of the dense slots (the callers have
  // admitted the call): px = x / (d + fac); px = x / (da + fac db) of the pencil; the harness' lrprec_1 / lrprec_2 (variant 1 / 2)
  // on the diagonals of A+B, A-B and S+D.  kname: the kernel name the launch is booked under, empty for none.
  int launch_diag_precnd(const char* kname, int n, int m, double fac, const double* d, const double* x, double* px)
  {
    Scope s(this, DLA_OP_PRECND, 8.0 * n * (2.0 * m + 1.0), (double)n * m, kname);
    DLA_LAUNCH(diag_precnd_kernel, dim3(grid_blocks(env(), n, 256)), dim3(256), 0, st, n, m, fac, d, x, px);
    HIPCHK(hipGetLastError());
    return DLA_OK;
  }
  int launch_pencil_precnd(const char* kname, int n, int m, double fac, const double* da, const double* db, const double* x, double* px)
  {
    Scope s(this, DLA_OP_PRECND, 16.0 * (double)n * m + 16.0 * (double)n, 2.0 * (double)n * m, kname);
    DLA_LAUNCH(pencil_precnd_kernel, dim3(grid_blocks(env(), n, 256)), dim3(256), 0, st, n, m, fac, da, db, x, px);
    HIPCHK(hipGetLastError());
    return DLA_OK;
  }
  int launch_lr_precnd(const char* kname, int variant, int n, int m, double fac, const double* da, const double* dm, const double* ds,
                       const double* xp, const double* xm, double* yp, double* ym)
  {
    Scope s(this, DLA_OP_PRECND, 32.0 * (double)n * m + 24.0 * (double)n, 8.0 * (double)n * m, kname);
    const bool vec2 = on_16_bytes(n, xp, xm, yp, ym);
    const size_t nv = (size_t)n / (vec2 ? 2 : 1);
    const int blocks = grid_blocks(env(), (long long)nv, 256);
    if (vec2) DLA_LAUNCH(lr_precnd_kernel<2>, dim3(blocks), dim3(256), 0, st, n, m, variant, fac, da, dm, ds, xp, xm, yp, ym);
    else      DLA_LAUNCH(lr_precnd_kernel<1>, dim3(blocks), dim3(256), 0, st, n, m, variant, fac, da, dm, ds, xp, xm, yp, ym);
    HIPCHK(hipGetLastError());
    return DLA_OK;
  }
  int spmm_precnd(int n, int m, double fac, const double* x, double* px) override
  {
    if (n != ops[dla::SPMM_A].n || !ops[dla::SPMM_A].diag) { err = "spmm_precnd: n differs from setup"; return DLA_ERR_ARG; }
    return launch_diag_precnd("", n, m, fac, ops[dla::SPMM_A].diagonal(), x, px);
  }
  // ---- ... of the pencil A - lambda B of a generalised problem (the metric B: bvec of reference diaglib.f90:1855)
  int spmm_precnd_pencil(int n, int m, double fac, const double* x, double* px) override
  {
    if (ops[dla::SPMM_A].fmt < 0 || !ops[dla::SPMM_A].diag) { err = "spmm_precnd_pencil: no operator has been set up"; return DLA_ERR_ARG; }
    if (ops[dla::SPMM_B].fmt < 0) { err = "spmm_precnd_pencil: no metric has been set up (dla_spmm_setup_metric_csr)"; return DLA_ERR_ARG; }
    if (ops[dla::SPMM_A].n != ops[dla::SPMM_B].n) { err = "spmm_precnd_pencil: the operator has " + std::to_string(ops[dla::SPMM_A].n) + " rows and the metric " + std::to_string(ops[dla::SPMM_B].n); return DLA_ERR_ARG; }
    if (n != ops[dla::SPMM_A].n) { err = "spmm_precnd_pencil: n differs from setup"; return DLA_ERR_ARG; }
    return launch_pencil_precnd("", n, m, fac, ops[dla::SPMM_A].diagonal(), ops[dla::SPMM_B].diagonal(), x, px);
  }

  // ---- the stored dense matrices (the contract: include/diaglib_amd.h, dla_dense_setup and dla_dense_setup_lr; the kernels: beside
  // dense_mfma_kernel).  Six slots -- the operator, the metric and the four parts A+B, A-B, S+D, S-D of the linear-response pencil
  // (dla::DenseSlot) -- each the packed copy, its diagonal and the workspace of a split product.  The blocks only grow: a
  // smaller matrix after a larger one keeps the larger blocks (the kernels go by n / n_pad).
  struct DenseOp {
    int n = 0;                       // 0: nothing stored
    int last_m = 1;                  // width of the first pass of the most recent product (what dense_info describes)
    char uplo = 0;                   // 0: stored in full; 'L' / 'U': one triangle (dla_dense_setup_sym), the triangle that was referenced
    DeviceBuffer<double> a, diag, ws;
    void drop() { a.reset(); diag.reset(); ws.reset(); n = 0; last_m = 1; uplo = 0; }
  } dense[dla::DENSE_SLOTS];
  // The words a message about a dense slot needs: what the slot is called, the name of each public entry that reaches it (setup is
  // also the set-up a callback names while the slot is empty) and the rule quoted for a public number out of range.
  struct DenseWords { const char *noun, *setup, *setup_dev, *info, *mul, *range; };
  static const DenseWords& dense_words(int slot)
  {
    static constexpr const char* which_rule = "which must be 0 (the operator) or 1 (the metric)";
    static constexpr const char* part_rule = "part must be 0 (A+B), 1 (A-B), 2 (S+D) or 3 (S-D)";
#define LR_WORDS(P, SUM) {"dense part " P " (" SUM ")", "dla_dense_setup_lr", "dla_dense_setup_lr_dev", "dla_dense_lr_info", "dense_" P "mul", part_rule}
    static const DenseWords table[dla::DENSE_SLOTS] = {
      {"dense operator", "dla_dense_setup", "dla_dense_setup_dev", "dla_dense_info", "dense_matvec", which_rule},
      {"dense metric", "dla_dense_setup", "dla_dense_setup_dev", "dla_dense_info", "dense_bvec", which_rule},
      LR_WORDS("apb", "A+B"), LR_WORDS("amb", "A-B"), LR_WORDS("spd", "S+D"), LR_WORDS("smd", "S-D")};
#undef LR_WORDS
    // (a number out of range is refused in the words of the entries that take such a number)
    return table[slot == dla::DENSE_NO_PART ? dla::DENSE_APB : (slot < 0 || slot >= dla::DENSE_SLOTS) ? dla::DENSE_A : slot];
  }
  // The one place that decides whether a call on a dense slot is admitted; entry: the name of the public entry or of the callback.
  // A set-up or a drop needs the slot to exist (DENSE_EXISTS), an info needs it to hold a matrix (DENSE_STORED), a callback needs
  // that matrix to have n rows and names the set-up that is missing (DENSE_ROWS).  Leaves the refusal in err.
  enum DenseNeed { DENSE_EXISTS, DENSE_STORED, DENSE_ROWS };
  int dense_admit(int slot, const char* entry, DenseNeed need, int n = 0)
  {
    // (an admitted call -- every callback of a solve -- builds no string)
    const DenseWords& w = dense_words(slot);
    const auto refuse = [&](const std::string& why) { err = std::string(entry) + ": " + why; return (int)DLA_ERR_ARG; };
    if (slot < 0 || slot >= dla::DENSE_SLOTS) return refuse(w.range);
    if (need == DENSE_EXISTS) return DLA_OK;
    const DenseOp& op = dense[slot];
    if (op.n <= 0) return refuse(std::string("no ") + w.noun + " has been set up" + (need == DENSE_ROWS ? std::string(" (") + w.setup + ")" : std::string()));
    if (need == DENSE_ROWS && n != op.n) return refuse("n = " + std::to_string(n) + " differs from the " + std::to_string(op.n) + " rows of the " + w.noun);
    return DLA_OK;
  }
  // what every dense set-up refuses of one array; who: the entry's name with ": ", what: the array's name in the message
  int dense_array_ok(const std::string& who, const char* what, const char* ld, int n, const double* a, int lda)
  {
    if (!a) { err = who + "the " + what + " is a null pointer"; return DLA_ERR_ARG; }
    if (n <= 0) { err = who + "n must be positive"; return DLA_ERR_ARG; }
    if (lda < n) { err = who + ld + " = " + std::to_string(lda) + " is below n = " + std::to_string(n); return DLA_ERR_ARG; }
    return DLA_OK;
  }
  // the copy and the diagonal of a checked array into one slot; uplo: 0 for the full copy, 'L' / 'U' for the triangular one
  int dense_store(const std::string& who, DenseOp& op, bool dev, int n, const double* a, int lda, char uplo = 0)
  {
    const int n_pad = dense_n_pad(n);
    const size_t total = uplo ? dense_sym_doubles(n_pad) : (size_t)n_pad * n_pad;
    std::vector<double> packed, diag;
    if (!dev) {
      try { packed.resize(total); diag.resize((size_t)n); }
      catch (const std::bad_alloc&) { err = who + "no host memory for the packed copy"; return DLA_ERR_ALLOC; }
      if (uplo) dense_sym_pack(n, a, (size_t)lda, uplo, packed.data(), diag.data());
      else dense_pack(n, a, (size_t)lda, packed.data(), diag.data());
    }
    bind();
    HIPCHK(hipStreamSynchronize(st));      // (queued products may still read the old blocks)
    // (a block that has to grow is released first: from here on a failure leaves the slot empty, not half replaced)
    op.n = 0; op.last_m = 1; op.uplo = 0;
    if (op.a.reserve(total) != hipSuccess || op.diag.reserve((size_t)n) != hipSuccess) {
      op.drop();
      err = who + "no device memory for " + std::to_string(8 * total + 8 * (size_t)n) + " bytes";
      return DLA_ERR_ALLOC;
    }
    if (dev) {
      if (uplo) DLA_LAUNCH(dense_sym_pack_kernel, dim3(grid_blocks(env(), (long long)total, 256)), dim3(256), 0, st, n, n_pad, uplo == 'L', a, (size_t)lda, (double*)op.a);
      else DLA_LAUNCH(dense_pack_kernel, dim3(grid_blocks(env(), (long long)total, 256)), dim3(256), 0, st, n, n_pad, a, (size_t)lda, (double*)op.a);
      HIPCHK(hipGetLastError());
      DLA_LAUNCH(dense_diag_kernel, dim3(grid_blocks(env(), n, 256)), dim3(256), 0, st, n, a, (size_t)lda, (double*)op.diag);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(st));
    } else {
      HIPCHK(hipMemcpy(op.a, packed.data(), sizeof(double) * total, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(op.diag, diag.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    }
    op.n = n;
    op.uplo = uplo;
    return DLA_OK;
  }
  // one triangle of a symmetric operator or metric (dla_dense_setup_sym): the checks of dense_setup, then the triangle's letter
  int dense_setup_sym(int slot, int via, int n, const double* a, int lda, char uplo) override
  {
    const bool dev = via == dla::SPMM_VIA_DEVICE;
    const char* entry = dev ? "dla_dense_setup_sym_dev" : "dla_dense_setup_sym";
    const std::string who = std::string(entry) + ": ";
    { const int stc = dense_admit(slot, entry, DENSE_EXISTS); if (stc) return stc; }
    { const int stc = dense_array_ok(who, "matrix", "lda", n, a, lda); if (stc) return stc; }
    const char up = uplo == 'l' ? 'L' : uplo == 'u' ? 'U' : uplo;
    if (up != 'L' && up != 'U') { err = who + "uplo must be 'L' or 'U' (the triangle of the array that is referenced)"; return DLA_ERR_ARG; }
    return dense_store(who, dense[slot], dev, n, a, lda, up);
  }
  int dense_sym_info(int slot, struct dla_dense_sym_info* out) override
  {
    const char* entry = "dla_dense_sym_info";
    { const int stc = dense_admit(slot, entry, DENSE_EXISTS); if (stc) return stc; }
    if (!out) { err = std::string(entry) + ": out is a null pointer"; return DLA_ERR_ARG; }
    { const int stc = dense_admit(slot, entry, DENSE_STORED); if (stc) return stc; }
    const DenseOp& op = dense[slot];
    if (!op.uplo) { err = std::string(entry) + ": the " + dense_words(slot).noun + " is stored in full (dla_dense_setup), not as a triangle"; return DLA_ERR_ARG; }
    const DenseSymPlan p = dense_sym_plan(ncu, op.n, op.last_m);
    out->uplo = op.uplo; out->panels = p.panels; out->chunk_blocks = p.chunk_blocks; out->max_partials = p.max_partials;
    return DLA_OK;
  }
  int dense_setup(int slot, int via, int n, const double* a, int lda) override
  {
    const bool dev = via == dla::SPMM_VIA_DEVICE;
    const char* entry = dev ? dense_words(slot).setup_dev : dense_words(slot).setup;
    const std::string who = std::string(entry) + ": ";
    { const int stc = dense_admit(slot, entry, DENSE_EXISTS); if (stc) return stc; }
    { const int stc = dense_array_ok(who, "matrix", "lda", n, a, lda); if (stc) return stc; }
    return dense_store(who, dense[slot], dev, n, a, lda);
  }
  // p + q and p - q into the two slots of a pair, both or neither: every check and both allocations come before the first write.
  // A slot whose blocks have to grow gets new ones while it still holds the old, so a failed allocation leaves both slots as they were.
  int dense_setup_pair(int pair, int via, int n, const double* p, int ldp, const double* q, int ldq) override
  {
    const bool dev = via == dla::SPMM_VIA_DEVICE;
    const std::string who = dev ? "dla_dense_setup_lr_pair_dev: " : "dla_dense_setup_lr_pair: ";
    if (pair != 0 && pair != 1) { err = who + "pair must be 0 (A and B: fills A+B, A-B) or 1 (S and D: fills S+D, S-D)"; return DLA_ERR_ARG; }
    { const int stc = dense_array_ok(who, "first matrix (p)", "ldp", n, p, ldp); if (stc) return stc; }
    { const int stc = dense_array_ok(who, "second matrix (q)", "ldq", n, q, ldq); if (stc) return stc; }
    DenseOp* op[2] = {&dense[dla::DENSE_APB + 2 * pair], &dense[dla::DENSE_APB + 2 * pair + 1]};
    const int n_pad = dense_n_pad(n);
    const size_t total = (size_t)n_pad * n_pad;
    std::vector<double> packed[2], diag[2];
    if (!dev) {
      try { for (int s = 0; s < 2; ++s) { packed[s].resize(total); diag[s].resize((size_t)n); } }
      catch (const std::bad_alloc&) { err = who + "no host memory for the packed copies"; return DLA_ERR_ALLOC; }
      dense_pack_pair(n, p, (size_t)ldp, q, (size_t)ldq, packed[0].data(), diag[0].data(), packed[1].data(), diag[1].data());
    }
    bind();
    DeviceBuffer<double> grown_a[2], grown_diag[2];
    for (int s = 0; s < 2; ++s) {
      const bool ok = (total <= op[s]->a.capacity() || grown_a[s].reserve(total) == hipSuccess) &&
                      ((size_t)n <= op[s]->diag.capacity() || grown_diag[s].reserve((size_t)n) == hipSuccess);
      if (!ok) { err = who + "no device memory for " + std::to_string(2 * (8 * total + 8 * (size_t)n)) + " bytes"; return DLA_ERR_ALLOC; }
    }
    HIPCHK(hipStreamSynchronize(st));      // (queued products may still read the old blocks)
    for (int s = 0; s < 2; ++s) {
      op[s]->n = 0; op[s]->last_m = 1;
      if (grown_a[s]) op[s]->a.swap(grown_a[s]);
      if (grown_diag[s]) op[s]->diag.swap(grown_diag[s]);
    }
    if (dev) {
      DLA_LAUNCH(dense_pack_pair_kernel, dim3(grid_blocks(env(), (long long)total, 256)), dim3(256), 0, st, n, n_pad, p, (size_t)ldp, q, (size_t)ldq,
                 (double*)op[0]->a, (double*)op[1]->a);
      HIPCHK(hipGetLastError());
      DLA_LAUNCH(dense_diag_pair_kernel, dim3(grid_blocks(env(), n, 256)), dim3(256), 0, st, n, p, (size_t)ldp, q, (size_t)ldq,
                 (double*)op[0]->diag, (double*)op[1]->diag);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(st));
    } else {
      for (int s = 0; s < 2; ++s) {
        HIPCHK(hipMemcpy(op[s]->a, packed[s].data(), sizeof(double) * total, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(op[s]->diag, diag[s].data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
      }
    }
    op[0]->n = op[1]->n = n;
    return DLA_OK;
  }
  int dense_info(int slot, struct dla_dense_info* out) override
  {
    const char* entry = dense_words(slot).info;
    { const int stc = dense_admit(slot, entry, DENSE_EXISTS); if (stc) return stc; }
    if (!out) { err = std::string(entry) + ": out is a null pointer"; return DLA_ERR_ARG; }
    { const int stc = dense_admit(slot, entry, DENSE_STORED); if (stc) return stc; }
    const DenseOp& op = dense[slot];
    if (op.uplo) {
      const DenseSymPlan p = dense_sym_plan(ncu, op.n, op.last_m);
      out->n = op.n; out->n_pad = p.n_pad; out->row_tile = DENSE_TILE * DENSE_WAVE_TILES; out->k_chunks = p.max_chunks;
      out->device_bytes = 8LL * (long long)dense_sym_doubles(p.n_pad) + 8LL * op.n;
      out->workspace_bytes = 8LL * (long long)p.ws_doubles;
      return DLA_OK;
    }
    const DensePlan p = dense_plan(ncu, op.n, op.last_m);
    out->n = op.n; out->n_pad = p.n_pad; out->row_tile = DENSE_TILE * DENSE_WAVE_TILES; out->k_chunks = p.k_chunks;
    out->device_bytes = 8LL * p.n_pad * p.n_pad + 8LL * op.n;
    out->workspace_bytes = 8LL * (long long)p.ws_doubles;
    return DLA_OK;
  }
  // (nothing stored: neither the device nor the stream is touched; a number out of range comes from dla_dense_drop alone)
  int dense_drop(int first, int last) override
  {
    { const int stc = dense_admit(first, "dla_dense_drop", DENSE_EXISTS); if (stc) return stc; }
    bool any = false;
    for (int s = first; s <= last; ++s) any = any || dense[s].n > 0 || dense[s].a;
    if (!any) return DLA_OK;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamSynchronize(st));     // (products of these slots may still be queued)
    for (int s = first; s <= last; ++s) dense[s].drop();
    return DLA_OK;
  }
  // y = (slot) x: the passes of one product on the slot's copy and the slot's own workspace; the words of a refusal are the
  // callback's (DenseWords::mul).  (The callbacks of host_logic.cpp pass their own DenseSlot: no number out of range gets here.)
  int dense_mul(int slot, int n, int m, const double* x, double* y) override
  {
    { const int stc = dense_admit(slot, dense_words(slot).mul, DENSE_ROWS, n); if (stc) return stc; }
    if (m <= 0) return DLA_OK;
    DenseOp& op = dense[slot];
    op.last_m = std::min(m, DENSE_MAX_COLS);
    if (op.uplo) return dense_mul_sym(op, n, m, x, y);
    for (int c0 = 0; c0 < m; c0 += DENSE_MAX_COLS) {
      const int mp = std::min(DENSE_MAX_COLS, m - c0);
      const DensePlan p = dense_plan(ncu, n, mp);
      if (p.ws_doubles > op.ws.capacity()) {
        bind();
        HIPCHK(hipStreamSynchronize(st));       // (queued products may still use the old block)
        HIPCHK(op.ws.reserve(p.ws_doubles));
      }
      const double* xc = x + (size_t)c0 * n;
      double* yc = y + (size_t)c0 * n;
      const dim3 grid((p.row_groups + 3) / 4, p.k_chunks);
      {
        Scope s(this, DLA_OP_MATVEC, 8.0 * (double)n * n + 16.0 * (double)n * mp, 2.0 * (double)n * n * mp, p.name());
        const bool hit = first_instance<DENSE_MAX_COLS / 16>([&](auto i) {
          constexpr int G = (int)decltype(i)::value + 1;
          if (p.acc_groups != G) return false;
          DLA_LAUNCH((dense_mfma_kernel<G>), grid, dim3(256), 0, st, n, mp, p.n_pad, p.chunk_groups, (const double*)op.a, xc, yc, (double*)op.ws);
          return true;
        });
        if (!hit) { err = "dense product: no kernel instance"; return DLA_ERR_RUNTIME; }
        HIPCHK(hipGetLastError());
      }
      if (p.k_chunks > 1) {
        // (the partial sums are not compulsory traffic: the launch is booked without algorithmic bytes)
        Scope s(this, DLA_OP_MATVEC, 0.0, 0.0, "dense_combine_kernel");
        const size_t total = (size_t)n * mp;
        DLA_LAUNCH(dense_combine_kernel, dim3(grid_blocks(env(), (long long)total, 256)), dim3(256), 0, st, total, p.k_chunks, (const double*)op.ws, yc);
        HIPCHK(hipGetLastError());
      }
    }
    return DLA_OK;
  }
  // y = (slot) x on a triangular copy (dla_dense_setup_sym): the passes of dense_sym_plan on the slot's own workspace.  Booked with
  // the bytes a pass has to move -- the triangle with its diagonal once, 4 n (n + 1), and x and y -- and the flops of the full product.
  int dense_mul_sym(DenseOp& op, int n, int m, const double* x, double* y)
  {
    for (int c0 = 0; c0 < m; c0 += DENSE_MAX_COLS) {
      const int mp = std::min(DENSE_MAX_COLS, m - c0);
      const DenseSymPlan p = dense_sym_plan(ncu, n, mp);
      if (p.ws_doubles > op.ws.capacity()) {
        bind();
        HIPCHK(hipStreamSynchronize(st));       // (queued products may still use the old block)
        HIPCHK(op.ws.reserve(p.ws_doubles));
      }
      const double* xc = x + (size_t)c0 * n;
      double* yc = y + (size_t)c0 * n;
      const dim3 grid(p.max_chunks, p.panels);
      {
        Scope s(this, DLA_OP_MATVEC, 4.0 * (double)n * (n + 1.0) + 16.0 * (double)n * mp, 2.0 * (double)n * n * mp, p.name());
        const bool hit = first_instance<DENSE_MAX_COLS / 16>([&](auto i) {
          constexpr int G = (int)decltype(i)::value + 1;
          if (p.acc_groups != G) return false;
          DLA_LAUNCH((dense_sym_mfma_kernel<G>), grid, dim3(256), 0, st, n, mp, p.row_tiles, p.chunk_panels, p.t_base, (const double*)op.a, xc, yc,
                     (double*)op.ws);
          return true;
        });
        if (!hit) { err = "dense symmetric product: no kernel instance"; return DLA_ERR_RUNTIME; }
        HIPCHK(hipGetLastError());
      }
      if (p.row_tiles > 1) {
        // (the partial sums are not compulsory traffic: the launch is booked without algorithmic bytes)
        Scope s(this, DLA_OP_MATVEC, 0.0, 0.0, "dense_sym_combine_kernel");
        DLA_LAUNCH(dense_sym_combine_kernel, dim3(grid_blocks(env(), (long long)n * mp, 256)), dim3(256), 0, st, n, mp, p.row_tiles, p.chunk_panels, p.t_base,
                   (const double*)op.ws, yc);
        HIPCHK(hipGetLastError());
      }
    }
    return DLA_OK;
  }
  // y = A^T x on the copy of the operator slot (dla_dense_matvec_t): the passes of dense_t_plan on the slot's own workspace.  The slot's
  // description (dense_info: the first pass of the most recent forward product) is left as it is.
  int dense_mul_t(int n, int m, const double* x, double* y) override
  {
    { const int stc = dense_admit(dla::DENSE_A, "dense_matvec_t", DENSE_ROWS, n); if (stc) return stc; }
    if (m <= 0) return DLA_OK;
    DenseOp& op = dense[dla::DENSE_A];
    if (op.uplo) return dense_mul_sym(op, n, m, x, y);    // (A^T = A: the symmetric product, the slot's description left as it is)
    for (int c0 = 0; c0 < m; c0 += DENSE_MAX_COLS) {
      const int mp = std::min(DENSE_MAX_COLS, m - c0);
      const DenseTPlan p = dense_t_plan(ncu, n, mp);
      if (p.ws_doubles > op.ws.capacity()) {
        bind();
        HIPCHK(hipStreamSynchronize(st));       // (queued products may still use the old block)
        HIPCHK(op.ws.reserve(p.ws_doubles));
      }
      const double* xc = x + (size_t)c0 * n;
      double* yc = y + (size_t)c0 * n;
      const dim3 grid((p.strips + 3) / 4, p.row_chunks);
      {
        Scope s(this, DLA_OP_MATVEC, 8.0 * (double)n * n + 16.0 * (double)n * mp, 2.0 * (double)n * n * mp, p.name());
        const bool hit = first_instance<DENSE_MAX_COLS / 16>([&](auto i) {
          constexpr int G = (int)decltype(i)::value + 1;
          if (p.acc_groups != G) return false;
          DLA_LAUNCH((dense_t_mfma_kernel<G>), grid, dim3(256), 0, st, n, mp, p.n_pad, p.chunk_tiles, (const double*)op.a, xc, yc, (double*)op.ws);
          return true;
        });
        if (!hit) { err = "dense transposed product: no kernel instance"; return DLA_ERR_RUNTIME; }
        HIPCHK(hipGetLastError());
      }
      if (p.row_chunks > 1) {
        Scope s(this, DLA_OP_MATVEC, 0.0, 0.0, "dense_combine_kernel");
        const size_t total = (size_t)n * mp;
        DLA_LAUNCH(dense_combine_kernel, dim3(grid_blocks(env(), (long long)total, 256)), dim3(256), 0, st, total, p.row_chunks, (const double*)op.ws, yc);
        HIPCHK(hipGetLastError());
      }
    }
    return DLA_OK;
  }
  // the diagonal kernels of the sparse operator on the stored dense diagonals
  int dense_precnd(bool pencil, int n, int m, double fac, const double* x, double* px) override
  {
    const char* who = pencil ? "dense_precnd_pencil" : "dense_precnd";
    const DenseOp &a = dense[dla::DENSE_A], &b = dense[dla::DENSE_B];
    { const int stc = dense_admit(dla::DENSE_A, who, DENSE_ROWS, n); if (stc) return stc; }
    if (pencil) {
      if (b.n <= 0) { err = std::string(who) + ": no dense metric has been set up (dla_dense_setup with which = 1)"; return DLA_ERR_ARG; }
      if (b.n != a.n) { err = std::string(who) + ": the operator has " + std::to_string(a.n) + " rows and the metric " + std::to_string(b.n); return DLA_ERR_ARG; }
    }
    if (m <= 0) return DLA_OK;
    return pencil ? launch_pencil_precnd("pencil_precnd_kernel", n, m, fac, a.diag, b.diag, x, px)
                  : launch_diag_precnd("diag_precnd_kernel", n, m, fac, a.diag, x, px);
  }
  // lr_precnd_kernel on the stored diagonals of the dense parts A+B, A-B and S+D (S-D is not read)
  int dense_lrprec(int variant, int n, int m, double fac, const double* xp, const double* xm, double* yp, double* ym) override
  {
    for (int slot : {(int)dla::DENSE_APB, (int)dla::DENSE_AMB, (int)dla::DENSE_SPD}) {
      const int stc = dense_admit(slot, variant == 1 ? "dense_lrprec1" : "dense_lrprec2", DENSE_ROWS, n);
      if (stc) return stc;
    }
    if (m <= 0) return DLA_OK;
    return launch_lr_precnd("", variant, n, m, fac, dense[dla::DENSE_APB].diag, dense[dla::DENSE_AMB].diag, dense[dla::DENSE_SPD].diag, xp, xm, yp, ym);
  }

  // ---- the Chebyshev polynomial of A + fac I as a preconditioner (the contract: include/diaglib_amd.h, dla_spmm_precnd_cheb; the
  // kernels: beside ell_cheb_step_kernel).  The configuration and the work panels are the context's; the Gershgorin bound is the
  // stored matrix's and is formed again after every set-up, refresh or drop of slot A (upper_valid).
  struct Cheb {
    int steps = 0;
    double lo_fraction = 0.0;
    bool upper_valid = false;
    double upper = 0.0;
    DeviceBuffer<double> z[2];         // the iterates z_k, z_{k-1}: n x m each
    DeviceBuffer<double> au;           // A u of the tail rows of a sliced operator, and of every row on the un-fused path: n x m
    DeviceBuffer<double> partial;      // the block maxima of the Gershgorin kernels
    // the diagonally scaled form (dla_spmm_precnd_cheb_jacobi)
    bool off_valid = false;            // off holds the off-diagonal row sums of the stored A
    DeviceBuffer<double> off;          // n doubles: the stored matrix's, formed on first use
    DeviceBuffer<double> r;            // n doubles: 1 / den_i of the last call's fac
    DeviceBuffer<double> y;            // the panel y = x o r: n x m
    // the pencil form (dla_spmm_precnd_cheb_pencil)
    bool offb_valid = false;           // offb holds the off-diagonal row sums of the stored metric
    DeviceBuffer<double> offb;         // n doubles: the stored metric's, formed on first use
    DeviceBuffer<double> bu;           // B u wherever the two matrices do not share a row loop: n x m
  } cheb;
  int spmm_cheb_config(int steps, double lo_fraction) override
  {
    if (steps < 0) { err = "spmm_cheb_config: steps = " + std::to_string(steps) + " must not be negative"; return DLA_ERR_ARG; }
    if (steps > 0 && !(lo_fraction > 0.0 && lo_fraction < 1.0)) {
      err = "spmm_cheb_config: lo_fraction = " + std::to_string(lo_fraction) + " must lie inside (0, 1)";
      return DLA_ERR_ARG;
    }
    if (steps == 0) {
      if (cheb.z[0] || cheb.z[1] || cheb.au || cheb.partial || cheb.off || cheb.r || cheb.y || cheb.offb || cheb.bu) {
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipStreamSynchronize(st));     // (a queued call may still use the panels)
        cheb.z[0].reset(); cheb.z[1].reset(); cheb.au.reset(); cheb.partial.reset();
        cheb.off.reset(); cheb.r.reset(); cheb.y.reset(); cheb.off_valid = false;
        cheb.offb.reset(); cheb.bu.reset(); cheb.offb_valid = false;
      }
      cheb.steps = 0; cheb.lo_fraction = 0.0;
      return DLA_OK;
    }
    cheb.steps = steps; cheb.lo_fraction = lo_fraction;
    return DLA_OK;
  }
  // The three Gershgorin kernels on the rows of op: a wavefront per slice and per tail row under 4 blocks per compute unit, a thread
  // per ELLPACK row under 8.  ROWS = false: the block maxima go to partial, *count of them; ROWS = true: the row sums go to off.
  template <bool ROWS>
  int gershgorin(const SparseOp& op, double* partial, double* off, int* count = nullptr)
  {
    int b0 = 0, b1 = 0;
    if (op.fmt == DLA_SPMM_SELL) {
      const SparseOp::Slices sl = op.slices();
      const SparseOp::Tail t = op.tail();
      b0 = grid_blocks(env(), sl.count, 4, 4);
      DLA_LAUNCH(sell_gershgorin_kernel<ROWS>, dim3(b0), dim3(256), 0, st, op.n, sl.count, sl.ptr, sl.perm, sl.col, sl.val, op.diagonal(), partial, off);
      HIPCHK(hipGetLastError());
      if (t.rows > 0) {
        b1 = grid_blocks(env(), t.rows, 4, 4);
        DLA_LAUNCH(tail_gershgorin_kernel<ROWS>, dim3(b1), dim3(256), 0, st, t.rows, t.long_ptr, t.long_row, t.col, t.val, op.diagonal(),
                   ROWS ? partial : partial + b0, off);
        HIPCHK(hipGetLastError());
      }
    } else {
      const SparseOp::Ell e = op.ell();
      b0 = grid_blocks(env(), op.n, 256);
      DLA_LAUNCH(ell_gershgorin_kernel<ROWS>, dim3(b0), dim3(256), 0, st, op.n, e.w, e.col, e.val, op.diagonal(), partial, off);
      HIPCHK(hipGetLastError());
    }
    if (count) *count = b0 + b1;
    return DLA_OK;
  }
  // the maximum of `count` block maxima, taken on the host behind what is queued on the stream (one host wait)
  int max_of_blocks(const double* buffer, int count, double* g)
  {
    std::vector<double> h((size_t)count);
    HIPCHK(hipMemcpyAsync(h.data(), buffer, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *g = *std::max_element(h.begin(), h.end());
    return DLA_OK;
  }
  // g of the stored A (single rank), from the blocks: at most ncu x 8 block maxima come to the host.  Synchronous, once per stored
  // matrix; like the set-up kernels it is not booked into the statistics.
  int cheb_upper()
  {
    if (cheb.upper_valid) return DLA_OK;
    bind();
    int count = 0;
    { const int stc = cheb_panel(cheb.partial, (size_t)grid_cap(env())); if (stc) return stc; }
    { const int stc = gershgorin<false>(ops[dla::SPMM_A], cheb.partial, nullptr, &count); if (stc) return stc; }
    { const int stc = max_of_blocks(cheb.partial, count, &cheb.upper); if (stc) return stc; }
    cheb.upper_valid = true;
    return DLA_OK;
  }
  // what both entries refuse first; who: the entry's name
  int cheb_admit(const char* who)
  {
    if (ops[dla::SPMM_A].fmt < 0 || !ops[dla::SPMM_A].diag) { err = std::string(who) + ": no operator has been set up (dla_spmm_setup_csr)"; return DLA_ERR_ARG; }
    if (shard.on) { err = std::string(who) + ": the operator of this context is row-sharded, and the Chebyshev preconditioner on a row-sharded operator is not supported"; return DLA_ERR_ARG; }
    if (cheb.steps <= 0) { err = std::string(who) + ": nothing is configured (dla_spmm_cheb_config)"; return DLA_ERR_ARG; }
    return DLA_OK;
  }
  int spmm_cheb_info(struct dla_spmm_cheb_info* out) override
  {
    { const int stc = cheb_admit("spmm_cheb_info"); if (stc) return stc; }
    { const int stc = cheb_upper(); if (stc) return stc; }
    out->steps = cheb.steps; out->lo_fraction = cheb.lo_fraction; out->upper = cheb.upper;
    return DLA_OK;
  }
  // a work panel of at least `need` doubles, grown behind a stream wait as long_part is
  int cheb_panel(DeviceBuffer<double>& b, size_t need)
  {
    if (need <= b.capacity()) return DLA_OK;
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(b.reserve(need));
    return DLA_OK;
  }
  // one step out = alpha u + beta v + gamma x + eta (A u) on the stored A; out may be v's buffer, never u's
  // F (ChebForm): scaled and pencil are the steps where x is the panel y = x o r and r = cheb.r; booked under their own kernel names
  // with the 8 n bytes of r and the 3 n m flops of the scaling on top.  Pencil: B u comes from the metric's own product in the panel
  // cheb.bu (8 n m bytes more) -- or, where both matrices are ELLPACK, from the second gather loop of ell_cheb_pencil_step_kernel.
  static constexpr int PAIR_WIDTHS[] = {4, 8, 16, 0};
  bool cheb_pencil_fused() const { return !knobs.cheb_unfused() && ops[dla::SPMM_A].fmt != DLA_SPMM_SELL && ops[dla::SPMM_B].fmt != DLA_SPMM_SELL; }
  template <int F>
  int cheb_step(SparseOp& op, int n, int m, const dla::ChebStep& k, const double* u, const double* v, const double* x, double* out, double fac)
  {
    constexpr bool J = F != CHEB_PLAIN, P = F == CHEB_PENCIL;
    const double nm = (double)n * m, rb = (J ? 8.0 * n : 0.0) + (P ? 8.0 * nm : 0.0), cf = (J ? 10.0 : 7.0) * nm;
    const double *r = J ? (const double*)cheb.r : nullptr, *au = cheb.au, *bu = P ? (const double*)cheb.bu : nullptr;
    if constexpr (P) {
      SparseOp& opb = ops[dla::SPMM_B];
      if (cheb_pencil_fused()) {
        const SparseOp::Ell ea = op.ell(), eb = opb.ell();
        Scope s(this, DLA_OP_PRECND, 12.0 * (double)(ea.w + eb.w) * n + 32.0 * nm + 8.0 * n, 2.0 * (double)(ea.w + eb.w) * nm + cf,
                "ell_cheb_pencil_step_kernel");
        const dim3 grid(grid_blocks(env(), n, 256));
        const int wide = std::max(ea.w, eb.w);
        first_instance<std::size(PAIR_WIDTHS)>([&](auto i) {
          constexpr int W = PAIR_WIDTHS[decltype(i)::value];
          if (W > 0 && wide > W) return false;
          DLA_LAUNCH((ell_cheb_pencil_step_kernel<W>), grid, dim3(256), 0, st, n, m, ea.w, ea.col, ea.val, eb.w, eb.col, eb.val, k, u, v, x, out, fac, r);
          return true;
        });
        HIPCHK(hipGetLastError());
        return DLA_OK;
      }
      { const int stc = op_matvec(opb, n, m, u, cheb.bu); if (stc) return stc; }
    }
    if (knobs.cheb_unfused()) {
      { const int stc = op_matvec(op, n, m, u, cheb.au); if (stc) return stc; }
      Scope s(this, DLA_OP_PRECND, 40.0 * nm + rb, cf, P ? "cheb_pencil_combine_kernel" : J ? "cheb_jacobi_combine_kernel" : "cheb_combine_kernel");
      const size_t total = (size_t)n * m;
      if constexpr (P) DLA_LAUNCH(cheb_pencil_combine_kernel, dim3(grid_blocks(env(), n, 256)), dim3(256), 0, st, n, m, k, fac, r, u, v, x, au, bu, out);
      else if constexpr (J) DLA_LAUNCH(cheb_jacobi_combine_kernel, dim3(grid_blocks(env(), n, 256)), dim3(256), 0, st, n, m, k, fac, r, u, v, x, au, out);
      else DLA_LAUNCH(cheb_combine_kernel, dim3(grid_blocks(env(), (long long)total, 256)), dim3(256), 0, st, total, k, u, v, x, au, out);
      HIPCHK(hipGetLastError());
      return DLA_OK;
    }
    if (op.fmt == DLA_SPMM_SELL) {
      const LongRowsPlan p = long_rows_plan(env(), op.sell_long_segments, op.sell_multi_rows, op.sell_multi_segments, m, LONG_MC);
      // (the tail's partial sums and its rows of the scratch panel are written once and read once)
      Scope s(this, DLA_OP_PRECND, 12.0 * (double)(op.sell_stored + op.sell_long_entries) + 4.0 * n + 32.0 * nm + 16.0 * (double)p.part_doubles +
                                       16.0 * (double)op.sell_long_rows * m + rb,
              2.0 * (double)op.nnz * m + cf, P ? "sell_cheb_pencil_panel_step_kernel" : J ? "sell_cheb_jacobi_step_kernel" : "sell_cheb_step_kernel");
      const SparseOp::Slices sl = op.slices();
      DLA_LAUNCH((sell_cheb_step_kernel<SELL_MC, F>), dim3(grid_blocks(env(), sl.count, 4)), dim3(256), 0, st, n, m, sl.count, sl.ptr, sl.perm, sl.col,
                 sl.val, k, u, v, x, out, fac, r, bu);
      HIPCHK(hipGetLastError());
      if (op.sell_long_segments > 0) {
        // (A u) of the tail rows to the scratch panel, then their combination
        { const int stc = tail_product(op, p, n, m, u, cheb.au); if (stc) return stc; }
        const SparseOp::Tail t = op.tail();
        DLA_LAUNCH(tail_cheb_combine_kernel<F>, dim3(grid_blocks(env(), (long long)t.rows * m, 256)), dim3(256), 0, st, n, m, t.rows, t.long_row, k, u, v, x,
                   au, out, fac, r, bu);
        HIPCHK(hipGetLastError());
      }
      return DLA_OK;
    }
    Scope s(this, DLA_OP_PRECND, 12.0 * (double)op.w * n + 32.0 * nm + rb, 2.0 * (double)op.w * nm + cf,
            P ? "ell_cheb_pencil_panel_step_kernel" : J ? "ell_cheb_jacobi_step_kernel" : "ell_cheb_step_kernel");
    const SparseOp::Ell e = op.ell();
    const dim3 grid(grid_blocks(env(), n, 256));
    ell_width(e.w, [&](auto W) {
      DLA_LAUNCH((ell_cheb_step_kernel<decltype(W)::value, F>), grid, dim3(256), 0, st, n, m, e.w, e.col, e.val, k, u, v, x, out, fac, r, bu);
    });
    HIPCHK(hipGetLastError());
    return DLA_OK;
  }
  // What the three entries share, once.  F: the form (ChebForm); admit(who): what the entry refuses first.  interval(&hi, &shift) leaves the upper end of the entry's interval and the
  // shift its coefficients take; first(cf, &y) launches the entry's own sweep -- with one step the whole polynomial, written to px --
  // and leaves in y the panel that stands in the place of x in the recurrence.
  template <int F, class Interval, class First>
  int cheb_apply(const char* who, int n, int m, double fac, const double* x, double* px, Interval&& interval, First&& first)
  {
    constexpr bool J = F != CHEB_PLAIN, P = F == CHEB_PENCIL;
    { const int stc = P ? cheb_pencil_admit(who) : cheb_admit(who); if (stc) return stc; }
    SparseOp& op = ops[dla::SPMM_A];
    if (n != op.n) { err = std::string(who) + ": n = " + std::to_string(n) + " differs from the " + std::to_string(op.n) + " rows of the operator"; return DLA_ERR_ARG; }
    if (m <= 0) return DLA_OK;
    const int d = cheb.steps;
    const size_t total = (size_t)n * m;
    // every buffer of the call before its first launch: a growing one waits for the stream
    if (J && d >= 2) { const int stc = cheb_panel(cheb.y, total); if (stc) return stc; }
    if (d >= 3) { const int stc = cheb_panel(cheb.z[0], total); if (stc) return stc; }
    if (d >= 4) { const int stc = cheb_panel(cheb.z[1], total); if (stc) return stc; }
    if (d >= 2 && (knobs.cheb_unfused() || (op.fmt == DLA_SPMM_SELL && op.sell_long_segments > 0))) { const int stc = cheb_panel(cheb.au, total); if (stc) return stc; }
    if (P && d >= 2 && !cheb_pencil_fused()) {
      { const int stc = cheb_panel(cheb.bu, total); if (stc) return stc; }
      // (... and the workspaces of the two tails, which the products would otherwise grow between the launches)
      for (SparseOp* o : {&op, &ops[dla::SPMM_B]}) {
        if (o->fmt != DLA_SPMM_SELL) continue;
        const LongRowsPlan p = long_rows_plan(env(), o->sell_long_segments, o->sell_multi_rows, o->sell_multi_segments, m, LONG_MC);
        const int stc = cheb_panel(o->long_part, p.part_doubles);
        if (stc) return stc;
      }
    }
    double hi = 0.0, shift = 0.0;
    { const int stc = interval(&hi, &shift); if (stc) return stc; }
    if (hi <= 1.0e-5) {       // (the harness' guard on the interval's upper end: px = x)
      Scope s(this, DLA_OP_PRECND, 16.0 * (double)n * m, 0.0, "cheb_identity_copy");
      if (!lc.dry) HIPCHK(hipMemcpyAsync(px, x, sizeof(double) * total, hipMemcpyDeviceToDevice, st));
      return DLA_OK;
    }
    const dla::ChebCoefficients cf = dla::cheb_coefficients(hi, cheb.lo_fraction * hi, shift, d);
    const double* y = x;
    { const int stc = first(cf, &y); if (stc) return stc; }
    // step k writes z_{k+1}: to px when it is the last, else to z[(k - 1) & 1], which held z_{k-1}
    for (int k = 1; k < d; ++k) {
      const double* u = k == 1 ? y : (const double*)cheb.z[(k - 2) & 1];
      const double* v = k <= 2 ? y : (const double*)cheb.z[(k - 1) & 1];
      double* out = k == d - 1 ? px : (double*)cheb.z[(k - 1) & 1];
      const int stc = cheb_step<F>(op, n, m, cf.steps[(size_t)k - 1], u, v, y, out, J ? fac : 0.0);
      if (stc) return stc;
    }
    return DLA_OK;
  }
  int spmm_precnd_cheb(int n, int m, double fac, const double* x, double* px) override
  {
    return cheb_apply<CHEB_PLAIN>(
        "spmm_precnd_cheb", n, m, fac, x, px,
        [&](double* hi, double* shift) -> int {
          const int stc = cheb_upper();
          *hi = cheb.upper + fac; *shift = fac;
          return stc;
        },
        [&](const dla::ChebCoefficients& cf, const double**) -> int {
          if (cheb.steps > 1) return DLA_OK;
          const size_t total = (size_t)n * m;
          Scope s(this, DLA_OP_PRECND, 16.0 * (double)n * m, (double)n * m, "cheb_scale_kernel");
          DLA_LAUNCH(cheb_scale_kernel, dim3(grid_blocks(env(), (long long)total, 256)), dim3(256), 0, st, total, cf.theta, x, px);
          HIPCHK(hipGetLastError());
          return DLA_OK;
        });
  }

  // ---- ... and on the diagonally scaled operator D^-1 (A + fac I), D = |diag(A) + fac| (the contract: include/diaglib_amd.h,
  // dla_spmm_precnd_cheb_jacobi).  off, the off-diagonal row sums, is the stored matrix's like the Gershgorin bound; r and the
  // interval depend on fac and are formed by every call.
  int cheb_off() { return cheb_off_rows(ops[dla::SPMM_A], cheb.off, cheb.off_valid); }
  // (of the stored metric, for the pencil form: invalidated by every accepted set-up, refresh or drop of slot B)
  int cheb_off_b() { return cheb_off_rows(ops[dla::SPMM_B], cheb.offb, cheb.offb_valid); }
  int cheb_off_rows(SparseOp& op, DeviceBuffer<double>& off, bool& valid)
  {
    if (valid) return DLA_OK;
    bind();
    { const int stc = cheb_panel(off, (size_t)op.n); if (stc) return stc; }
    { const int stc = gershgorin<true>(op, nullptr, off); if (stc) return stc; }
    valid = true;
    return DLA_OK;
  }
  // r = 1 / den and hi = max_i q_i for this fac: one kernel, then the block maxima come to the host (one host wait per call)
  int cheb_jacobi_bound(double fac, double* hi)
  {
    SparseOp& op = ops[dla::SPMM_A];
    const int n = op.n;
    { const int stc = cheb_off(); if (stc) return stc; }
    { const int stc = cheb_panel(cheb.r, (size_t)n); if (stc) return stc; }
    const int blocks = grid_blocks(env(), n, 256);
    { const int stc = cheb_panel(cheb.partial, (size_t)grid_cap(env())); if (stc) return stc; }
    {
      Scope s(this, DLA_OP_PRECND, 24.0 * n, 4.0 * n, "cheb_jacobi_bound_kernel");
      DLA_LAUNCH(cheb_jacobi_bound_kernel, dim3(blocks), dim3(256), 0, st, n, fac, op.diagonal(), (const double*)cheb.off, (double*)cheb.r,
                 (double*)cheb.partial);
      HIPCHK(hipGetLastError());
    }
    { const int stc = max_of_blocks(cheb.partial, blocks, hi); if (stc) return stc; }
    stats.host_syncs++;
    return DLA_OK;
  }
  int spmm_cheb_jacobi_upper(double fac, double* hi) override
  {
    { const int stc = cheb_admit("spmm_cheb_jacobi_upper"); if (stc) return stc; }
    return cheb_jacobi_bound(fac, hi);
  }
  // the scale sweep of the scaled and the pencil form: y = x o r, or with one step px = (x o r) / theta at once
  int cheb_scale_sweep(int n, int m, const dla::ChebCoefficients& cf, const double* x, double* px, const double** y)
  {
    const bool one = cheb.steps == 1;
    const dim3 grid(grid_blocks(env(), n, 256));
    const double* r = cheb.r;
    Scope s(this, DLA_OP_PRECND, 16.0 * (double)n * m + 8.0 * n, (one ? 2.0 : 1.0) * (double)n * m, "cheb_jacobi_scale_kernel");
    if (one) DLA_LAUNCH(cheb_jacobi_scale_kernel<true>, grid, dim3(256), 0, st, n, m, cf.theta, r, x, px);
    else DLA_LAUNCH(cheb_jacobi_scale_kernel<false>, grid, dim3(256), 0, st, n, m, cf.theta, r, x, (double*)cheb.y);
    HIPCHK(hipGetLastError());
    *y = cheb.y;
    return DLA_OK;
  }
  int spmm_precnd_cheb_jacobi(int n, int m, double fac, const double* x, double* px) override
  {
    return cheb_apply<CHEB_SCALED>(
        "spmm_precnd_cheb_jacobi", n, m, fac, x, px,
        [&](double* hi, double* shift) -> int { *shift = 0.0; return cheb_jacobi_bound(fac, hi); },
        [&](const dla::ChebCoefficients& cf, const double** y) -> int { return cheb_scale_sweep(n, m, cf, x, px, y); });
  }

  // ---- ... and on the scaled pencil D^-1 (A + fac B), D = |diag(A) + fac diag(B)|, B the stored metric (the contract:
  // include/diaglib_amd.h, dla_spmm_precnd_cheb_pencil).  offB is the stored metric's as off is the stored operator's.
  int cheb_pencil_admit(const char* who)
  {
    const SparseOp &a = ops[dla::SPMM_A], &b = ops[dla::SPMM_B];
    if (a.fmt < 0 || !a.diag) { err = std::string(who) + ": no operator has been set up (dla_spmm_setup_csr)"; return DLA_ERR_ARG; }
    if (shard.on) { err = std::string(who) + ": the operator of this context is row-sharded, and the Chebyshev preconditioner on a row-sharded operator is not supported"; return DLA_ERR_ARG; }
    if (b.fmt < 0 || !b.diag) { err = std::string(who) + ": no metric has been set up (dla_spmm_setup_metric_csr)"; return DLA_ERR_ARG; }
    if (a.n != b.n) { err = std::string(who) + ": the operator has " + std::to_string(a.n) + " rows and the metric " + std::to_string(b.n); return DLA_ERR_ARG; }
    if (cheb.steps <= 0) { err = std::string(who) + ": nothing is configured (dla_spmm_cheb_config)"; return DLA_ERR_ARG; }
    return DLA_OK;
  }
  // r = 1 / den and hi = max_i q_i of the pencil for this fac: one kernel, one host wait per call
  int cheb_pencil_bound(double fac, double* hi)
  {
    SparseOp &op = ops[dla::SPMM_A], &opb = ops[dla::SPMM_B];
    const int n = op.n;
    { const int stc = cheb_off(); if (stc) return stc; }
    { const int stc = cheb_off_b(); if (stc) return stc; }
    { const int stc = cheb_panel(cheb.r, (size_t)n); if (stc) return stc; }
    const int blocks = grid_blocks(env(), n, 256);
    { const int stc = cheb_panel(cheb.partial, (size_t)grid_cap(env())); if (stc) return stc; }
    {
      Scope s(this, DLA_OP_PRECND, 40.0 * n, 7.0 * n, "cheb_pencil_bound_kernel");
      DLA_LAUNCH(cheb_pencil_bound_kernel, dim3(blocks), dim3(256), 0, st, n, fac, op.diagonal(), opb.diagonal(), (const double*)cheb.off,
                 (const double*)cheb.offb, (double*)cheb.r, (double*)cheb.partial);
      HIPCHK(hipGetLastError());
    }
    { const int stc = max_of_blocks(cheb.partial, blocks, hi); if (stc) return stc; }
    stats.host_syncs++;
    return DLA_OK;
  }
  int spmm_cheb_pencil_upper(double fac, double* hi) override
  {
    { const int stc = cheb_pencil_admit("spmm_cheb_pencil_upper"); if (stc) return stc; }
    double g = 0.0;
    { const int stc = cheb_pencil_bound(fac, &g); if (stc) return stc; }
    *hi = g;
    return DLA_OK;
  }
  int spmm_precnd_cheb_pencil(int n, int m, double fac, const double* x, double* px) override
  {
    return cheb_apply<CHEB_PENCIL>(
        "spmm_precnd_cheb_pencil", n, m, fac, x, px,
        [&](double* hi, double* shift) -> int { *shift = 0.0; return cheb_pencil_bound(fac, hi); },
        [&](const dla::ChebCoefficients& cf, const double** y) -> int { return cheb_scale_sweep(n, m, cf, x, px, y); });
  }

  // ---- ... and the four parts of the linear-response pencil (A B; B A)(Y Z) = w (S D; -D -S)(Y Z): A+B, A-B, S+D, S-D as the
  // callbacks apbmul / ambmul / spdmul / smdmul of caslr_eff_driver / caslr_driver apply them (reference diaglib.f90:1024-1025),
  // single rank.  Set-up, refresh, info and products are the operator's own functions on another SparseOp; nothing here or in the
  // product kernels assumes a symmetric matrix (S+D and S-D are not).
  int spmm_lrprec(int variant, int n, int m, double fac, const double* xp, const double* xm, double* yp, double* ym) override
  {
    const std::string who = variant == 1 ? "spmm_lrprec1" : "spmm_lrprec2";
    for (int slot : {(int)dla::SPMM_APB, (int)dla::SPMM_AMB, (int)dla::SPMM_SPD}) {
      const SparseOp& op = ops[slot];
      if (op.fmt < 0 || !op.diag) { err = who + ": " + words(slot).missing + " (dla_spmm_setup_lr_csr)"; return DLA_ERR_ARG; }
      if (n != op.n) { err = who + ": n = " + std::to_string(n) + " differs from the " + std::to_string(op.n) + " rows of " + words(slot).noun; return DLA_ERR_ARG; }
    }
    return launch_lr_precnd("", variant, n, m, fac, ops[dla::SPMM_APB].diag, ops[dla::SPMM_AMB].diag, ops[dla::SPMM_SPD].diag, xp, xm, yp, ym);
  }

  // ---- built-in operator
  int synth_setup(long long n_global, long long row0, int n_local, int rank_w, double sigma) override
  {
    (void)n_global;
    if (rank_w != 4) { err = "synth operator: rank_w must be 4"; return DLA_ERR_ARG; }
    bind();
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(d_t.reserve(4 * 64));
    HIPCHK(d_w.reserve((size_t)n_local * rank_w));
    HIPCHK(d_diag.reserve((size_t)n_local));
    HIPCHK(d_wsq.reserve((size_t)n_local));
    syn_row0 = row0; syn_n = n_local; syn_rw = rank_w; syn_sigma = sigma;
    DLA_LAUNCH(synth_build_kernel, dim3((n_local + 255) / 256), dim3(256), 0, st, row0, n_local, rank_w, sigma, d_w, d_diag, d_wsq);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return DLA_OK;
  }

  int synth_matvec(int n, int m, const double* x, double* ax) override { return synth_apply(SYN_A, n, m, x, ax); }
  // y = d x + W C W^T x for one of the sample operators (SynthKind)
  int synth_apply(int kind, int n, int m, const double* x, double* ax) override
  {
    if (n != syn_n) { err = "synth operator: n differs from setup"; return DLA_ERR_ARG; }
    if (m > 64) { err = "synth operator: m > 64"; return DLA_ERR_ARG; }
    if (kind < SYN_A || kind > SYN_METRIC) { err = "synth operator: unknown kind"; return DLA_ERR_ARG; }
    StepOut t_out;
    int stc = gram_dev(n, syn_rw, d_w, m, x, t_out, DLA_OP_MATVEC);   // t = W^T x (4 x m), reduced over ranks, on device
    if (stc) return stc;
    SynthCoupling cp{};
    const double tau = 0.05;
    for (int q = 0; q < 4; ++q) {
      if (kind == SYN_A || kind == SYN_APB) cp.c[q + 4 * q] = syn_sigma;
      else if (kind == SYN_AMB) cp.c[q + 4 * q] = 0.2 * syn_sigma;
      else if (kind == SYN_METRIC) cp.c[q + 4 * q] = 0.1;
    }
    if (kind == SYN_SPD || kind == SYN_SMD) {
      const double tj = kind == SYN_SPD ? tau : -tau;       // J: (0,1) = 1, (1,0) = -1, (2,3) = 1, (3,2) = -1
      cp.c[0 + 4 * 1] = tj; cp.c[1 + 4 * 0] = -tj; cp.c[2 + 4 * 3] = tj; cp.c[3 + 4 * 2] = -tj;
    }
    Scope s(this, DLA_OP_MATVEC, 8.0 * n * (2.0 * m + syn_rw), 2.0 * (double)n * m * (2 * syn_rw + 1));
    // (t = W^T x sits in d_small, reduced over ranks; nothing else touches that buffer before the kernel below has read it)
    const int blocks = grid_blocks(env(), n, 256);
    DLA_LAUNCH((synth_apply_kernel<4>), dim3(blocks), dim3(256), sizeof(double) * 4 * m, st,
                       syn_row0, n, m, kind, cp, d_w, (const double*)d_small, x, ax);
    HIPCHK(hipGetLastError());
    return DLA_OK;
  }
  int synth_lrprec(int variant, int n, int m, double fac, const double* xp, const double* xm, double* yp, double* ym) override
  {
    if (n != syn_n) { err = "synth_lrprec: n differs from setup"; return DLA_ERR_ARG; }
    Scope s(this, DLA_OP_PRECND, 8.0 * n * (4.0 * m + 1.0), 8.0 * (double)n * m);
    const int blocks = grid_blocks(env(), n, 256);
    DLA_LAUNCH(synth_lrprec_kernel, dim3(blocks), dim3(256), 0, st, syn_row0, n, m, variant, fac, syn_sigma, (const double*)d_wsq, xp, xm, yp, ym);
    HIPCHK(hipGetLastError());
    return DLA_OK;
  }

  int synth_precnd(int n, int m, double fac, const double* x, double* px) override
  {
    if (n != syn_n) { err = "synth_precnd: n differs from setup"; return DLA_ERR_ARG; }
    const bool vec2 = on_16_bytes(n, x, px);
    // (booked under the instance's name: which of the two ran is a decision of the alignment and of the peers' shards)
    Scope s(this, DLA_OP_PRECND, 8.0 * n * (2.0 * m + 1.0), (double)n * m, vec2 ? "synth_precnd_kernel<2>" : "synth_precnd_kernel<1>");
    const size_t nv = (size_t)n / (vec2 ? 2 : 1);
    const int blocks = grid_blocks(env(), (long long)nv, 256);
    if (vec2) DLA_LAUNCH(synth_precnd_kernel<2>, dim3(blocks), dim3(256), 0, st, n, m, fac, d_diag, x, px);
    else      DLA_LAUNCH(synth_precnd_kernel<1>, dim3(blocks), dim3(256), 0, st, n, m, fac, d_diag, x, px);
    HIPCHK(hipGetLastError());
    return DLA_OK;
  }
};

}  // namespace

namespace dla {

Engine* make_engine(int device, std::string& err)
{
  HipEngine* e = new HipEngine();
  if (e->init(device) != DLA_OK) {
    err = e->err;
    delete e;
    return nullptr;
  }
  return e;
}

int engine_unique_id(char id[128])
{
  ncclUniqueId uid;
  if (ncclGetUniqueId(&uid) != ncclSuccess) return DLA_ERR_COMM;
  std::memcpy(id, &uid, 128);
  return DLA_OK;
}

}  // namespace dla
