// What the HIP engine DECIDES before it launches: tile shape, passes and blocks of a sweep, its LDS bytes, quarter tiles,
// pipeline depth and row groups, the name its launch is booked under, and which schedule an orthogonalisation chain runs.
// Host-only (no HIP include): pure functions of a few integers, alignment booleans, the device's CU count and LDS limit, the
// knobs and the chain policy.  The planners have no members and touch no global; the engine owns every piece of state
// (remembered plans, the cooldown, the LDS limit, pointers) and passes what a decision reads.  hip_engine.hip takes a plan,
// books plan.name() and dispatches on the plan's fields; tests/plans_driver.cpp calls the same functions on the CPU.
// Which template instances of the Gram, pending-factor, panel-product and Ritz kernels exist is spelled once, in the lists below
// (GRAM_TILES, gram_direct_instance, GRAM_LOW_TILES, GRAM_LDS_FORMS, WP_TILES, GEMM_INSTANCES, RITZ_INSTANCES, RITZ2_INSTANCES): the
// planners round to a listed width, the engine's ladders instantiate exactly the listed instances and launch the one whose template
// arguments equal the plan's fields, or none, and tests/test_plans.py holds its own transcription against what the driver prints.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <iterator>
#include <string>
#include <tuple>
#include <vector>
#include "dla_internal.h"

namespace dla_plans {

// The experiment knobs (options DLA_OPT_TUNE0 + i, i = 0 .. 7): what the tests, the benchmark ($DIAGLIB_BENCH_TUNE) and the A/B and fuzz
// tools switch by number.  All 0 is the product; a value that is not named here selects nothing.  The numbers stand in this struct
// and nowhere else: the engine asks one predicate per decision.  (The same table for the tools' side: tools/README.md.)
struct Knobs {
  int tune[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  void set(int i, int v) { if (i >= 0 && i < 8) tune[i] = v; }
  int get(int i) const { return (i >= 0 && i < 8) ? tune[i] : 0; }
  // ---- knob 0: the Ritz sweep (ritz_residual_once, ritz_residual_p, ritz_residual2)
  // 1 / 4: column-step pipeline of depth 0 / 4 for plain blocks of two and three tiles, no quarter tiles; -1: the kernel's own (tools/tune_ab.py)
  int ritz_pipe_depth() const { return tune[0] == 1 ? 0 : tune[0] == 4 ? 4 : -1; }
  // 5: Ritz step and P products never in one pass (A/B switch, no record kept)
  bool ritz_p_separate() const { return tune[0] == 5; }
  // 6: the two-coefficient sweep ritz2_kernel off, three sweeps instead (A/B switch, no record kept)
  bool no_ritz2() const { return tune[0] == 6; }
  // 16: the Ritz sweep that also forms and measures the next block (davidson_expand_kernel) off: dla_ritz_expand is dla_ritz_residual
  // (A/B and parity switch, tests/test_ritz_expand_solves_gpu.py)
  bool no_ritz_expand() const { return tune[0] == 16; }
  // 17: the Davidson driver predicts one lock more than its rule says, so that fused sweeps are discarded (same test)
  bool ritz_expand_overpredict() const { return tune[0] == 17; }
  // ---- knob 1: blocks of a Ritz sweep, as a multiple of the built-in count (tools/tune_ab.py)
  int ritz_grid_factor() const { return tune[1] > 0 ? tune[1] : 1; }
  // ---- knob 2: the plain panel product (gemm_chunk)
  // 1 / 4: as knob 0 = 1 / 4, for the plain product and update of two and three tiles (tools/tune_ab.py)
  int gemm_pipe_depth() const { return tune[2] == 1 ? 0 : tune[2] == 4 ? 4 : -1; }
  // ---- knob 3: > 0: cap on resident blocks per CU of the panel-product kernels (tools/tune_fused.py)
  int gemm_blocks_per_cu() const { return tune[3] > 0 ? tune[3] : 0; }
  // ---- knob 4: blocks of the Gram sweeps
  // > 0: blocks per pass of gram_plan and wp_plan (tools/tune_ab.py, tools/ab/combox_ab.py)
  int gram_blocks_override() const { return tune[4] > 0 ? tune[4] : 0; }
  // -1: the measuring sweeps of up to five X tiles with one block per CU (measured r05, see wp_plan)
  bool wp_one_block_per_cu() const { return tune[4] == -1; }
  // ---- knob 5: the Gram kernels and their reduction
  // 2: the direct-load gram_kernel everywhere (tools/tune_gram.py)
  bool direct_gram() const { return tune[5] == 2; }
  // 3: GramReduceArgs::fenced (tests/test_ortho_chain_gpu.py requires identical bits)
  bool fenced_reduce() const { return tune[5] == 3; }
  // ---- knob 6: the orthogonalisation chain
  // 2: the host polls the stream, no event packet (wait_stream)
  bool poll_stream() const { return tune[6] == 2; }
  // 3: no chain, the host-driven loop (parity knob of tests/test_ortho_chain_gpu.py, tools/fuzz_parity.py)
  bool host_loop() const { return tune[6] == 3; }
  // 4: the cross-rank exchange as a launch of its own, not in the reduction kernel (A/B switch, no record kept; bench.py's own example)
  bool exchange_own_launch() const { return tune[6] == 4; }
  // 5: one-tile blocks keep the LDS-loop k x k step of ortho_tail_kernel (A/B switch, no record kept)
  bool no_mfma_kxk() const { return tune[6] == 5; }
  // 6: one-tile blocks on the sweep-per-update schedule (A/B switch, no record kept)
  bool no_pending_factor() const { return tune[6] == 6; }
  // 7 / 8: wide blocks without the one-sweep [X | U] Gram (tools/wide_solve_ab.py, tools/iters_probe.py)
  bool no_wide_gramx() const { return tune[6] == 7 || tune[6] == 8; }
  // 7 also: the leading ortho_cd runs to convergence (OrthoTailArgs::lead_once = 0)
  bool lead_full() const { return tune[6] == 7; }
  // 9: wide blocks without the storing sweep OP_XW (tools/ab/wide_xw_ab.py)
  bool no_wide_xw() const { return tune[6] == 9; }
  // 10: the storing sweep for three-tile blocks too (measured r04, see chain_choice)
  bool wide_xw_three_tiles() const { return tune[6] == 10; }
  // 11: b_ortho_ahead declines: the metric Cholesky-QR waits for the chain (A/B switch, no record kept)
  bool no_b_ortho_ahead() const { return tune[6] == 11; }
  // 12: never the three-pass schedule (tests, tools/fuzz_ortho.py, tools/profile_all.sh)
  bool five_sweep() const { return tune[6] == 12; }
  // 13: the three-pass schedule from the first chain, no cooldown (same)
  bool three_pass_always() const { return tune[6] == 13; }
  // 14: basis_exact_ok() answers no (tools/ab/exact_ab.sh, tests/test_pending_basis_gpu.py)
  bool mode5_as_mode4() const { return tune[6] == 14; }
  // what basis_exact_ok() needs of the three above
  bool no_exact_basis() const { return host_loop() || no_mfma_kxk() || mode5_as_mode4(); }
  // OrthoTailArgs::gp; 15: from U^T U as the reference's, 16: level shifts on the projected block's Gram matrix (tools/ab/exact_ab.sh, see launch_op)
  int first_factor_source() const { return tune[6] == 15 ? 0 : tune[6] == 16 ? 2 : 1; }
  // 17: plans keep OP_CLOSE / OP_FINAL where the caller takes the closing block (r05 trace, see chain_lean)
  bool keep_closing_launches() const { return tune[6] == 17; }
  // ---- knob 7: kernel variants of the wide blocks (tools/quarter_tile_ab.py unless another record is named)
  // 1: full 16x16x4 tiles only (tests/test_quarter_tiles_gpu.py compares both)
  bool no_quarter_tiles() const { return tune[7] == 1; }
  // 2: GramArgs::noskip, the loads of fully padded column groups are issued too
  bool gram_load_pads() const { return tune[7] == 2; }
  // 3: Gram passes of at most 12 accumulator tiles
  bool narrow_gram_passes() const { return tune[7] == 3; }
  // 4: the row products do not load the next row tile ahead (GemmArgs::xpf = 0)
  bool no_next_tile_prefetch() const { return tune[7] == 4; }
  // 5: 64-row wave tiles (RTP = 2) in the fused three-tile sweep
  bool fused3_two_row_groups() const { return tune[7] == 5; }
  // 8: the lower triangle of two panels in several passes, not gram_lds_kernel LOW
  bool no_low_single() const { return tune[7] == 8; }
  // 9: small_copy_kernel instead of the runtime's copy (see stage_slot)
  bool own_copy_kernel() const { return tune[7] == 9; }
  // 22 / 23: one first-level group per 16 / 64 block partials (measured r06, DESIGN "Measured and rejected")
  int reduce_group_size() const { return tune[7] == 22 ? 16 : tune[7] == 23 ? 64 : 32; }
  // 30: a step of the Chebyshev preconditioner as the product kernel plus one combining sweep, not fused (tools/cheb_precnd_ab.py)
  bool cheb_unfused() const { return tune[7] == 30; }
};

// Sizes the engine's buffers and the tail kernels' LDS are built with, and that decisions read (one spelling: the engine and its kernels
// use these).  DMAT_LD: columns of the device copy of the caller's pending blocks, the rows of the coefficient block that the exact
// projection of ortho_tail16 keeps in LDS; XUG_DOUBLES: the buffer that takes X^T U | U^T U of a storing sweep; P2P_MAX_DOUBLES: one
// mailbox slot of the peer-to-peer transport (128 KB: the widest projection block of BASELINE cfg 4/5 fits); PEND_ROWS: rows of the
// pending-block buffer
constexpr int DMAT_LD = 320, XUG_DOUBLES = 640 * 16, P2P_MAX_DOUBLES = 16384, PEND_ROWS = 640;

// what every planner needs of the engine
struct PlanEnv { int ncu; size_t lds_limit; const Knobs& knobs; };

// The grid of a grid-stride kernel on blocks of 256 threads: `items` things to do, `per_block` of them to a block (256: one per
// thread; 4: one per wavefront), at most per_cu blocks per compute unit (grid_cap) and at least one.
inline int grid_cap(const PlanEnv& env, int per_cu = 8) { return std::max(1, env.ncu * per_cu); }
inline int grid_blocks(const PlanEnv& env, long long items, long long per_block, int per_cu = 8)
{
  return (int)std::max(1LL, std::min((long long)grid_cap(env, per_cu), (items + per_block - 1) / per_block));
}

template <typename... A>
inline std::string plan_name(const char* fmt, A... a)
{
  char kn[96];
  std::snprintf(kn, sizeof kn, fmt, a...);
  return kn;
}

// quarter tiles of the last 16-column tile (0: none): blocks of 17..24 and 33..40 columns on the 16-byte path
inline int quarter_tiles(const PlanEnv& env, int k, bool vec2)
{
  const int kt = (k + 15) / 16, rem = k - 16 * (kt - 1);
  return (vec2 && kt >= 2 && kt <= 3 && rem <= 8 && !env.knobs.no_quarter_tiles()) ? (rem + 3) / 4 : 0;
}
// resident blocks per CU that the dynamic LDS of a panel-product or Ritz sweep leaves room for
inline int blocks_per_cu(size_t lds) { return lds > 80 * 1024 ? 1 : lds > 40 * 1024 ? 2 : 4; }

// ---- the instance lists: one row per template instance the engine's ladders can launch (plain integers, compile-time); for a family
// that is a product of flags, the rows that a predicate over the flags admits
// gram_kernel / gram_lds_kernel passes of kt U-tiles x tlw X-tiles
struct GramTile { int tlw, kt; };
constexpr GramTile GRAM_TILES[] = {
  {1, 1}, {2, 1}, {3, 1}, {4, 1}, {5, 1}, {6, 1}, {7, 1}, {8, 1}, {10, 1}, {12, 1},
  {1, 2}, {2, 2}, {3, 2}, {4, 2}, {5, 2}, {6, 2}, {7, 2}, {8, 2},
  {1, 3}, {2, 3}, {3, 3}, {4, 3}, {5, 3}, {6, 3}, {7, 3},
  {1, 4}, {2, 4}, {3, 4}};
// ... of which the direct-load gram_kernel has these (the LDS-staged kernel has every listed pair of up to three U tiles)
constexpr bool gram_direct_instance(int tlw, int kt)
{
  return !(tlw == 5 || tlw == 7 || tlw == 10 || (tlw == 12 && kt > 1) || (tlw == 3 && kt >= 2 && kt <= 3) || (tlw >= 5 && kt == 3) ||
           (tlw >= 7 && kt == 2));
}
// gram_lds_kernel<tlw, kt, 1, R, self, qt> of a listed pass: SELF (a block against itself, staged once) only where both sides have the
// same tiles, quarter tiles of the last U tile only behind a full one
struct GramLdsForm { int self, qt; };
constexpr GramLdsForm GRAM_LDS_FORMS[] = {{0, 0}, {0, 1}, {0, 2}, {1, 0}, {1, 1}, {1, 2}};
constexpr bool gram_lds_form(int tlw, int kt, const GramLdsForm& f) { return !(f.self && tlw != kt) && !(f.qt > 0 && kt < 2); }
// tiles per side of the single-pass lower triangle (gram_lds_kernel LOW)
constexpr int GRAM_LOW_TILES[] = {4, 5, 6, 7};
// sweeps of the pending-factor schedule (gram_lds_kernel WP), with the rows R of a staged tile
struct WpTile { int tlw, kt, R; };
constexpr WpTile WP_TILES[] = {
  {1, 1, 32}, {2, 1, 32}, {3, 1, 16}, {4, 1, 16}, {5, 1, 16}, {6, 1, 16}, {7, 1, 16}, {8, 1, 16}, {10, 1, 16}, {12, 1, 16},
  {1, 2, 16}, {2, 2, 16}, {3, 2, 16}, {4, 2, 16}, {5, 2, 16}, {6, 2, 16}, {7, 2, 16}, {8, 2, 16},
  {1, 3, 16}, {2, 3, 16}, {3, 3, 16}, {4, 3, 16}, {5, 3, 16}};
// ritz_kernel<kt, vec, 3, pipe, qt, xp>
struct RitzInstance { int kt, vec, pipe, qt; bool xp; };
constexpr RitzInstance RITZ_INSTANCES[] = {
  // [Y | C2] with extra products (16-byte path only); (pipeline depth 2 / 4 of the five-tile one measured: 8.9 / 7.9 ms against 7.5
  // at 37 + 37 columns)
  {2, 2, 2, 1, true}, {3, 2, 3, 1, true}, {2, 2, 2, 2, true}, {3, 2, 3, 2, true},
  {1, 2, 0, 0, true}, {2, 2, 2, 0, true}, {3, 2, 3, 0, true}, {4, 2, 3, 0, true}, {5, 2, 3, 0, true},
  // plain, 16-byte path: the depths of Knobs::ritz_pipe_depth, quarter tiles, the kernels' own depth
  {2, 2, 0, 0, false}, {3, 2, 0, 0, false}, {2, 2, 4, 0, false}, {3, 2, 4, 0, false},
  {2, 2, 2, 1, false}, {3, 2, 3, 1, false}, {2, 2, 2, 2, false}, {3, 2, 3, 2, false},
  {1, 2, 0, 0, false}, {2, 2, 2, 0, false}, {3, 2, 3, 0, false},
  // plain, 8-byte path
  {1, 1, 0, 0, false}, {2, 1, 2, 0, false}, {3, 1, 3, 0, false}};
// ritz2_kernel<kt, vec>: the sweep with two coefficient blocks
struct Ritz2Instance { int kt, vec; };
constexpr Ritz2Instance RITZ2_INSTANCES[] = {{1, 1}, {1, 2}, {2, 1}, {2, 2}, {3, 1}, {3, 2}};
// davidson_expand_kernel<tx>: the Ritz sweep that also forms and measures the next block, tx column tiles of the basis
constexpr int RITZ_EXPAND_TILES[] = {1, 2, 3, 4, 5, 6, 7};
// gemm_kernel<kt, vec, mode, inl ? GemmArgsInl : GemmArgs, fuse, mode == 2 ? 0 : 1, pipe, 9, qt, rtp>: a product of independent flags, so the
// set is a predicate over them; GEMM_INSTANCES below is the same set as rows, for the ladder
struct GemmInstance { int kt, vec, mode; bool inl, fuse; int pipe, qt, rtp; };
constexpr bool gemm_instance(const GemmInstance& g)
{
  if (g.fuse && g.mode == 3) return false;                                       // the fused form: Z = XC, Z -= XC and U <- U W only
  if (g.inl && g.kt != 1) return false;                                          // 16 x 16 coefficients fit the kernel arguments
  if (g.qt > 0 && !(g.vec == 2 && g.kt >= 2)) return false;                      // quarter tiles: the 16-byte path, behind a full tile
  if (g.qt > 0 && !g.fuse && g.mode == 1 && g.kt == 2) return false;             // ... and never the plain two-tile update (gemm_plan)
  if (g.rtp == 1 && !(g.fuse && g.kt == 3 && g.vec == 2)) return false;          // one row group: the fused three-tile sweep only
  if (g.pipe == ((g.fuse && g.kt >= 3) ? 3 : g.kt >= 2 ? 2 : 0)) return true;    // the kernel's own depth: 0 / 2 / 2 plain, 0 / 2 / 3 fused
  // the depths of Knobs::gemm_pipe_depth: the plain product and update of two and three tiles, no quarter tiles
  return (g.pipe == 0 || g.pipe == 4) && !g.fuse && g.vec == 2 && g.kt >= 2 && g.mode <= 1 && g.qt == 0;
}
// candidate c of the box kt 1 .. 3 x vec 1 .. 2 x mode 0 .. 3 x inl x fuse x depth 0 .. 4 x qt 0 .. 2 x rtp 1 .. 2
constexpr int GEMM_CANDIDATES = 3 * 2 * 4 * 2 * 2 * 5 * 3 * 2;
constexpr GemmInstance gemm_candidate(int c)
{
  GemmInstance g{};
  g.rtp = 1 + c % 2; c /= 2;  g.qt = c % 3; c /= 3;  g.pipe = c % 5; c /= 5;  g.fuse = c % 2; c /= 2;  g.inl = c % 2; c /= 2;
  g.mode = c % 4; c /= 4;  g.vec = 1 + c % 2; c /= 2;  g.kt = 1 + c;
  return g;
}
constexpr int gemm_instance_count()
{
  int n = 0;
  for (int c = 0; c < GEMM_CANDIDATES; ++c) n += gemm_instance(gemm_candidate(c)) ? 1 : 0;
  return n;
}
struct GemmInstanceList { GemmInstance row[gemm_instance_count()]; };
constexpr GemmInstanceList gemm_instances()
{
  GemmInstanceList list{};
  int n = 0;
  for (int c = 0; c < GEMM_CANDIDATES; ++c)
    if (gemm_instance(gemm_candidate(c))) list.row[n++] = gemm_candidate(c);
  return list;
}
constexpr GemmInstanceList GEMM_INSTANCES = gemm_instances();
// "round up to an instantiated width": the narrowest listed pass of kt U-tiles that holds `want` X-tiles and that `ok` admits; null
// when the list has none (the planner keeps its width, and the ladder reports that there is no kernel instance)
template <typename Tile, size_t N, typename Ok>
constexpr const Tile* listed_pass(const Tile (&list)[N], int kt, int want, Ok ok)
{
  const Tile* best = nullptr;
  for (const Tile& t : list)
    if (t.kt == kt && t.tlw >= want && ok(t) && (!best || t.tlw < best->tlw)) best = &t;
  return best;
}

// ---- Gram
// whether a pass of tlw + kt tiles can be staged 32 rows at a time at all, and the rows per step of the direct-load kernel
constexpr bool gram_can32(int tlw, int kt) { return sizeof(double) * 4 * 16 * (tlw + kt) * 34 <= 150 * 1024 && tlw + kt <= 7; }
constexpr int gram_rs(int tlw, int kt) { return (tlw * kt >= 6) ? 2 : 4; }
// tile rows of the LDS-staged kernel: 32 for narrow passes (few loads per tile otherwise) and for 3-tile U blocks,
// 16 elsewhere (A/B at n = 2e6, tools/tune_gram.py)
inline int lds_rows(const PlanEnv& env, int tlw, int kt)
{
  const int r = ((tlw <= 2 || kt == 3) && tlw + kt <= 7) ? 32 : 16;   // (more than 7 tiles of 32 rows: too many staging registers)
  return (r == 32 && sizeof(double) * 4 * 16 * (size_t)(tlw + kt) * 34 > env.lds_limit) ? 16 : r;
}
// (a pass narrower than one tile, e.g. the 4-column W^T x of the benchmark operator, would stage mostly
// duplicates of its last column: it keeps the direct-load kernel)
inline bool use_lds_gram(const PlanEnv& env, bool vec2, int l, int kt) { return vec2 && kt <= 3 && l > 8 && !env.knobs.direct_gram(); }

// dynamic LDS of a gram_lds_kernel launch: per wave the staged columns of one pass (one operand for SELF, both panels for LOW), rows + 2
// doubles each.  The launch templates size their launch with it from their own template arguments, the plan from its fields.
constexpr size_t gram_lds_bytes(int tlw, int kt, int rows, bool self, bool low)
{
  return sizeof(double) * 4 * 16 * (size_t)(low ? 2 * tlw : self ? tlw : tlw + kt) * (size_t)(rows + 2);
}
// Pass shape of one Gram launch (gram_plan): the kernel's name for the statistics and the instance that is launched are both
// read from it.
struct GramPlan {
  int tlw, kt;           // tile shape of one pass: KT U-tiles x TLW X-tiles
  int px, passes;        // passes over X, passes in all
  int rows;              // rows of a staged tile (LDS-staged kernel): 16 or 32
  bool lds;              // the LDS-staged kernel (gram_lds_kernel), else the direct-load one (gram_kernel)
  bool self;             // ... a block against itself in one pass: staged once (gram_lds_kernel SELF)
  int qt;                // ... quarter tiles of its last U tile (gram_lds_kernel QT)
  bool low_single;       // ... the lower triangle of two different panels in a single pass (gram_lds_kernel LOW)
  bool lower;            // only the tile pairs on or below the block diagonal are formed
  int blocks_per_pass;
  bool vec2;             // the 16-byte path
  // the name rocprofv3 prints for the instance gram_dev_once picks from GRAM_TILES / GRAM_LOW_TILES
  std::string name() const
  {
    if (lds) return plan_name("gram_lds_kernel<%d, %d, 1, %d, %d, %d, %d, 0>", tlw, kt, rows, self ? 1 : 0, qt, low_single ? 1 : 0);
    return plan_name("gram_kernel<%d, %d, %d, %d, 0, -1>", tlw, kt, vec2 ? 2 : 1, gram_rs(tlw, kt));
  }
  size_t lds_bytes() const { return lds ? gram_lds_bytes(tlw, kt, rows, self, low_single) : 0; }
};
// same: x == u; aligned: both panels start on 16 bytes and every rank has an even row count -- with n even that is the 16-byte path,
// the `vec2` that the callers of the other planners pass ready-made
inline GramPlan gram_plan(const PlanEnv& env, int n, int l, int k, bool same, bool aligned, bool lower)
{
  const Knobs& knobs = env.knobs;
  const int tx = (l + 15) / 16, tu = (k + 15) / 16;
  // tile shape of one pass: KT U-tiles x TLW X-tiles, at most 12 accumulators
  const bool vec2 = n % 2 == 0 && aligned;
  // (even n: at most 3 U tiles per pass, so that the LDS-staged kernel serves every pass -- the direct-load kernel a
  // fourth tile would need measured 2.6 TB/s on the 111-column S^T A S of LOBPCG at n_max = 37)
  int kt = std::min(tu, (vec2 && l > 8 && !knobs.direct_gram()) ? 3 : 4);
  const int passes_u = (tu + kt - 1) / kt;
  kt = (tu + passes_u - 1) / passes_u;
  const bool ldsk = use_lds_gram(env, vec2, l, kt);
  // widest pass: the direct-load kernel loses its register prefetch stage beyond 8 tiles (measured); the LDS-staged
  // one keeps all of X's columns of up to 12 tiles in one pass, so U is read once for L <= 192
  static const int maxtl[5] = {0, 8, 6, 4, 3};
  // (the LDS-staged kernel runs at one wave per SIMD for wide passes anyway; its accumulators spill over into the
  // AGPRs, up to 21 tiles: fewer passes = fewer re-reads of U, and `lower` passes skip the tiles above the diagonal)
  static const int maxtl_lds[4] = {0, 12, 8, 7};
  int mt = ldsk ? maxtl_lds[kt] : maxtl[kt];
  if (knobs.narrow_gram_passes()) mt = (ldsk && kt == 1) ? 12 : maxtl[kt];       // A/B: the narrower passes
  // the LDS-staged kernel stages 16 (tlw + kt) columns of 18 doubles per wave: keep the pass inside lds_limit
  if (ldsk) mt = std::max(1, std::min(mt, (int)(env.lds_limit / (sizeof(double) * 4 * 16 * 18)) - kt));
  const int passes_x = (tx + mt - 1) / mt;
  int tlw = (tx + passes_x - 1) / passes_x;
  // round up to an instantiated width
  if (const GramTile* t = listed_pass(GRAM_TILES, kt, tlw, [&](const GramTile& g) { return ldsk || gram_direct_instance(g.tlw, g.kt); })) tlw = t->tlw;
  int px = (tx + tlw - 1) / tlw;
  int passes = px * passes_u;
  // a block against itself in a single pass: one staged image serves both operands, and only the tile pairs on or
  // below the diagonal are formed (the host side mirrors, see gram())
  const bool self = ldsk && same && l == k && passes == 1 && tlw == kt;
  if (self) lower = true;
  int qt = (ldsk && passes_u == 1 && kt >= 2) ? quarter_tiles(env, k, vec2) : 0;
  // the lower triangle of X^T U for two different panels of 49..112 columns (S^T A S of LOBPCG at n_max = 21 / 37):
  // one pass over both panels with the 10..28 tile pairs on or below the diagonal (gram_lds_kernel LOW)
  const bool low_single = lower && ldsk && !self && l == k && tx >= 4 && tx <= 7 && passes > 1 && !knobs.no_low_single() &&
                          sizeof(double) * 4 * 16 * (size_t)(2 * tx) * 18 <= env.lds_limit;
  if (low_single) { kt = tlw = tx; px = 1; passes = 1; qt = 0; }
  const int ch = vec2 ? 32 : 16;
  long long nchunks = ((long long)n + ch - 1) / ch;
  long long want = (nchunks + 4 * 4 - 1) / (4 * 4);   // >= 4 chunks per wave
  // one 4-wave block per CU and pass (256 on MI355X) measured best: 512 is -1.5 %, 384 / 128 are -15 / -30 %
  int blocks_per_pass = (int)std::max(1LL, std::min((long long)env.ncu, want));
  // the narrowest sweeps (a block against itself, or fewer than 8 columns against a block) have too few loads in
  // flight with one block per CU: two per CU measured +11 % / +19 % there and -1..-3 % everywhere else
  if (tlw * kt == 1 && ((same && l == k) || l <= 8)) blocks_per_pass = (int)std::max(1LL, std::min(2LL * env.ncu, want));
  if (knobs.gram_blocks_override()) blocks_per_pass = (int)std::max(1LL, std::min((long long)knobs.gram_blocks_override(), want));
  const int rows = (ldsk && !low_single && gram_can32(tlw, kt) && lds_rows(env, tlw, kt) == 32) ? 32 : 16;
  return GramPlan{tlw, kt, px, passes, rows, ldsk, self, qt, low_single, lower, blocks_per_pass, vec2};
}

// ---- sweeps of the pending-factor schedule (gram_lds_kernel WP)
// widest X pass of the pending-factor sweeps: 12 X tiles beside one U tile, 8 beside two (16 + 3 accumulator tiles), 5 beside
// three (15 + 6)
inline int wp_max_tlw(int kt) { return kt <= 1 ? 12 : kt == 2 ? 8 : 5; }
// pass shape of a pending-factor sweep: what the kernel's name, its instance and the reduction behind it are all read from
struct WpPlan {
  int tlw, kt, R, passes, blocks, extra, slots;
  bool self;             // m == 0: the block against itself
  bool project;          // the projection sweep that measures what it stores (WP == 2), else the measuring / storing one (WP == 1)
  std::string name() const { return plan_name("gram_lds_kernel<%d, %d, 1, %d, %d, 0, 0, %d>", tlw, kt, R, self ? 1 : 0, project ? 2 : 1); }  size_t lds_bytes() const { return gram_lds_bytes(tlw, kt, R, self, false); }
};
inline WpPlan wp_plan(const PlanEnv& env, int n, int m, int k, bool project)
{
  const Knobs& knobs = env.knobs;
  WpPlan p{};
  p.self = (m == 0);
  p.project = project;
  p.kt = (k + 15) / 16;
  const int tx = p.self ? 1 : (m + 15) / 16;
  p.passes = p.self ? 1 : (tx + wp_max_tlw(p.kt) - 1) / wp_max_tlw(p.kt);
  p.tlw = (tx + p.passes - 1) / p.passes;
  // the staged image of the widest pass: 13 tiles of 16 rows (4 waves x 13 x 16 x 18 doubles = 117 KiB); under a refused
  // LDS raise the chain is not taken at all (ortho_chain).  (A block against itself is one tile beside one: 32 rows.)
  p.R = 16;
  if (const WpTile* t = listed_pass(WP_TILES, p.kt, p.tlw, [](const WpTile&) { return true; })) { p.tlw = t->tlw; p.R = t->R; }
  const long long nchunks = ((long long)n + 31) / 32;
  const long long want = (nchunks + 15) / 16;
  // (one U tile beside up to five X tiles: at most 212 / 252 registers and 55 KB of LDS per block -- two blocks per CU, two waves
  //  per SIMD: measured r05 at n = 2e6, interleaved: +5 ... 11 % for the projection sweep, +3 ... 9 % for the storing one; beyond
  //  five tiles the kernels need more than 256 registers and a second block per CU only runs behind the first)
  p.blocks = (int)std::max(1LL, std::min((long long)env.ncu * ((p.self || (p.kt == 1 && p.tlw <= 5 && !knobs.wp_one_block_per_cu())) ? 2 : 1), want));
  if (knobs.gram_blocks_override()) p.blocks = (int)std::max(1LL, std::min((long long)knobs.gram_blocks_override(), want));
  p.extra = p.self ? 0 : p.kt * (p.kt + 1) / 2;          // tiles (qi >= qj) of the Gram matrix of the U block
  p.slots = p.self ? 1 : p.tlw * p.kt + p.extra;
  return p;
}

// ---- panel product (gemm_kernel)
// The variant, decided once: quarter tiles, pipeline depth and row groups go into the booked name AND pick the instance.
struct GemmPlan {
  int kt, l4;
  bool inl;              // the coefficient block travels in the kernel arguments (GemmArgsInl)
  int qt;                // quarter tiles of the last column tile
  size_t lds;
  int per_cu, rtp, pipe, blocks;
  bool vec2, fuse;
  int mode;
  // whether g is the instance this plan names
  bool names(const GemmInstance& g) const
  {
    return kt == g.kt && (vec2 ? 2 : 1) == g.vec && mode == g.mode && inl == g.inl && fuse == g.fuse && pipe == g.pipe && qt == g.qt && rtp == g.rtp;
  }
  std::string name() const
  {
    return plan_name("gemm_kernel<%d, %d, %d, %s, %s, %d, %d, 9, %d, %d>", kt, vec2 ? 2 : 1, mode, inl ? "GemmArgsInl" : "GemmArgs",
                     fuse ? "true" : "false", mode == 2 ? 0 : 1, pipe, qt, rtp);
  }
};
// fuse: the variant that also leaves the partials of the result's Gram matrix; packed_on_device: the coefficient block is already
// packed in device memory
inline GemmPlan gemm_plan(const PlanEnv& env, int n, int l, int k, int mode, bool fuse, bool packed_on_device, bool vec2)
{
  const Knobs& knobs = env.knobs;
  const int kt = (k + 15) / 16;
  const int l4 = ((l + 3) / 4) * 4;
  const bool inl = (!packed_on_device && kt == 1 && l4 <= 16);
  const int ab_depth = fuse ? -1 : knobs.gemm_pipe_depth();
  int qt = ab_depth >= 0 ? 0 : quarter_tiles(env, k, vec2);
  // (the plain two-tile update is the one sweep that measured slower with quarter tiles, -9 % at L = 63, k = 21:
  // tools/quarter_tile_ab.py)
  if (!fuse && mode == 1 && kt == 2) qt = 0;
  // LDS copy of C (a quarter-tile kernel keeps 8 columns of the last tile); the fused variant adds 4 wave tiles of
  // 16 rows x (16 kt + 9) doubles, and needs >= 8 KiB for the final reduction
  const size_t lds_c = sizeof(double) * (size_t)l4 * (qt > 0 ? 16 * (kt - 1) + 8 : 16 * kt);
  const size_t lds = fuse ? std::max(lds_c + sizeof(double) * 4 * 16 * (16 * kt + 9), (size_t)8192) : lds_c;
  int per_cu = blocks_per_cu(lds);
  if (knobs.gemm_blocks_per_cu()) per_cu = (int)std::max((size_t)1, std::min((size_t)knobs.gemm_blocks_per_cu(), (size_t)(156 * 1024) / std::max(lds, (size_t)4096)));
  // row groups per wave tile (gemm_kernel RTP): the fused three-tile sweeps need > 256 registers with two groups, one
  // wave per SIMD; with one group two fit -- when the LDS leaves room for a second block per CU (measured +9..20 %,
  // and -26 % when it does not)
  const int rtp = (fuse && kt == 3 && vec2 && per_cu >= 2 && !knobs.fused3_two_row_groups()) ? 1 : 2;
  const int pipe = (ab_depth >= 0 && vec2 && kt >= 2 && (mode == 0 || mode == 1)) ? ab_depth : (fuse && kt >= 3) ? 3 : kt >= 2 ? 2 : 0;
  const int wt = (vec2 ? 32 : 16) * rtp;
  const long long ntiles = ((long long)n + wt - 1) / wt;
  const int blocks = (int)std::max(1LL, std::min((long long)env.ncu * per_cu, (ntiles + 3) / 4));
  return GemmPlan{kt, l4, inl, qt, lds, per_cu, rtp, pipe, blocks, vec2, fuse, mode};
}

// dynamic LDS of a fused sweep as the engine's decisions read it (can_combo, the fused update and triangular update, ChainIn::fused_lds_kk):
// packed C (l rows) + 4 wave-private transpose tiles.  Not GemmPlan::lds, which knows the quarter tiles of the launch itself.
inline size_t fused_lds(int l, int k)
{
  const int kt = (k + 15) / 16, l4 = ((l + 3) / 4) * 4;
  return std::max(sizeof(double) * ((size_t)kt * l4 * 16 + (size_t)4 * 16 * (16 * kt + 9)), (size_t)8192);
}

// ---- Ritz sweep (ritz_kernel, ritz2_kernel)
// dynamic LDS a Ritz sweep may ask for: the four- and five-tile kernels keep their norm accumulators in 48.6 KiB of static LDS
inline size_t ritz_lds_cap(int kt) { return (size_t)(kt >= 4 ? 100 : 150) * 1024; }
// static LDS of ritz_kernel: theta / active, and for four and five tiles the per-lane norm accumulators (s_nrm, 48 KiB)
inline size_t ritz_static_lds(int kt) { return (size_t)1024 + (kt >= 4 ? sizeof(double) * 4 * 48 * 16 * 2 : 0); }
// dynamic LDS a Ritz sweep of kt column tiles may ask for: its own cap, and the engine's limit minus what the kernel holds statically
inline size_t ritz_dyn_limit(const PlanEnv& env, int kt)
{
  const size_t st_ = ritz_static_lds(kt);
  return std::min(ritz_lds_cap(kt), env.lds_limit > st_ ? env.lds_limit - st_ : (size_t)0);
}
// what ritz_kernel and ritz2_kernel share: the launch's LDS and grid, and the reduction behind it
struct RitzGrid {
  size_t lds;
  int per_cu, blocks;
  int ncol, nslots;      // columns of the reduction, and one slot of maxima per rank behind the sums
  size_t small_doubles() const { return (size_t)ncol * (1 + nslots); }
};
inline RitzGrid ritz_grid(const PlanEnv& env, int n, bool vec2, int kt, size_t lds_c, int grid_factor, int nranks_slots)
{
  const int rg = vec2 ? 32 : 16;
  const long long ntiles = ((long long)n + rg - 1) / rg;
  const size_t lds = std::max(lds_c, sizeof(double) * 4 * 16 * kt * 2);
  const int per_cu = blocks_per_cu(lds);
  const int blocks = (int)std::max(1LL, std::min((long long)env.ncu * per_cu * grid_factor, (ntiles + 7) / 8));
  return RitzGrid{lds, per_cu, blocks, 16 * kt, nranks_slots};
}
// The variant, decided once: quarter tiles, pipeline depth and extra products go into the booked name AND pick the instance.
struct RitzPlan : RitzGrid {
  int kt;                // column tiles of [Y | C2]
  int l4, qt;
  bool xp;               // extra products ride along (k2 > 0)
  int pipe;
  size_t lds_c;          // LDS copy of Y (a quarter-tile kernel keeps 8 columns of the last tile)
  bool fits;             // ... within ritz_dyn_limit(kt): otherwise nothing is launched
  bool vec2;
  // (the name rocprofv3 prints; the last argument is ritz_kernel's reserved one)
  std::string name() const { return plan_name("ritz_kernel<%d, %d, 3, %d, %d, %s, 0>", kt, vec2 ? 2 : 1, pipe, qt, xp ? "true" : "false"); }
};
inline RitzPlan ritz_plan(const PlanEnv& env, int n, int l, int m, int k2, bool vec2, int nranks_slots)
{
  const Knobs& knobs = env.knobs;
  RitzPlan p{};
  p.vec2 = vec2;
  p.kt = (m + k2 + 15) / 16;
  p.l4 = ((l + 3) / 4) * 4;
  const int ab_depth = knobs.ritz_pipe_depth();
  p.qt = ab_depth >= 0 ? 0 : quarter_tiles(env, m + k2, vec2);
  p.xp = k2 > 0;
  p.pipe = (ab_depth >= 0 && !p.xp && vec2 && p.kt >= 2) ? ab_depth : p.kt >= 3 ? 3 : p.kt >= 2 ? 2 : 0;
  p.lds_c = sizeof(double) * (size_t)p.l4 * (p.qt > 0 ? 16 * (p.kt - 1) + 8 : 16 * p.kt);
  p.fits = p.lds_c <= ritz_dyn_limit(env, p.kt);
  static_cast<RitzGrid&>(p) = ritz_grid(env, n, vec2, p.kt, p.lds_c, knobs.ritz_grid_factor(), nranks_slots);
  return p;
}
// the sweep with two coefficient blocks: [Y1 | Y2] packed as 2 kt tiles
struct Ritz2Plan : RitzGrid {
  int kt, l4;
  size_t lds_c;
  bool fits;             // the shape is one ritz2_kernel takes under this LDS limit
  bool vec2;
  std::string name() const { return plan_name("ritz2_kernel<%d, %d>", kt, vec2 ? 2 : 1); }
};
inline Ritz2Plan ritz2_plan(const PlanEnv& env, int n, int l, int m, bool vec2, int nranks_slots)
{
  Ritz2Plan p{};
  p.vec2 = vec2;
  p.kt = (m + 15) / 16;
  p.l4 = ((l + 3) / 4) * 4;
  p.lds_c = sizeof(double) * (size_t)p.l4 * 16 * 2 * p.kt;
  p.fits = m > 0 && m <= 48 && l > 0 && p.lds_c <= std::min((size_t)150 * 1024, env.lds_limit > 2048 ? env.lds_limit - 2048 : (size_t)0) &&
           !env.knobs.no_ritz2();
  static_cast<RitzGrid&>(p) = ritz_grid(env, n, vec2, p.kt, p.lds_c, 1, nranks_slots);
  return p;
}

// The Ritz sweep that also forms the next Davidson block and measures it against the basis (davidson_expand_kernel): a wave stages 16
// rows of the tx tiles of V, the tx tiles of AV and one output tile, 18 doubles per column.  16-byte path only, one output tile
// (block <= 16 columns), the whole of V in one pass; anything else, or an image beyond the LDS limit, does not fit and the caller
// runs the plain sweep.  m: columns of the basis, nb: columns of the Ritz block, first0: first predicted column (0-based), so the
// new block has nb - first0 columns.
constexpr size_t ritz_expand_lds_bytes(int tx) { return sizeof(double) * 4 * 16 * (size_t)(2 * tx + 1) * 18; }
struct RitzExpandPlan {
  int tx;                // column tiles of the basis (and of its operator image)
  int staged_tiles;      // 2 tx + 1
  size_t lds;
  bool fits;
  int blocks;
  int rows;              // rows a wave takes at a time: 16, or 32 (two consecutive tiles) where the measuring sweep stages 32
  int ncol, nslots;      // the norm reduction behind it (ritz_reduce_kernel): 16 columns, one slot of maxima
  int gram_slots;        // output tiles of [V | U0]^T U0: tx + 1, in the layout of a one-pass gram_lds_kernel WP sweep
  size_t small_doubles() const { return (size_t)ncol * (1 + nslots); }
  // (not a name of the `ritz` family: the statistics' consumers key that family by ritz_kernel's seven template arguments and hold
  //  every booked name that starts with `ritz` to them, tests/test_knobs_gpu.py; the launch is booked in the class DLA_OP_RITZ)
  std::string name() const { return plan_name("davidson_expand_kernel<%d>", tx); }
};
inline RitzExpandPlan ritz_expand_plan(const PlanEnv& env, int n, int m, int nb, int first0, bool vec2)
{
  RitzExpandPlan p{};
  p.tx = (m + 15) / 16;
  p.staged_tiles = 2 * p.tx + 1;
  p.lds = ritz_expand_lds_bytes(p.tx);
  bool listed = false;
  for (int t : RITZ_EXPAND_TILES) listed = listed || t == p.tx;
  p.fits = vec2 && n > 0 && n % 2 == 0 && m > 0 && nb > 0 && nb <= 16 && first0 >= 0 && first0 < nb && listed && p.lds <= env.lds_limit &&
           !env.knobs.no_ritz_expand();
  // The grid and the rows per step are those of the measuring sweep the chain would otherwise run on the stored block (wp_plan, OP_GRAMX):
  // the same rows then go through the same wave in the same order, and the block partials are that sweep's bit for bit.  (Two blocks
  // per CU up to five basis tiles: from three tiles on this kernel needs more than 256 registers, so the second block runs behind the
  // first, each over half the rows.)
  const WpPlan w = wp_plan(env, n, m, std::min(16, std::max(1, nb - first0)), false);     // (a one-tile block: wider ones do not fit)
  p.blocks = w.blocks;
  p.rows = w.R;
  p.ncol = 16; p.nslots = 1;
  p.gram_slots = p.tx + 1;
  return p;
}

// ---- the CSR tail of the sliced sparse operator (csr_long_segments_kernel, long_rows_combine_kernel)
// One wavefront per segment of a tail row, four per block, grid-stride beyond 8 blocks per CU (the cap of the other operator
// kernels); rows of more than one segment leave one partial sum per segment and right-hand side in a workspace, which one thread per
// (row, right-hand side) adds in segment order.  A function of the layout's counts (dla::SellLayout) and the block width only.
struct LongRowsPlan {
  int mc;                // right-hand sides per load of a matrix entry
  int seg_blocks;        // blocks of 256 threads of the segments kernel (>= 1)
  int combine_blocks;    // ... of the combine kernel; 0: no row has more than one segment, nothing is launched
  size_t part_doubles;   // the workspace: multi_segments x m
  // (the product of an operator with a tail is booked under the name of the kernel that walks it)
  std::string name() const { return plan_name("csr_long_segments_kernel<%d>", mc); }
};
inline LongRowsPlan long_rows_plan(const PlanEnv& env, int long_segments, int multi_rows, int multi_segments, int m, int mc)
{
  const long long cap = (long long)env.ncu * 8;
  LongRowsPlan p{};
  p.mc = mc;
  p.seg_blocks = (int)std::max(1LL, std::min(cap, ((long long)long_segments + 3) / 4));
  p.combine_blocks = multi_segments > 0 ? (int)std::max(1LL, std::min(cap, ((long long)multi_rows * m + 255) / 256)) : 0;
  p.part_doubles = (size_t)std::max(0, multi_segments) * (size_t)std::max(0, m);
  return p;
}

// ---- set-up of the sparse operator from CSR arrays in device memory (csr_check_cols_kernel, ell_fill_kernel, sell_fill_kernel,
// tail_copy_kernel, csr_diag_kernel, pattern_compare_kernel)
// All of them are grid-stride over blocks of 256 threads under the cap of the other operator kernels, 8 blocks per CU: one thread per
// entry (the column check), one thread per row with a wavefront on 64 consecutive rows (the ELLPACK fill, the diagonal, the row
// pointers of the comparison), one wavefront per slice and per segment of a tail row, four to a block (the sliced fill, the tail).
// A function of the counts alone: n rows, nnz entries, and the layout's slices and tail segments (both 0 for ELLPACK).
struct SpmmSetupPlan {
  int entry_blocks;      // csr_check_cols_kernel (>= 1)
  int row_blocks;        // ell_fill_kernel, csr_diag_kernel, the row part of pattern_compare_kernel (>= 1)
  int slice_blocks;      // sell_fill_kernel; 0: ELLPACK, nothing is launched
  int seg_blocks;        // tail_copy_kernel; 0: no tail, nothing is launched
};
inline SpmmSetupPlan spmm_setup_plan(const PlanEnv& env, long long n, long long nnz, long long slices, long long long_segments)
{
  SpmmSetupPlan p{};
  p.entry_blocks = grid_blocks(env, nnz, 256);
  p.row_blocks = grid_blocks(env, n, 256);
  p.slice_blocks = slices > 0 ? grid_blocks(env, slices, 4) : 0;
  p.seg_blocks = long_segments > 0 ? grid_blocks(env, long_segments, 4) : 0;
  return p;
}

// ---- the orthogonalisation chain
// The sweeps of a chain, as the host plans them and as the tail kernels name the next one in device memory (OrthoDev::phase).
// OP_GRAMX / OP_GRAMW / OP_XW belong to the pending-factor schedule (k <= 16, even n; see ortho_tail16): X^T U and U^T U in one
// sweep over [X | U]; the Gram matrix of U W formed on the fly; both at once
// OP_COMBOX / OP_CLOSE belong to the three-pass schedule (OrthoTailArgs::x3, see ortho_tail16): the projection sweep that also
// measures X^T U and U^T U of what it stores, and the closing projection that measures nothing.  OP_TRMMC is OP_TRMMG (the written
// update U <- U W with the Gram matrix of what it stores) behind a measuring sweep whose X^T U is carried through it, S W: the
// macro-iteration of ortho_cd that a caller with pending blocks gets instead of one more projection (see ortho_tail16)
enum { OP_NONE = 0, OP_GRAM_UU = 1, OP_TRMMG = 2, OP_XU = 3, OP_COMBO = 4, OP_FINAL = 5, OP_GRAMX = 6, OP_GRAMW = 7, OP_XW = 8,
       OP_COMBOX = 9, OP_CLOSE = 10, OP_TRMMC = 11 };

// What tells two chains apart.  Plans are remembered per shape with wide_gramx and dropf (vsx follows from m there); the walked
// launch paths depend on neither, so chain_verified keeps those two fields false; kind() forgets the basis width.
struct ChainShape {
  int k = 0, m = 0, fold = 0;
  bool vsx = false, wide_gramx = false, wide_xw = false, dropf = false, x3 = false;
  bool operator<(const ChainShape& o) const
  {
    return std::tie(k, m, fold, vsx, wide_gramx, wide_xw, dropf, x3) < std::tie(o.k, o.m, o.fold, o.vsx, o.wide_gramx, o.wide_xw, o.dropf, o.x3);
  }
  ChainShape kind() const { ChainShape s = *this; s.m = 0; return s; }
};

// what chain_choice reads of one call and of the engine's state
struct ChainIn {
  int m, k;              // basis columns in front of the block (0: the block alone), columns of the block
  bool vec2;             // even rows, and u, x and bx all start on 16 bytes
  bool bx_is_x;          // the standard inner product: the panel the projection subtracts is the panel it measures against
  bool combo_ok;         // U follows X in one panel and the fused projection takes the shape (can_combo)
  bool host_between;     // hook reductions / local_only: the host is needed between sweeps
  int x3_cooldown;       // > 0: a recent chain needed a level shift, or the solve is new
  int dmat_cols;         // columns of the caller's pending blocks the device copy describes (dla_basis_sync) ...
  bool dmat_nontrivial;  // ... some entry of them differs from the identity
  size_t fused_lds_kk;   // dynamic LDS of the fused sweep of a k x k update
};
struct ChainChoice {
  enum Take { chain, host_loop, nothing } take;
  int fold;              // 0: LDS-loop tail; 2: k x k steps on the matrix cores, sweep per update; 1: ... with the pending-factor schedule
  bool x3, wide_gramx, wide_xw;
};
inline ChainChoice chain_choice(const PlanEnv& env, const dla::ChainPolicy& policy, const ChainIn& in)
{
  const Knobs& knobs = env.knobs;
  const int m = in.m, k = in.k;
  const ChainChoice decline{ChainChoice::host_loop, 0, false, false, false};
  if (knobs.host_loop() || policy.chain_off) return decline;                      // A/B / the caller's request: host-driven loop
  if (in.host_between || k <= 0 || k > 48) return decline;     // hook reductions need the host between sweeps
  const bool vsx = m > 0;
  if (vsx && !in.combo_ok) return decline;
  if (!vsx && in.fused_lds_kk > env.lds_limit) return ChainChoice{ChainChoice::nothing, 0, false, false, false};
  // k x k steps on the matrix cores (ortho_tail16) for one-tile blocks; with them, on the 16-byte path and while X^T U fits one
  // pass of the storing sweep (12 tiles), the pending-factor schedule (fold = 1); otherwise the sweep-per-update one (fold = 2)
  const bool vec2 = in.vec2;
  int fold = (k <= 16 && !knobs.no_mfma_kxk()) ? 2 : 0;
  if (fold && vsx && vec2 && m <= 192 && !knobs.no_pending_factor() && env.lds_limit > (size_t)128 * 1024) fold = 1;
  // ... and with the standard inner product (bx == x: the panel the projection subtracts is the panel it measures against) the
  // three-pass schedule: projections that measure X^T U and U^T U of what they store (Knobs::five_sweep keeps the five-sweep one)
  // For callers that finish their blocks in memory (plain ortho_vs_x, dla_expand_project modes 0 / 1 / 4) not while expansion blocks
  // come out of their first projection numerically rank deficient (level shifts: the benchmark operator's rank-4 coupling leaves 4
  // new directions per 13-column block): there the written update and the storing sweep follow whatever the projection measured
  // and the closing projection only needs its Gram matrix (measured r05, interleaved: 17.0 against 16.35 ms per benchmark solve;
  // 138.5 against 144.3 ms on the random-guess leg, which never shifts).  A chain that reports a level shift switches the schedule
  // off for the next 16 chains, and every solve starts with two chains of the five-sweep schedule (on the benchmark the first one
  // shifts).  Callers that take the closing block on their small matrices (modes 3 and 5) always run it: `rebuilt`, `policy.basis_exact`.
  // (A block that is used once and rebuilt -- LOBPCG's W, dla_expand_project mode 3: pending blocks without a bound on the Gram
  //  matrix -- leaves nothing in a basis: the three-pass schedule always; measured r05, n = 2e6, 8 roots: 15.99 against 17.07 ms.)
  const bool rebuilt = policy.rebuilt();
  // (policy.basis_exact: the caller keeps its pending blocks on the device (dla_basis_sync) and every projection of this chain is exact
  //  against the FINISHED basis -- a loose stored basis costs later chains nothing, so the schedule that ends soonest always)
  if (policy.basis_exact && vsx && (fold == 0 || in.dmat_cols != m || (in.dmat_nontrivial && m > DMAT_LD))) return decline;
  const bool x3 = fold == 1 && in.bx_is_x && !knobs.five_sweep() && (in.x3_cooldown <= 0 || knobs.three_pass_always() || rebuilt || policy.basis_exact);
  // wider blocks (LDS-loop tail): X^T U and U^T U in ONE sweep when [X | U] fits one pass of the Gram kernel (the plain
  // product with the contiguous panel [X | U] on the left: U follows X, bx == x) and the leading ortho_cd takes one step
  const int ktw = (k + 15) / 16;
  const bool wide_gramx = fold == 0 && vsx && vec2 && in.bx_is_x && !knobs.no_wide_gramx() && ktw >= 2 && ktw <= 3 &&
                          (m + k + 15) / 16 <= (ktw == 2 ? 8 : 7) && env.lds_limit > (size_t)128 * 1024;
  // ([X | U] in TWO passes of that sweep -- the 18-column block behind 125 basis columns of the cfg 4 shape would then take
  //  `6 4 2 8 4 5` instead of `1 3 4 2 2 3 4 5` -- measured r06: 32.23-32.27 against 32.24-32.38 ms per solve, no gain; not built in)
  // ... and inside the loop the triangular update is stored together with X^T U and U^T U of what it stores (OP_XW, the sweep the
  // one-tile schedule closes with) while X^T U fits one pass beside the block's tiles: 5 sweeps per call instead of 6
  // (two-tile blocks: measured r04 at n = 1e7, m = 64, k = 32: 1777 us against 937 + 1010 for the two sweeps it replaces; the
  //  three-tile sweep does 108 MFMAs per 16 rows with one wave per SIMD and runs at 3.9 TB/s -- 2960 us against 1212 + 1682: it
  //  stays off unless Knobs::wide_xw_three_tiles asks for it)
  const bool wide_xw = wide_gramx && (ktw == 2 || knobs.wide_xw_three_tiles()) && (m + 15) / 16 <= wp_max_tlw(ktw) && (m + k) * k <= XUG_DOUBLES && !knobs.no_wide_xw();
  return ChainChoice{ChainChoice::chain, fold, x3, wide_gramx, wide_xw};
}

// the plan of a shape no chain of this context has run yet
inline std::vector<int> default_plan(const ChainShape& s)
{
  // the schedule measured on the reference: cd x2, [projection, cd x2], [projection, cd x1]
  if (s.x3) return {OP_GRAMX, OP_COMBOX, OP_COMBOX, OP_CLOSE, OP_FINAL};
  if (s.fold == 1) return {OP_GRAMX, OP_COMBO, OP_TRMMG, OP_XW, OP_COMBO, OP_FINAL};
  if (s.wide_xw) return {OP_GRAMX, OP_COMBO, OP_XW, OP_COMBO, OP_FINAL};
  if (s.wide_gramx) return {OP_GRAMX, OP_COMBO, OP_TRMMG, OP_XU, OP_COMBO, OP_FINAL};
  if (s.vsx) return {OP_GRAM_UU, OP_TRMMG, OP_XU, OP_COMBO, OP_TRMMG, OP_XU, OP_COMBO, OP_FINAL};
  return {OP_GRAM_UU, OP_TRMMG, OP_FINAL};
}

// how the engine's ranks exchange a reduced matrix
struct Transport { bool p2p_on; int nranks; bool comm; };
// Callers that take the closing block on their small matrices without a bound on the factor (dla_expand_project modes 3 and 5: the
// machine ends with the block pending and never asks for OP_CLOSE / OP_FINAL) get plans without them: the fused step of the
// last planned sweep reports where the machine stands whether or not it was that sweep's turn (gram_reduce_kernel<true>).  Two
// predicated-off sweeps and two k x k launches less per chain: 19 us (r05 trace: 0.15 ms per benchmark solve, 0.23 per LOBPCG solve).
inline bool chain_lean(const PlanEnv& env, const dla::ChainPolicy& policy, int m, int k, const Transport& t)
{
  const bool fused_steps = t.p2p_on ? (!env.knobs.exchange_own_launch() && (m + k) * k <= P2P_MAX_DOUBLES) : (t.nranks <= 1 && !t.comm);
  return m > 0 && policy.rebuilt() && m + k <= PEND_ROWS && fused_steps && !env.knobs.keep_closing_launches();
}
// a lean plan carries no closing / final sweep behind its last measuring one
inline void trim_closing(std::vector<int>& plan)
{
  while (plan.size() > 1 && (plan.back() == OP_FINAL || plan.back() == OP_CLOSE)) plan.pop_back();
}
// Every plan ends with OP_FINAL: its tail is a launch of its own that always runs and reports where the machine stands (a
// fused tail is skipped together with a sweep whose turn it is not).  With drop_final the machine never asks for the sweep
// itself, and the executed list a plan is remembered from does not contain it.  Lean plans (chain_lean) end without it.
inline std::vector<int> close_plan(std::vector<int> plan, bool lean, bool x3)
{
  if (lean) trim_closing(plan);
  else if (plan.empty() || plan.back() != OP_FINAL) plan.push_back(OP_FINAL);
  // (three-pass schedule: whether a chain ends with its closing block pending or with the closing sweep depends on the last bits
  //  of a Gram matrix -- a plan remembered from a chain that ended pending keeps the sweep in place: an empty launch when it
  //  is not needed, against a host round trip and a repeated operator call when it is)
  if (x3 && !lean && std::find(plan.begin(), plan.end(), (int)OP_CLOSE) == plan.end()) plan.insert(plan.end() - 1, (int)OP_CLOSE);
  return plan;
}

// ---- the dense operator and metric (include/diaglib_amd.h, dla_dense_setup): the stored layout and the plan of a product
// The library's copy of a(lda, n) is laid out for the B operand of v_mfma_f64_16x16x4 (one f64 per lane, element [k = lane >> 4]
// [j = lane & 15]): the matrix is cut into tiles of DENSE_TILE = 16 rows, every tile into groups of DENSE_GROUP = 8 consecutive
// contraction indices, and a group stores 128 doubles, lane-major -- lane l = 16 (k mod 4) + (i mod 16) holds the pair
// [a(i, 8 g + l / 16), a(i, 8 g + 4 + l / 16)], the operands of two consecutive MFMA steps.  A wavefront's load of a group is one
// 16-byte load per lane over 1024 contiguous bytes with no bounds check: rows and contraction indices are zero-padded to
// n_pad = n rounded up to 16 (zeros add no rounding).  Groups of a tile are consecutive, tiles follow each other.
constexpr int DENSE_TILE = 16, DENSE_GROUP = 8, DENSE_MAX_COLS = 48;
// row tiles a wavefront multiplies with one X fragment (64 rows).  A starting value.  The one alternative measured so far, two
// tiles for passes of two and three accumulator groups (fewer registers, more wavefronts per SIMD), was slower at n = 8192 and 32768,
// m = 37 (0.32 against 0.23 ms, 4.66 against 3.28 ms): such a pass reads more bytes of X fragments through the caches than of A
// from HBM, and halving the tiles doubles them.
constexpr int DENSE_WAVE_TILES = 4;
// a contraction chunk is at least this many groups (64 indices), and the partial sums of a split product may move at most
// 1 / DENSE_WS_SHARE of the matrix's bytes.  Starting values as well.
constexpr int DENSE_MIN_CHUNK_GROUPS = 8, DENSE_WS_SHARE = 8;

constexpr int dense_n_pad(int n) { return (n + DENSE_TILE - 1) / DENSE_TILE * DENSE_TILE; }
// where a(i, k) lives in the stored copy (0-based, both below n_pad)
constexpr size_t dense_index(int n_pad, int i, int k)
{
  return (((size_t)(i / DENSE_TILE) * (size_t)(n_pad / DENSE_GROUP) + (size_t)(k / DENSE_GROUP)) * 64 + (size_t)((k % 4) * 16 + i % DENSE_TILE)) * 2 +
         (size_t)((k % DENSE_GROUP) / 4);
}
// ... and back: the row and the contraction index of stored element d (what the pack kernel runs, one thread per element)
constexpr int dense_row_of(int n_pad, size_t d) { return (int)(d / 128 / (size_t)(n_pad / DENSE_GROUP)) * DENSE_TILE + (int)((d >> 1) & 15); }
constexpr int dense_col_of(int n_pad, size_t d)
{
  return (int)(d / 128 % (size_t)(n_pad / DENSE_GROUP)) * DENSE_GROUP + (int)(d & 1) * 4 + (int)((d >> 5) & 3);
}
// the copy (n_pad x n_pad doubles) and the diagonal (n doubles) of a column-major host array: what dla_dense_setup uploads
inline void dense_pack(int n, const double* a, size_t lda, double* stored, double* diag)
{
  const int n_pad = dense_n_pad(n);
  std::fill(stored, stored + (size_t)n_pad * n_pad, 0.0);
  for (int k = 0; k < n; ++k)
    for (int i = 0; i < n; ++i) stored[dense_index(n_pad, i, k)] = a[(size_t)k * lda + i];
  for (int i = 0; i < n; ++i) diag[i] = a[(size_t)i * lda + i];
}
// ... and of the sum and the difference of two column-major host arrays p(ldp, n), q(ldq, n) at once (include/diaglib_amd.h,
// dla_dense_setup_lr_pair): what dense_pack stores for the arrays p + q and p - q, every element one rounded addition or one rounded
// subtraction, the padding 0.0, every source element read once
inline void dense_pack_pair(int n, const double* p, size_t ldp, const double* q, size_t ldq, double* sum, double* sum_diag, double* dif,
                            double* dif_diag)
{
  const int n_pad = dense_n_pad(n);
  std::fill(sum, sum + (size_t)n_pad * n_pad, 0.0);
  std::fill(dif, dif + (size_t)n_pad * n_pad, 0.0);
  for (int k = 0; k < n; ++k)
    for (int i = 0; i < n; ++i) {
      const double pv = p[(size_t)k * ldp + i], qv = q[(size_t)k * ldq + i];
      const size_t d = dense_index(n_pad, i, k);
      sum[d] = pv + qv;
      dif[d] = pv - qv;
      if (i == k) { sum_diag[i] = pv + qv; dif_diag[i] = pv - qv; }
    }
}

// One pass of a product Y(n x m) = A X, m <= DENSE_MAX_COLS: a pure function of n, m and the CU count.
// A wavefront owns DENSE_WAVE_TILES row tiles and one chunk of the contraction, so there are row_groups x k_chunks of them.  The rule
// for k_chunks: as many as give every SIMD of the device a wavefront (4 ncu / row_groups, rounded up), but
//   * the partial sums are written and read once, 2 k_chunks n m 8 bytes, and that may be at most 1 / DENSE_WS_SHARE of the 8 n^2
//     bytes of the matrix: k_chunks <= n / (2 DENSE_WS_SHARE m);
//   * a chunk keeps at least DENSE_MIN_CHUNK_GROUPS groups: k_chunks <= groups / DENSE_MIN_CHUNK_GROUPS;
// and never less than 1.  Chunks are chunk_groups = ceil(groups / k_chunks) groups long -- chunk c covers the contraction indices
// [8 c chunk_groups, min(n_pad, 8 (c + 1) chunk_groups)) -- and k_chunks is then the number of chunks that are not empty.
struct DensePlan {
  int n_pad, row_tiles, row_groups, groups;   // groups: n_pad / DENSE_GROUP
  int acc_groups;                             // accumulator groups of 16 columns (the kernel's instance): 1 .. 3
  int k_chunks, chunk_groups;
  size_t ws_doubles;                          // the workspace of partial sums: k_chunks x m x n, 0 with one chunk
  std::string name() const { return plan_name("dense_mfma_kernel<%d>", acc_groups); }
};
inline DensePlan dense_plan(int ncu, int n, int m)
{
  DensePlan p{};
  p.n_pad = dense_n_pad(n);
  p.row_tiles = p.n_pad / DENSE_TILE;
  p.acc_groups = (m + 15) / 16;
  p.row_groups = (p.row_tiles + DENSE_WAVE_TILES - 1) / DENSE_WAVE_TILES;
  p.groups = p.n_pad / DENSE_GROUP;
  const long long want = (4LL * std::max(1, ncu) + p.row_groups - 1) / p.row_groups;
  const long long traffic = (long long)n / (2LL * DENSE_WS_SHARE * m), length = p.groups / DENSE_MIN_CHUNK_GROUPS;
  const int chunks = (int)std::max(1LL, std::min(want, std::min(traffic, length)));
  p.chunk_groups = (p.groups + chunks - 1) / chunks;
  p.k_chunks = (p.groups + p.chunk_groups - 1) / p.chunk_groups;
  p.ws_doubles = p.k_chunks > 1 ? (size_t)p.k_chunks * (size_t)m * (size_t)n : 0;
  return p;
}

// One pass of the transposed product Y(n x m) = A^T X, m <= DENSE_MAX_COLS, on the same stored copy (include/diaglib_amd.h,
// dla_dense_matvec_t): a pure function of n, m and the CU count.  The output index is now the matrix's column, the contraction runs
// down its rows.  A wavefront owns a strip of DENSE_T_WAVE_BLOCKS blocks of 16 matrix columns -- 2 DENSE_T_WAVE_BLOCKS adjacent groups,
// 8 KB contiguous in every row tile -- and one chunk of the row tiles, so there are strips x row_chunks of them.  The rule for
// row_chunks is dense_plan's for k_chunks: as many as give every SIMD a wavefront (4 ncu / strips, rounded up), but
//   * the partial sums may move at most 1 / DENSE_WS_SHARE of the matrix's bytes: row_chunks <= n / (2 DENSE_WS_SHARE m);
//   * a chunk keeps at least DENSE_T_MIN_CHUNK_TILES row tiles: row_chunks <= row_tiles / DENSE_T_MIN_CHUNK_TILES;
// and never less than 1.  Chunk c covers the row tiles [c chunk_tiles, min(row_tiles, (c + 1) chunk_tiles)), chunk_tiles =
// ceil(row_tiles / chunks), and row_chunks is the number of chunks that are not empty.  Partial sums: ws[chunk][m][n], added in
// ascending chunk order by dense_combine_kernel.  Starting values, like dense_plan's.
constexpr int DENSE_T_WAVE_BLOCKS = 4, DENSE_T_MIN_CHUNK_TILES = 4;
struct DenseTPlan {
  int n_pad, row_tiles, col_blocks, strips;   // col_blocks: n_pad / 16; strips: ceil(col_blocks / DENSE_T_WAVE_BLOCKS)
  int acc_groups;                             // groups of 16 columns of X (the kernel's instance): 1 .. 3
  int row_chunks, chunk_tiles;
  size_t ws_doubles;                          // row_chunks x m x n, 0 with one chunk
  std::string name() const { return plan_name("dense_t_mfma_kernel<%d>", acc_groups); }
};
inline DenseTPlan dense_t_plan(int ncu, int n, int m)
{
  DenseTPlan p{};
  p.n_pad = dense_n_pad(n);
  p.row_tiles = p.n_pad / DENSE_TILE;
  p.col_blocks = p.n_pad / 16;
  p.strips = (p.col_blocks + DENSE_T_WAVE_BLOCKS - 1) / DENSE_T_WAVE_BLOCKS;
  p.acc_groups = (m + 15) / 16;
  const long long want = (4LL * std::max(1, ncu) + p.strips - 1) / p.strips;
  const long long traffic = (long long)n / (2LL * DENSE_WS_SHARE * m), length = p.row_tiles / DENSE_T_MIN_CHUNK_TILES;
  const int chunks = (int)std::max(1LL, std::min(want, std::min(traffic, length)));
  p.chunk_tiles = (p.row_tiles + chunks - 1) / chunks;
  p.row_chunks = (p.row_tiles + p.chunk_tiles - 1) / p.chunk_tiles;
  p.ws_doubles = p.row_chunks > 1 ? (size_t)p.row_chunks * (size_t)m * (size_t)n : 0;
  return p;
}

// ---- a symmetric dense operator or metric stored as one triangle (include/diaglib_amd.h, dla_dense_setup_sym)
// The tile and group format of the full copy, but row tile T (16 rows) keeps only its groups 0 .. 2 T + 1, that is the 16 x 16
// blocks of the column blocks 0 .. T.  Groups of a tile are consecutive and tiles follow each other: tile T starts at group
// T (T + 1), the two groups of a block stay adjacent (2 KB), and the copy holds 128 nt (nt + 1) doubles, nt = n_pad / 16 --
// n_pad^2 / 2 + 8 n_pad.  A diagonal block is stored whole, mirrored from the referenced triangle, so it is a plain forward block;
// padding is 0.0.
constexpr size_t dense_sym_doubles(int n_pad) { return (size_t)128 * (size_t)(n_pad / DENSE_TILE) * (size_t)(n_pad / DENSE_TILE + 1); }
// where a(i, k) lives in the triangular copy (0-based, both below n_pad, k / 16 <= i / 16)
constexpr size_t dense_sym_index(int i, int k)
{
  const size_t t = (size_t)(i / DENSE_TILE);
  return ((t * (t + 1) + (size_t)(k / DENSE_GROUP)) * 64 + (size_t)((k % 4) * 16 + i % DENSE_TILE)) * 2 + (size_t)((k % DENSE_GROUP) / 4);
}
// ... and back: the row tile of stored group gi (the largest T with T (T + 1) <= gi, bit by bit: T < 2^16), then the row and the
// column of stored element d (what the pack kernel runs, one thread per element)
constexpr int dense_sym_tile_of(size_t gi)
{
  size_t t = 0;
  for (size_t bit = (size_t)1 << 15; bit; bit >>= 1)
    if ((t | bit) * ((t | bit) + 1) <= gi) t |= bit;
  return (int)t;
}
constexpr int dense_sym_row_of(size_t d) { return dense_sym_tile_of(d / 128) * DENSE_TILE + (int)((d >> 1) & 15); }
constexpr int dense_sym_col_of(size_t d)
{
  const size_t t = (size_t)dense_sym_tile_of(d / 128);
  return (int)(d / 128 - t * (t + 1)) * DENSE_GROUP + (int)(d & 1) * 4 + (int)((d >> 5) & 3);
}
// a(i, k) of a symmetric matrix of which only the triangle uplo ('L' or 'U') of the column-major array is referenced
constexpr size_t dense_sym_source(size_t lda, bool lower, int i, int k) { return (i >= k) == lower ? (size_t)k * lda + i : (size_t)i * lda + k; }
// the triangular copy and the diagonal (n doubles) of such an array: what dla_dense_setup_sym uploads.  The other strict triangle
// is never read, inside diagonal blocks either.
inline void dense_sym_pack(int n, const double* a, size_t lda, char uplo, double* stored, double* diag)
{
  const int n_pad = dense_n_pad(n);
  const bool lower = uplo == 'L' || uplo == 'l';
  std::fill(stored, stored + dense_sym_doubles(n_pad), 0.0);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < std::min(n, (i / DENSE_TILE + 1) * DENSE_TILE); ++k) stored[dense_sym_index(i, k)] = a[dense_sym_source(lda, lower, i, k)];
  for (int i = 0; i < n; ++i) diag[i] = a[(size_t)i * lda + i];
}

// One pass of a product Y(n x m) = A X on the triangular copy, m <= DENSE_MAX_COLS: a pure function of n, m and the CU count.
// A workgroup of four wavefronts owns a panel of DENSE_SYM_PANEL_TILES = 4 DENSE_WAVE_TILES row tiles (256 rows; wavefront w the tiles
// 16 P + 4 w .. + 3 of panel P) and one chunk of the column blocks 0 .. last tile of the panel.  A stored block (T, b) is loaded once
// and used twice: A_Tb x_b goes to the forward sums of rows of tile T, and for T > b A_Tb^T x_T to the transposed sums of the rows of
// block b.  Chunks are chunk_blocks = 16 chunk_panels blocks long, so panel P has P / chunk_panels + 1 of them (the last one ends
// with the panel's diagonal blocks) and a pass has items = sum over P of that.  The rule for chunk_panels:
//   * enough items to give every SIMD of the device DENSE_SYM_ITEMS_PER_CU wavefronts: the largest chunk_panels with items >=
//     DENSE_SYM_ITEMS_PER_CU ncu.  The items are not equal -- the last chunk of a panel ends on the diagonal -- and with one item per
//     CU the longest one sets the time of the pass; several shorter ones per CU even that out (DESIGN section 3 has both measured),
//   * but at least 1 (a chunk keeps at least the 16 column blocks of one panel),
//   * and then the smallest one at or above it for which the forward partial sums, written and read once -- 16 bytes each -- stay
//     within 1 / DENSE_WS_SHARE of the 8 dense_sym_doubles bytes of the copy, or chunk_panels = panels (one chunk per panel).
// The transposed partial sums are not the chunking's to decide: one per panel and column block below the panel's last tile,
// 16 rows x m, about m / 256 of the copy's bytes written and read.  The panel height is a starting value, like the constants above.
// Workspace (doubles, every one written by one thread of the product kernel and read by one of the combine kernel):
//   forward, from 0: panel P, chunk c at m (256 F(P) + c rows(P)), [column][row] with rows(P) = min(256, n - 256 P) rows,
//     F(P) = sum over P' < P of (P' / chunk_panels + 1) (dense_sym_chunks_before);
//   transposed, from t_base = m (256 F(last panel) + chunks(last panel) rows(last panel)): panel P, block b < min(16 P + 15, nt - 1)
//     at t_base + 16 m (8 P^2 + 7 P + b), [column][16 rows].
// A matrix of one tile (n <= 16) has nothing to combine: its one workgroup writes y, ws_doubles = 0.
// max_partials: the largest number of partial sums added into one element of y.
constexpr int DENSE_SYM_PANEL_TILES = 4 * DENSE_WAVE_TILES, DENSE_SYM_ITEMS_PER_CU = 4;
constexpr long long dense_sym_chunks_before(int panel, int chunk_panels)
{
  const long long q = panel / chunk_panels, r = panel % chunk_panels;
  return panel + (long long)chunk_panels * q * (q - 1) / 2 + r * q;
}
// the first panel that holds a transposed partial sum for column block b (panels at or above it all do)
constexpr int dense_sym_first_panel(int nt, int b)
{
  return b / DENSE_SYM_PANEL_TILES + ((b % DENSE_SYM_PANEL_TILES == DENSE_SYM_PANEL_TILES - 1 || b == nt - 1) ? 1 : 0);
}
struct DenseSymPlan {
  int n_pad, row_tiles, panels;
  int acc_groups;                             // groups of 16 columns of X (the kernel's instance): 1 .. 3
  int chunk_panels, chunk_blocks, max_chunks; // max_chunks: the chunks of the last panel (the launch's grid.x)
  long long items;
  int max_partials;
  size_t t_base, ws_doubles;
  std::string name() const { return plan_name("dense_sym_mfma_kernel<%d>", acc_groups); }
};
inline DenseSymPlan dense_sym_plan(int ncu, int n, int m)
{
  DenseSymPlan p{};
  p.n_pad = dense_n_pad(n);
  p.row_tiles = p.n_pad / DENSE_TILE;
  p.panels = (p.row_tiles + DENSE_SYM_PANEL_TILES - 1) / DENSE_SYM_PANEL_TILES;
  p.acc_groups = (m + 15) / 16;
  const int last = p.panels - 1, rows_last = n - 256 * last;
  const auto forward = [&](int cp) { return (size_t)m * ((size_t)256 * (size_t)dense_sym_chunks_before(last, cp) + (size_t)(last / cp + 1) * (size_t)rows_last); };
  int cp = 1;
  while (cp < p.panels && dense_sym_chunks_before(p.panels, cp + 1) >= (long long)DENSE_SYM_ITEMS_PER_CU * std::max(1, ncu)) ++cp;
  while (cp < p.panels && 16 * forward(cp) * DENSE_WS_SHARE > 8 * dense_sym_doubles(p.n_pad)) ++cp;
  p.chunk_panels = cp;
  p.chunk_blocks = DENSE_SYM_PANEL_TILES * cp;
  p.max_chunks = last / cp + 1;
  p.items = dense_sym_chunks_before(p.panels, cp);
  p.max_partials = 0;
  for (int b = 0; b < p.row_tiles; ++b)
    p.max_partials = std::max(p.max_partials, b / DENSE_SYM_PANEL_TILES / cp + 1 + p.panels - dense_sym_first_panel(p.row_tiles, b));
  if (p.row_tiles == 1) return p;             // (one block: t_base = ws_doubles = 0)
  p.t_base = forward(cp);
  const size_t t_blocks = (size_t)8 * last * last + (size_t)7 * last + (size_t)std::min(16 * last + 15, p.row_tiles - 1);
  p.ws_doubles = p.t_base + (size_t)16 * (size_t)m * t_blocks;
  return p;
}

}  // namespace dla_plans
