// diaglib_amd/csrc/host_logic.cpp -- host side of the C-ABI (include/diaglib_amd.h):
// context, callback trampolines, and the control flow of the orthogonalisation kernels
// (Cholesky-QR with refinement, block Gram-Schmidt).  All O(n) work is delegated to the
// device engine (dla_internal.h); this file only sees the small k x k / m x k matrices.
//
// Behavioural spec: reference diaglib.f90:3185-3341 (ortho_cd), :3481-3574 (ortho_vs_x),
// :3094-3183 (b_ortho), :3576-3663 (b_ortho_vs_x), :3734-3786 (check_guess),
// :3686-3732 (get_coeffs) -- see SURVEY.md 8a rows A8, A10, A12, A14, A15.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>
#include <sys/syscall.h>
#include <unistd.h>
#include "dla_internal.h"

using dla::Engine;

// ---- $DIAGLIB_AMD_HOSTTIME accounting
#include <map>
#include <string>
#include <time.h>
namespace dla {
namespace { std::map<std::string, std::pair<double, long>>& api_tab() { static std::map<std::string, std::pair<double, long>> t; return t; } }
bool ApiTimer::on() { static const bool v = std::getenv("DIAGLIB_AMD_HOSTTIME") != nullptr; return v; }
double ApiTimer::now() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }
void ApiTimer::add(const char* name, double dt) { auto& e = api_tab()[name]; e.first += dt; e.second += 1; }
namespace { const char* g_prev_api = nullptr; double g_prev_exit = 0.0; int g_api_depth = 0; }
void ApiTimer::enter(const char* name, double t)
{
  // (only outermost entry points, and only gaps below 10 ms: the caller's own work between solves is not ours to report)
  if (g_api_depth++ == 0 && g_prev_api && name[0] != ' ' && t - g_prev_exit < 0.01)
    add((std::string("  caller between ") + g_prev_api + " .. " + name).c_str(), t - g_prev_exit);
}
void ApiTimer::leave(const char* name, double t) { if (--g_api_depth == 0 && name[0] != ' ') { g_prev_api = name; g_prev_exit = t; } }
void ApiTimer::report()
{
  if (!on()) return;
  for (auto& kv : api_tab())
    std::fprintf(stderr, "[dla] api %-22s %9.3f ms %7ld calls\n", kv.first.c_str(), kv.second.first * 1e3, kv.second.second);
}
}  // namespace dla

namespace {

const double kEps = DBL_EPSILON;           // epsilon(one)
const double kTolOrtho = 2.0 * DBL_EPSILON;  // tol_ortho, diaglib.f90:151

// Re-entrancy (the reference keeps LAPACK work arrays and timers in its module, diaglib.f90:155-161, and
// cannot run two solves at once): nothing here is process-global.  The context the Fortran drivers use belongs to
// the CALLING THREAD -- its own engine (stream, scratch, panel cache, statistics, options) -- so two host threads can
// solve different problems with different operators at the same time.  It is created on the thread's first use and
// lives until dla_destroy(dla_default_ctx()) or the end of the process.
// The thread's context is released when the thread ends (the owner's destructor runs at thread exit): a caller that solves
// from short-lived threads does not leave a stream, pinned buffers and a panel cache behind per thread.  The process' main
// thread is the exception -- its thread-local destructors run during process exit, when the HIP runtime may already be
// gone -- its context goes with the process (or through dla_destroy / diaglib_amd_config(release_context=.true.)).
struct DefaultCtxOwner {
  dla_ctx* c = nullptr;
  ~DefaultCtxOwner();
};
thread_local DefaultCtxOwner g_default_owner;
#define g_default (g_default_owner.c)
// built-in operator callbacks have the reference's context-free shape; they act on the calling thread's setup
thread_local dla_ctx* g_synth_ctx = nullptr;
thread_local dla_ctx* g_spmm_ctx = nullptr;
thread_local dla_ctx* g_dense_ctx = nullptr;   // the dense operator / metric (dla_dense_setup): a binding of its own
// The sample operators have the reference's callback shape -- void, no status (README.md:34-35) -- so a failure inside one (used before
// its setup, an engine error) is left here for the trampoline that called it: dla_call_matvec / dla_call_precnd / dla_call_lrprec
// return it as their own status (the Fortran drivers then end the program the way they end it for every engine failure).  Nothing
// in the library calls abort() once a context exists (round-5 review: the process holds the GPU).
thread_local int g_cb_status = 0;
thread_local std::string g_cb_msg;
void callback_failed(int code, const std::string& msg)
{
  if (g_cb_status == 0) { g_cb_status = code; g_cb_msg = msg; }
  std::fprintf(stderr, "diaglib_amd: %s\n", msg.c_str());
}

int fail(dla_ctx* c, int code, const std::string& msg)
{
  if (c) c->err = msg;
  return code;
}

// status a sample-operator callback left behind (see g_cb_status); clears it
int callback_status(dla_ctx* c)
{
  if (g_cb_status == 0) return DLA_OK;
  const int code = g_cb_status;
  g_cb_status = 0;
  return fail(c, code, g_cb_msg);
}

int engfail(dla_ctx* c, int code)
{
  if (code != 0 && c) c->err = c->eng->err;
  return code;
}

long long global_rows(dla_ctx* c, int n) { return c->n_global > 0 ? c->n_global : (long long)n; }

// failure of a block operation: its message becomes the context's
int opsfail(dla_ctx* c, dla::BlockOps* ops, int code)
{
  if (code != 0 && c) c->err = ops->err;
  return code;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ context
int dla_create(dla_ctx** out, int device)
{
  if (!out) return DLA_ERR_ARG;
  *out = nullptr;
  if (device < 0) {
    const char* lr = std::getenv("LOCAL_RANK");
    device = lr ? std::atoi(lr) : 0;
  }
  std::string err;
  Engine* e = dla::make_engine(device, err);
  if (!e) {
    std::fprintf(stderr, "diaglib_amd: cannot create the HIP engine: %s\n", err.c_str());
    return DLA_ERR_NO_DEVICE;
  }
  dla_ctx* c = new dla_ctx();
  c->eng = e;
  if (std::getenv("DIAGLIB_AMD_NO_PENDING") != nullptr) c->pending_blocks = 0;     // (default of new contexts; DLA_OPT_PENDING_BLOCKS)
  *out = c;
  return DLA_OK;
}

}  // extern "C" (reopened below)

namespace {
DefaultCtxOwner::~DefaultCtxOwner()
{
  if (!c) return;
  if ((long)syscall(SYS_gettid) == (long)getpid()) return;      // main thread: process exit, leave it to the process
  dla_ctx* mine = c;
  c = nullptr;
  (void)dla_destroy(mine);
}
}  // namespace

extern "C" {

int dla_destroy(dla_ctx* c)
{
  if (!c) return DLA_OK;
  dla::ApiTimer::report();
  if (c->stage_x) c->eng->host_free(c->stage_x);
  if (c->stage_y) c->eng->host_free(c->stage_y);
  delete c->eng;
  if (g_default == c) g_default = nullptr;
  if (g_synth_ctx == c) g_synth_ctx = nullptr;
  if (g_spmm_ctx == c) g_spmm_ctx = nullptr;
  if (g_dense_ctx == c) g_dense_ctx = nullptr;
  delete c;
  return DLA_OK;
}

dla_ctx* dla_default_ctx(void)
{
  if (!g_default) {
    dla_ctx* c = nullptr;
    if (dla_create(&c, -1) != DLA_OK) {
      // fail loudly: the product has no CPU path
      std::fprintf(stderr, "diaglib_amd: no usable MI355X/HIP device -- aborting (there is no CPU fallback)\n");
      std::abort();
    }
    g_default = c;
  }
  return g_default;
}

int dla_set_option(dla_ctx* c, int option, int value)
{
  if (!c) return DLA_ERR_ARG;
  switch (option) {
    case DLA_OPT_CALLBACKS_ON_DEVICE: c->callbacks_on_device = value; break;
    case DLA_OPT_EVEC_ON_DEVICE: c->evec_on_device = value; break;
    case DLA_OPT_PROFILE: c->eng->profile = value != 0; break;
    case DLA_OPT_VERBOSE_ORTHO: c->verbose_ortho = value; break;
    case DLA_OPT_STAGE_CHUNKS:
      if (value < 0 || value > 16) return fail(c, DLA_ERR_ARG, "stage chunks must be 0..16");
      c->stage_chunks = value;
      break;
    case DLA_OPT_CASLR_ALGORITHM:
      if (value < 0 || value > 1) return fail(c, DLA_ERR_ARG, "caslr algorithm must be 0 or 1");
      c->caslr_algorithm = value;
      break;
    case DLA_OPT_ORTHO_MAXIT:
      if (value < 1 || value > 10) return fail(c, DLA_ERR_ARG, "ortho maxit must be 1..10");
      c->eng->ortho_maxit = value;
      break;
    case DLA_OPT_P2P_TIMEOUT_MS:
      if (value < 0) return fail(c, DLA_ERR_ARG, "p2p timeout must be >= 0 ms (0 = no limit)");
      c->p2p_timeout_ms = value;
      return engfail(c, c->eng->set_p2p_timeout(value));
    case DLA_OPT_RUN_AHEAD:
      if (value < 0 || value > 2) return fail(c, DLA_ERR_ARG, "run-ahead must be 0, 1 or 2");
      c->run_ahead = value;
      break;
    case DLA_OPT_CALLBACK_ORDER:
      if (value < 0 || value > 2) return fail(c, DLA_ERR_ARG, "callback order must be 0, 1 or 2");
      c->callback_order = value;
      break;
    case DLA_OPT_PENDING_BLOCKS:
      if (value < 0 || value > 1) return fail(c, DLA_ERR_ARG, "pending blocks must be 0 or 1");
      c->pending_blocks = value;
      break;
    default:
      if (option >= DLA_OPT_TUNE0 && option < DLA_OPT_TUNE0 + 8) { c->eng->set_tune(option - DLA_OPT_TUNE0, value); break; }
      return fail(c, DLA_ERR_ARG, "unknown option");
  }
  return DLA_OK;
}

int dla_begin_solve(dla_ctx* c)
{
  if (!c) return DLA_ERR_ARG;
  c->eng->begin_solve();
  return DLA_OK;
}

int dla_get_option(dla_ctx* c, int option)
{
  if (!c) return -1;
  if (option >= DLA_OPT_TUNE0 && option < DLA_OPT_TUNE0 + 8) return c->eng->get_tune(option - DLA_OPT_TUNE0);
  switch (option) {
    case DLA_OPT_CALLBACKS_ON_DEVICE: return c->callbacks_on_device;
    case DLA_OPT_EVEC_ON_DEVICE: return c->evec_on_device;
    case DLA_OPT_PROFILE: return c->eng->profile ? 1 : 0;
    case DLA_OPT_VERBOSE_ORTHO: return c->verbose_ortho;
    case DLA_OPT_CALLBACK_ORDER: return c->callback_order;
    case DLA_OPT_ORTHO_MAXIT: return c->eng->ortho_maxit;
    case DLA_OPT_CASLR_ALGORITHM: return c->caslr_algorithm;
    case DLA_OPT_STAGE_CHUNKS: return c->stage_chunks;
    case DLA_OPT_P2P_TIMEOUT_MS: return c->p2p_timeout_ms;
    case DLA_OPT_RUN_AHEAD: return c->run_ahead;
    case DLA_OPT_PENDING_BLOCKS: return c->pending_blocks;
    default: return -1;
  }
}

const char* dla_last_error(dla_ctx* c) { return c ? c->err.c_str() : "null context"; }
const char* dla_backend_name(dla_ctx* c) { return c ? c->eng->name() : "none"; }
void* dla_stream(dla_ctx* c) { return c ? c->eng->stream() : nullptr; }

int dla_get_stats(dla_ctx* c, dla_stats* out)
{
  if (!c || !out) return DLA_ERR_ARG;
  c->eng->collect_times();
  *out = c->eng->stats;
  return DLA_OK;
}

// HIP-event time per kernel class in milliseconds (DLA_OPT_PROFILE must be on while the work runs), in the order of the DLA_OP_*
// ids -- the door through which a Fortran caller reaches the breakdown SURVEY section 5 asks for beside the reference's four timers
int dla_class_times(dla_ctx* c, double* ms)
{
  if (!c || !ms) return DLA_ERR_ARG;
  c->eng->collect_times();
  for (int i = 0; i < DLA_OP_COUNT; ++i) ms[i] = c->eng->stats.ms[i];
  return DLA_OK;
}

int dla_reset_stats(dla_ctx* c)
{
  if (!c) return DLA_ERR_ARG;
  c->eng->collect_times();
  std::memset(&c->eng->stats, 0, sizeof(dla_stats));
  c->eng->reset_kernel_stats();
  return DLA_OK;
}

int dla_get_kernel_stats(dla_ctx* c, dla_kernel_stat* out, int cap)
{
  if (!c || !out || cap <= 0) return 0;
  return c->eng->kernel_stats(out, cap);
}

// ------------------------------------------------------------------ multi-GPU
int dla_comm_unique_id(char id[128]) { return dla::engine_unique_id(id); }

static int agree_on_shards(dla_ctx* c);

// Attaching a transport after the shard has been announced ends with the collective agreement on the shard layout
// (agree_on_shards); when THAT fails -- a layout the ranks refuse, or ranks that announce in different orders -- the transport just
// attached is taken down again, so that "failed" means "nothing attached" on every rank (round-4 advisor).
int dla_comm_init(dla_ctx* c, int nranks, int rank, const char id[128])
{
  if (!c) return DLA_ERR_ARG;
  int st = engfail(c, c->eng->comm_init(nranks, rank, id));
  if (st) return st;
  st = agree_on_shards(c);
  if (st) { const std::string keep = c->err; (void)c->eng->comm_finalize(); c->eng->peers_even = true; c->err = keep; }
  return st;
}

int dla_comm_finalize(dla_ctx* c)
{
  if (!c) return DLA_ERR_ARG;
  c->eng->peers_even = true;       // (comm_finalize takes every transport down: one rank again)
  return engfail(c, c->eng->comm_finalize());
}

// one-shot peer-to-peer all-reduce: see include/diaglib_amd.h
int dla_p2p_export(dla_ctx* c, int nranks, char handles[128])
{
  if (!c || !handles) return DLA_ERR_ARG;
  return engfail(c, c->eng->p2p_export(nranks, handles));
}

int dla_p2p_attach(dla_ctx* c, int nranks, int rank, const char* all_handles)
{
  if (!c || !all_handles) return DLA_ERR_ARG;
  int st = engfail(c, c->eng->p2p_attach(nranks, rank, all_handles));
  if (st) return st;
  st = agree_on_shards(c);
  if (st) { const std::string keep = c->err; (void)c->eng->p2p_detach(); c->err = keep; }
  return st;
}

// The mailboxes go; another transport (RCCL, a hook) may stay attached: what the ranks agreed on (Engine::peers_even) belongs to the
// layout, not to the transport, and is agreed again over what is left -- collectively, like the detach itself.
int dla_p2p_detach(dla_ctx* c)
{
  if (!c) return DLA_ERR_ARG;
  const int st = engfail(c, c->eng->p2p_detach());
  if (st) return st;
  if (c->eng->has_transport()) return agree_on_shards(c);
  c->eng->peers_even = true;
  return DLA_OK;
}

int dla_comm_info(dla_ctx* c, int* nranks, int* rank)
{
  if (!c) return DLA_ERR_ARG;
  if (nranks) *nranks = c->eng->nranks;
  if (rank) *rank = c->eng->rank;
  return DLA_OK;
}

int dla_set_allreduce_hook(dla_ctx* c, dla_allreduce_fn fn, void* user, int nranks, int rank)
{
  if (!c) return DLA_ERR_ARG;
  c->eng->hook = fn;
  c->eng->hook_user = user;
  c->eng->nranks = nranks;
  c->eng->rank = rank;
  if (fn) {
    const int st = agree_on_shards(c);
    if (st) { c->eng->hook = nullptr; c->eng->hook_user = nullptr; c->eng->nranks = 1; c->eng->rank = 0; c->eng->peers_even = true; }
    return st;
  }
  // the hook goes: whatever is still attached carries the agreement from now on
  if (c->eng->has_transport()) return agree_on_shards(c);
  c->eng->peers_even = true;
  return DLA_OK;
}

// The ranks agree on what every schedule decision may depend on (dla_internal.h: Engine::peers_even): the shard heights, gathered
// through the small-product transport.  Runs when both the shard and the transport are known, whichever comes last; collective.
static int agree_on_shards(dla_ctx* c)
{
  dla::Engine* e = c->eng;
  e->peers_even = true;
  if (e->nranks <= 1 || c->n_global <= 0) return DLA_OK;
  // [row0 of every rank | a tag per rank | n_global per rank]: the tag = a fixed word + the number of agreements this context has
  // taken part in.  Ranks that announce their shards in different orders relative to attaching the transport, or one that announces
  // once more than its peers, pair exchanges that do not belong together: the tags then differ and every rank that sees it says so
  // (round-4 advisor) instead of adopting a layout made of unrelated numbers.  Required order: every rank makes the same sequence
  // of dla_set_shard / dla_comm_init / dla_p2p_attach / dla_set_allreduce_hook calls.
  const int nr = e->nranks;
  const double tag = 4.0e15 + (double)(++c->agree_seq);
  std::vector<double> r0((size_t)3 * nr, 0.0);
  r0[e->rank] = (double)c->row0;
  r0[(size_t)nr + e->rank] = tag;
  r0[(size_t)2 * nr + e->rank] = (double)c->n_global;
  const int st = e->allreduce_host(r0.data(), 3 * nr, 0);
  if (st) return engfail(c, st);
  for (int r = 0; r < nr; ++r) {
    if (r0[(size_t)nr + r] != tag)
      return fail(c, DLA_ERR_COMM, "dla_set_shard: the ranks are not at the same agreement (shards announced / transports attached in different orders)");
    if (r0[(size_t)2 * nr + r] != (double)c->n_global)
      return fail(c, DLA_ERR_ARG, "dla_set_shard: the ranks announce different global row counts");
  }
  bool even = true;
  for (int r = 0; r < e->nranks; ++r) {
    const long long lo = (long long)r0[r], hi = r + 1 < e->nranks ? (long long)r0[r + 1] : c->n_global;
    if (hi < lo) return fail(c, DLA_ERR_ARG, "dla_set_shard: the shards are not contiguous in rank order");
    // (every rank sees the same layout and refuses it alike: no rank is left waiting for a peer that has given up)
    if (hi == lo) return fail(c, DLA_ERR_ARG, "dla_set_shard: a rank holds no rows (fewer rows than the layout needs for this many ranks)");
    if ((hi - lo) % 2 != 0) even = false;
  }
  e->peers_even = even;
  return DLA_OK;
}

int dla_set_shard(dla_ctx* c, long long n_global, long long row0)
{
  if (!c) return DLA_ERR_ARG;
  c->n_global = n_global;
  c->row0 = row0;
  return agree_on_shards(c);
}

// ------------------------------------------------------------------ memory
int dla_alloc(dla_ctx* c, size_t bytes, void** dev) { DLA_T("dla_alloc"); return engfail(c, c->eng->alloc(bytes, dev)); }
int dla_free(dla_ctx* c, void* dev) { DLA_T("dla_free"); return engfail(c, c->eng->free_(dev)); }
int dla_zero(dla_ctx* c, void* dev, size_t bytes) { DLA_T("dla_zero"); return engfail(c, c->eng->zero(dev, bytes)); }
int dla_upload(dla_ctx* c, void* dev, const void* host, size_t bytes) { DLA_T("dla_upload"); return engfail(c, c->eng->h2d(dev, host, bytes)); }
int dla_download(dla_ctx* c, void* host, const void* dev, size_t bytes) { DLA_T("dla_download"); return engfail(c, c->eng->d2h(host, dev, bytes)); }
int dla_copy(dla_ctx* c, void* dst, const void* src, size_t bytes) { DLA_T("dla_copy"); return engfail(c, c->eng->d2d(dst, src, bytes)); }
int dla_trim(dla_ctx* c, size_t* released) { if (!c) return DLA_ERR_ARG; return engfail(c, c->eng->trim(released)); }
int dla_sync(dla_ctx* c) { DLA_T("dla_sync"); return engfail(c, c->eng->sync()); }

// ------------------------------------------------------------------ block algebra
// Reference-schedule flops ("the flops of the BLAS calls the reference would issue for the iterations performed"): counted
// per LOGICAL operation at the entry point the driver calls -- the dgemm / dtrmm / daxpy / dnrm2 calls of the reference routine
// that entry stands for -- whatever the engine launches for it (fused, left pending, skipped).  Entry points that call other entry
// points count once, at the outermost level.  dla_stats::ref_flops; bench.py's `value` numerator.
namespace {
struct RefFlops {
  dla_ctx* c;
  RefFlops(dla_ctx* c_, double f) : c(c_) { if (c && c->ref_depth++ == 0) c->eng->stats.ref_flops += f; }
  ~RefFlops() { if (c) --c->ref_depth; }
};
// ortho_vs_x with the schedule measured on the reference: 5 x (Gram + dtrmm) on U, 2 x (X^T U, U -= X C)
inline double ortho_vs_x_flops(double n, double m, double k) { return 2.0 * n * (4.0 * m * k) + 15.0 * n * k * k; }
}  // namespace

int dla_gram(dla_ctx* c, int n, int l, const double* x, int k, const double* u, double* ch, int ldc)
{
  DLA_T("dla_gram");
  RefFlops rf(c, 2.0 * n * (double)l * k);                       // dgemm 't','n' (:1691, 3543)
  if (l <= 0 || k <= 0) return DLA_OK;
  return engfail(c, c->eng->gram(n, l, x, k, u, ch, ldc));
}

int dla_gram_lower(dla_ctx* c, int n, int l, const double* x, const double* u, double* ch, int ldc)
{
  DLA_T("dla_gram_lower");
  RefFlops rf(c, 2.0 * n * (double)l * l);                       // the reference forms the full product (:403)
  if (l <= 0) return DLA_OK;
  return engfail(c, c->eng->gram_lower(n, l, x, u, ch, ldc));
}

int dla_panel_gemm(dla_ctx* c, int n, int l, const double* x, int k, const double* ch, int ldc, double* z)
{
  DLA_T("dla_panel_gemm");
  RefFlops rf(c, 2.0 * n * (double)l * k);
  if (k <= 0) return DLA_OK;
  return engfail(c, c->eng->gemm(n, l, x, k, ch, ldc, z, 0));
}

int dla_panel_update(dla_ctx* c, int n, int l, const double* x, int k, const double* ch, int ldc, double* u)
{
  DLA_T("dla_panel_update");
  RefFlops rf(c, 2.0 * n * (double)l * k);
  if (k <= 0 || l <= 0) return DLA_OK;
  return engfail(c, c->eng->gemm(n, l, x, k, ch, ldc, u, 1));
}

int dla_trmm_linvt(dla_ctx* c, int n, int k, double* u, const double* linv, int ld)
{
  DLA_T("dla_trmm_linvt");
  // U <- U * Linv^T : W = Linv^T is upper triangular, W(p,j) = Linv(j,p) for p <= j
  std::vector<double> w((size_t)k * k, 0.0);
  for (int j = 0; j < k; ++j)
    for (int p = 0; p <= j; ++p) w[(size_t)p + (size_t)j * k] = linv[(size_t)j + (size_t)p * ld];
  return engfail(c, c->eng->trmm(n, k, u, w.data(), k));
}

// The fused sweeps of the orthogonalisation loops, exposed for direct parity tests (tests/test_kernels_gpu.py): the
// update and the Gram matrix of its result in one pass over the panel.
int dla_trmm_gram(dla_ctx* c, int n, int k, double* u, const double* w, int ldw, double* g, int ldg)
{
  DLA_T("dla_trmm_gram");
  if (k <= 0) return DLA_OK;
  return engfail(c, c->eng->trmm_gram(n, k, u, w, ldw, g, ldg));
}

int dla_update_gram(dla_ctx* c, int n, int l, const double* x, int k, const double* ch, int ldc, double* u, double* g, int ldg)
{
  DLA_T("dla_update_gram");
  if (k <= 0) return DLA_OK;
  return engfail(c, c->eng->update_gram(n, l, x, k, ch, ldc, u, g, ldg));
}

int dla_combo_gram(dla_ctx* c, int n, int m, const double* x, int k, const double* ch, int ldc, double* u, double* g, int ldg)
{
  DLA_T("dla_combo_gram");
  if (k <= 0) return DLA_OK;
  if (!c->eng->can_combo(m, k) || u != x + (size_t)n * m) return fail(c, DLA_ERR_ARG, "combo_gram: U must follow X in one panel, k <= 48");
  return engfail(c, c->eng->combo_gram(n, m, x, k, ch, ldc, u, g, ldg));
}

int dla_ritz_residual(dla_ctx* c, int n, int l, int m, const double* v, const double* av, const double* y, int ldy,
                      const double* eig, int n_res, const int* skip, double* evec, double* r, double* avy,
                      double* rnorm)
{
  DLA_T("dla_ritz_residual");
  {
    int act = 0;
    for (int i = 0; i < n_res; ++i) if (!(skip && skip[i])) ++act;
    // two dgemms (:1717, 1721) + daxpy / dnrm2 / maxval per open root (:1723-1732): the reference forms the Ritz vectors every time
    RefFlops rf(c, 4.0 * n * (double)l * m + 5.0 * n * (double)act);
  }
  std::vector<double> sm((size_t)2 * (n_res > 0 ? n_res : 1), 0.0);
  int st = c->eng->ritz_residual(n, l, m, v, av, y, ldy, eig, n_res, skip, evec, r, avy, sm.data());
  if (st) return engfail(c, st);
  double sqrtn = std::sqrt((double)global_rows(c, n));
  for (int i = 0; i < n_res; ++i) {
    if (skip && skip[i]) continue;
    rnorm[2 * i] = std::sqrt(sm[2 * i]) / sqrtn;     // dnrm2/sqrtn, diaglib.f90:1730
    rnorm[2 * i + 1] = sm[2 * i + 1];                // maxval(abs(r)), :1731
  }
  return DLA_OK;
}

int dla_ritz_residual_p(dla_ctx* c, int n, int l, int m, const double* v, const double* av, const double* y, int ldy,
                        const double* eig, int n_res, const int* skip, double* evec, double* r, double* avy,
                        double* rnorm, int k2, const double* c2, int ldc2, double* p, double* ap)
{
  DLA_T("dla_ritz_residual_p");
  {
    int act = 0;
    for (int i = 0; i < n_res; ++i) if (!(skip && skip[i])) ++act;
    RefFlops rf(c, 4.0 * n * (double)l * m + 5.0 * n * (double)act + 4.0 * n * (double)l * (k2 > 0 ? k2 : 0));     // + P = S cp, AP = AS cp (:495-501)
  }
  if (k2 < 0 || (k2 > 0 && (!c2 || !p || !ap || ldc2 < l))) return fail(c, DLA_ERR_ARG, "ritz_residual_p: bad extra block");
  std::vector<double> sm((size_t)2 * (n_res > 0 ? n_res : 1), 0.0);
  int st = c->eng->ritz_residual_p(n, l, m, v, av, y, ldy, eig, n_res, skip, evec, r, avy, sm.data(), k2, c2, ldc2, p, ap);
  if (st) return engfail(c, st);
  double sqrtn = std::sqrt((double)global_rows(c, n));
  for (int i = 0; i < n_res; ++i) {
    if (skip && skip[i]) continue;
    rnorm[2 * i] = std::sqrt(sm[2 * i]) / sqrtn;
    rnorm[2 * i + 1] = sm[2 * i + 1];
  }
  return DLA_OK;
}

int dla_ritz_residual2(dla_ctx* c, int n, int l, int m, const double* v, const double* av, const double* y1, int ldy1,
                       const double* y2, int ldy2, const double* eig, int n_res, const int* skip, double* e, double* r,
                       double* t_work, double* junk, double* rnorm)
{
  DLA_T("dla_ritz_residual2");
  if (c && n > 0 && l > 0 && m > 0) {
    int act = 0;
    for (int i = 0; i < n_res; ++i) if (!(skip && skip[i])) ++act;
    RefFlops rf(c, 4.0 * n * (double)l * m + 5.0 * n * (double)act);
  }
  if (!c || !v || !av || !y1 || !y2 || !eig || !e || !r || !t_work || !junk || !rnorm || n <= 0 || l <= 0 || m <= 0 || ldy1 < l || ldy2 < l ||
      n_res < 0 || n_res > m)
    return fail(c, DLA_ERR_ARG, "dla_ritz_residual2: bad argument");
  std::vector<double> sm((size_t)2 * (n_res > 0 ? n_res : 1), 0.0);
  int st = c->eng->ritz_residual2(n, l, m, v, av, y1, ldy1, y2, ldy2, eig, n_res, skip, e, r, t_work, junk, sm.data());
  if (st) return engfail(c, st);
  const double sqrtn = std::sqrt((double)global_rows(c, n));
  for (int i = 0; i < n_res; ++i) {
    if (skip && skip[i]) continue;
    rnorm[2 * i] = std::sqrt(sm[2 * i]) / sqrtn;
    rnorm[2 * i + 1] = sm[2 * i + 1];
  }
  return DLA_OK;
}

int dla_axpy(dla_ctx* c, size_t len, double alpha, const double* x, double* y)
{
  DLA_T("dla_axpy");
  RefFlops rf(c, 2.0 * (double)len);
  return engfail(c, c->eng->axpy(len, alpha, x, y));
}

int dla_nrm2(dla_ctx* c, size_t len, const double* x, double* out)
{
  DLA_T("dla_nrm2");
  RefFlops rf(c, 2.0 * (double)len);
  double s = 0.0;
  int st = c->eng->sumsq(len, x, &s);
  if (st) return engfail(c, st);
  *out = std::sqrt(s);
  return DLA_OK;
}

// measurement aid: device STREAM triad on len doubles, best of reps repetitions (bench.py's practical HBM ceiling)
int dla_stream_triad(dla_ctx* c, size_t len, int reps, double* gbps)
{
  if (!c || !gbps) return DLA_ERR_ARG;
  return engfail(c, c->eng->stream_triad(len, reps, gbps));
}

int dla_random_fill(dla_ctx* c, int n, int m, double* evec) { return engfail(c, c->eng->random_fill(n, m, evec, c->row0, 7ULL, 0.0, 0)); }

// benchmark guess (b) of SURVEY 8d: uniform [-0.5, 0.5) from the documented counter-based generator, GLOBAL row indices
int dla_fill_guess(dla_ctx* c, int n, int m, double* evec, unsigned long long seed, long long support_rows)
{
  return engfail(c, c->eng->random_fill(n, m, evec, c->row0, seed, -0.5, support_rows));
}

// ------------------------------------------------------------------ orthogonalisation
// ortho_cd, diaglib.f90:3185-3341.  The reference's macro-iteration is: Gram sweep, host Cholesky /
// triangular inverse / norm estimates, triangular update sweep.  Here the update sweep also returns
// the Gram matrix of the panel it has just written (Engine::trmm_gram), which is exactly the matrix
// the next macro-iteration starts from, so a macro-iteration costs one sweep instead of two.
// g_in (optional): Gram matrix of u already known to the caller (k x k, ld k).
// w_defer (optional, k x k): when given, the LAST triangular update may be left pending: if the caller is
// going to project U against X next anyway (always = force_defer, or only when growth*eps >= tol_ortho,
// i.e. when ortho_vs_x will do another pass), W = Linv^T is returned in w_defer with *deferred = true and
// the panel in memory still holds U before that update.  The caller folds W into its next sweep.
static int ortho_cd_impl(dla_ctx* c, dla::BlockOps* ops, int n, int k, double* u, double* growth, int* ok, const double* g_in,
                         double* w_defer = nullptr, bool* deferred = nullptr, bool force_defer = false)
{
  *growth = 1.0;
  *ok = 0;
  if (deferred) *deferred = false;
  if (k <= 0) { *ok = 1; return DLA_OK; }
  std::vector<double> metric((size_t)k * k), msave((size_t)k * k), gnext((size_t)k * k), w((size_t)k * k);
  bool have_g = (g_in != nullptr);
  if (have_g) gnext.assign(g_in, g_in + (size_t)k * k);
  int it = 0;
  bool macro_done = false;
  const int kMaxIt = ops->ortho_maxit;    // maxit, diaglib.f90:3224
  while (!macro_done) {
    if (++it > kMaxIt) {
      // reference prints and returns with ok=.false. (:3252-3254)
      std::printf("  ortho_cd failed with the following error: maximum number of iterations reached.\n");
      *ok = 0;
      return DLA_OK;
    }
    if (have_g) {
      metric = gnext;
    } else {
      int st = ops->gram(n, k, u, k, u, metric.data(), k);   // :3256
      if (st) return opsfail(c, ops, st);
    }
    msave = metric;
    int info = dla_potrf_lower(k, metric.data(), k);
    if (info != 0) {
      // level-shift ladder (:3265-3295): shift = max(eps*alpha*||U||_F, 2 eps), alpha = 100, 1000, ...
      double alpha = 100.0;
      double tr = 0.0;
      for (int i = 0; i < k; ++i) tr += msave[(size_t)i + (size_t)i * k];
      double unorm = std::sqrt(tr > 0.0 ? tr : 0.0);  // ||U||_F = sqrt(trace(U^T U)), dnrm2 at :3268
      int it_micro = 0;
      bool micro_done = false;
      while (!micro_done) {
        if (++it_micro > kMaxIt) {
          std::printf("  ortho_cd failed with the following error: maximum number of iterations for factorization reached.\n");
          *ok = 0;
          return fail(c, DLA_ERR_ORTHO, "ortho_cd: factorization failed after level shifting");  // reference: stop (:3283)
        }
        double shift = std::fmax(kEps * alpha * unorm, kTolOrtho);
        metric = msave;
        for (int i = 0; i < k; ++i) metric[(size_t)i + (size_t)i * k] += shift;
        info = dla_potrf_lower(k, metric.data(), k);
        alpha *= 10.0;
        micro_done = (info == 0);
      }
    }
    msave = metric;
    dla_trtri_lower(k, msave.data(), k);
    double l_norm = dla_norm_est(k, metric.data(), k);
    double linv_norm = dla_norm_est(k, msave.data(), k);
    double rcond = l_norm * linv_norm;
    *growth *= linv_norm;
    double error = kEps * rcond * rcond;
    macro_done = error < kTolOrtho;
    // U <- U Linv^T (:3327): W = Linv^T is upper triangular, W(p,j) = Linv(j,p) for p <= j
    std::fill(w.begin(), w.end(), 0.0);
    for (int j = 0; j < k; ++j)
      for (int p = 0; p <= j; ++p) w[(size_t)p + (size_t)j * k] = msave[(size_t)j + (size_t)p * k];
    int st;
    if (macro_done && w_defer && (force_defer || *growth * kEps >= kTolOrtho)) {
      std::copy(w.begin(), w.end(), w_defer);                                         // caller applies it in its next sweep
      *deferred = true;
      st = DLA_OK;
    } else if (macro_done) {
      st = ops->trmm(n, k, u, w.data(), k);                                        // last pass: no further Gram needed
    } else {
      st = ops->trmm_gram(n, k, u, w.data(), k, gnext.data(), k);
      have_g = true;
    }
    if (st) return opsfail(c, ops, st);
  }
  if (c->verbose_ortho) std::printf("  [dla] ortho_cd: %d macro iterations, growth %.3e\n", it, *growth);
  *ok = 1;
  return DLA_OK;
}

int dla_ortho_cd(dla_ctx* c, int n, int k, double* u, double* growth, int* ok)
{
  DLA_T("dla_ortho_cd");
  RefFlops rf(c, 6.0 * n * (double)k * k);                       // two macro-iterations of (dgemm 't','n' + dtrmm), :3256, 3327
  if (k > 0) {
    dla::OrthoReport rep;
    int stc = c->eng->ortho_chain(n, 0, k, nullptr, nullptr, u, &rep);
    if (stc) return engfail(c, stc);
    if (rep.handled) {
      *growth = rep.growth;
      *ok = rep.status == 1;
      if (c->verbose_ortho) std::printf("  [dla] ortho_cd (device chain): %d macro iterations, growth %.3e\n", rep.macro_its, rep.growth);
      if (rep.status == 2) std::printf("  ortho_cd failed with the following error: maximum number of iterations reached.\n");
      if (rep.status == 3) {
        std::printf("  ortho_cd failed with the following error: maximum number of iterations for factorization reached.\n");
        return fail(c, DLA_ERR_ORTHO, "ortho_cd: factorization failed after level shifting");
      }
      return DLA_OK;
    }
  }
  return ortho_cd_impl(c, c->eng, n, k, u, growth, ok, nullptr);
}

// The reference's fallback `ortho` (diaglib.f90:3052-3092): Householder QR of a copy (dgeqrf), then U <- U R^-1 (dtrsm).
// U R^-1 is the orthonormal factor Q of U = Q R with LAPACK's sign convention r_jj = -sign(alpha_j) ||x_j||, i.e. the
// Cholesky-QR factor Q+ (positive diagonal) with some columns negated.  Here:
//   1. Q+ comes from a column-wise Gram-Schmidt with re-orthogonalisation on the device -- robust exactly where this routine is
//      needed, after ortho_cd has given up on an ill-conditioned block;
//   2. the signs come from running the SAME Householder recurrence on a 2k x k host matrix M that is isometric to U:
//      M holds the columns of U in an orthonormal basis [e_1..e_k, Z] of span(U) + span(e_1..e_k); every Householder
//      vector of U lies in that span, so the reflections of M are those of U and diag(R) has the same signs.
// r (k x k, column-major): the triangular factor, U_in = Q r, accumulated from the projection coefficients
static int gram_schmidt2(dla_ctx* c, dla::BlockOps* ops, long long row0, int n, int k, double* u, double* r)
{
  std::fill(r, r + (size_t)k * k, 0.0);
  // column by column, each column projected against the finished ones TWICE before it is normalised ("twice is
  // enough": the second projection removes what the first one left behind for an ill-conditioned block)
  for (int j = 0; j < k; ++j) {
    double* uj = u + (size_t)n * j;
    double g0 = 0.0;
    int st = ops->gram(n, 1, uj, 1, uj, &g0, 1);
    if (st) return opsfail(c, ops, st);
    // A column that lies in the span of the finished ones (to rounding) has no direction of its own: what two projections
    // leave of it is noise that normalisation would blow up into a vector that is NOT orthogonal to the others.  LAPACK's
    // dgeqrf / dorgqr (the reference's `ortho`, diaglib.f90:3052-3092) return an arbitrary unit vector orthogonal to the
    // finished columns there (H_1 ... H_j-1 e_j, R(j, j) = 0); so does this: the column is replaced by a generated one
    // (counter-based generator on global row indices, the same on every rank layout) and orthogonalised like any other.
    for (int attempt = 0;; ++attempt) {
      for (int rep = 0; rep < 2 && j > 0; ++rep) {
        std::vector<double> h(j);
        st = ops->gram(n, j, u, 1, uj, h.data(), j);
        if (st) return opsfail(c, ops, st);
        st = ops->gemm(n, j, u, 1, h.data(), j, uj, 1);
        if (st) return opsfail(c, ops, st);
        if (attempt == 0) for (int p = 0; p < j; ++p) r[(size_t)p + (size_t)j * k] += h[p];
      }
      double g = 0.0;
      st = ops->gram(n, 1, uj, 1, uj, &g, 1);
      if (st) return opsfail(c, ops, st);
      const double floor2 = 4096.0 * kEps * kEps * (double)(j + 1) * g0;      // (64 eps)^2 (j + 1) ||u_j||^2
      if (g > floor2 && g > 0.0) {
        if (attempt == 0) r[(size_t)j + (size_t)j * k] = std::sqrt(g);      // (a replaced column has R(j, j) = 0)
        double w = 1.0 / std::sqrt(g);
        st = ops->trmm(n, 1, uj, &w, 1);
        if (st) return opsfail(c, ops, st);
        break;
      }
      if (attempt >= 3) return fail(c, DLA_ERR_ORTHO, "ortho: a column without a direction of its own");
      st = ops->fresh_column(n, uj, row0, 0x51EDULL + 131ULL * (unsigned long long)j + (unsigned long long)attempt);
      if (st) return opsfail(c, ops, st);
      st = ops->gram(n, 1, uj, 1, uj, &g0, 1);
      if (st) return opsfail(c, ops, st);
    }
  }
  return DLA_OK;
}

// signs of diag(R) of the Householder QR (dgeqr2 / dlarfg rules) of the rows x cols column-major matrix m (overwritten)
static void householder_diag_signs(int rows, int cols, std::vector<double>& m, std::vector<double>& sign)
{
  sign.assign(cols, 1.0);
  std::vector<double> v(rows);
  for (int j = 0; j < cols && j < rows; ++j) {
    double* cj = m.data() + (size_t)j * rows;
    const double alpha = cj[j];
    double xnorm2 = 0.0;
    for (int i = j + 1; i < rows; ++i) xnorm2 += cj[i] * cj[i];
    if (xnorm2 == 0.0) {                       // dlarfg: H = I, beta = alpha
      sign[j] = alpha < 0.0 ? -1.0 : 1.0;
      continue;
    }
    const double nrm = std::sqrt(alpha * alpha + xnorm2);
    const double beta = alpha >= 0.0 ? -nrm : nrm;
    sign[j] = beta < 0.0 ? -1.0 : 1.0;
    for (int i = 0; i < rows; ++i) v[i] = i < j ? 0.0 : cj[i];
    v[j] = alpha - beta;
    double vtv = 0.0;
    for (int i = j; i < rows; ++i) vtv += v[i] * v[i];
    for (int cc = j; cc < cols; ++cc) {
      double* col = m.data() + (size_t)cc * rows;
      double dot = 0.0;
      for (int i = j; i < rows; ++i) dot += v[i] * col[i];
      const double f = 2.0 * dot / vtv;
      for (int i = j; i < rows; ++i) col[i] -= f * v[i];
    }
  }
}

static int ortho_qr_impl(dla_ctx* c, dla::BlockOps* ops, long long row0, long long n_rows_global, int n, int k, double* u)
{
  if (k <= 0) return DLA_OK;
  if (n_rows_global < k) return fail(c, DLA_ERR_ARG, "ortho: more columns than rows");
  // 1. U = Q+ R+ on the device (Q+ replaces U)
  std::vector<double> rp((size_t)k * k);
  int st = gram_schmidt2(c, ops, row0, n, k, u, rp.data());
  if (st) return st;
  // 2. top k (global) rows of Q+ (the device engine gets them as E^T Q+ through the Gram door, so a row-sharded panel
  //    needs nothing new; host-size blocks are read directly)
  std::vector<double> qt((size_t)k * k);
  st = ops->top_rows(n, k, u, row0, qt.data());
  if (st) return opsfail(c, ops, st);
  // 3. the isometric small matrix.  With Q_low = Q+ without its top k rows, Q_low^T Q_low = I - Qt^T Qt = C C^T and
  //    Z = Q_low C^-T has orthonormal columns, so  U = [e_1..e_k, Z] [Qt; C^T] R+ :  M = [Qt; C^T] R+.  (Formed from the
  //    well-conditioned pieces Qt, C and the triangular R+, column by column -- the small singular directions of an
  //    ill-conditioned U keep their relative accuracy, which a Cholesky factor of U^T U - T^T T would not give them.)
  std::vector<double> sm((size_t)k * k);
  for (int j = 0; j < k; ++j)
    for (int i = 0; i < k; ++i) {
      double acc = (i == j) ? 1.0 : 0.0;
      for (int p = 0; p < k; ++p) acc -= qt[(size_t)p + (size_t)i * k] * qt[(size_t)p + (size_t)j * k];
      sm[(size_t)i + (size_t)j * k] = acc;
    }
  std::vector<double> cl = sm;
  if (dla_potrf_lower(k, cl.data(), k) != 0) {
    // (nearly) all of Q+ sits in its top k rows: a tiny shift keeps the factor defined; only signs are read off below
    cl = sm;
    for (int i = 0; i < k; ++i) cl[(size_t)i + (size_t)i * k] += 1e-14;
    if (dla_potrf_lower(k, cl.data(), k) != 0) std::fill(cl.begin(), cl.end(), 0.0);
  }
  std::vector<double> mm((size_t)2 * k * k, 0.0), sign;
  for (int j = 0; j < k; ++j)
    for (int p = 0; p <= j; ++p) {
      const double rpj = rp[(size_t)p + (size_t)j * k];
      if (rpj == 0.0) continue;
      for (int i = 0; i < k; ++i) mm[(size_t)i + (size_t)j * 2 * k] += qt[(size_t)i + (size_t)p * k] * rpj;        // Qt R+
      for (int i = 0; i <= p; ++i) mm[(size_t)(k + i) + (size_t)j * 2 * k] += cl[(size_t)p + (size_t)i * k] * rpj; // C^T R+
    }
  householder_diag_signs(2 * k, k, mm, sign);
  bool any = false;
  for (int j = 0; j < k; ++j) any = any || sign[j] < 0.0;
  if (!any) return DLA_OK;
  std::vector<double> w((size_t)k * k, 0.0);
  for (int j = 0; j < k; ++j) w[(size_t)j + (size_t)j * k] = sign[j];
  return engfail(c, ops->trmm(n, k, u, w.data(), k));
}

int dla_ortho_qr(dla_ctx* c, int n, int k, double* u)
{
  DLA_T("dla_ortho_qr");
  return ortho_qr_impl(c, c->eng, c->row0, global_rows(c, n), n, k, u);
}

// ortho_vs_x from the device chain's report onwards (`chain` = nullptr: no chain has run, the host-driven loop does it all)
static int ortho_vs_x_after_chain(dla_ctx* c, dla::BlockOps* ops, long long row0, long long n_rows_global, int n, int m, int k,
                                  const double* x, const double* bx, double* u, const dla::OrthoReport* chain);

// dla_expand_project mode 4 (ChainPolicy::tight()): the stored basis is orthonormal to 1e-8 per block only, and a projection against
// it leaves that share of what it removes.  The device chains know (TIGHT_REMOVES in hip_engine.hip); the host-driven loop follows the reference, whose
// growth test ends after one projection -- there the whole ortho_vs_x runs a second time: its first product X^T U is then what the
// first run left, 1e-8 |S|, and what the second run leaves of it is below rounding (tools/fuzz_pending_basis.py, FUZZ_WIDE).

static int ortho_vs_x_impl(dla_ctx* c, dla::BlockOps* ops, long long row0, long long n_rows_global, int n, int m, int k,
                           const double* x, const double* bx, double* u)
{
  if (k <= 0) return DLA_OK;
  // device-driven chain first (one host wait per call); shapes / modes it does not take run the host-driven loop
  dla::OrthoReport rep;
  int stc = ops->ortho_chain(n, m, k, x, bx, u, &rep);
  if (stc) return opsfail(c, ops, stc);
  int st = ortho_vs_x_after_chain(c, ops, row0, n_rows_global, n, m, k, x, bx, u, rep.handled ? &rep : nullptr);
  if (st == DLA_OK && m > 0 && c->eng->policy.tight() && !(rep.handled && rep.status == 1))
    st = ortho_vs_x_after_chain(c, ops, row0, n_rows_global, n, m, k, x, bx, u, nullptr);
  return st;
}

static int ortho_vs_x_after_chain(dla_ctx* c, dla::BlockOps* ops, long long row0, long long n_rows_global, int n, int m, int k,
                                  const double* x, const double* bx, double* u, const dla::OrthoReport* chain)
{
  const int kMaxIt = ops->ortho_maxit;    // maxit, diaglib.f90:3521
  bool resume = false;                    // the device chain stopped in ortho_cd and the Householder fallback has run
  int resume_it = 0;                      // ... after this many outer iterations
  {
    if (chain) {
      const dla::OrthoReport& rep = *chain;
      if (c->verbose_ortho)
        std::printf("  [dla] ortho_vs_x (device chain): %d outer iterations, %d macro iterations, status %d\n", rep.outer_its,
                    rep.macro_its, rep.status);
      if (rep.status == 1) return DLA_OK;
      if (rep.status == 3) {
        std::printf("  ortho_cd failed with the following error: maximum number of iterations for factorization reached.\n");
        return fail(c, DLA_ERR_ORTHO, "ortho_cd: factorization failed after level shifting");
      }
      // ortho_cd ran out of iterations on the device: U has had its maxit triangular updates, exactly what the
      // reference's ortho_cd leaves behind when it returns ok = .false.; the reference then calls `ortho` (:3534, :3549).
      // Do the same and go on where the reference goes on: after the ortho_cd in front of the loop (no outer iteration
      // yet) with the loop itself; inside the loop with the explicit ||X^T U|| test of :3559-3564.
      if (rep.status == 2) {
        std::printf("  ortho_cd failed with the following error: maximum number of iterations reached.\n");
        int stq = ortho_qr_impl(c, ops, row0, n_rows_global, n, k, u);
        if (stq) return stq;
        resume = true;
        resume_it = rep.outer_its;
      }
      // (status 4, the outer loop ran out of iterations: the host-driven loop repeats it and reports the failure)
    }
  }
  int ok = 0, it = 0;
  bool done = false;
  double growth = 1.0, xu_norm;
  std::vector<double> xu((size_t)(m > 0 ? m : 1) * k), gu((size_t)k * k);
  // When U is the block that follows X in the same panel (the drivers' layout: space(:,i_beg) after
  // space(:,1:ldu)), the last triangular update of an ortho_cd that is followed by a projection pass is not
  // applied on its own: with W = Linv^T pending,  X^T (U W) = (X^T U) W  and  U W - X (X^T U W) = [X | U] [-xu; W],
  // so the pass costs one Gram sweep and ONE sweep over [X | U] instead of a U sweep more (16 n k B).
  const bool combo = m > 0 && u == x + (size_t)n * m && ops->can_combo(m, k);
  std::vector<double> wdef(combo ? (size_t)k * k : 1), cprime(combo ? (size_t)(m + k) * k : 1);
  bool pending = false;
  int st = DLA_OK;
  if (resume) {
    it = resume_it;
    if (resume_it > 0) {
      // the failure was inside the loop: ||X^T U|| of the Householder factor decides (:3559-3564)
      double s2 = 0.0;
      if (m > 0) {
        st = ops->gram(n, m, bx, k, u, xu.data(), m);
        if (st) return opsfail(c, ops, st);
        for (size_t i = 0; i < (size_t)m * k; ++i) s2 += xu[i] * xu[i];
      }
      done = std::sqrt(s2) < kTolOrtho;
      if (!done && it > kMaxIt) return fail(c, DLA_ERR_ORTHO, " catastrophic failure of ortho_vs_x");
    }
  } else {
    st = ortho_cd_impl(c, ops, n, k, u, &growth, &ok, nullptr, combo ? wdef.data() : nullptr, &pending, true);   // :3533
    if (st) return st;
    if (!ok) { st = ortho_qr_impl(c, ops, row0, n_rows_global, n, k, u); if (st) return st; }         // :3534
  }
  while (!done) {
    ++it;
    if (m > 0) {
      st = ops->gram(n, m, bx, k, u, xu.data(), m);     // xu = X^T U  (:3543) / (BX)^T U (:3632)
      if (st) return opsfail(c, ops, st);
      // (dla_expand_project mode 5: the stored columns are X_c with X = X_c D the finished basis -- project with X_c (D D^T) X_c^T)
      st = ops->basis_dd(m, k, xu.data(), m);
      if (st) return opsfail(c, ops, st);
      if (pending) {
        // xu <- xu W ; C' = [-xu ; W]
        const int ldc = m + k;
        for (int j = 0; j < k; ++j) {
          for (int i = 0; i < m; ++i) {
            double sacc = 0.0;
            for (int p = 0; p <= j; ++p) sacc += xu[(size_t)i + (size_t)p * m] * wdef[(size_t)p + (size_t)j * k];
            cprime[(size_t)i + (size_t)j * ldc] = -sacc;
          }
          for (int p = 0; p < k; ++p) cprime[(size_t)(m + p) + (size_t)j * ldc] = wdef[(size_t)p + (size_t)j * k];
        }
        st = ops->combo_gram(n, m, x, k, cprime.data(), ldc, u, gu.data(), k);
        pending = false;
      } else {
        st = ops->update_gram(n, m, x, k, xu.data(), m, u, gu.data(), k);   // U -= X xu (:3544) + U^T U for :3548
      }
      if (st) return opsfail(c, ops, st);
    }
    st = ortho_cd_impl(c, ops, n, k, u, &growth, &ok, m > 0 ? gu.data() : nullptr,
                       combo ? wdef.data() : nullptr, &pending, false);          // :3548
    if (st) return st;
    if (!ok) {
      st = ortho_qr_impl(c, ops, row0, n_rows_global, n, k, u);                      // :3549
      if (st) return st;
      double s = 0.0;
      if (m > 0) {
        st = ops->gram(n, m, bx, k, u, xu.data(), m);   // :3559-3560
        if (st) return opsfail(c, ops, st);
        for (size_t i = 0; i < (size_t)m * k; ++i) s += xu[i] * xu[i];
      }
      xu_norm = std::sqrt(s);
    } else {
      xu_norm = growth * kEps;                             // :3562
    }
    done = xu_norm < kTolOrtho;                            // :3564  (pending implies !done, see ortho_cd_impl)
    if (it > kMaxIt) return fail(c, DLA_ERR_ORTHO, " catastrophic failure of ortho_vs_x");  // :3568
  }
  if (c->verbose_ortho) std::printf("  [dla] ortho_vs_x: %d outer iterations\n", it);
  return DLA_OK;
}

int dla_ortho_vs_x(dla_ctx* c, int n, int m, int k, const double* x, double* u)
{
  DLA_T("dla_ortho_vs_x");
  RefFlops rf(c, ortho_vs_x_flops(n, m, k));
  return ortho_vs_x_impl(c, c->eng, c->row0, global_rows(c, n), n, m, k, x, x, u);
}

int dla_b_ortho_vs_x(dla_ctx* c, int n, int m, int k, const double* x, const double* bx, double* u)
{
  DLA_T("dla_b_ortho_vs_x");
  RefFlops rf(c, ortho_vs_x_flops(n, m, k));
  return ortho_vs_x_impl(c, c->eng, c->row0, global_rows(c, n), n, m, k, x, bx, u);
}

// b_ortho, diaglib.f90:3094-3183 (use_svd=.false.): M = U^T BU, L = chol(M) (no failure
// handling in the reference: a failed factorisation is reported here as an error), then
// U <- U L^-T, BU <- BU L^-T.  The reference solves with dtrsm (:3177-3178); we apply the
// explicit inverse like ortho_cd does, which is the same linear map.
int dla_b_ortho(dla_ctx* c, int n, int m, double* u, double* bu)
{
  DLA_T("dla_b_ortho");
  RefFlops rf(c, 4.0 * n * (double)m * m);                       // U^T BU + two dtrsm (:3170-3178)
  if (m <= 0) return DLA_OK;
  std::vector<double> metric((size_t)m * m);
  int st = c->eng->gram(n, m, u, m, bu, metric.data(), m);
  if (st) return engfail(c, st);
  if (dla_potrf_lower(m, metric.data(), m) != 0) return fail(c, DLA_ERR_LAPACK, "b_ortho: metric not positive definite");
  dla_trtri_lower(m, metric.data(), m);
  st = dla_trmm_linvt(c, n, m, u, metric.data(), m);
  if (st) return st;
  return dla_trmm_linvt(c, n, m, bu, metric.data(), m);
}

// check_guess, diaglib.f90:3734-3786
int dla_check_guess(dla_ctx* c, int n, int m, double* evec)
{
  DLA_T("dla_check_guess");
  RefFlops rf(c, 2.0 * n * (double)m * m);                       // the Gram matrix of the guess (:3762)
  double growth;
  int ok;
  // one reduction serves both tests of the reference: ||evec||_F (dnrm2 at :3749) is sqrt(trace) of the Gram matrix (:3762)
  std::vector<double> ov((size_t)m * m);
  int st = c->eng->gram(n, m, evec, m, evec, ov.data(), m);
  if (st) return engfail(c, st);
  double tr = 0.0;
  for (int i = 0; i < m; ++i) tr += ov[(size_t)i + (size_t)i * m];
  if (tr == 0.0) {
    st = dla_random_fill(c, n, m, evec);
    if (st) return st;
    return dla_ortho_cd(c, n, m, evec, &growth, &ok);
  }
  double dn = 0.0, on = 0.0;
  for (int i = 0; i < m; ++i) {
    dn += ov[(size_t)i + (size_t)i * m] * ov[(size_t)i + (size_t)i * m];
    for (int j = 0; j < i; ++j) on += ov[(size_t)j + (size_t)i * m] * ov[(size_t)j + (size_t)i * m];
  }
  dn /= (double)m;
  if (dn != 1.0 || on != 0.0) {
    st = dla_ortho_cd(c, n, m, evec, &growth, &ok);   // :3774-3779
    if (st) return st;
    // The reference ignores ortho_cd's `ok` here (:3779) and goes on with what a failed factorisation left behind: a guess with
    // a repeated or a zero column then ends in duplicate eigenvectors and ok = .true. (tools/fuzz_degenerate_drivers.py).
    // Deliberate difference: such a guess is completed with the Householder fallback, as ortho_vs_x does when ortho_cd gives
    // up (:3534) -- the dependent columns are replaced by generated ones; a full-rank guess never gets here.
    if (!ok) return dla_ortho_qr(c, n, m, evec);
  }
  return DLA_OK;
}

// Plain host loops for the host-size coefficient blocks of get_coeffs (column-major, ld = rows): the few block
// operations the orthogonalisation control flow needs (dla::BlockOps), nothing else -- no memory management, no
// reductions over ranks (the coefficient blocks are replicated on every rank).
namespace {
struct CoeffOps final : dla::BlockOps {
  // (four columns of the right-hand block per pass over a column of the left-hand one: the loops below sit on the critical
  //  path of every LOBPCG iteration -- the device waits for the P coefficients -- and at n_max = 37 the plain triple loops
  //  took 190 us per get_coeffs call)
  int gram(int n, int l, const double* x, int k, const double* u, double* ch, int ldc) override
  {
    int j = 0;
    for (; j + 4 <= k; j += 4) {
      const double* u0 = u + (size_t)j * n; const double* u1 = u0 + n; const double* u2 = u1 + n; const double* u3 = u2 + n;
      for (int i = 0; i < l; ++i) {
        const double* xi = x + (size_t)i * n;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int r = 0; r < n; ++r) { const double xv = xi[r]; a0 += xv * u0[r]; a1 += xv * u1[r]; a2 += xv * u2[r]; a3 += xv * u3[r]; }
        ch[(size_t)i + (size_t)j * ldc] = a0; ch[(size_t)i + (size_t)(j + 1) * ldc] = a1;
        ch[(size_t)i + (size_t)(j + 2) * ldc] = a2; ch[(size_t)i + (size_t)(j + 3) * ldc] = a3;
      }
    }
    for (; j < k; ++j)
      for (int i = 0; i < l; ++i) {
        const double* xi = x + (size_t)i * n;
        const double* uj = u + (size_t)j * n;
        double acc = 0.0;
        for (int r = 0; r < n; ++r) acc += xi[r] * uj[r];
        ch[(size_t)i + (size_t)j * ldc] = acc;
      }
    return DLA_OK;
  }
  // out(:, j .. j+3) (+)= X C(:, j .. j+3), the columns of X read once per four output columns
  static void mul4(int n, int l, const double* x, const double* ch, int ldc, int j, int jn, double* o0, double* o1, double* o2, double* o3)
  {
    for (int i = 0; i < l; ++i) {
      const double* xi = x + (size_t)i * n;
      const double c0 = ch[(size_t)i + (size_t)j * ldc];
      const double c1 = jn > 1 ? ch[(size_t)i + (size_t)(j + 1) * ldc] : 0.0;
      const double c2 = jn > 2 ? ch[(size_t)i + (size_t)(j + 2) * ldc] : 0.0;
      const double c3 = jn > 3 ? ch[(size_t)i + (size_t)(j + 3) * ldc] : 0.0;
      if (c0 == 0.0 && c1 == 0.0 && c2 == 0.0 && c3 == 0.0) continue;      // (triangular factors)
      for (int r = 0; r < n; ++r) { const double xv = xi[r]; o0[r] += xv * c0; o1[r] += xv * c1; o2[r] += xv * c2; o3[r] += xv * c3; }
    }
  }
  int gemm(int n, int l, const double* x, int k, const double* ch, int ldc, double* z, int mode) override
  {
    std::vector<double> col((size_t)4 * n);
    for (int j = 0; j < k; j += 4) {
      const int jn = std::min(4, k - j);
      std::fill(col.begin(), col.end(), 0.0);
      mul4(n, l, x, ch, ldc, j, jn, &col[0], &col[n], &col[(size_t)2 * n], &col[(size_t)3 * n]);
      for (int q = 0; q < jn; ++q) {
        double* zj = z + (size_t)(j + q) * n;
        const double* cq = &col[(size_t)q * n];
        if (mode == 0) for (int r = 0; r < n; ++r) zj[r] = cq[r];
        else if (mode == 1) for (int r = 0; r < n; ++r) zj[r] -= cq[r];
        else for (int r = 0; r < n; ++r) zj[r] += cq[r];
      }
    }
    return DLA_OK;
  }
  int trmm(int n, int k, double* u, const double* w, int ld) override
  {
    std::vector<double> out((size_t)n * (k + 3), 0.0);
    for (int j = 0; j < k; j += 4) {
      const int jn = std::min(4, k - j);
      double* o = out.data() + (size_t)j * n;
      mul4(n, k, u, w, ld, j, jn, o, o + n, o + (size_t)2 * n, o + (size_t)3 * n);
    }
    std::memcpy(u, out.data(), sizeof(double) * (size_t)n * k);
    return DLA_OK;
  }
  int top_rows(int n, int k, const double* u, long long, double* qt) override
  {
    for (int j = 0; j < k; ++j)
      for (int i = 0; i < k; ++i) qt[(size_t)i + (size_t)j * k] = (i < n) ? u[(size_t)i + (size_t)j * n] : 0.0;
    return DLA_OK;
  }
};
}  // namespace

// get_coeffs, diaglib.f90:3686-3732.  Host-size (len_u <= 3 n_max) problem: the same
// The coefficient vectors are replicated on every rank, hence nothing is reduced over ranks here.
int dla_get_coeffs(dla_ctx* c, int len_a, int len_u, int n_max, int n_act, const double* a_red, double* u_x, double* u_p)
{
  DLA_T("dla_get_coeffs");
  int off_x = n_max - n_act;
  for (int j = 0; j < n_max; ++j)
    for (int i = 0; i < len_u; ++i) u_x[(size_t)i + (size_t)j * len_u] = a_red[(size_t)i + (size_t)j * len_a];
  for (int j = 0; j < n_act; ++j)
    for (int i = 0; i < len_u; ++i) u_p[(size_t)i + (size_t)j * len_u] = u_x[(size_t)i + (size_t)(off_x + j) * len_u];
  for (int j = 0; j < n_act; ++j) u_p[(size_t)(off_x + j) + (size_t)j * len_u] -= 1.0;
  if (n_act <= 0) return DLA_OK;
  // u_x / u_p are len_u x n_max coefficient blocks (len_u <= 3 n_max rows, O(1) in n), identical on every
  // rank: like the Cholesky factors and the projected eigenproblem they are host-size data, so the same
  // ortho_vs_x control flow runs on them through the coefficient algebra below -- no launches, no reductions.
  CoeffOps small;
  small.ortho_maxit = c->eng->ortho_maxit;
  return ortho_vs_x_impl(c, &small, 0, len_u, len_u, n_max, n_act, u_x, u_x, u_p);
}

// ------------------------------------------------------------------ callbacks
static int ensure_stage(dla_ctx* c, size_t bytes)
{
  if (bytes <= c->stage_bytes) return DLA_OK;
  (void)c->eng->sync();                    // uploads of an earlier callback may still read the old buffers
  if (c->stage_x) c->eng->host_free(c->stage_x);
  if (c->stage_y) c->eng->host_free(c->stage_y);
  c->stage_x = c->stage_y = nullptr;
  c->stage_bytes = 0;
  void *a = nullptr, *b = nullptr;
  if (c->eng->host_alloc(bytes, &a) || c->eng->host_alloc(bytes, &b)) return fail(c, DLA_ERR_ALLOC, "pinned staging allocation failed");
  c->stage_x = (double*)a;
  c->stage_y = (double*)b;
  c->stage_bytes = bytes;
  return DLA_OK;
}

// Host-mode callback on an n x m block: the block is cut into column chunks (the reference contract lets m vary from call to
// call, reference diaglib.f90:1685-1786) that flow through  download | user routine | upload  concurrently.
// The staging buffers must outlive the uploads still in flight when this returns: they are only reused by the next
// callback, whose stage_begin() follows those uploads on the engine's stream (ensure_stage reallocations drain first).
static int staged_callback(dla_ctx* c, int n, int m, const double* x, double* y,
                           const std::function<void(int, const double*, double*)>& call,
                           const std::function<int(int, int)>& after_upload = nullptr, int min_chunks = 1)
{
  const size_t col = sizeof(double) * (size_t)n;
  int st = ensure_stage(c, col * m);
  if (st) return st;
  // One call of the caller's routine per block, like the reference (diaglib.f90:1685, 1786: matvec / precnd see every block
  // exactly once, whole).  Column chunks (DLA_OPT_STAGE_CHUNKS >= 2) overlap a chunk's transfers with the routine's work on
  // its neighbours, but every chunk is another call: an operator pays its own fixed traffic (its matrix) per call and a
  // caller may count calls.  Measured r04 on the benchmark with the harness' operator (tools/host_mode_timeline.py, time
  // inside the caller's routine per solve): 74 ms in 17 calls, 113 ms in 34 half-block calls, 184 ms in 66, 284 ms in 113 --
  // 231 / 216 / 255 / 350 ms per solve: what the overlap gains the extra calls take back.  Hence opt-in.
  int nchunk = 1;
  nchunk = std::min(std::max(nchunk, min_chunks), m);
  if (c->stage_chunks > 0) nchunk = std::min(c->stage_chunks, m);
  const int per = (m + nchunk - 1) / nchunk;
  st = c->eng->stage_begin();
  if (st) return engfail(c, st);
  int slot = 0;
  for (int c0 = 0; c0 < m; c0 += per, ++slot) {
    const int mc = std::min(per, m - c0);
    DLA_T("  stage d2h (enqueue)");
    st = c->eng->stage_d2h(c->stage_x + (size_t)c0 * n, x + (size_t)c0 * n, col * mc, slot);
    if (st) return engfail(c, st);
  }
  slot = 0;
  for (int c0 = 0; c0 < m; c0 += per, ++slot) {
    int mc = std::min(per, m - c0);
    { DLA_T("  stage d2h (wait)"); st = c->eng->stage_wait(slot); }
    if (st) return engfail(c, st);
    { DLA_T("  user callback"); call(mc, c->stage_x + (size_t)c0 * n, c->stage_y + (size_t)c0 * n); }
    DLA_T("  stage h2d (enqueue)");
    st = c->eng->stage_h2d(y + (size_t)c0 * n, c->stage_y + (size_t)c0 * n, col * mc);
    if (st) return engfail(c, st);
    if (after_upload) { st = after_upload(c0, mc); if (st) return st; }     // (device work on this chunk, behind its upload)
  }
  return engfail(c, c->eng->stage_end());
}

// The library's own device-resident callbacks.  All of them enqueue on the engine's stream (ordering contract 2 whatever the
// context says); the operators among them are pure functions of their input block (safe to call again on the same block).
struct OwnCallback { void* fn; bool pure_operator, on_engine_stream; };
static const OwnCallback* own_callback(void* fn)
{
  static const OwnCallback table[] = {
    {(void*)&dla_synth_matvec, true, true}, {(void*)&dla_synth_apbmul, true, true}, {(void*)&dla_synth_ambmul, true, true},
    {(void*)&dla_synth_spdmul, true, true}, {(void*)&dla_synth_smdmul, true, true}, {(void*)&dla_synth_metric, true, true},
    {(void*)&dla_spmm_matvec, true, true}, {(void*)&dla_spmm_bvec, true, true}, {(void*)&dla_spmm_apbmul, true, true},
    {(void*)&dla_spmm_ambmul, true, true}, {(void*)&dla_spmm_spdmul, true, true}, {(void*)&dla_spmm_smdmul, true, true},
    {(void*)&dla_synth_precnd, false, true}, {(void*)&dla_spmm_precnd, false, true}, {(void*)&dla_spmm_precnd_pencil, false, true},
    {(void*)&dla_synth_lrprec1, false, true}, {(void*)&dla_synth_lrprec2, false, true}, {(void*)&dla_spmm_lrprec1, false, true},
    {(void*)&dla_spmm_lrprec2, false, true}, {(void*)&dla_spmm_precnd_cheb, false, true},
    {(void*)&dla_spmm_precnd_cheb_jacobi, false, true}, {(void*)&dla_spmm_precnd_cheb_pencil, false, true},
    {(void*)&dla_dense_matvec, true, true}, {(void*)&dla_dense_bvec, true, true}, {(void*)&dla_dense_matvec_t, true, true},
    {(void*)&dla_spmm_matvec_t, true, true},
    {(void*)&dla_dense_apbmul, true, true}, {(void*)&dla_dense_ambmul, true, true}, {(void*)&dla_dense_spdmul, true, true},
    {(void*)&dla_dense_smdmul, true, true},
    {(void*)&dla_dense_precnd, false, true}, {(void*)&dla_dense_precnd_pencil, false, true},
    {(void*)&dla_dense_lrprec1, false, true}, {(void*)&dla_dense_lrprec2, false, true}};
  for (const OwnCallback& r : table)
    if (r.fn == fn) return &r;
  return nullptr;
}
static bool builtin_operator(dla_matvec_fn fn)
{
  const OwnCallback* r = own_callback((void*)fn);
  return r && r->pure_operator;
}
// the ordering contract of a device-mode callback: 2 for the library's own, else the context's
static int callback_order_of(dla_ctx* c, void* fn)
{
  const OwnCallback* r = own_callback(fn);
  return r && r->on_engine_stream ? 2 : c->callback_order;
}

// which of the library's diagonal preconditioners on a device-resident diagonal fn is (Engine::ritz_expand); -1: none of them
static int diagonal_precnd_kind(dla_precnd_fn fn)
{
  if (!own_callback((void*)fn)) return -1;
  return fn == &dla_synth_precnd ? 0 : fn == &dla_spmm_precnd ? 1 : fn == &dla_dense_precnd ? 2 : -1;
}

int dla_ritz_expand(dla_ctx* c, int n, int l, int m, const double* v, const double* av, const double* y, int ldy,
                    const double* eig, int n_res, const int* skip, double* evec, double* r, double* avy, double* rnorm,
                    dla_precnd_fn precnd, double fac, int first, int k, double* u0, int* fused)
{
  if (fused) *fused = 0;
  const int kind = precnd ? diagonal_precnd_kind(precnd) : -1;
  const bool may_fuse = c && fused && kind >= 0 && c->callbacks_on_device && !evec && !avy && u0 && r && v && av && y && eig && rnorm &&
                        n > 0 && l > 0 && m > 0 && m <= 16 && ldy >= l && n_res >= 0 && n_res <= m && first >= 1 && first <= m && k == m - first + 1;
  if (may_fuse) {
    DLA_T("dla_ritz_expand");
    std::vector<double> sm((size_t)2 * (n_res > 0 ? n_res : 1), 0.0);
    int ran = 0;
    const int st = c->eng->ritz_expand(n, l, m, v, av, y, ldy, eig, n_res, skip, r, sm.data(), kind, fac, first - 1, k, u0, &ran);
    if (st) return engfail(c, st);
    if (ran) {
      int act = 0;
      for (int i = 0; i < n_res; ++i) if (!(skip && skip[i])) ++act;
      // (the logical operation is dla_ritz_residual's: the block's diagonal scaling and its measurement belong to the calls that
      //  the caller leaves out or that find their first sweep done, and those book themselves)
      { RefFlops rf(c, 4.0 * n * (double)l * m + 5.0 * n * (double)act); }
      const double sqrtn = std::sqrt((double)global_rows(c, n));
      for (int i = 0; i < n_res; ++i) {
        if (skip && skip[i]) continue;
        rnorm[2 * i] = std::sqrt(sm[2 * i]) / sqrtn;
        rnorm[2 * i + 1] = sm[2 * i + 1];
      }
      *fused = 1;
      return DLA_OK;
    }
  }
  return dla_ritz_residual(c, n, l, m, v, av, y, ldy, eig, n_res, skip, evec, r, avy, rnorm);
}

int dla_ritz_expand_counts(dla_ctx* c, long long* run, long long* discarded)
{
  if (!c || !run || !discarded) return fail(c, DLA_ERR_ARG, "dla_ritz_expand_counts: bad argument");
  c->eng->ritz_expand_counts(run, discarded);
  return DLA_OK;
}

int dla_ritz_expand_measured(dla_ctx* c, int m, int k, double* xug, int ld)
{
  if (!c || !xug || m <= 0 || k <= 0 || ld < m + k) return fail(c, DLA_ERR_ARG, "dla_ritz_expand_measured: bad argument");
  return engfail(c, c->eng->ritz_expand_measured(m, k, xug, ld));
}

int dla_call_matvec(dla_ctx* c, dla_matvec_fn fn, int n, int m, const double* x, double* ax)
{
  DLA_T("dla_call_matvec");
  if (m <= 0) return DLA_OK;
  if (c->callbacks_on_device) {
    // the built-in operators run on the engine's own stream: nothing to order
    const int order = callback_order_of(c, (void*)fn);
    int st = c->eng->callback_begin(order);
    if (st) return engfail(c, st);
    fn(&n, &m, x, ax);
    if (int cbs = callback_status(c)) { (void)c->eng->callback_end(order); return cbs; }
    return engfail(c, c->eng->callback_end(order));
  }
  const int sts = staged_callback(c, n, m, x, ax, [&](int mc, const double* hx, double* hy) { fn(&n, &mc, hx, hy); });
  if (int cbs = callback_status(c)) return cbs;
  return sts;
}

// Expansion step of the Davidson / LOBPCG drivers (include/diaglib_amd.h).  The three operations form a dependent chain on
// the device and the host has nothing to decide between them unless the orthogonalisation takes an unusual turn -- so they
// are enqueued back to back and the chain's report comes in with the projected block.
static int expand_apply_project(dla_ctx* c, int mode, int n, int m, int k, double* basis, double* abasis, dla_matvec_fn fn,
                                double shift, double* h, int ldh)
{
  double* u = basis + (size_t)n * m;
  double* au = abasis + (size_t)n * m;
  int st = dla_call_matvec(c, fn, n, k, u, au);
  if (st) return st;
  if (shift != 0.0) { st = dla_axpy(c, (size_t)n * k, shift, u, au); if (st) return st; }
  if (mode == 0) return dla_gram(c, n, m + k, basis, k, au, h, ldh);
  return dla_gram_lower(c, n, m + k, basis, abasis, h, ldh);
}

static int expand_project_impl(dla_ctx* c, int mode, int n, int m, int k, double* basis, double* abasis, dla_matvec_fn fn,
                               double shift, double* h, int ldh);

// dot product with four partial sums, so that the compiler may keep them in one vector register
static inline double dot4(const double* a, const double* b, int n)
{
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int i = 0;
  for (; i + 4 <= n; i += 4) { s0 += a[i] * b[i]; s1 += a[i + 1] * b[i + 1]; s2 += a[i + 2] * b[i + 2]; s3 += a[i + 3] * b[i + 3]; }
  for (; i < n; ++i) s0 += a[i] * b[i];
  return (s0 + s1) + (s2 + s3);
}

// The closing pass of ortho_vs_x on the small side.  A device chain that ends with a pending block hands over p = [E' ; T]: the
// stored block U_c has the measured products S = X_c^T U_c and G = U_c^T U_c, T is the inverse Cholesky factor of G
// (T^T G T = I) and E' = -S T -- the reference's closing pass (diaglib.f90:3543-3544, then one macro-iteration of ortho_cd,
// :3256-3327) written as coefficients of the stored columns.  Two things are still open and are settled here, exactly:
//   * the stored columns X_c are themselves unfinished blocks, X = X_c D with D upper triangular (dmat; nullptr: D = I), so
//     X_c^T X_c = (D D^T)^-1 and the projection that makes the new block orthogonal to X is E = -(X_c^T X_c)^-1 S T = D D^T E';
//   * the Gram matrix of U_c T + X_c E is I - F^T F with F = D^T E' (G was measured before the projection, not after it):
//     one more k x k Cholesky factor R, R^T (I - F^T F) R = I.
// Out: p = [E ; T] R -- the finished block is [X_c | U_c] p, orthogonal to X_c D and orthonormal, to the accuracy S and G were
// measured with.  E' = 0 (nothing but a triangular factor pending) is left alone.
// applied: the chain's closing sweep has already applied [E' ; T] to the block in memory (it measured nothing behind it); what is
// still owed is the difference, [E - E' ; I] R.
static int close_pending_block(int m, int k, double* p, int ldp, const double* dmat, int ld, int applied)
{
  double emax = 0.0;
  for (int j = 0; j < k; ++j)
    for (int i = 0; i < m; ++i) emax = std::max(emax, std::fabs(p[(size_t)i + (size_t)j * ldp]));
  if (emax == 0.0) return DLA_OK;
  // TEST hook ($DIAGLIB_AMD_FAIL_CLOSE = n: the n-th closing pass of the calling thread reports a factor that is not positive
  // definite): nothing bounds |D| |T| where a chain ended, so the failure exists in principle and its recovery -- the block is finished
  // in memory instead, dla_expand_project mode 6 / the repeat inside mode 3 -- must be exercised (tests/test_pending_basis_gpu.py)
  {
    static thread_local long n_close = 0;
    const char* fc = std::getenv("DIAGLIB_AMD_FAIL_CLOSE");
    if (fc != nullptr && ++n_close == std::atol(fc)) return DLA_ERR_ORTHO;
  }
  // (D = I + N: the products with N matter only when |N| |E'| m reaches rounding level in E -- skip them otherwise)
  double nmax = 0.0;
  if (dmat)
    for (int q = 0; q < m; ++q) {
      const double* dq = dmat + (size_t)q * ld;
      for (int i = 0; i < q; ++i) nmax = std::max(nmax, std::fabs(dq[i]));
      nmax = std::max(nmax, std::fabs(dq[q] - 1.0));
    }
  const bool with_d = dmat != nullptr && nmax * emax * (double)m > 1.0e-19;
  std::vector<double> f((size_t)m * k), mm((size_t)k * k), e((size_t)m * k, 0.0);
  for (int j = 0; j < k; ++j) {
    const double* ej = p + (size_t)j * ldp;
    double* fj = &f[(size_t)j * m];
    if (with_d) for (int r = 0; r < m; ++r) fj[r] = dot4(dmat + (size_t)r * ld, ej, r + 1);      // F = D^T E'
    else for (int r = 0; r < m; ++r) fj[r] = ej[r];
  }
  for (int j = 0; j < k; ++j)
    for (int i = j; i < k; ++i)
      mm[(size_t)i + (size_t)j * k] = (i == j ? 1.0 : 0.0) - dot4(&f[(size_t)i * m], &f[(size_t)j * m], m);
  if (dla_potrf_lower(k, mm.data(), k) != 0) return DLA_ERR_ORTHO;
  if (dla_trtri_lower(k, mm.data(), k) != 0) return DLA_ERR_ORTHO;          // mm = L^-1 (lower); R = L^-T
  for (int j = 0; j < k; ++j) {                  // E = D F
    const double* fj = &f[(size_t)j * m];
    double* ej = &e[(size_t)j * m];
    if (with_d) {
      for (int q = 0; q < m; ++q) {
        const double fq = fj[q];
        if (fq == 0.0) continue;
        const double* dq = dmat + (size_t)q * ld;
        for (int i = 0; i <= q; ++i) ej[i] += dq[i] * fq;
      }
    } else {
      for (int i = 0; i < m; ++i) ej[i] = fj[i];
    }
  }
  for (int j = 0; j < k; ++j) {
    for (int i = 0; i < m; ++i) p[(size_t)i + (size_t)j * ldp] = e[(size_t)i + (size_t)j * m] - (applied ? p[(size_t)i + (size_t)j * ldp] : 0.0);
    if (applied) for (int i = 0; i < k; ++i) p[(size_t)(m + i) + (size_t)j * ldp] = (i == j) ? 1.0 : 0.0;
  }
  // p <- p R, R(q, j) = Linv(j, q) for q <= j: columns from the right, in place
  const int l = m + k;
  for (int j = k - 1; j >= 0; --j) {
    double* pj = p + (size_t)j * ldp;
    const double rjj = mm[(size_t)j + (size_t)j * k];
    for (int i = 0; i < l; ++i) pj[i] *= rjj;
    for (int q = 0; q < j; ++q) {
      const double rq = mm[(size_t)j + (size_t)q * k];
      if (rq == 0.0) continue;
      const double* pq = p + (size_t)q * ldp;
      for (int i = 0; i < l; ++i) pj[i] += pq[i] * rq;
    }
  }
  return DLA_OK;
}

// What a call of dla_expand_project gets, from the mode it asked for and what the context and the engine can do
enum class Treatment { Plain0, Plain1, Rebuild, Stay, StayExact, HostLoopExact, Refused };

// bs = basis_state(m), exact_ok = basis_exact_ok(), capacity = basis_capacity() of the engine
static Treatment resolve_treatment(int mode, bool pending_blocks, int bs, bool exact_ok, int k, int m, int capacity)
{
  // (DLA_OPT_PENDING_BLOCKS = 0 makes modes 3 / 4 / 5 behave like 1 / 0 / 0: the chain finishes the block in memory)
  if (mode == 3 && !pending_blocks) return Treatment::Plain1;
  if ((mode == 4 || mode == 5) && !pending_blocks && bs <= 0) return Treatment::Plain0;
  if (mode == 5 || mode == 6) {
    // mode 5 = mode 4 with the caller's pending blocks kept on the device as well (ChainPolicy::stay(true))
    // (where the device cannot project with D -- wider blocks, a wider basis, an all-reduce hook -- the block is finished in memory,
    //  mode 0: nothing of it stays pending in a basis that later blocks are projected against)
    const bool exact = mode == 5 && pending_blocks && exact_ok && k <= 16 && m + k <= capacity;
    // What the copy of the caller's D says about the m stored columns decides what a call that cannot be exact may do (round-5
    // advisor: the device's ability can change between two calls of one solve -- a refused LDS request lowers the engine's limit --
    // and earlier blocks of the basis may already be pending with max |S| up to 0.05, i.e. the stored columns are not orthonormal):
    //   D = I there:         the stored columns are a finished basis; mode 0 is exact against it;
    //   D != I:              the block is finished in memory by the host-driven loop, which multiplies every X^T U with D D^T
    //                        (BlockOps::basis_dd) -- exact against the finished basis X D, nothing stays pending;
    //   no copy of these m:  refused -- a plain projection against unfinished columns would lose orthogonality without a word.
    // mode 6 asks for the second treatment outright: a block whose closing algebra the caller could not complete (dla_basis_admit
    // answered DLA_ERR_ORTHO: I - F^T F not positive definite) is finished in memory from what the chain stored.
    if (bs < 0) return Treatment::Refused;
    if (mode == 6 || (!exact && bs > 0)) return Treatment::HostLoopExact;
    return exact ? Treatment::StayExact : Treatment::Plain0;
  }
  return mode == 4 ? Treatment::Stay : mode == 3 ? Treatment::Rebuild : mode == 1 ? Treatment::Plain1 : Treatment::Plain0;
}

// a chain that failed behind a finished orthogonalisation must not leave its block to the next call (round-4 advisor)
namespace {
struct Forget { dla_ctx* c; int m, k; bool keep = false; ~Forget() { if (!keep) { std::vector<double> junk((size_t)(m + k) * k); (void)c->eng->pending_block(m, k, junk.data(), m + k, nullptr); } } };
}  // namespace

// expand_project_impl under a policy that publishes; on success what the chain left pending becomes the context's pending block
static int run_and_take_pending(dla_ctx* c, const dla::ChainPolicy& policy, int impl_mode, int n, int m, int k, double* basis,
                                double* abasis, dla_matvec_fn fn, double shift, double* h, int ldh)
{
  dla::PolicyScope scope(c->eng, policy);
  Forget forget{c, m, k};
  const int st = expand_project_impl(c, impl_mode, n, m, k, basis, abasis, fn, shift, h, ldh);
  if (st) return st;
  forget.keep = true;
  c->pending_p.assign((size_t)(m + k) * k, 0.0);
  const int stp = c->eng->pending_block(m, k, c->pending_p.data(), m + k, &c->pending_applied);
  if (stp) return engfail(c, stp);
  c->pending_k = k; c->pending_m = m;
  return DLA_OK;
}

// mode 3: the projection of the stored blocks is corrected for the closed pending block p ((m + k) x k, ld m + k),
// H <- D^T H D with D = [I E ; 0 T] = [I_x | p]
static void fold_pending_into_projection(int m, int k, const double* p, double* h, int ldh)
{
  const int l = m + k;
  bool ident = true;
  for (int j = 0; j < k && ident; ++j)
    for (int i = 0; i < l; ++i) if (p[(size_t)i + (size_t)j * l] != (i == m + j ? 1.0 : 0.0)) { ident = false; break; }
  if (ident) return;
  // lower triangle of H (l x l): the W rows become  p^T H_full [I_x | p]  (H_xx is untouched)
  std::vector<double> hf((size_t)l * l), g((size_t)l * k);
  for (int j = 0; j < l; ++j)
    for (int i = 0; i < l; ++i) hf[(size_t)i + (size_t)j * l] = (i >= j) ? h[(size_t)i + (size_t)j * ldh] : h[(size_t)j + (size_t)i * ldh];
  // g = H_full p  (l x k)
  for (int j = 0; j < k; ++j) {
    double* gj = &g[(size_t)j * l];
    for (int q = 0; q < l; ++q) {
      const double pq = p[(size_t)q + (size_t)j * l];
      if (pq == 0.0) continue;
      const double* hq = &hf[(size_t)q * l];
      for (int i = 0; i < l; ++i) gj[i] += hq[i] * pq;
    }
  }
  // rows m .. l-1, columns 0 .. m-1:  (p^T H_full)(:, x) = g(x, :)^T by symmetry;  columns m .. : p^T g
  for (int i = 0; i < k; ++i) {
    for (int b = 0; b < m; ++b) h[(size_t)(m + i) + (size_t)b * ldh] = g[(size_t)b + (size_t)i * l];
    for (int j = 0; j <= i; ++j) {
      double acc = 0.0;
      for (int q = 0; q < l; ++q) acc += p[(size_t)q + (size_t)i * l] * g[(size_t)q + (size_t)j * l];
      h[(size_t)(m + i) + (size_t)(m + j) * ldh] = acc;
    }
  }
}

int dla_expand_project(dla_ctx* c, int mode, int n, int m, int k, double* basis, double* abasis, dla_matvec_fn fn,
                       double shift, double* h, int ldh)
{
  DLA_T("dla_expand_project");
  // ortho_vs_x (:1790 / 523-529) + the projection (:1691 / 401-403) [+ daxpy :397]; the operator is the caller's
  RefFlops rf(c, c && n > 0 && k > 0 ? ortho_vs_x_flops(n, m, k) + (shift != 0.0 ? 2.0 * n * (double)k : 0.0) +
                                       ((mode == 0 || mode >= 4) ? 2.0 * n * (double)(m + k) * k : 2.0 * n * (double)(m + k) * (m + k)) : 0.0);
  if (!c || !basis || !abasis || !h || !fn || mode < 0 || mode == 2 || mode > 6 || n <= 0 || m < 0 || k <= 0 || ldh < m + k)
    return fail(c, DLA_ERR_ARG, "dla_expand_project: bad argument (n > 0, m >= 0, k > 0, ldh >= m + k)");
  c->pending_k = 0; c->pending_m = 0; c->pending_applied = 0;
  switch (resolve_treatment(mode, c->pending_blocks != 0, c->eng->basis_state(m), c->eng->basis_exact_ok(), k, m, c->eng->basis_capacity())) {
  case Treatment::Refused:
    return fail(c, DLA_ERR_ARG, "dla_expand_project: the engine's copy of the caller's pending blocks does not describe the columns in front of "
                                "this block (dla_basis_sync after every block of the basis, identity ones included)");
  case Treatment::Plain0: return expand_project_impl(c, 0, n, m, k, basis, abasis, fn, shift, h, ldh);
  case Treatment::Plain1: return expand_project_impl(c, 1, n, m, k, basis, abasis, fn, shift, h, ldh);
  case Treatment::HostLoopExact: {
    dla::PolicyScope scope(c->eng, dla::ChainPolicy::host_loop_exact());
    return expand_project_impl(c, 0, n, m, k, basis, abasis, fn, shift, h, ldh);
  }
  case Treatment::Stay: return run_and_take_pending(c, dla::ChainPolicy::stay(false), 0, n, m, k, basis, abasis, fn, shift, h, ldh);
  case Treatment::StayExact: return run_and_take_pending(c, dla::ChainPolicy::stay(true), 0, n, m, k, basis, abasis, fn, shift, h, ldh);
  case Treatment::Rebuild: break;
  }
  int st = run_and_take_pending(c, dla::ChainPolicy::rebuild(), 1, n, m, k, basis, abasis, fn, shift, h, ldh);
  if (st) return st;
  st = close_pending_block(m, k, c->pending_p.data(), m + k, nullptr, 0, c->pending_applied);       // ([X P] is a finished block: D = I)
  c->pending_applied = 0;
  if (st) {
    // I - (S T)^T (S T) is not positive definite: nothing bounds |T| where the chain ended (round-5 advisor).  The block in memory
    // is intact -- what the chain stored -- so it is finished there: the orthogonalisation runs again on it, without anything left
    // pending, and the operator and the projection are repeated on the finished block (p = [0 ; I]).
    c->pending_k = 0; c->pending_m = 0;
    return expand_project_impl(c, 1, n, m, k, basis, abasis, fn, shift, h, ldh);
  }
  fold_pending_into_projection(m, k, c->pending_p.data(), h, ldh);
  return DLA_OK;
}

int dla_basis_sync(dla_ctx* c, int m, int k, const double* dmat, int ld)
{
  if (!c || (k > 0 && (!dmat || m < 0 || ld < m + k))) return fail(c, DLA_ERR_ARG, "dla_basis_sync: bad argument");
  return engfail(c, c->eng->basis_sync(m, k, dmat, ld));
}

int dla_pending_factor(dla_ctx* c, int k, double* t, int ldt)
{
  if (!c || !t || k <= 0 || ldt < k) return fail(c, DLA_ERR_ARG, "dla_pending_factor: bad argument");
  for (int j = 0; j < k; ++j)
    for (int i = 0; i < k; ++i) t[(size_t)i + (size_t)j * ldt] = (i == j) ? 1.0 : 0.0;
  if (c->pending_k == k) {
    const int l = c->pending_m + k;
    for (int j = 0; j < k; ++j)
      for (int i = 0; i <= j; ++i) t[(size_t)i + (size_t)j * ldt] = c->pending_p[(size_t)(c->pending_m + i) + (size_t)j * l];
  }
  return DLA_OK;
}

int dla_pending_block(dla_ctx* c, int m, int k, double* p, int ldp, int* applied)
{
  if (!c || !p || k <= 0 || m < 0 || ldp < m + k) return fail(c, DLA_ERR_ARG, "dla_pending_block: bad argument");
  for (int j = 0; j < k; ++j)
    for (int i = 0; i < m + k; ++i) p[(size_t)i + (size_t)j * ldp] = (i == m + j) ? 1.0 : 0.0;
  if (applied) *applied = 0;
  if (c->pending_k == k && c->pending_m == m) {
    for (int j = 0; j < k; ++j)
      for (int i = 0; i < m + k; ++i) p[(size_t)i + (size_t)j * ldp] = c->pending_p[(size_t)i + (size_t)j * (m + k)];
    if (applied) *applied = c->pending_applied;
  }
  return DLA_OK;
}

// ---- pending blocks of a basis that grows block by block (Davidson, dla_expand_project mode 4).  The panel holds the blocks as the
// device chains left them; the orthonormal basis is panel * D with D upper triangular: column block i of D is the pending block
// [E_i ; T_i] of block i (the identity where nothing stayed pending).  All matrices are column-major host arrays with leading
// dimension ld; no device work, no context.
//   dla_basis_admit: a block of k columns has come in behind m stored ones with the pending block p ((m + k) x k).  hcols = columns
//   m .. m+k-1 of the caller's projected matrix h hold the RAW product [X | U]_stored^T A U_stored (rows 0 .. m+k-1); they are
//   recorded in hraw (both triangles), p goes into D, and hcols become the columns of D^T hraw D -- the projected matrix of the
//   orthonormal basis.
int dla_basis_admit(int m, int k, double* p, int ldp, int applied, double* hraw, double* dmat, double* h, int ld)
{
  DLA_T("dla_basis_admit");
  if (m < 0 || k <= 0 || !p || !hraw || !dmat || !h || ldp < m + k || ld < m + k) return DLA_ERR_ARG;
  const int l = m + k;
  {
    const int stc = close_pending_block(m, k, p, ldp, dmat, ld, applied);      // the closing pass against X = X_c D, exactly (p in / out)
    if (stc) return stc;
  }
  double* hc = h + (size_t)m * ld;
  for (int j = 0; j < k; ++j) {
    for (int i = 0; i < l; ++i) hraw[(size_t)i + (size_t)(m + j) * ld] = hc[(size_t)i + (size_t)j * ld];
    for (int i = 0; i < m; ++i) hraw[(size_t)(m + j) + (size_t)i * ld] = hc[(size_t)i + (size_t)j * ld];
    for (int i = 0; i < k; ++i)        // (the diagonal block arrives complete; keep it symmetric to the last bit)
      if (i < j) hraw[(size_t)(m + j) + (size_t)(m + i) * ld] = hraw[(size_t)(m + i) + (size_t)(m + j) * ld];
    for (int i = 0; i < l; ++i) dmat[(size_t)i + (size_t)(m + j) * ld] = p[(size_t)i + (size_t)j * ldp];
  }
  // g = hraw(0:l, 0:l) p
  // (four columns of p / g at a time: a column of hraw / of D is loaded once for the four -- the arithmetic of every entry, and its
  //  order, is that of the plain loops; this runs in the Rayleigh-Ritz gap of every iteration while the device waits)
  static thread_local std::vector<double> g;
  g.assign((size_t)l * k, 0.0);
  int j = 0;
  for (; j + 4 <= k; j += 4) {
    double* g0 = &g[(size_t)j * l]; double* g1 = g0 + l; double* g2 = g1 + l; double* g3 = g2 + l;
    for (int q = 0; q < l; ++q) {
      const double p0 = p[(size_t)q + (size_t)j * ldp], p1 = p[(size_t)q + (size_t)(j + 1) * ldp],
                   p2 = p[(size_t)q + (size_t)(j + 2) * ldp], p3 = p[(size_t)q + (size_t)(j + 3) * ldp];
      if (p0 == 0.0 && p1 == 0.0 && p2 == 0.0 && p3 == 0.0) continue;
      const double* hq = hraw + (size_t)q * ld;
      for (int i = 0; i < l; ++i) { const double hv = hq[i]; g0[i] += hv * p0; g1[i] += hv * p1; g2[i] += hv * p2; g3[i] += hv * p3; }
    }
  }
  for (; j < k; ++j) {
    double* gj = &g[(size_t)j * l];
    for (int q = 0; q < l; ++q) {
      const double pq = p[(size_t)q + (size_t)j * ldp];
      if (pq == 0.0) continue;
      const double* hq = hraw + (size_t)q * ld;
      for (int i = 0; i < l; ++i) gj[i] += hq[i] * pq;
    }
  }
  // hcols = D(0:l, 0:l)^T g: row r of the result is column r of D against g
  for (j = 0; j + 4 <= k; j += 4) {
    const double* g0 = &g[(size_t)j * l]; const double* g1 = g0 + l; const double* g2 = g1 + l; const double* g3 = g2 + l;
    for (int r = 0; r < l; ++r) {
      const double* dr = dmat + (size_t)r * ld;
      const int nn = r + 1;
      double s[4][4] = {{0.0}};
      int i = 0;
      for (; i + 4 <= nn; i += 4)
        for (int e = 0; e < 4; ++e) { const double dv = dr[i + e]; s[0][e] += dv * g0[i + e]; s[1][e] += dv * g1[i + e]; s[2][e] += dv * g2[i + e]; s[3][e] += dv * g3[i + e]; }
      for (; i < nn; ++i) { const double dv = dr[i]; s[0][0] += dv * g0[i]; s[1][0] += dv * g1[i]; s[2][0] += dv * g2[i]; s[3][0] += dv * g3[i]; }
      for (int c4 = 0; c4 < 4; ++c4) hc[(size_t)r + (size_t)(j + c4) * ld] = (s[c4][0] + s[c4][1]) + (s[c4][2] + s[c4][3]);
    }
  }
  for (; j < k; ++j) {
    const double* gj = &g[(size_t)j * l];
    for (int r = 0; r < l; ++r) hc[(size_t)r + (size_t)j * ld] = dot4(dmat + (size_t)r * ld, gj, r + 1);
  }
  return DLA_OK;
}

//   dla_basis_fold: c(0:rows, 0:ncol) <- D(0:rows, 0:rows) c -- coefficients for the STORED blocks, before every product with the panel
int dla_basis_fold(int rows, int ncol, const double* dmat, int ld, double* cf, int ldc)
{
  DLA_T("dla_basis_fold");
  if (rows < 0 || ncol < 0 || !dmat || !cf || ld < rows || ldc < rows) return DLA_ERR_ARG;
  std::vector<double> t((size_t)rows);
  for (int j = 0; j < ncol; ++j) {
    double* cj = cf + (size_t)j * ldc;
    std::fill(t.begin(), t.end(), 0.0);
    for (int q = 0; q < rows; ++q) {
      const double cq = cj[q];
      if (cq == 0.0) continue;
      const double* dq = dmat + (size_t)q * ld;
      for (int i = 0; i <= q; ++i) t[i] += dq[i] * cq;
    }
    for (int i = 0; i < rows; ++i) cj[i] = t[i];
  }
  return DLA_OK;
}

static int expand_project_impl(dla_ctx* c, int mode, int n, int m, int k, double* basis, double* abasis, dla_matvec_fn fn,
                               double shift, double* h, int ldh)
{
  double* u = basis + (size_t)n * m;
  const long long nglob = global_rows(c, n);
  const bool builtin = builtin_operator(fn);
  const int order = builtin ? 2 : c->callback_order;
  // The run-ahead may call the operator a second time on the same block (and drop the first result) when the chain takes
  // another route than planned.  The reference calls matvec exactly once per block (diaglib.f90:1685, 394-397), and a
  // caller's operator may count its calls or keep state between them: by default only the library's own operators -- pure
  // functions of their input -- run ahead; DLA_OPT_RUN_AHEAD = 2 is the caller's statement that theirs is pure too.
  const bool ahead = c->run_ahead == 2 || (c->run_ahead == 1 && builtin);
  if (ahead && c->callbacks_on_device && order != 1 && m > 0) {
    dla::OrthoReport rep;
    int st = c->eng->ortho_chain_begin(n, m, k, basis, basis, u, &rep);
    if (st) return engfail(c, st);
    if (rep.handled) {
      // in flight: the operator and the projection follow on the same stream; the projection's wait covers the chain
      c->eng->spec_stats_begin();
      int sta = expand_apply_project(c, mode, n, m, k, basis, abasis, fn, shift, h, ldh);
      c->eng->spec_stats_end(false);
      st = c->eng->ortho_chain_finish(&rep, sta == DLA_OK);
      c->eng->spec_stats_end(!(st == DLA_OK && sta == DLA_OK && rep.status == 1 && rep.clean));
      if (st) return engfail(c, st);
      if (sta) return sta;
      if (rep.status == 1 && rep.clean) {
        if (c->verbose_ortho)
          std::printf("  [dla] ortho_vs_x (device chain): %d outer iterations, %d macro iterations, status %d\n", rep.outer_its,
                      rep.macro_its, rep.status);
        return DLA_OK;
      }
      // the chain took more launches than planned, or stopped: what ran behind it has read an unfinished block
      st = ortho_vs_x_after_chain(c, c->eng, c->row0, nglob, n, m, k, basis, basis, u, &rep);
      if (st) return st;
      if (c->eng->policy.tight() && rep.status != 1) { st = ortho_vs_x_after_chain(c, c->eng, c->row0, nglob, n, m, k, basis, basis, u, nullptr); if (st) return st; }
      return expand_apply_project(c, mode, n, m, k, basis, abasis, fn, shift, h, ldh);
    }
    st = ortho_vs_x_after_chain(c, c->eng, c->row0, nglob, n, m, k, basis, basis, u, nullptr);
    if (st) return st;
    if (c->eng->policy.tight()) { st = ortho_vs_x_after_chain(c, c->eng, c->row0, nglob, n, m, k, basis, basis, u, nullptr); if (st) return st; }
    return expand_apply_project(c, mode, n, m, k, basis, abasis, fn, shift, h, ldh);
  }
  int st = ortho_vs_x_impl(c, c->eng, c->row0, nglob, n, m, k, basis, basis, u);
  if (st) return st;
  if (!c->callbacks_on_device && mode == 0 && shift == 0.0 && k >= 2 && c->eng->gram_chunks_ok(n, m + k, k)) {
    // host-mode callback (the block goes through the caller's routine in column chunks): the projection of a chunk is
    // enqueued behind its upload and runs while the caller's routine works on the next one
    double* au = abasis + (size_t)n * m;
    st = staged_callback(c, n, k, u, au, [&](int mc, const double* hx, double* hy) { fn(&n, &mc, hx, hy); },
                         [&](int c0, int mc) { return engfail(c, c->eng->gram_chunk(n, m + k, basis, k, c0, mc, au + (size_t)c0 * n)); });
    if (st) return st;
    return engfail(c, c->eng->gram_chunks_collect(m + k, k, h, ldh));
  }
  return expand_apply_project(c, mode, n, m, k, basis, abasis, fn, shift, h, ldh);
}

// The same expansion step with a metric B (gen_david_driver, reference diaglib.f90:2170-2190; LOBPCG gen_eig, :523-529 + 394-403):
//   b_ortho_vs_x(X, BX, U) -> BU = B U -> b_ortho(U, BU) -> AU = A U [+ shift U] -> projection.
// With device-mode callbacks that may run ahead (see dla_expand_project) everything is enqueued behind the orthogonalisation
// chain: the k x k factorisation of b_ortho runs on the device and goes on only when the chain in front of it has ended well
// (bortho_tail_kernel), the chain's report and b_ortho's outcome are read at the projection's host wait -- one wait per
// expansion instead of three.  When the chain took another route, everything behind it is repeated on the finished block.
static int metric_tail_steps(dla_ctx* c, int mode, int n, int m, int k, double* basis, double* bbasis, double* abasis, dla_matvec_fn op,
                             dla_matvec_fn metric, double shift, double* h, int ldh, bool ahead, bool behind_chain, int* b_handled)
{
  double* u = basis + (size_t)n * m;
  double* bu = bbasis + (size_t)n * m;
  int st = dla_call_matvec(c, metric, n, k, u, bu);
  if (st) return st;
  *b_handled = 0;
  if (ahead) { st = c->eng->b_ortho_ahead(n, k, u, bu, behind_chain, b_handled); if (st) return engfail(c, st); }
  if (!*b_handled) { st = dla_b_ortho(c, n, k, u, bu); if (st) return st; }
  if (mode == 2) return DLA_OK;            // (no operator, no projection: the linear-response expansion, see below)
  return expand_apply_project(c, mode, n, m, k, basis, abasis, op, shift, h, ldh);
}

int dla_expand_project_metric(dla_ctx* c, int mode, int n, int m, int k, double* basis, double* bbasis, double* abasis, dla_matvec_fn op,
                              dla_matvec_fn metric, double shift, double* h, int ldh)
{
  DLA_T("dla_expand_project_metric");
  // b_ortho_vs_x + b_ortho [+ the projection]
  RefFlops rf(c, c && n > 0 && k > 0 ? ortho_vs_x_flops(n, m, k) + 4.0 * n * (double)k * k + (shift != 0.0 ? 2.0 * n * (double)k : 0.0) +
                                       (mode == 0 ? 2.0 * n * (double)(m + k) * k : mode == 1 ? 2.0 * n * (double)(m + k) * (m + k) : 0.0) : 0.0);
  // mode 2: b_ortho_vs_x -> metric -> b_ortho only (abasis, op, h unused) -- the expansion of caslr_eff_driver, whose blocks are
  // made orthonormal in the metric (A+B) resp. (A-B) right after they have been orthogonalised against the basis (reference
  // diaglib.f90:1417-1424)
  if (!c || !basis || !bbasis || !metric || mode < 0 || mode > 2 || n <= 0 || m < 0 || k <= 0 ||
      (mode != 2 && (!abasis || !h || !op || ldh < m + k)))
    return fail(c, DLA_ERR_ARG, "dla_expand_project_metric: bad argument (n > 0, m >= 0, k > 0, ldh >= m + k)");
  double* u = basis + (size_t)n * m;
  const long long nglob = global_rows(c, n);
  const bool builtin = (mode == 2 || builtin_operator(op)) && builtin_operator(metric);
  const int order = builtin ? 2 : c->callback_order;
  const bool ahead = (c->run_ahead == 2 || (c->run_ahead == 1 && builtin)) && c->callbacks_on_device && order != 1;
  int b_handled = 0;
  dla::PolicyScope drop_guard(c->eng, dla::ChainPolicy::metric_drop());
  if (ahead && m > 0) {
    dla::OrthoReport rep;
    int st = c->eng->ortho_chain_begin(n, m, k, basis, bbasis, u, &rep);
    if (st) return engfail(c, st);
    if (rep.handled) {
      c->eng->spec_stats_begin();
      int sta = metric_tail_steps(c, mode, n, m, k, basis, bbasis, abasis, op, metric, shift, h, ldh, true, true, &b_handled);
      c->eng->spec_stats_end(false);
      // (modes 0 / 1: the projection's host wait has covered the chain; mode 2 has none of its own: the report's wait is the one)
      st = c->eng->ortho_chain_finish(&rep, sta == DLA_OK && mode != 2);
      const int bst = b_handled ? c->eng->b_ortho_ahead_status() : 1;
      const bool good = st == DLA_OK && sta == DLA_OK && rep.status == 1 && rep.clean && bst == 1;
      c->eng->spec_stats_end(!good);
      if (st) return engfail(c, st);
      if (sta) return sta;
      if (rep.status == 1 && rep.clean && bst < 0) return fail(c, DLA_ERR_LAPACK, "b_ortho: metric not positive definite");
      if (good) return DLA_OK;
      // The chain took another route than planned (or stopped).  When it stopped half way the device step of b_ortho did not go on
      // and nothing behind the chain has touched U.  When it ENDED WELL, only later than planned -- continuation launches, enqueued by
      // ortho_chain_finish, completed it -- the b_ortho step that was already in the queue may have seen a finished chain and applied
      // U <- U W, BU <- BU W to a block the operator had already read unfinished (round-4 advisor): U is then B-orthonormal against
      // a stale BU.  Either way everything behind the chain is repeated on the block as it stands: the metric image is formed
      // again, and b_ortho on a block that is already B-orthonormal is a factorisation of the identity.
      st = ortho_vs_x_after_chain(c, c->eng, c->row0, nglob, n, m, k, basis, bbasis, u, &rep);
      if (st) return st;
      return metric_tail_steps(c, mode, n, m, k, basis, bbasis, abasis, op, metric, shift, h, ldh, false, false, &b_handled);
    }
    st = ortho_vs_x_after_chain(c, c->eng, c->row0, nglob, n, m, k, basis, bbasis, u, nullptr);
    if (st) return st;
  } else {
    int st = ortho_vs_x_impl(c, c->eng, c->row0, nglob, n, m, k, basis, bbasis, u);
    if (st) return st;
  }
  // one call after the other; the factorisation of b_ortho still runs on the device when the callbacks allow it (its outcome is
  // read at the projection's wait)
  int st = metric_tail_steps(c, mode, n, m, k, basis, bbasis, abasis, op, metric, shift, h, ldh, ahead, false, &b_handled);
  if (st) return st;
  if (b_handled) {
    if (mode == 2) { st = c->eng->sync(); if (st) return engfail(c, st); }      // (no projection whose wait would cover the device step)
    const int bst = c->eng->b_ortho_ahead_status();
    if (bst < 0) return fail(c, DLA_ERR_LAPACK, "b_ortho: metric not positive definite");
    if (bst == 0) return fail(c, DLA_ERR_RUNTIME, "b_ortho: the device step did not run");
  }
  return DLA_OK;
}

int dla_call_precnd(dla_ctx* c, dla_precnd_fn fn, int n, int m, double fac, const double* x, double* px)
{
  DLA_T("dla_call_precnd");
  if (m <= 0) return DLA_OK;
  if (c->callbacks_on_device) {
    const int order = callback_order_of(c, (void*)fn);
    int st = c->eng->callback_begin(order);
    if (st) return engfail(c, st);
    fn(&n, &m, &fac, x, px);
    if (int cbs = callback_status(c)) { (void)c->eng->callback_end(order); return cbs; }
    return engfail(c, c->eng->callback_end(order));
  }
  const int sts = staged_callback(c, n, m, x, px, [&](int mc, const double* hx, double* hy) { fn(&n, &mc, &fac, hx, hy); });
  if (int cbs = callback_status(c)) return cbs;
  return sts;
}

// linear-response preconditioner lrprec(n,m,fac,xp,xm,yp,ym) (reference diaglib.f90:1317, caller main.f90:257-281):
// two inputs, two outputs, one scalar by reference
int dla_call_lrprec(dla_ctx* c, dla_lrprec_fn fn, int n, int m, double fac, const double* xp, const double* xm,
                    double* yp, double* ym)
{
  DLA_T("dla_call_lrprec");
  if (m <= 0) return DLA_OK;
  if (c->callbacks_on_device) {
    const int order = callback_order_of(c, (void*)fn);
    int st = c->eng->callback_begin(order);
    if (st) return engfail(c, st);
    fn(&n, &m, &fac, xp, xm, yp, ym);
    if (int cbs = callback_status(c)) { (void)c->eng->callback_end(order); return cbs; }
    return engfail(c, c->eng->callback_end(order));
  }
  const size_t bytes = sizeof(double) * (size_t)n * m;
  int st = ensure_stage(c, 2 * bytes);
  if (st) return st;
  double* hx = c->stage_x;
  double* hy = c->stage_y;
  st = c->eng->d2h(hx, xp, bytes);
  if (!st) st = c->eng->d2h(hx + (size_t)n * m, xm, bytes);
  if (st) return engfail(c, st);
  fn(&n, &m, &fac, hx, hx + (size_t)n * m, hy, hy + (size_t)n * m);
  if (int cbs = callback_status(c)) return cbs;
  st = c->eng->h2d(yp, hy, bytes);
  if (!st) st = c->eng->h2d(ym, hy + (size_t)n * m, bytes);
  return engfail(c, st);
}

// ------------------------------------------------------------------ solve report
static thread_local int g_info[3] = {0, 0, 0};     // report of the calling thread's last driver call
void dla_set_solve_info(int iters, int matvec_cols, int restarts) { g_info[0] = iters; g_info[1] = matvec_cols; g_info[2] = restarts; }
void dla_last_solve_info(int* iters, int* matvec_cols, int* restarts)
{
  if (iters) *iters = g_info[0];
  if (matvec_cols) *matvec_cols = g_info[1];
  if (restarts) *restarts = g_info[2];
}

// ------------------------------------------------------------------ built-in operator
int dla_synth_setup(dla_ctx* c, long long n_global, long long row0, int n_local, int rank_w, double sigma)
{
  if (!c) return DLA_ERR_ARG;
  g_synth_ctx = c;
  return engfail(c, c->eng->synth_setup(n_global, row0, n_local, rank_w, sigma));
}

void dla_synth_matvec(const int* n, const int* m, const double* x, double* ax)
{
  dla_ctx* c = g_synth_ctx;
  if (!c) { callback_failed(DLA_ERR_ARG, "dla_synth_matvec before dla_synth_setup"); return; }
  if (int st = c->eng->synth_matvec(*n, *m, x, ax)) callback_failed(st, "synth_matvec failed: " + c->eng->err);
}

void dla_synth_precnd(const int* n, const int* m, const double* fac, const double* x, double* px)
{
  dla_ctx* c = g_synth_ctx;
  if (!c) { callback_failed(DLA_ERR_ARG, "dla_synth_precnd before dla_synth_setup"); return; }
  if (int st = c->eng->synth_precnd(*n, *m, *fac, x, px)) callback_failed(st, "synth_precnd failed: " + c->eng->err);
}

// sample operators of the linear-response / generalised drivers (hip_engine.hip SynthKind), reference callback shapes
static void synth_kind(int kind, const char* what, const int* n, const int* m, const double* x, double* y)
{
  dla_ctx* c = g_synth_ctx;
  if (!c) { callback_failed(DLA_ERR_ARG, std::string(what) + " before dla_synth_setup"); return; }
  if (int st = c->eng->synth_apply(kind, *n, *m, x, y)) callback_failed(st, std::string(what) + " failed: " + c->eng->err);
}
void dla_synth_apbmul(const int* n, const int* m, const double* x, double* y) { synth_kind(1, "dla_synth_apbmul", n, m, x, y); }
void dla_synth_ambmul(const int* n, const int* m, const double* x, double* y) { synth_kind(2, "dla_synth_ambmul", n, m, x, y); }
void dla_synth_spdmul(const int* n, const int* m, const double* x, double* y) { synth_kind(3, "dla_synth_spdmul", n, m, x, y); }
void dla_synth_smdmul(const int* n, const int* m, const double* x, double* y) { synth_kind(4, "dla_synth_smdmul", n, m, x, y); }
void dla_synth_metric(const int* n, const int* m, const double* x, double* y) { synth_kind(5, "dla_synth_metric", n, m, x, y); }
static void synth_lrp(int variant, const int* n, const int* m, const double* fac, const double* xp, const double* xm, double* yp, double* ym)
{
  dla_ctx* c = g_synth_ctx;
  if (!c) { callback_failed(DLA_ERR_ARG, "dla_synth_lrprec before dla_synth_setup"); return; }
  if (int st = c->eng->synth_lrprec(variant, *n, *m, *fac, xp, xm, yp, ym)) callback_failed(st, "synth_lrprec failed: " + c->eng->err);
}
void dla_synth_lrprec1(const int* n, const int* m, const double* fac, const double* xp, const double* xm, double* yp, double* ym) { synth_lrp(1, n, m, fac, xp, xm, yp, ym); }
void dla_synth_lrprec2(const int* n, const int* m, const double* fac, const double* xp, const double* xm, double* yp, double* ym) { synth_lrp(2, n, m, fac, xp, xm, yp, ym); }

// ------------------------------------------------------------------ the stored sparse matrices (dla_internal.h, SpmmSlot)
// Every entry below is one of six calls on a slot (set-up, refresh, info, drop, product, preconditioner).  What differs between the entries besides the slot:
//   * which context the thread's callbacks act on (g_spmm_ctx): a set-up of A binds its context before the engine is asked, so also
//     when the set-up is refused; a set-up of B or of a part binds it once the set-up is accepted; info, refresh and drop never do;
//   * the text a callback fails with (the SpmmCallback rows).
using dla::SPMM_A; using dla::SPMM_B; using dla::SPMM_APB; using dla::SPMM_SMD;
static int spmm_set_up(dla_ctx* c, int slot, int via, int n, const long long* rowptr, const int* colind, const double* values, int format)
{
  if (!c) return DLA_ERR_ARG;
  if (slot == SPMM_A) g_spmm_ctx = c;
  const int st = engfail(c, c->eng->spmm_setup(slot, via, n, rowptr, colind, values, format));
  if (st == DLA_OK) g_spmm_ctx = c;
  return st;
}
static int spmm_refresh(dla_ctx* c, int slot, int n, const long long* rowptr_dev, const int* colind_dev, const double* values_dev)
{
  if (!c) return DLA_ERR_ARG;
  return engfail(c, c->eng->spmm_refresh_dev(slot, n, rowptr_dev, colind_dev, values_dev));
}
static int spmm_slot_info(dla_ctx* c, int slot, struct dla_spmm_info* out)
{
  if (!c || !out) return DLA_ERR_ARG;
  return engfail(c, c->eng->spmm_info(slot, out));
}
static int spmm_slot_drop(dla_ctx* c, int first, int last)
{
  if (!c) return DLA_ERR_ARG;
  return engfail(c, c->eng->spmm_drop(first, last));
}
// the callbacks: what each says before any set-up has bound a context, and in front of the engine's refusal
struct SpmmCallback { const char *unbound, *failed; };
static const SpmmCallback spmm_mul_words[dla::SPMM_SLOTS] = {
  {"dla_spmm_matvec before dla_spmm_setup_csr", "spmm_matvec failed: "},
  {"dla_spmm_bvec before dla_spmm_setup_metric_csr", "dla_spmm_bvec failed: "},
  {"dla_spmm_apbmul before dla_spmm_setup_lr_csr", "dla_spmm_apbmul failed: "},
  {"dla_spmm_ambmul before dla_spmm_setup_lr_csr", "dla_spmm_ambmul failed: "},
  {"dla_spmm_spdmul before dla_spmm_setup_lr_csr", "dla_spmm_spdmul failed: "},
  {"dla_spmm_smdmul before dla_spmm_setup_lr_csr", "dla_spmm_smdmul failed: "}};
static void spmm_product(int slot, const int* n, const int* m, const double* x, double* y)
{
  dla_ctx* c = g_spmm_ctx;
  if (!c) { callback_failed(DLA_ERR_ARG, spmm_mul_words[slot].unbound); return; }
  if (int st = c->eng->spmm_mul(slot, *n, *m, x, y)) callback_failed(st, spmm_mul_words[slot].failed + c->eng->err);
}
// kind 0: dla_spmm_precnd, 1: dla_spmm_precnd_pencil, 2 / 3: dla_spmm_lrprec1 / 2 (xm, ym: the second pair of the latter two)
static void spmm_precondition(int kind, const int* n, const int* m, const double* fac, const double* x, const double* xm, double* y, double* ym)
{
  static const SpmmCallback words[4] = {
    {"dla_spmm_precnd before dla_spmm_setup_csr", "spmm_precnd failed: "},
    {"dla_spmm_precnd_pencil before dla_spmm_setup_csr and dla_spmm_setup_metric_csr", "dla_spmm_precnd_pencil failed: "},
    {"dla_spmm_lrprec1 before dla_spmm_setup_lr_csr", "dla_spmm_lrprec1 failed: "},
    {"dla_spmm_lrprec2 before dla_spmm_setup_lr_csr", "dla_spmm_lrprec2 failed: "}};
  dla_ctx* c = g_spmm_ctx;
  if (!c) { callback_failed(DLA_ERR_ARG, words[kind].unbound); return; }
  const int st = kind == 0 ? c->eng->spmm_precnd(*n, *m, *fac, x, y) : kind == 1 ? c->eng->spmm_precnd_pencil(*n, *m, *fac, x, y)
                                                                     : c->eng->spmm_lrprec(kind - 1, *n, *m, *fac, x, xm, y, ym);
  if (st) callback_failed(st, words[kind].failed + c->eng->err);
}

// ---- the operator A (single rank in a storage format, or on a row shard) ...
int dla_spmm_setup_csr(dla_ctx* c, int n, const long long* rowptr, const int* colind, const double* values) { return spmm_set_up(c, SPMM_A, dla::SPMM_VIA_PLAIN, n, rowptr, colind, values, DLA_SPMM_ELL); }
int dla_spmm_setup_csr_fmt(dla_ctx* c, int n, const long long* rowptr, const int* colind, const double* values, int format) { return spmm_set_up(c, SPMM_A, dla::SPMM_VIA_HOST, n, rowptr, colind, values, format); }
int dla_spmm_info(dla_ctx* c, struct dla_spmm_info* out) { return spmm_slot_info(c, SPMM_A, out); }
int dla_spmm_setup_csr_sharded(dla_ctx* c, int n_local, long long row0, long long n_global, const long long* rowptr,
                               const long long* colind, const double* values)
{
  DLA_T("dla_spmm_setup_csr_sharded");
  if (!c) return DLA_ERR_ARG;
  g_spmm_ctx = c;
  return engfail(c, c->eng->spmm_setup_csr_sharded(n_local, row0, n_global, rowptr, colind, values));
}
void dla_spmm_matvec(const int* n, const int* m, const double* x, double* ax) { spmm_product(SPMM_A, n, m, x, ax); }
void dla_spmm_precnd(const int* n, const int* m, const double* fac, const double* x, double* px) { spmm_precondition(0, n, m, fac, x, nullptr, px, nullptr); }
// ... and its transposed index: y = A^T x from the stored values of A (the engine drops the index with every accepted set-up of A)
int dla_spmm_transpose_prepare(dla_ctx* c, int format)
{
  DLA_T("dla_spmm_transpose_prepare");
  if (!c) return DLA_ERR_ARG;
  return engfail(c, c->eng->spmm_transpose_prepare(format));
}
int dla_spmm_transpose_info(dla_ctx* c, struct dla_spmm_info* out)
{
  if (!c || !out) return DLA_ERR_ARG;
  return engfail(c, c->eng->spmm_transpose_info(out));
}
int dla_spmm_drop_transpose(dla_ctx* c)
{
  if (!c) return DLA_ERR_ARG;
  return engfail(c, c->eng->spmm_transpose_drop());
}
void dla_spmm_matvec_t(const int* n, const int* m, const double* x, double* y)
{
  dla_ctx* c = g_spmm_ctx;
  if (!c) { callback_failed(DLA_ERR_ARG, "dla_spmm_matvec_t before dla_spmm_setup_csr: no operator has been set up"); return; }
  if (int st = c->eng->spmm_mul_t(*n, *m, x, y)) callback_failed(st, "dla_spmm_matvec_t failed: " + c->eng->err);
}
// ... and the Chebyshev polynomial of A + fac I as its preconditioner.  The configuration is the context's and binds nothing: like
// info, refresh and drop it leaves the thread's callbacks on the context they act on.
int dla_spmm_cheb_config(dla_ctx* c, int steps, double lo_fraction)
{
  if (!c) return DLA_ERR_ARG;
  return engfail(c, c->eng->spmm_cheb_config(steps, lo_fraction));
}
int dla_spmm_cheb_info(dla_ctx* c, struct dla_spmm_cheb_info* out)
{
  if (!c || !out) return DLA_ERR_ARG;
  return engfail(c, c->eng->spmm_cheb_info(out));
}
void dla_spmm_precnd_cheb(const int* n, const int* m, const double* fac, const double* x, double* px)
{
  dla_ctx* c = g_spmm_ctx;
  if (!c) { callback_failed(DLA_ERR_ARG, "dla_spmm_precnd_cheb before dla_spmm_setup_csr: no operator has been set up"); return; }
  if (int st = c->eng->spmm_precnd_cheb(*n, *m, *fac, x, px)) callback_failed(st, "dla_spmm_precnd_cheb failed: " + c->eng->err);
}
// ... on the diagonally scaled operator, under the same configuration
int dla_spmm_cheb_jacobi_upper(dla_ctx* c, double fac, double* hi)
{
  if (!c || !hi) return DLA_ERR_ARG;
  return engfail(c, c->eng->spmm_cheb_jacobi_upper(fac, hi));
}
void dla_spmm_precnd_cheb_jacobi(const int* n, const int* m, const double* fac, const double* x, double* px)
{
  dla_ctx* c = g_spmm_ctx;
  if (!c) { callback_failed(DLA_ERR_ARG, "dla_spmm_precnd_cheb_jacobi before dla_spmm_setup_csr: no operator has been set up"); return; }
  if (int st = c->eng->spmm_precnd_cheb_jacobi(*n, *m, *fac, x, px)) callback_failed(st, "dla_spmm_precnd_cheb_jacobi failed: " + c->eng->err);
}
// ... and on the scaled pencil A + fac B with the stored metric
int dla_spmm_cheb_pencil_upper(dla_ctx* c, double fac, double* hi)
{
  if (!c || !hi) return DLA_ERR_ARG;
  return engfail(c, c->eng->spmm_cheb_pencil_upper(fac, hi));
}
void dla_spmm_precnd_cheb_pencil(const int* n, const int* m, const double* fac, const double* x, double* px)
{
  dla_ctx* c = g_spmm_ctx;
  if (!c) { callback_failed(DLA_ERR_ARG, "dla_spmm_precnd_cheb_pencil before dla_spmm_setup_csr: no operator has been set up"); return; }
  if (int st = c->eng->spmm_precnd_cheb_pencil(*n, *m, *fac, x, px)) callback_failed(st, "dla_spmm_precnd_cheb_pencil failed: " + c->eng->err);
}

// ---- ... the metric of a generalised problem beside it (bvec of reference diaglib.f90:1855; the harness' smult, main.f90:115-144) ...
int dla_spmm_setup_metric_csr(dla_ctx* c, int n, const long long* rowptr, const int* colind, const double* values, int format) { return spmm_set_up(c, SPMM_B, dla::SPMM_VIA_HOST, n, rowptr, colind, values, format); }
int dla_spmm_metric_info(dla_ctx* c, struct dla_spmm_info* out) { return spmm_slot_info(c, SPMM_B, out); }
int dla_spmm_drop_metric(dla_ctx* c) { return spmm_slot_drop(c, SPMM_B, SPMM_B); }
void dla_spmm_bvec(const int* n, const int* m, const double* x, double* bx) { spmm_product(SPMM_B, n, m, x, bx); }
void dla_spmm_precnd_pencil(const int* n, const int* m, const double* fac, const double* x, double* px) { spmm_precondition(1, n, m, fac, x, nullptr, px, nullptr); }

// ---- ... either of the two from CSR arrays in device memory, and new values for a stored pattern ...
int dla_spmm_setup_csr_dev(dla_ctx* c, int which, int n, const long long* rowptr_dev, const int* colind_dev, const double* values_dev, int format)
{
  DLA_T("dla_spmm_setup_csr_dev");
  return spmm_set_up(c, dla::spmm_slot_of_which(which), dla::SPMM_VIA_DEVICE, n, rowptr_dev, colind_dev, values_dev, format);
}
int dla_spmm_refresh_values_dev(dla_ctx* c, int which, int n, const long long* rowptr_dev, const int* colind_dev, const double* values_dev)
{
  DLA_T("dla_spmm_refresh_values_dev");
  return spmm_refresh(c, dla::spmm_slot_of_which(which), n, rowptr_dev, colind_dev, values_dev);
}

// ---- ... and the four parts of a linear-response pencil (apbmul / ambmul / spdmul / smdmul of reference diaglib.f90:1024-1025,
// lrprec of :1317; the harness' lrprec_1 / lrprec_2, main.f90:234-281)
int dla_spmm_setup_lr_csr(dla_ctx* c, int part, int n, const long long* rowptr, const int* colind, const double* values, int format) { return spmm_set_up(c, dla::spmm_slot_of_part(part), dla::SPMM_VIA_HOST, n, rowptr, colind, values, format); }
int dla_spmm_setup_lr_csr_dev(dla_ctx* c, int part, int n, const long long* rowptr_dev, const int* colind_dev, const double* values_dev, int format)
{
  DLA_T("dla_spmm_setup_lr_csr_dev");
  return spmm_set_up(c, dla::spmm_slot_of_part(part), dla::SPMM_VIA_DEVICE, n, rowptr_dev, colind_dev, values_dev, format);
}
int dla_spmm_refresh_lr_values_dev(dla_ctx* c, int part, int n, const long long* rowptr_dev, const int* colind_dev, const double* values_dev)
{
  DLA_T("dla_spmm_refresh_lr_values_dev");
  return spmm_refresh(c, dla::spmm_slot_of_part(part), n, rowptr_dev, colind_dev, values_dev);
}
int dla_spmm_lr_info(dla_ctx* c, int part, struct dla_spmm_info* out) { return spmm_slot_info(c, dla::spmm_slot_of_part(part), out); }
int dla_spmm_drop_lr(dla_ctx* c) { return spmm_slot_drop(c, SPMM_APB, SPMM_SMD); }
void dla_spmm_apbmul(const int* n, const int* m, const double* x, double* y) { spmm_product(dla::SPMM_APB, n, m, x, y); }
void dla_spmm_ambmul(const int* n, const int* m, const double* x, double* y) { spmm_product(dla::SPMM_AMB, n, m, x, y); }
void dla_spmm_spdmul(const int* n, const int* m, const double* x, double* y) { spmm_product(dla::SPMM_SPD, n, m, x, y); }
void dla_spmm_smdmul(const int* n, const int* m, const double* x, double* y) { spmm_product(dla::SPMM_SMD, n, m, x, y); }
void dla_spmm_lrprec1(const int* n, const int* m, const double* fac, const double* xp, const double* xm, double* yp, double* ym) { spmm_precondition(2, n, m, fac, xp, xm, yp, ym); }
void dla_spmm_lrprec2(const int* n, const int* m, const double* fac, const double* xp, const double* xm, double* yp, double* ym) { spmm_precondition(3, n, m, fac, xp, xm, yp, ym); }

// ------------------------------------------------------------------ the stored dense matrices (include/diaglib_amd.h, dla_dense_setup
// and dla_dense_setup_lr): the operator A, the metric B and the four parts of the linear-response pencil, six slots (dla::DenseSlot)
// reached like the sparse ones above.  An accepted set-up -- of a slot or of a pair -- binds its context to the calling thread's dense
// callbacks (g_dense_ctx); info and drop never do.  dla_dense_info and dla_dense_lr_info pass a null `out` on: the engine words it.
using dla::DENSE_A; using dla::DENSE_B; using dla::DENSE_APB; using dla::DENSE_SMD;
static int dense_set_up(dla_ctx* c, int st)
{
  st = engfail(c, st);
  if (st == DLA_OK) g_dense_ctx = c;
  return st;
}
static int dense_slot_info(dla_ctx* c, int slot, struct dla_dense_info* out)
{
  if (!c) return DLA_ERR_ARG;
  return engfail(c, c->eng->dense_info(slot, out));
}
static int dense_slot_drop(dla_ctx* c, int first, int last)
{
  if (!c) return DLA_ERR_ARG;
  return engfail(c, c->eng->dense_drop(first, last));
}
static const SpmmCallback dense_mul_words[dla::DENSE_SLOTS] = {
  {"dla_dense_matvec before dla_dense_setup: no dense operator has been set up", "dla_dense_matvec failed: "},
  {"dla_dense_bvec before dla_dense_setup: no dense metric has been set up", "dla_dense_bvec failed: "},
  {"dla_dense_apbmul before dla_dense_setup_lr: no dense part apb (A+B) has been set up", "dla_dense_apbmul failed: "},
  {"dla_dense_ambmul before dla_dense_setup_lr: no dense part amb (A-B) has been set up", "dla_dense_ambmul failed: "},
  {"dla_dense_spdmul before dla_dense_setup_lr: no dense part spd (S+D) has been set up", "dla_dense_spdmul failed: "},
  {"dla_dense_smdmul before dla_dense_setup_lr: no dense part smd (S-D) has been set up", "dla_dense_smdmul failed: "}};
static void dense_product(int slot, const int* n, const int* m, const double* x, double* y)
{
  dla_ctx* c = g_dense_ctx;
  if (!c) { callback_failed(DLA_ERR_ARG, dense_mul_words[slot].unbound); return; }
  if (int st = c->eng->dense_mul(slot, *n, *m, x, y)) callback_failed(st, dense_mul_words[slot].failed + c->eng->err);
}
// kind 0: dla_dense_precnd, 1: dla_dense_precnd_pencil, 2 / 3: dla_dense_lrprec1 / 2 (xm, ym: the second pair of the latter two)
static void dense_precondition(int kind, const int* n, const int* m, const double* fac, const double* x, const double* xm, double* y, double* ym)
{
  static const SpmmCallback words[4] = {
    {"dla_dense_precnd before dla_dense_setup: no dense operator has been set up", "dla_dense_precnd failed: "},
    {"dla_dense_precnd_pencil before dla_dense_setup: no dense operator has been set up", "dla_dense_precnd_pencil failed: "},
    {"dla_dense_lrprec1 before dla_dense_setup_lr: no dense part has been set up", "dla_dense_lrprec1 failed: "},
    {"dla_dense_lrprec2 before dla_dense_setup_lr: no dense part has been set up", "dla_dense_lrprec2 failed: "}};
  dla_ctx* c = g_dense_ctx;
  if (!c) { callback_failed(DLA_ERR_ARG, words[kind].unbound); return; }
  const int st = kind < 2 ? c->eng->dense_precnd(kind == 1, *n, *m, *fac, x, y) : c->eng->dense_lrprec(kind - 1, *n, *m, *fac, x, xm, y, ym);
  if (st) callback_failed(st, words[kind].failed + c->eng->err);
}

// ---- the operator A and the metric B ...
int dla_dense_setup(dla_ctx* c, int which, int n, const double* a_host, int lda)
{
  DLA_T("dla_dense_setup");
  return c ? dense_set_up(c, c->eng->dense_setup(dla::dense_slot_of_which(which), dla::SPMM_VIA_HOST, n, a_host, lda)) : DLA_ERR_ARG;
}
int dla_dense_setup_dev(dla_ctx* c, int which, int n, const double* a_dev, int lda)
{
  DLA_T("dla_dense_setup_dev");
  return c ? dense_set_up(c, c->eng->dense_setup(dla::dense_slot_of_which(which), dla::SPMM_VIA_DEVICE, n, a_dev, lda)) : DLA_ERR_ARG;
}
int dla_dense_setup_sym(dla_ctx* c, int which, int n, const double* a_host, int lda, char uplo)
{
  DLA_T("dla_dense_setup_sym");
  return c ? dense_set_up(c, c->eng->dense_setup_sym(dla::dense_slot_of_which(which), dla::SPMM_VIA_HOST, n, a_host, lda, uplo)) : DLA_ERR_ARG;
}
int dla_dense_setup_sym_dev(dla_ctx* c, int which, int n, const double* a_dev, int lda, char uplo)
{
  DLA_T("dla_dense_setup_sym_dev");
  return c ? dense_set_up(c, c->eng->dense_setup_sym(dla::dense_slot_of_which(which), dla::SPMM_VIA_DEVICE, n, a_dev, lda, uplo)) : DLA_ERR_ARG;
}
int dla_dense_sym_info(dla_ctx* c, int which, struct dla_dense_sym_info* out)
{
  if (!c) return DLA_ERR_ARG;
  return engfail(c, c->eng->dense_sym_info(dla::dense_slot_of_which(which), out));
}
int dla_dense_info(dla_ctx* c, int which, struct dla_dense_info* out) { return dense_slot_info(c, dla::dense_slot_of_which(which), out); }
int dla_dense_drop(dla_ctx* c, int which) { const int slot = dla::dense_slot_of_which(which); return dense_slot_drop(c, slot, slot); }
void dla_dense_matvec(const int* n, const int* m, const double* x, double* ax) { dense_product(DENSE_A, n, m, x, ax); }
void dla_dense_bvec(const int* n, const int* m, const double* x, double* bx) { dense_product(DENSE_B, n, m, x, bx); }
void dla_dense_matvec_t(const int* n, const int* m, const double* x, double* y)
{
  dla_ctx* c = g_dense_ctx;
  if (!c) { callback_failed(DLA_ERR_ARG, "dla_dense_matvec_t before dla_dense_setup: no dense operator has been set up"); return; }
  if (int st = c->eng->dense_mul_t(*n, *m, x, y)) callback_failed(st, "dla_dense_matvec_t failed: " + c->eng->err);
}
void dla_dense_precnd(const int* n, const int* m, const double* fac, const double* x, double* px) { dense_precondition(0, n, m, fac, x, nullptr, px, nullptr); }
void dla_dense_precnd_pencil(const int* n, const int* m, const double* fac, const double* x, double* px) { dense_precondition(1, n, m, fac, x, nullptr, px, nullptr); }

// ---- ... and the four parts of a linear-response pencil, one at a time or two from a pair
int dla_dense_setup_lr(dla_ctx* c, int part, int n, const double* a_host, int lda)
{
  DLA_T("dla_dense_setup_lr");
  return c ? dense_set_up(c, c->eng->dense_setup(dla::dense_slot_of_part(part), dla::SPMM_VIA_HOST, n, a_host, lda)) : DLA_ERR_ARG;
}
int dla_dense_setup_lr_dev(dla_ctx* c, int part, int n, const double* a_dev, int lda)
{
  DLA_T("dla_dense_setup_lr_dev");
  return c ? dense_set_up(c, c->eng->dense_setup(dla::dense_slot_of_part(part), dla::SPMM_VIA_DEVICE, n, a_dev, lda)) : DLA_ERR_ARG;
}
int dla_dense_setup_lr_pair(dla_ctx* c, int pair, int n, const double* p_host, int ldp, const double* q_host, int ldq)
{
  DLA_T("dla_dense_setup_lr_pair");
  return c ? dense_set_up(c, c->eng->dense_setup_pair(pair, dla::SPMM_VIA_HOST, n, p_host, ldp, q_host, ldq)) : DLA_ERR_ARG;
}
int dla_dense_setup_lr_pair_dev(dla_ctx* c, int pair, int n, const double* p_dev, int ldp, const double* q_dev, int ldq)
{
  DLA_T("dla_dense_setup_lr_pair_dev");
  return c ? dense_set_up(c, c->eng->dense_setup_pair(pair, dla::SPMM_VIA_DEVICE, n, p_dev, ldp, q_dev, ldq)) : DLA_ERR_ARG;
}
int dla_dense_lr_info(dla_ctx* c, int part, struct dla_dense_info* out) { return dense_slot_info(c, dla::dense_slot_of_part(part), out); }
int dla_dense_drop_lr(dla_ctx* c) { return dense_slot_drop(c, DENSE_APB, DENSE_SMD); }
void dla_dense_apbmul(const int* n, const int* m, const double* x, double* y) { dense_product(dla::DENSE_APB, n, m, x, y); }
void dla_dense_ambmul(const int* n, const int* m, const double* x, double* y) { dense_product(dla::DENSE_AMB, n, m, x, y); }
void dla_dense_spdmul(const int* n, const int* m, const double* x, double* y) { dense_product(dla::DENSE_SPD, n, m, x, y); }
void dla_dense_smdmul(const int* n, const int* m, const double* x, double* y) { dense_product(dla::DENSE_SMD, n, m, x, y); }
void dla_dense_lrprec1(const int* n, const int* m, const double* fac, const double* xp, const double* xm, double* yp, double* ym) { dense_precondition(2, n, m, fac, xp, xm, yp, ym); }
void dla_dense_lrprec2(const int* n, const int* m, const double* fac, const double* xp, const double* xm, double* yp, double* ym) { dense_precondition(3, n, m, fac, xp, xm, yp, ym); }

}  // extern "C"
