// diaglib_amd/csrc/dla_internal.h -- internal seam between the host logic (host_logic.cpp:
// ortho_cd / ortho_vs_x control flow, callback trampolines, statistics) and the device
// engine (hip_engine.hip: HIP kernels, streams, RCCL).  The product library links exactly
// one engine, the HIP one; there is no CPU engine in the product.
#pragma once
#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>
#include "../../include/diaglib_amd.h"

namespace dla {

// Outcome of a device-driven orthogonalisation (Engine::ortho_chain)
struct OrthoReport {
  int handled = 0;      // 0: the engine does not take this shape / mode, run the host-driven loop
  int status = 0;       // 1 done, 2 ortho_cd ran out of iterations, 3 factorisation failed after level shifting,
                        // 4 ortho_vs_x ran out of iterations
  int outer_its = 0, macro_its = 0, shifts = 0;
  double growth = 1.0;
  int clean = 1;        // ortho_chain_finish: 1 when the launches enqueued by ortho_chain_begin were the whole chain
};

// What the caller of an orthogonalisation wants from the chain.  One value, held in BlockOps::policy and installed for the length of
// a call by PolicyScope below; one named constructor per treatment that exists.
struct ChainPolicy {
  // set by a caller that B-orthonormalises the block by Cholesky-QR right behind ortho_vs_x (dla_expand_project_metric): a device
  // chain may then end without applying its last pending triangular factor (OrthoTailArgs::drop_final in hip_engine.hip)
  bool drop_final = false;
  // ... and with publish_pending the chain hands what it left undone to the host instead (BlockOps::pending_block): for a caller that
  // folds it into its small matrices and coefficient blocks (dla_expand_project modes 3 and 4)
  bool publish_pending = false;
  // basis_exact (dla_expand_project mode 5): the stored columns X are not a finished basis but X D is, with the caller's upper-
  // triangular D kept on the device block by block (BlockOps::basis_sync).  Device chains then project with X (D D^T) X^T, and a block
  // may stay pending however far the stored columns are from orthonormal.
  bool basis_exact = false;
  // the device-driven chain must not take the next calls: the host-driven loop runs (dla_expand_project mode 5 on a shape the device
  // cannot project exactly, mode 6)
  bool chain_off = false;
  double drop_tol = 0.0;      // > 0: the block stays pending only when the closing pass found max |U^T U - I| below it
  double drop_stol = 1.0e-4;  // ... and max |X^T U| of the stored block below this (three-pass schedule)

  // the intents the engine and the host-driven loop ask about:
  // the caller takes the closing block on its small matrices without a bound on the factor (mode 3, exact mode 5)
  bool rebuilt() const { return drop_final && publish_pending && drop_tol <= 0.0; }
  // what the chain leaves undone goes to pending_block
  bool publishes() const { return drop_final && publish_pending; }
  // the block stays in a basis that is orthonormal to drop_tol per block only (mode 4)
  bool tight() const { return drop_final && drop_tol > 0.0; }

  // default: the chain applies everything to the block in memory
  static ChainPolicy finish() { return ChainPolicy(); }
  // dla_expand_project_metric: b_ortho follows b_ortho_vs_x at once (reference :2170 / :2185, :523-529): its Cholesky-QR gives the same
  // block whether the chain's last pending factor -- upper triangular, positive diagonal -- has been applied or not, so the chain may
  // end without the sweep U <- U W (the host-driven loop has nothing pending and is not affected)
  static ChainPolicy metric_drop() { ChainPolicy p; p.drop_final = true; return p; }
  // mode 3 = mode 1 for a block that is used once and rebuilt (LOBPCG's W, reference diaglib.f90:518-529, 394-403): what the chain
  // left undone -- its last triangular factor T (near the identity) and, with the three-pass schedule, the closing projection E --
  // is not applied to the block; the projection of the stored blocks is corrected on the host, H <- D^T H D with D = [I E ; 0 T], and
  // the caller folds D into every coefficient block it multiplies the panel with (dla_pending_block): the closing sweeps are never run
  static ChainPolicy rebuild() { ChainPolicy p; p.drop_final = true; p.publish_pending = true; return p; }
  // mode 4 = mode 0 for a block that STAYS in the basis (Davidson, reference diaglib.f90:1790 + 1685 + 1691): what the chain
  // left undone stays pending only when the closing pass found the block orthonormal to 1e-8 -- later blocks are projected
  // against the stored block as if it were orthonormal, twice, the second time on a measured product.  h_host comes back RAW,
  // for the stored block: the caller keeps the pending blocks of its whole basis (an upper-triangular D, dla_basis_admit) and
  // multiplies the rows of its coefficient blocks by D before any product with the panel (dla_basis_fold)
  // (1e-8 / 1e-9: a later block's first projection against the stored columns leaves that share of what it removes, and the block
  //  that comes out of it can be as ill-conditioned as 1e7 -- the leftover must stay below its smallest directions)
  // exact: mode 5 = mode 4 with the caller's pending blocks kept on the device as well (dla_basis_sync after every block): the chain's
  // projections are exact against the FINISHED basis X D, so what a block leaves pending is bounded only by what keeps the host
  // algebra well conditioned (max |S| < 0.05, Gram matrix factorable in one step) -- not by what later projections could absorb
  static ChainPolicy stay(bool exact)
  {
    ChainPolicy p = rebuild();
    p.drop_tol = exact ? 0.0 : 1.0e-8; p.drop_stol = exact ? 5.0e-2 : 1.0e-9; p.basis_exact = exact;
    return p;
  }
  // mode 6, and mode 5 where the device cannot project with a D that is not the identity: the block is finished in memory by the
  // host-driven loop, which multiplies every X^T U with D D^T (BlockOps::basis_dd) -- exact against the finished basis X D, nothing
  // stays pending
  static ChainPolicy host_loop_exact() { ChainPolicy p; p.basis_exact = true; p.chain_off = true; return p; }
};

// The block operations the orthogonalisation control flow (ortho_cd / ortho_vs_x / ortho in host_logic.cpp) is written
// over.  The device engine implements them on n-length panels in HBM; get_coeffs runs the same control flow on
// host-size coefficient blocks through a plain-loop implementation (CoeffOps in host_logic.cpp) -- it implements these
// few operations and nothing else.  Panels are column-major, ld = n; small matrices are host arrays.
struct BlockOps {
  virtual ~BlockOps() {}
  // C = X^T U (cross-rank reduced when the panels are row shards)
  virtual int gram(int n, int l, const double* x, int k, const double* u, double* c_host, int ldc) = 0;
  // mode 0: Z = X C ; mode 1: Z -= X C (Z read and written)
  virtual int gemm(int n, int l, const double* x, int k, const double* c_host, int ldc, double* z, int mode) = 0;
  // in place U <- U W, W (k x k, host, general) -- used for the triangular update
  virtual int trmm(int n, int k, double* u, const double* w_host, int ld) = 0;
  // fused sweeps: the update plus the Gram matrix of its result.  Default = two sweeps.
  virtual int trmm_gram(int n, int k, double* u, const double* w_host, int ld, double* g_host, int ldg)
  {
    int st = trmm(n, k, u, w_host, ld);
    return st ? st : gram(n, k, u, k, u, g_host, ldg);
  }
  virtual int update_gram(int n, int l, const double* x, int k, const double* c_host, int ldc, double* u, double* g_host, int ldg)
  {
    int st = gemm(n, l, x, k, c_host, ldc, u, 1);
    return st ? st : gram(n, k, u, k, u, g_host, ldg);
  }
  // One sweep over the contiguous panel [X | U] (n x (m+k)):  U <- [X | U] * C'  (C' is (m+k) x k) plus the
  // Gram matrix of the new U.  Used to fold a pending triangular update into the projection step.
  virtual bool can_combo(int /*m*/, int /*k*/) { return false; }
  virtual int combo_gram(int, int, const double*, int, const double*, int, double*, double*, int) { return DLA_ERR_ARG; }
  // ortho_vs_x (m > 0: U is the block that follows X in one panel; bx = X, or B X for the B-metric variant) or plain
  // ortho_cd (m == 0) with the k x k factorisations and the loop decisions on the device: one host wait per call.
  virtual int ortho_chain(int /*n*/, int /*m*/, int /*k*/, const double* /*x*/, const double* /*bx*/, double* /*u*/,
                          OrthoReport* rep) { rep->handled = 0; return 0; }
  // The same in two halves (dla_expand_project): begin enqueues the planned launches and returns with the chain in flight
  // (rep->handled = 1, status 0); finish reads the device's report -- `waited`: the caller has waited for the stream in
  // between -- and completes the chain when it went another way than planned (rep->clean = 0 then: whatever the caller
  // enqueued in between has read an unfinished block).  Nothing but launches on the engine's stream may come in between.
  virtual int ortho_chain_begin(int, int, int, const double*, const double*, double*, OrthoReport* rep) { rep->handled = 0; return 0; }
  virtual int ortho_chain_finish(OrthoReport*, bool /*waited*/) { return DLA_ERR_ARG; }
  // b_ortho (M = U^T BU, L = chol(M), U <- U L^-T, BU <- BU L^-T) enqueued without a host wait, optionally only behind a chain
  // that ended well; *handled = 0: not taken (the caller runs the host-driven b_ortho).  b_ortho_ahead_status() after the
  // caller's next host wait: 1 done, 0 did not run, -1 the metric is not positive definite.
  virtual int b_ortho_ahead(int /*n*/, int /*k*/, double* /*u*/, double* /*bu*/, bool /*behind_chain*/, int* handled) { *handled = 0; return 0; }
  virtual int b_ortho_ahead_status() { return 0; }
  // the top k GLOBAL rows of the n x k block u (row0 = global index of local row 0), k x k to the host
  virtual int top_rows(int n, int k, const double* u, long long row0, double* qt_host) = 0;
  // replace column uj (n local rows, global index of row 0 = row0) by a generated one -- the Householder fallback's answer to
  // a column that lies in the span of its predecessors (gram_schmidt2 in host_logic.cpp).  Default: host memory.
  virtual int fresh_column(int n, double* uj, long long row0, unsigned long long seed)
  {
    for (int i = 0; i < n; ++i) {
      unsigned long long s = (seed + 0x9E3779B97F4A7C15ULL * (unsigned long long)(row0 + i + 1));
      s ^= s >> 30; s *= 0xBF58476D1CE4E5B9ULL; s ^= s >> 27; s *= 0x94D049BB133111EBULL; s ^= s >> 31;
      uj[i] = (double)(s >> 11) * (1.0 / 9007199254740992.0) - 0.5;
    }
    return 0;
  }
  ChainPolicy policy = ChainPolicy::finish();   // what the current caller wants from a chain (PolicyScope)
  // The block a chain with policy.publishes() left pending.  p = [E ; T] is (m + k) x k: the finished block is [X | U_stored] p -- T the
  // upper-triangular factor that was not applied, E the closing projection that was not run (only the three-pass schedule of the
  // device chain leaves one).  Default: [0 ; I] (nothing is ever pending in the host-driven loops).
  // *applied = 1: the chain's closing sweep HAS applied p to the block in memory (it ran without measuring anything): the block in
  // memory is [X | U_measured] p, and what the caller still owes it is the k x k factor of its Gram matrix I - E^T E
  virtual int pending_block(int m, int k, double* p, int ldp, int* applied)
  {
    for (int j = 0; j < k; ++j)
      for (int i = 0; i < m + k; ++i) p[(size_t)i + (size_t)j * ldp] = (i == m + j) ? 1.0 : 0.0;
    if (applied) *applied = 0;
    return 0;
  }
  // policy.basis_exact: the caller's upper-triangular D, block by block (m = columns in front of the block, k <= 0: forget everything)
  virtual int basis_sync(int /*m*/, int /*k*/, const double* /*dmat*/, int /*ld*/) { return 0; }
  virtual bool basis_exact_ok() const { return false; }   // the device-driven chain takes one-tile blocks on this context
  // xu <- D D^T xu (m x k, leading dimension ld) while policy.basis_exact is set: what the host-driven loop multiplies X^T U with before a
  // projection, so that it projects with X (D D^T) X^T as the device chain does (a chain that stopped half way -- ortho_cd out of
  // iterations, Householder fallback -- is continued there)
  virtual int basis_dd(int /*m*/, int /*k*/, double* /*xu*/, int /*ld*/) { return 0; }
  // What the engine's copy of the caller's D says about the m columns in front of a block: 0 = D is the identity there (the stored
  // columns are finished: engines that never leave anything pending always answer this), 1 = the copy describes exactly these m
  // columns and is NOT the identity (a projection against the stored columns alone would leave |X_c^T X_c - I| of what it removes),
  // -1 = the copy does not describe them.
  virtual int basis_state(int /*m*/) const { return 0; }
  // basis columns (block included) up to which the device-driven chain can project with the caller's D (0: not at all)
  virtual int basis_capacity() const { return 0; }
  int ortho_maxit = 10;      // maxit of ortho_cd / ortho_vs_x (diaglib.f90:3224,3521); DLA_OPT_ORTHO_MAXIT lowers it in tests
  std::string err;
};

// installs a policy for the length of a call and puts back what was there before
struct PolicyScope {
  BlockOps* o; ChainPolicy saved;
  PolicyScope(BlockOps* o_, const ChainPolicy& p) : o(o_), saved(o_->policy) { o->policy = p; }
  ~PolicyScope() { o->policy = saved; }
  PolicyScope(const PolicyScope&) = delete;
  PolicyScope& operator=(const PolicyScope&) = delete;
};

// The stored sparse matrices of a context (Engine::spmm_* below says what they are and which rules tie them together).  Internal:
// the public entries number the operator and the metric by `which` and the parts by DLA_SPMM_LR_APB .. _SMD.
enum SpmmSlot { SPMM_NO_PART = -2, SPMM_NO_WHICH = -1, SPMM_A = 0, SPMM_B, SPMM_APB, SPMM_AMB, SPMM_SPD, SPMM_SMD, SPMM_SLOTS };
// where the CSR arrays of a set-up live; PLAIN: host arrays through dla_spmm_setup_csr, the entry without a format (A in ELLPACK,
// its own name in messages)
enum SpmmVia { SPMM_VIA_PLAIN, SPMM_VIA_HOST, SPMM_VIA_DEVICE };
inline int spmm_slot_of_which(int which) { return which == 0 ? SPMM_A : which == 1 ? SPMM_B : SPMM_NO_WHICH; }
inline int spmm_slot_of_part(int part) { return part >= 0 && part < SPMM_SLOTS - SPMM_APB ? SPMM_APB + part : SPMM_NO_PART; }
// ... and the six stored dense matrices, numbered the same way (dla_dense_setup: which, dla_dense_setup_lr: part)
enum DenseSlot { DENSE_NO_PART = -2, DENSE_NO_WHICH = -1, DENSE_A = 0, DENSE_B, DENSE_APB, DENSE_AMB, DENSE_SPD, DENSE_SMD, DENSE_SLOTS };
inline int dense_slot_of_which(int which) { return which == 0 ? DENSE_A : which == 1 ? DENSE_B : DENSE_NO_WHICH; }
inline int dense_slot_of_part(int part) { return part >= 0 && part < DENSE_SLOTS - DENSE_APB ? DENSE_APB + part : DENSE_NO_PART; }

// What the host logic needs from a device.  All panel pointers are device addresses,
// column-major, ld = n.  Reductions (gram / residual norms / nrm2) return host-visible,
// cross-rank-reduced results and imply a stream synchronisation.
struct Engine : BlockOps {
  virtual const char* name() const = 0;
  virtual void* stream() = 0;

  virtual int alloc(size_t bytes, void** dev) = 0;
  virtual int free_(void* dev) = 0;
  virtual int zero(void* dev, size_t bytes) = 0;
  virtual int trim(size_t* released) { if (released) *released = 0; return 0; }   // release cached free blocks
  virtual int h2d(void* dev, const void* host, size_t bytes) = 0;
  virtual int d2h(void* host, const void* dev, size_t bytes) = 0;
  virtual int d2d(void* dst, const void* src, size_t bytes) = 0;
  virtual int sync() = 0;

  // C = X^T U for two n x l panels when only the lower triangle of C will be read (dsyev 'l'): entries above
  // the 16 x 16 block diagonal may be left zero.  Default = the full product.
  virtual int gram_lower(int n, int l, const double* x, const double* u, double* c_host, int ldc) { return gram(n, l, x, l, u, c_host, ldc); }
  // top rows through the Gram door, E^T U with E = (e_1 .. e_k): works for row-sharded panels with what every engine has
  int top_rows(int n, int k, const double* u, long long row0, double* qt_host) override
  {
    void* ev = nullptr;
    int st = alloc(sizeof(double) * (size_t)n * k, &ev);
    if (st) return st;
    st = zero(ev, sizeof(double) * (size_t)n * k);
    const double unit = 1.0;
    for (int j = 0; j < k && !st; ++j) {
      const long long lr = (long long)j - row0;             // global row j on this shard?
      if (lr >= 0 && lr < n) st = h2d((double*)ev + (size_t)j * n + lr, &unit, sizeof(double));
    }
    if (!st) st = gram(n, k, (const double*)ev, k, u, qt_host, k);
    int stf = free_(ev);
    return st ? st : stf;
  }
  virtual int ritz_residual(int n, int l, int m, const double* v, const double* av, const double* y_host, int ldy,
                            const double* eig, int n_res, const int* skip, double* evec, double* r,
                            double* avy /* optional n x m: uncorrected AV*Y */,
                            double* sumsq_max /* 2*n_res: sum r^2, max|r| */) = 0;
  // The Ritz sweep without Ritz vectors that also forms the next Davidson block from a PREDICTED first open root (dla_ritz_expand):
  // u0 = precnd(r(:, first0 ..), fac) with the device-resident diagonal of the library's preconditioner `precnd_kind` (0: sample
  // operator, 1: stored sparse, 2: stored dense), k = m - first0 columns, and [V | u0]^T u0 measured for the orthogonalisation chain
  // that follows (the engine remembers it until ortho_chain_begin on the same block, or until anything else is launched).
  // *ran = 0: the engine does not take the shape and NOTHING has been done -- the caller runs ritz_residual.  Default: never.
  virtual int ritz_expand(int /*n*/, int /*l*/, int /*m*/, const double* /*v*/, const double* /*av*/, const double* /*y_host*/, int /*ldy*/,
                          const double* /*eig*/, int /*n_res*/, const int* /*skip*/, double* /*r*/, double* /*sumsq_max*/,
                          int /*precnd_kind*/, double /*fac*/, int /*first0*/, int /*k*/, double* /*u0*/, int* ran)
  {
    *ran = 0;
    return 0;
  }
  // fused sweeps that ran, and records of them that were dropped unused (the prediction missed, or something else came between)
  virtual void ritz_expand_counts(long long* run, long long* discarded) { *run = 0; *discarded = 0; }
  // the measured matrices of the fused sweep on record, [V | u0]^T u0 ((m + k) x k, host), reduced as the chain would reduce them
  virtual int ritz_expand_measured(int /*m*/, int /*k*/, double* /*c_host*/, int /*ldc*/) { return DLA_ERR_ARG; }
  // the same sweep also forms P = V C2 and AP = AV C2 (k2 columns; LOBPCG's new P block, reference diaglib.f90:495-501,
  // whose products read the same two panels as the Ritz step).  Default: the Ritz step, then two panel products.
  virtual int ritz_residual_p(int n, int l, int m, const double* v, const double* av, const double* y_host, int ldy,
                              const double* eig, int n_res, const int* skip, double* evec, double* r, double* avy,
                              double* sumsq_max, int k2, const double* c2_host, int ldc2, double* p, double* ap)
  {
    int st = ritz_residual(n, l, m, v, av, y_host, ldy, eig, n_res, skip, evec, r, avy, sumsq_max);
    if (!st && k2 > 0) st = gemm(n, l, v, k2, c2_host, ldc2, p, 0);
    if (!st && k2 > 0) st = gemm(n, l, av, k2, c2_host, ldc2, ap, 0);
    return st;
  }
  // e = V Y1, r = AV Y2 - eig e for the first n_res columns (skip as above) with the norms of r: the residual blocks of the
  // linear-response drivers (two panels, two coefficient sets).  Default: two panel products (e, and t = AV Y2 in t_work) and
  // the Ritz sweep on the two n x m results with Y = identity (its copy of e goes to `junk`).
  virtual int ritz_residual2(int n, int l, int m, const double* v, const double* av, const double* y1_host, int ldy1,
                             const double* y2_host, int ldy2, const double* eig, int n_res, const int* skip,
                             double* e, double* r, double* t_work, double* junk, double* sumsq_max)
  {
    int st = gemm(n, l, v, m, y1_host, ldy1, e, 0);
    if (!st) st = gemm(n, l, av, m, y2_host, ldy2, t_work, 0);
    if (st) return st;
    std::string ident_s((size_t)m * m * sizeof(double), '\0');
    double* ident = (double*)&ident_s[0];
    for (int j = 0; j < m; ++j) ident[(size_t)j * m + j] = 1.0;
    return ritz_residual(n, m, m, e, t_work, ident, m, eig, n_res, skip, junk, r, nullptr, sumsq_max);
  }
  virtual int axpy(size_t len, double alpha, const double* x, double* y) = 0;
  virtual int sumsq(size_t len, const double* x, double* out) = 0;
  virtual int stream_triad(size_t /*len*/, int /*reps*/, double* gbps) { *gbps = 0.0; return DLA_ERR_ARG; }
  // evec(i,j) = u01(seed, row0+i+1, j+1) + offset (counter-based generator, global row indices); rows whose global
  // index exceeds support_rows (when > 0) are set to zero
  virtual int random_fill(int n, int m, double* evec, long long row0, unsigned long long seed, double offset,
                          long long support_rows) = 0;
  int fresh_column(int n, double* uj, long long row0, unsigned long long seed) override { return random_fill(n, 1, uj, row0, seed, -0.5, 0); }

  virtual int synth_setup(long long n_global, long long row0, int n_local, int rank_w, double sigma) = 0;
  virtual int synth_matvec(int n, int m, const double* x, double* ax) = 0;
  // the sample operators of the linear-response / generalised drivers around the same W (hip_engine.hip SynthKind)
  virtual int synth_apply(int /*kind*/, int /*n*/, int /*m*/, const double* /*x*/, double* /*y*/) { return DLA_ERR_ARG; }
  virtual int synth_lrprec(int /*variant*/, int /*n*/, int /*m*/, double /*fac*/, const double* /*xp*/, const double* /*xm*/,
                           double* /*yp*/, double* /*ym*/) { return DLA_ERR_ARG; }
  virtual int synth_precnd(int n, int m, double fac, const double* x, double* px) = 0;

  // Ordering of a DEVICE-mode callback against the engine's stream (the user's kernels may run on another stream):
  // mode 0 = stream-ordered through events (the legacy null stream waits for the engine's pending work before the
  // callback, the engine's stream waits for the null stream's work after it; no host wait), 1 = host-synchronise the
  // engine's stream before and the whole device after, 2 = nothing (the callback enqueues on dla_stream itself).
  virtual int callback_begin(int /*mode*/) { return 0; }
  virtual int callback_end(int /*mode*/) { return 0; }

  // ---- the stored sparse matrices.  A context stores up to six (SpmmSlot): the sample operator A (dla_spmm_matvec, dla_spmm_precnd),
  // the metric B of A x = lambda B x (dla_spmm_bvec, dla_spmm_precnd_pencil) and the four parts A+B, A-B, S+D, S-D of the
  // linear-response pencil (dla_spmm_apbmul .. smdmul, dla_spmm_lrprec1 / 2).  All six are single-rank matrices in any storage format
  // (DLA_SPMM_ELL / _SELL / _AUTO: sell_build below) with independent storage, set up, refreshed, asked about and multiplied by
  // through the same functions; setting or dropping one leaves the others alone.  Two rules tie them together: A alone may instead
  // live on a row shard (spmm_setup_csr_sharded), and while it does B and the parts are refused -- as the sharded set-up is while B
  // or a part is stored; and an accepted set-up of A through spmm_setup / spmm_setup_dev makes A whole again.  `slot` is an
  // SpmmSlot, or SPMM_NO_WHICH / SPMM_NO_PART for a public number out of range, which the engine refuses in the entry's words.
  // The host-memory test engine holds a sharded A only: it overrides spmm_matvec and keeps the defaults for the rest.
  // set-up from CSR arrays in host or device memory (via: SpmmVia), and new values from device arrays for the pattern a slot holds
  virtual int spmm_setup(int /*slot*/, int /*via*/, int /*n*/, const long long* /*rowptr*/, const int* /*colind*/, const double* /*values*/,
                         int /*format*/) { return DLA_ERR_ARG; }
  virtual int spmm_refresh_dev(int /*slot*/, int /*n*/, const long long* /*rowptr_dev*/, const int* /*colind_dev*/,
                               const double* /*values_dev*/) { return DLA_ERR_ARG; }
  // what a slot stores; the device blocks of slots first .. last given back (nothing happens where nothing is stored); y = (slot) x
  virtual int spmm_info(int /*slot*/, struct dla_spmm_info* /*out*/) { return DLA_ERR_ARG; }
  virtual int spmm_drop(int /*first*/, int /*last*/) { return DLA_ERR_ARG; }
  // (an engine that stores no sparse matrix but A overrides the product of A alone)
  virtual int spmm_mul(int slot, int n, int m, const double* x, double* y) { return slot == SPMM_A ? spmm_matvec(n, m, x, y) : DLA_ERR_ARG; }
  virtual int spmm_matvec(int /*n*/, int /*m*/, const double* /*x*/, double* /*ax*/) { return DLA_ERR_ARG; }
  // the transposed index of A (TransposeIndex below; the contract: include/diaglib_amd.h, dla_spmm_transpose_prepare) and y = A^T x
  // through it.  An engine without one (the host-memory test engine) refuses every call.
  int no_transpose(const char* entry) { err = std::string(entry) + ": this engine keeps no transposed index"; return DLA_ERR_ARG; }
  virtual int spmm_transpose_prepare(int /*format*/) { return no_transpose("spmm_transpose_prepare"); }
  virtual int spmm_transpose_info(struct dla_spmm_info* /*out*/) { return no_transpose("spmm_transpose_info"); }
  virtual int spmm_transpose_drop() { return DLA_OK; }
  virtual int spmm_mul_t(int /*n*/, int /*m*/, const double* /*x*/, double* /*y*/) { return no_transpose("spmm_matvec_t"); }
  // A on a row shard: rows row0 .. row0 + n_local - 1 of A with GLOBAL column indices.  Columns outside the shard must lie within
  // `halo` rows of it (a banded matrix); every rank publishes its first and last `halo` rows of x through the all-reduce of the
  // small-product transport (disjoint slots: a sum that gathers), see sharded_ell_* below.  Collective: every rank calls it (the
  // halo width is agreed by a max-reduction).
  virtual int spmm_setup_csr_sharded(int /*n_local*/, long long /*row0*/, long long /*n_global*/, const long long* /*rowptr*/,
                                     const long long* /*colind*/, const double* /*values*/) { return DLA_ERR_ARG; }
  // the diagonal preconditioners: px = x / (a_ii + fac), px = x / (a_ii + fac b_ii) of the pencil, and the harness' lrprec_1 /
  // lrprec_2 (variant 1 / 2) on the diagonals of A+B, A-B and S+D
  virtual int spmm_precnd(int /*n*/, int /*m*/, double /*fac*/, const double* /*x*/, double* /*px*/) { return DLA_ERR_ARG; }
  virtual int spmm_precnd_pencil(int /*n*/, int /*m*/, double /*fac*/, const double* /*x*/, double* /*px*/) { return DLA_ERR_ARG; }
  virtual int spmm_lrprec(int /*variant*/, int /*n*/, int /*m*/, double /*fac*/, const double* /*xp*/, const double* /*xm*/,
                          double* /*yp*/, double* /*ym*/) { return DLA_ERR_ARG; }
  // the Chebyshev polynomial preconditioner on the stored A (the contract: include/diaglib_amd.h, dla_spmm_precnd_cheb): the
  // configuration belongs to the engine, not to the matrix; steps = 0 switches it off and gives the work panels back
  virtual int spmm_cheb_config(int /*steps*/, double /*lo_fraction*/) { return DLA_ERR_ARG; }
  virtual int spmm_cheb_info(struct dla_spmm_cheb_info* /*out*/) { return DLA_ERR_ARG; }
  virtual int spmm_precnd_cheb(int /*n*/, int /*m*/, double /*fac*/, const double* /*x*/, double* /*px*/) { return DLA_ERR_ARG; }
  // ... and the same iteration on the diagonally scaled operator D^-1 (A + fac I) (dla_spmm_precnd_cheb_jacobi), under the same
  // configuration; spmm_cheb_jacobi_upper: the upper end hi of its interval for one fac
  virtual int spmm_precnd_cheb_jacobi(int /*n*/, int /*m*/, double /*fac*/, const double* /*x*/, double* /*px*/) { return DLA_ERR_ARG; }
  virtual int spmm_cheb_jacobi_upper(double /*fac*/, double* /*hi*/) { return DLA_ERR_ARG; }
  // ... and on the scaled pencil D^-1 (A + fac B) with the stored metric B (dla_spmm_precnd_cheb_pencil); spmm_cheb_pencil_upper: hi
  virtual int spmm_precnd_cheb_pencil(int /*n*/, int /*m*/, double /*fac*/, const double* /*x*/, double* /*px*/) { return DLA_ERR_ARG; }
  virtual int spmm_cheb_pencil_upper(double /*fac*/, double* /*hi*/) { return DLA_ERR_ARG; }

  // ---- the stored dense matrices (the contract: include/diaglib_amd.h, dla_dense_setup and dla_dense_setup_lr).  A context stores up
  // to six (DenseSlot): the operator A, the metric B and the four parts A+B, A-B, S+D, S-D of the linear-response pencil, each the
  // library's own copy of a column-major a(lda, n) in host (via = SPMM_VIA_HOST) or device memory (SPMM_VIA_DEVICE) with its diagonal
  // beside it; independent of each other and of the sparse slots.  `slot` is a DenseSlot, or DENSE_NO_WHICH / DENSE_NO_PART for a
  // public number out of range, which the engine refuses in the entry's words.  dense_setup_pair fills two parts with p + q and
  // p - q (pair 0: A+B and A-B of A, B; pair 1: S+D and S-D of S, D), both or neither; dense_drop gives back slots first .. last
  // (nothing happens where nothing is stored).  dense_precnd: x / (a_ii + fac), or with pencil x / (a_ii + fac b_ii); dense_lrprec:
  // the harness' lrprec_1 / lrprec_2 (variant 1 / 2) on the stored diagonals of A+B, A-B and S+D.  An engine without them (the
  // host-memory test engine) refuses every call.
  int no_dense() { err = "this engine stores no dense matrix"; return DLA_ERR_ARG; }
  virtual int dense_setup(int /*slot*/, int /*via*/, int /*n*/, const double* /*a*/, int /*lda*/) { return no_dense(); }
  virtual int dense_setup_pair(int /*pair*/, int /*via*/, int /*n*/, const double* /*p*/, int /*ldp*/, const double* /*q*/, int /*ldq*/) { return no_dense(); }
  virtual int dense_info(int /*slot*/, struct dla_dense_info* /*out*/) { return no_dense(); }
  // one triangle of a symmetric operator or metric (dla_dense_setup_sym; uplo as the caller gave it) and what dla_dense_sym_info answers
  virtual int dense_setup_sym(int /*slot*/, int /*via*/, int /*n*/, const double* /*a*/, int /*lda*/, char /*uplo*/) { return no_dense(); }
  virtual int dense_sym_info(int /*slot*/, struct dla_dense_sym_info* /*out*/) { return no_dense(); }
  virtual int dense_drop(int /*first*/, int /*last*/) { return no_dense(); }
  virtual int dense_mul(int /*slot*/, int /*n*/, int /*m*/, const double* /*x*/, double* /*y*/) { return no_dense(); }
  // y = A^T x on the operator slot's copy (dla_dense_matvec_t)
  virtual int dense_mul_t(int /*n*/, int /*m*/, const double* /*x*/, double* /*y*/) { return no_dense(); }
  virtual int dense_precnd(bool /*pencil*/, int /*n*/, int /*m*/, double /*fac*/, const double* /*x*/, double* /*px*/) { return no_dense(); }
  virtual int dense_lrprec(int /*variant*/, int /*n*/, int /*m*/, double /*fac*/, const double* /*xp*/, const double* /*xm*/,
                           double* /*yp*/, double* /*ym*/) { return no_dense(); }

  // Staging pipeline of host-mode callbacks: column chunks of a block travel device -> host on one copy stream, the
  // user's routine works on the chunk that has arrived, finished chunks travel host -> device on a second copy stream
  // (PCIe is full duplex), and the engine's own stream only waits for the last upload -- no host wait at the end.
  //   stage_begin():            the copy streams may start once everything queued on the engine's stream is done
  //   stage_d2h(h, d, b, slot): enqueue a download; stage_wait(slot): host waits for that download
  //   stage_h2d(d, h, b):       enqueue an upload;  stage_end(): the engine's stream waits for all uploads
  // Defaults = plain synchronous copies (host-memory test engine).
  virtual int stage_begin() { return 0; }
  virtual int stage_d2h(void* host, const void* dev, size_t bytes, int /*slot*/) { return d2h(host, dev, bytes); }
  virtual int stage_wait(int /*slot*/) { return 0; }
  virtual int stage_h2d(void* dev, const void* host, size_t bytes) { return h2d(dev, host, bytes); }
  virtual int stage_end() { return 0; }
  // projection of a block that arrives in column chunks (dla_expand_project with host-mode callbacks): chunk c0 .. c0 + kc - 1
  // of C = X^T U (l x k_total) behind the uploads issued so far, no host wait; collect waits once and copies C out
  virtual bool gram_chunks_ok(int, int, int) { return false; }
  virtual int gram_chunk(int, int, const double*, int, int, int, const double*) { return DLA_ERR_ARG; }
  virtual int gram_chunks_collect(int, int, double*, int) { return DLA_ERR_ARG; }

  // pinned host staging for host-mode callbacks
  virtual int host_alloc(size_t bytes, void** p) = 0;
  virtual int host_free(void* p) = 0;

  // collectives
  virtual int comm_init(int nranks, int rank, const char id[128]) = 0;
  virtual int comm_finalize() { nranks = 1; rank = 0; hook = nullptr; return 0; }
  // one-shot peer-to-peer all-reduce over IPC mailboxes: export this rank's mailbox (2 handles of 64 bytes), then
  // attach all ranks' handles (rank order)
  virtual int p2p_export(int /*nranks*/, void* /*handles*/) { return DLA_ERR_COMM; }
  virtual int p2p_attach(int /*nranks*/, int /*rank*/, const void* /*handles*/) { return DLA_ERR_COMM; }
  virtual int p2p_detach() { return DLA_OK; }
  virtual int set_p2p_timeout(int /*ms*/) { return DLA_OK; }      // DLA_OPT_P2P_TIMEOUT_MS
  int nranks = 1, rank = 0;
  // Every rank's shard has an even number of rows (agreed when the shards are announced, dla_set_shard).  Whatever decides which
  // SWEEPS and REDUCTIONS a call consists of must not look at the local row count alone: a rank with an odd shard would take
  // another schedule than its peers, and the exchanges would no longer pair up (found by tools/fuzz_multirank.py: odd n on three
  // and four ranks).  even_rows(n) is the test to use.
  bool peers_even = true;
  bool even_rows(long long n) const { return n % 2 == 0 && peers_even; }
  // all-reduce of a few HOST values over the small-product transport (setup-time agreement between the ranks); collective
  virtual int allreduce_host(double* /*v*/, int /*count*/, int /*op: 0 sum, 1 max*/) { return nranks > 1 ? DLA_ERR_COMM : DLA_OK; }
  virtual bool has_transport() const { return hook != nullptr; }     // something that can carry a cross-rank reduction is attached
  bool local_only = false;   // true while working on data that is replicated on every rank (no reductions)
  dla_allreduce_fn hook = nullptr;
  void* hook_user = nullptr;

  // statistics
  dla_stats stats{};
  bool profile = false;
  virtual void collect_times() {}
  // dla_expand_project's run-ahead: what is launched between begin and end(discard = true) was speculation whose output
  // nobody uses -- it is taken out of the launch / byte / flop statistics (and its events out of the time statistics) again
  virtual void spec_stats_begin() {}
  virtual void spec_stats_end(bool /*discard*/) {}
  virtual int kernel_stats(dla_kernel_stat*, int) { return 0; }
  virtual void reset_kernel_stats() {}
  virtual void set_tune(int, int) {}
  virtual int get_tune(int) { return 0; }
  // a driver call starts: whatever the engine adapts from what earlier chains did is put back to its initial state, so that a solve's
  // sequence of sweeps -- and with it every bit of its result -- is a function of that solve alone
  virtual void begin_solve() {}
};

// $DIAGLIB_AMD_HOSTTIME=1: wall time spent inside each C-ABI entry point (printed by dla_destroy)
struct ApiTimer {
  static bool on();
  static void add(const char* name, double dt);
  static void report();
  static double now();
  static void enter(const char* name, double t);     // charges the time since the previous entry point returned to "<prev> .. <name>"
  static void leave(const char* name, double t);
  const char* name; double t0;
  explicit ApiTimer(const char* n) : name(n), t0(on() ? now() : 0.0) { if (on()) enter(name, t0); }
  ~ApiTimer() { if (on()) { const double t1 = now(); add(name, t1 - t0); leave(name, t1); } }
};
#define DLA_CAT2(a, b) a##b
#define DLA_CAT(a, b) DLA_CAT2(a, b)
#define DLA_T(name) dla::ApiTimer DLA_CAT(dla_api_timer_, __LINE__)(name)

// provided by the engine translation unit linked into the library
// ---- a row shard of a sparse matrix as ELLPACK with a halo (spmm_setup_csr_sharded of both engines)
// Column indices are kept relative to an EXTENDED local vector [halo rows of the previous rank | the shard's n rows | halo rows of
// the next rank]: index = global column - row0 + halo.
struct ShardedEll {
  int n = 0, w = 0, halo = 0;
  long long row0 = 0;
  std::vector<int> col;          // [w][n]
  std::vector<double> val, diag; // [w][n], [n]
};
// widest row and the number of rows of the neighbours this shard's columns reach into; checks the indices
inline int sharded_ell_need(int n, long long row0, long long n_global, const long long* rowptr, const long long* colind, int* w,
                            long long* need, std::string& err)
{
  *w = 0; *need = 0;
  if (n <= 0 || row0 < 0 || row0 + n > n_global || !rowptr || !colind) { err = "spmm_setup_csr_sharded: bad arguments"; return DLA_ERR_ARG; }
  for (int i = 0; i < n; ++i) {
    const long long p0 = rowptr[i], p1 = rowptr[i + 1];
    if (p1 < p0) { err = "spmm_setup_csr_sharded: row pointers not ascending"; return DLA_ERR_ARG; }
    if (p1 - p0 > *w) *w = (int)(p1 - p0);
    for (long long p = p0; p < p1; ++p) {
      const long long c = colind[p];
      if (c < 0 || c >= n_global) { err = "spmm_setup_csr_sharded: column index out of range"; return DLA_ERR_ARG; }
      if (c < row0 && row0 - c > *need) *need = row0 - c;
      if (c >= row0 + n && c - (row0 + n - 1) > *need) *need = c - (row0 + n - 1);
    }
  }
  if (*w <= 0) { err = "spmm_setup_csr_sharded: empty shard"; return DLA_ERR_ARG; }
  return DLA_OK;
}
inline void sharded_ell_build(int n, long long row0, const long long* rowptr, const long long* colind, const double* values,
                              int halo, ShardedEll& e)
{
  int w = 0;
  for (int i = 0; i < n; ++i) if ((int)(rowptr[i + 1] - rowptr[i]) > w) w = (int)(rowptr[i + 1] - rowptr[i]);
  e.n = n; e.w = w; e.halo = halo; e.row0 = row0;
  e.col.assign((size_t)w * n, 0); e.val.assign((size_t)w * n, 0.0); e.diag.assign((size_t)n, 0.0);
  for (int i = 0; i < n; ++i) {
    const long long p0 = rowptr[i], p1 = rowptr[i + 1];
    for (int q = 0; q < w; ++q) {
      const bool in = p0 + q < p1;
      const long long c = in ? colind[p0 + q] : row0 + i;      // (padding: a zero that points at the row itself)
      e.col[(size_t)q * n + i] = (int)(c - row0 + halo);
      e.val[(size_t)q * n + i] = in ? values[p0 + q] : 0.0;
      if (in && c == row0 + i) e.diag[i] += values[p0 + q];
    }
  }
}

// ---- the single-rank operator as sliced ELLPACK (SELL-C-sigma) with a CSR tail for long rows (spmm_setup_csr_fmt)
// Storage follows the non-zeros, not widest row x n: rows are sorted by descending length (stable) inside windows of SELL_SIGMA
// rows, cut into slices of SELL_C consecutive slots, and every slice is padded to ITS longest row only.  One wavefront owns a
// slice, so entry (q, lane) of slice s lives at slice_ptr[s] + q * SELL_C + lane and both matrix streams stay coalesced as in
// the plain ELLPACK kernel.  A row with more than SELL_LONG_ROW entries would widen its whole slice: it counts as an empty row
// in the slices (sorted and padded as one) and is kept whole, in the caller's order, in the CSR tail.
// A tail row is multiplied in segments of SELL_LONG_SEG entries, one wavefront each (the contract: include/diaglib_amd.h): segment s
// of a row with entries [p0, p1) covers [p0 + s SEG, min(p1, p0 + (s + 1) SEG)).  A row of one segment is stored by the wavefront
// that sums it; a longer row owns one slot per segment in a workspace of partial sums, added in segment order by one thread.
// The three constants are unmeasured starting values: SELL_C is the wavefront width, the other two are guesses.
constexpr int SELL_C = 64;
constexpr int SELL_SIGMA = 4096;
constexpr int SELL_LONG_ROW = 256;
// (a starting value as well; a multiple of the wavefront width, so that every lane of a full segment takes the same number of entries)
constexpr int SELL_LONG_SEG = 4096;
static_assert(SELL_LONG_SEG > 0 && SELL_LONG_SEG % 64 == 0, "a segment of a tail row is a positive multiple of 64 entries");
// AUTO keeps plain ELLPACK while its padding w n / nnz stays at or below this (a guess as well)
constexpr double SPMM_AUTO_ELL_PADDING = 1.25;

struct SellLayout {
  int n = 0, slices = 0;
  long long nnz = 0, stored = 0, long_entries = 0;   // stored: padded entries of the slices
  std::vector<long long> slice_ptr;   // [slices + 1], in entries; the width of slice s is (slice_ptr[s + 1] - slice_ptr[s]) / SELL_C
  std::vector<int> perm;              // [n]: slot -> row; ~row (negative) for a row that lives in the tail: its slot stores nothing
  std::vector<int> col;               // [stored], the caller's column numbering; padding points at the row itself with a zero
  std::vector<double> val, diag;      // [stored], [n]: diag[i] = sum of all (i, i) entries, tail rows included
  std::vector<int> long_row;          // the tail: rows, [long_rows + 1] offsets, columns and values in the caller's order
  std::vector<long long> long_ptr;
  std::vector<int> long_col;
  std::vector<double> long_val;
  // the segments of the tail rows, in row order: [long_segments + 1] first entries in long_col / long_val, the tail row (an index
  // into long_row) each belongs to, and its slot in the workspace of partial sums (-1: the only segment of its row, stored straight)
  int long_segments = 0, multi_segments = 0;   // all segments; segments of rows with more than one = slots of the workspace
  std::vector<long long> seg_ptr;
  std::vector<int> seg_row, seg_part;
  // the rows of more than one segment: the row, and [multi rows + 1] offsets of its slots (part_ptr[j + 1] - part_ptr[j] segments)
  std::vector<int> multi_row, part_ptr;
};
// what every single-rank setup from host arrays checks, in the words of spmm_setup_csr under the name of `entry`; w = widest row,
// nnz = entries
inline int spmm_csr_check(int n, const long long* rowptr, const int* colind, const double* values, int format, int* w, long long* nnz,
                          std::string& err, const char* entry = "spmm_setup_csr_fmt")
{
  const std::string who = std::string(entry) + ": ";
  *w = 0; *nnz = 0;
  if (format != DLA_SPMM_ELL && format != DLA_SPMM_SELL && format != DLA_SPMM_AUTO) { err = who + "unknown format"; return DLA_ERR_ARG; }
  if (n <= 0 || !rowptr || !colind || !values) { err = who + "bad arguments"; return DLA_ERR_ARG; }
  for (int i = 0; i < n; ++i) {
    if (rowptr[i + 1] < rowptr[i]) { err = who + "row pointers not ascending"; return DLA_ERR_ARG; }
    if (rowptr[i + 1] - rowptr[i] > *w) *w = (int)std::min<long long>(rowptr[i + 1] - rowptr[i], 2147483647LL);
  }
  if (*w <= 0) { err = who + "empty matrix"; return DLA_ERR_ARG; }
  for (long long p = rowptr[0]; p < rowptr[n]; ++p)
    if (colind[p] < 0 || colind[p] >= n) { err = who + "column index out of range"; return DLA_ERR_ARG; }
  *nnz = rowptr[n] - rowptr[0];
  return DLA_OK;
}
// the format a checked matrix is stored in
inline int spmm_pick_format(int format, int w, int n, long long nnz)
{
  if (format != DLA_SPMM_AUTO) return format;
  return (double)w * (double)n <= SPMM_AUTO_ELL_PADDING * (double)nnz ? DLA_SPMM_ELL : DLA_SPMM_SELL;
}
// The layout in two steps, so that a caller whose entries live in device memory runs the first on the row pointers alone and fills
// the blocks there (hip_engine.hip, setup_dev): sell_layout computes everything that depends on the row LENGTHS -- perm, slice_ptr,
// stored, the tail's rows, offsets and segment tables -- and never reads a column or a value; sell_fill scatters the entries of
// host arrays into col / val / long_col / long_val and sums the diagonal.  (the row pointers have passed spmm_csr_check)
inline void sell_layout(int n, const long long* rowptr, SellLayout& s)
{
  s.n = n; s.slices = (n + SELL_C - 1) / SELL_C; s.nnz = rowptr[n] - rowptr[0];
  auto tail = [&](int i) { return rowptr[i + 1] - rowptr[i] > SELL_LONG_ROW; };
  auto len = [&](int i) { return tail(i) ? 0 : (int)(rowptr[i + 1] - rowptr[i]); };   // what row i asks of its slice
  std::vector<int> order((size_t)n);
  for (int i = 0; i < n; ++i) order[i] = i;
  for (int w0 = 0; w0 < n; w0 += SELL_SIGMA)
    std::stable_sort(order.begin() + w0, order.begin() + std::min(n, w0 + SELL_SIGMA), [&](int a, int b) { return len(a) > len(b); });
  s.slice_ptr.assign((size_t)s.slices + 1, 0);
  for (int sl = 0; sl < s.slices; ++sl) {
    int width = 0;
    for (int slot = sl * SELL_C; slot < std::min(n, (sl + 1) * SELL_C); ++slot) width = std::max(width, len(order[slot]));
    s.slice_ptr[sl + 1] = s.slice_ptr[sl] + (long long)width * SELL_C;
  }
  s.stored = s.slice_ptr[s.slices];
  s.perm.assign((size_t)n, 0);
  for (int slot = 0; slot < n; ++slot) s.perm[slot] = tail(order[slot]) ? ~order[slot] : order[slot];
  s.col.clear(); s.val.clear(); s.diag.clear(); s.long_col.clear(); s.long_val.clear();
  s.long_row.clear(); s.long_ptr.assign(1, 0);
  for (int i = 0; i < n; ++i) {
    if (!tail(i)) continue;
    s.long_row.push_back(i);
    s.long_ptr.push_back(s.long_ptr.back() + (rowptr[i + 1] - rowptr[i]));
  }
  s.long_entries = s.long_ptr.back();
  s.seg_ptr.assign(1, 0); s.seg_row.clear(); s.seg_part.clear(); s.multi_row.clear(); s.part_ptr.assign(1, 0);
  for (size_t r = 0; r < s.long_row.size(); ++r) {
    const long long p0 = s.long_ptr[r], p1 = s.long_ptr[r + 1];
    const int segs = (int)((p1 - p0 + SELL_LONG_SEG - 1) / SELL_LONG_SEG);
    for (int g = 0; g < segs; ++g) {
      s.seg_row.push_back((int)r);
      s.seg_part.push_back(segs > 1 ? s.part_ptr.back() + g : -1);
      s.seg_ptr.push_back(std::min(p1, p0 + (long long)(g + 1) * SELL_LONG_SEG));
    }
    if (segs > 1) { s.multi_row.push_back(s.long_row[r]); s.part_ptr.push_back(s.part_ptr.back() + segs); }
  }
  s.long_segments = (int)s.seg_row.size(); s.multi_segments = s.part_ptr.back();
}
// (s comes from sell_layout of the same row pointers; the columns have passed spmm_csr_check)
inline void sell_fill(int n, const long long* rowptr, const int* colind, const double* values, SellLayout& s)
{
  s.col.assign((size_t)s.stored, 0); s.val.assign((size_t)s.stored, 0.0); s.diag.assign((size_t)n, 0.0);
  s.long_col.clear(); s.long_val.clear();
  for (int i = 0; i < n; ++i)
    for (long long p = rowptr[i]; p < rowptr[i + 1]; ++p) if (colind[p] == i) s.diag[i] += values[p];
  for (const int i : s.long_row) {
    s.long_col.insert(s.long_col.end(), colind + rowptr[i], colind + rowptr[i + 1]);
    s.long_val.insert(s.long_val.end(), values + rowptr[i], values + rowptr[i + 1]);
  }
  for (int sl = 0; sl < s.slices; ++sl) {
    const long long base = s.slice_ptr[sl];
    const int width = (int)((s.slice_ptr[sl + 1] - base) / SELL_C);
    for (int lane = 0; lane < SELL_C; ++lane) {
      const int slot = sl * SELL_C + lane;
      const bool tail = slot < n && s.perm[slot] < 0;
      const int i = slot < n ? (tail ? ~s.perm[slot] : s.perm[slot]) : 0;          // (slots past n pad with zeros that point at row 0)
      const int li = (slot < n && !tail) ? (int)(rowptr[i + 1] - rowptr[i]) : 0;   // (a tail row asks nothing of its slice)
      for (int q = 0; q < width; ++q) {
        const bool in = q < li;
        s.col[(size_t)(base + (long long)q * SELL_C + lane)] = in ? colind[rowptr[i] + q] : i;
        s.val[(size_t)(base + (long long)q * SELL_C + lane)] = in ? values[rowptr[i] + q] : 0.0;
      }
    }
  }
}
inline void sell_build(int n, const long long* rowptr, const int* colind, const double* values, SellLayout& s)
{
  sell_layout(n, rowptr, s);
  sell_fill(n, rowptr, colind, values, s);
}

// ---- the transposed index of the stored operator (include/diaglib_amd.h, dla_spmm_transpose_prepare): y = A^T x from the one stored
// copy of A's values.  The index is a sparse layout of its own -- ELLPACK, or slices with a tail, decided by the code above on the
// COLUMN lengths of A -- whose entries are two int32 instead of a column and a value: the source row, and the position of the value
// in A's stored val array (the tail of a sliced A lies behind its `stored` padded entries).  Padding has position -1 and takes part
// in no arithmetic.  The entries of column j stand in ascending order of the caller's CSR arrays, so the product walks them exactly
// as the forward product walks the rows of the explicitly (stably) transposed matrix stored in the index's format.
// The host twin below builds from host arrays what the engine builds on the device from A's stored blocks.
struct TransposeIndex {
  int n = 0, fmt = -1, w = 0;       // fmt: DLA_SPMM_ELL (w: the longest column) or DLA_SPMM_SELL (lay); -1: none
  long long nnz = 0;
  std::vector<long long> colptr;    // [n + 1], from 0: the column pointers of A, which are the row pointers of A^T
  SellLayout lay;                   // DLA_SPMM_SELL: sell_layout of colptr (col / val / diag stay empty)
  std::vector<int> row, pos;        // [entries()]
  long long entries() const { return fmt == DLA_SPMM_SELL ? lay.stored + lay.long_entries : (long long)w * n; }
};
// the stored position of every entry of a matrix in its val array, in the order of the caller's CSR arrays (entry p - rowptr[0]);
// L: sell_layout of the same row pointers for DLA_SPMM_SELL, else the matrix is ELLPACK
inline void spmm_stored_positions(int n, const long long* rowptr, int fmt, const SellLayout* L, std::vector<long long>& apos)
{
  const long long p0 = rowptr[0];
  apos.assign((size_t)(rowptr[n] - p0), -1);
  if (fmt != DLA_SPMM_SELL) {
    for (int i = 0; i < n; ++i)
      for (long long p = rowptr[i]; p < rowptr[i + 1]; ++p) apos[(size_t)(p - p0)] = (p - rowptr[i]) * n + i;
    return;
  }
  for (int slot = 0; slot < n; ++slot) {
    if (L->perm[slot] < 0) continue;
    const int i = L->perm[slot];
    const long long base = L->slice_ptr[slot / SELL_C] + slot % SELL_C;
    for (long long p = rowptr[i]; p < rowptr[i + 1]; ++p) apos[(size_t)(p - p0)] = base + (p - rowptr[i]) * SELL_C;
  }
  for (size_t r = 0; r < L->long_row.size(); ++r) {
    const int i = L->long_row[r];
    for (long long p = rowptr[i]; p < rowptr[i + 1]; ++p) apos[(size_t)(p - p0)] = L->stored + L->long_ptr[r] + (p - rowptr[i]);
  }
}
// the layout of the index from the column pointers: format, width or slices and tail.  a_entries: what A stores (w n, or stored +
// long_entries), the range of the positions
inline int spmm_transpose_layout(int n, const long long* colptr, int format, long long a_entries, TransposeIndex& t, std::string& err)
{
  if (format != DLA_SPMM_ELL && format != DLA_SPMM_SELL && format != DLA_SPMM_AUTO) { err = "spmm_transpose_prepare: unknown format"; return DLA_ERR_ARG; }
  if (a_entries > 2147483647LL) {
    err = "spmm_transpose_prepare: the operator stores " + std::to_string(a_entries) + " entries, and positions beyond 2147483647 do not fit the index";
    return DLA_ERR_ARG;
  }
  t.n = n; t.nnz = colptr[n] - colptr[0];
  t.colptr.assign(colptr, colptr + n + 1);
  long long w = 0;
  for (int j = 0; j < n; ++j) w = std::max(w, colptr[j + 1] - colptr[j]);
  t.fmt = spmm_pick_format(format, (int)std::min<long long>(w, 2147483647LL), n, t.nnz);
  t.w = t.fmt == DLA_SPMM_ELL ? (int)w : 0;
  t.lay = SellLayout();
  if (t.fmt == DLA_SPMM_SELL) sell_layout(n, t.colptr.data(), t.lay);
  t.row.clear(); t.pos.clear();
  return DLA_OK;
}
// fills row / pos of a laid-out index: src(k, &row, &pos) gives the k-th entry in transposed order (column by column, each in the
// caller's order).  Where each entry goes is what sell_fill and the ELLPACK set-up do with a column and a value.
template <class Src>
inline void spmm_transpose_fill(TransposeIndex& t, Src src)
{
  const int n = t.n;
  t.row.assign((size_t)t.entries(), 0); t.pos.assign((size_t)t.entries(), -1);
  const std::vector<long long>& cp = t.colptr;
  if (t.fmt != DLA_SPMM_SELL) {
    for (int j = 0; j < n; ++j)
      for (int q = 0; q < t.w; ++q) {
        const size_t d = (size_t)q * n + j;
        if (cp[j] + q < cp[j + 1]) src(cp[j] + q, &t.row[d], &t.pos[d]);
        else t.row[d] = j;
      }
    return;
  }
  const SellLayout& s = t.lay;
  for (int sl = 0; sl < s.slices; ++sl) {
    const long long base = s.slice_ptr[sl];
    const int width = (int)((s.slice_ptr[sl + 1] - base) / SELL_C);
    for (int lane = 0; lane < SELL_C; ++lane) {
      const int slot = sl * SELL_C + lane;
      const bool tail = slot < n && s.perm[slot] < 0;
      const int j = slot < n ? (tail ? ~s.perm[slot] : s.perm[slot]) : 0;
      const int lj = (slot < n && !tail) ? (int)(cp[j + 1] - cp[j]) : 0;
      for (int q = 0; q < width; ++q) {
        const size_t d = (size_t)(base + (long long)q * SELL_C + lane);
        if (q < lj) src(cp[j] + q, &t.row[d], &t.pos[d]);
        else t.row[d] = j;
      }
    }
  }
  for (size_t r = 0; r < s.long_row.size(); ++r) {
    const int j = s.long_row[r];
    for (long long e = s.long_ptr[r]; e < s.long_ptr[r + 1]; ++e) {
      const size_t d = (size_t)(s.stored + e);
      src(cp[j] + (e - s.long_ptr[r]), &t.row[d], &t.pos[d]);
    }
  }
}
// the whole index from host CSR arrays that have passed spmm_csr_check; a_fmt / a_layout: how A is stored (spmm_stored_positions)
inline int spmm_transpose_build(int n, const long long* rowptr, const int* colind, int a_fmt, int a_w, const SellLayout* a_layout, int format,
                                TransposeIndex& t, std::string& err)
{
  const long long p0 = rowptr[0], nnz = rowptr[n] - p0;
  const long long a_entries = a_fmt == DLA_SPMM_SELL ? a_layout->stored + a_layout->long_entries : (long long)a_w * n;
  std::vector<long long> colptr((size_t)n + 1, 0);
  for (long long p = p0; p < p0 + nnz; ++p) ++colptr[(size_t)colind[p] + 1];
  for (int j = 0; j < n; ++j) colptr[(size_t)j + 1] += colptr[j];
  { const int stc = spmm_transpose_layout(n, colptr.data(), format, a_entries, t, err); if (stc) return stc; }
  std::vector<long long> apos;
  spmm_stored_positions(n, rowptr, a_fmt, a_layout, apos);
  // a stable counting sort of the entries by column: ascending position in the caller's arrays inside every column
  std::vector<long long> next(colptr.begin(), colptr.end() - 1);
  std::vector<int> srow((size_t)nnz), spos((size_t)nnz);
  for (int i = 0; i < n; ++i)
    for (long long p = rowptr[i]; p < rowptr[i + 1]; ++p) {
      const size_t k = (size_t)next[(size_t)colind[p]]++;
      srow[k] = i; spos[k] = (int)apos[(size_t)(p - p0)];
    }
  spmm_transpose_fill(t, [&](long long k, int* row, int* pos) { *row = srow[(size_t)k]; *pos = spos[(size_t)k]; });
  return DLA_OK;
}

// ---- the scalars of the Chebyshev preconditioner (include/diaglib_amd.h, dla_spmm_precnd_cheb; Saad, Iterative Methods, Algorithm
// 12.1 from a zero start).  Host only; the results are doubles.  For the interval [lo, hi] and d steps: theta = (hi + lo) / 2,
// delta = (hi - lo) / 2, sigma = theta / delta, rho_0 = 1 / sigma, rho_k = 1 / (2 sigma - rho_{k-1}), and step k = 1 .. d - 1 is
//   z_{k+1} = alpha u + beta v + gamma x + eta (A u)
// with alpha = 1 + rho_k rho_{k-1} - (2 rho_k / delta) fac, beta = -rho_k rho_{k-1}, gamma = 2 rho_k / delta, eta = -gamma, u = z_k
// and v = z_{k-1}.  z_1 = x / theta is never stored: step 1 gathers u = x itself with alpha / theta and eta / theta (its beta is
// 0: z_0 = 0), and step 2 takes v = x with beta / theta.  d = 1 has no step: px = x / theta.
struct ChebStep { double alpha, beta, gamma, eta; };
struct ChebCoefficients { double theta = 0.0, delta = 0.0; std::vector<ChebStep> steps; };
inline ChebCoefficients cheb_coefficients(double hi, double lo, double fac, int d)
{
  // The recurrence of rho amplifies a rounding of sigma by 2 sigma / (2 sigma - rho), several-fold when lo_fraction is small, so it
  // is carried in long double and every coefficient is rounded to double once (tests/test_cheb_ref.py: within 8 ulp).
  typedef long double ld;
  ChebCoefficients c;
  const ld theta = ((ld)hi + (ld)lo) / 2, delta = ((ld)hi - (ld)lo) / 2, sigma = theta / delta;
  c.theta = (double)theta;
  c.delta = (double)delta;
  ld rho_prev = 1 / sigma;
  for (int k = 1; k < d; ++k) {
    const ld rho = 1 / (2 * sigma - rho_prev);
    const ld a = rho * rho_prev, b = 2 * rho / delta;
    ld alpha = 1 + a - b * (ld)fac, beta = -a, eta = -b;
    if (k == 1) { alpha /= theta; eta /= theta; beta = 0; }
    if (k == 2) beta /= theta;
    c.steps.push_back(ChebStep{(double)alpha, (double)beta, (double)b, (double)eta});
    rho_prev = rho;
  }
  return c;
}

Engine* make_engine(int device, std::string& err);
int engine_unique_id(char id[128]);

}  // namespace dla

struct dla_ctx {
  dla::Engine* eng = nullptr;
  int callbacks_on_device = 0;
  int evec_on_device = 0;
  int verbose_ortho = 0;
  int caslr_algorithm = 0;   // DLA_OPT_CASLR_ALGORITHM
  int stage_chunks = 0;      // DLA_OPT_STAGE_CHUNKS: 0 = automatic
  int callback_order = 1;    // DLA_OPT_CALLBACK_ORDER (default: host-synchronised, safe for callbacks on any stream)
  int p2p_timeout_ms = 5000; // DLA_OPT_P2P_TIMEOUT_MS
  int run_ahead = 1;         // DLA_OPT_RUN_AHEAD
  int pending_blocks = 1;    // DLA_OPT_PENDING_BLOCKS
  long long n_global = -1;   // -1: single shard, n_global == n
  long long row0 = 0;
  std::vector<double> pending_p;   // dla_expand_project modes 3 / 4: the block [E ; T] the last call left pending ((m + k) x k, ld m + k)
  int pending_k = 0, pending_m = 0, pending_applied = 0;
  int agree_seq = 0;         // agreements on the shard layout this context has taken part in (agree_on_shards)
  int ref_depth = 0;         // nesting of entry points (reference-schedule flops are counted at the outermost one)
  std::string err;
  // pinned staging buffers for host-mode callbacks
  double* stage_x = nullptr;
  double* stage_y = nullptr;
  size_t stage_bytes = 0;
};
