/*
 * include/diaglib_amd.h -- C-ABI of the MI355X-native diaglib hot path.
 *
 * This is the drop-in boundary.  The reference (Molecolab-Pisa/diaglib)
 * is a Fortran module whose drivers do all O(n) work through BLAS calls on column-major
 * n x k panels (ld = n).  Here the Fortran drivers (diaglib_amd/fortran/diaglib.f90,
 * same public names and argument lists as reference diaglib.f90:166-167) keep only the
 * control flow and reach the device through the entry points below via ISO_C_BINDING.
 * Every entry point names the reference line(s) it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types.
 *   - "dev" pointers are device (HBM) addresses obtained from dla_alloc(); panels are
 *     column-major float64 with leading dimension n (the local row count), columns
 *     contiguous -- exactly the reference layout, so a block of columns can be handed
 *     to a matvec(n,m,x,ax) callback unchanged.
 *   - small matrices (<= lda x lda) live on the host, column-major.
 *   - every function returns 0 on success, a DLA_ERR_* code otherwise; nothing calls
 *     exit().  dla_last_error() gives the message.  The Fortran layer maps failures to
 *     the reference behaviour (ok=.false. / stop with the reference's message).
 *   - with a communicator (dla_comm_init) n is the LOCAL row count of this rank's shard;
 *     every reduction below is summed (or max-ed) over ranks before it is returned, so the
 *     callers are unchanged.
 */
#ifndef DIAGLIB_AMD_H
#define DIAGLIB_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dla_ctx dla_ctx;

enum {
  DLA_OK = 0,
  DLA_ERR_NO_DEVICE = 1,   /* no HIP device / extension not usable: fail loudly      */
  DLA_ERR_ALLOC = 2,       /* reference: check_mem, diaglib.f90:3789-3803            */
  DLA_ERR_ARG = 3,
  DLA_ERR_RUNTIME = 4,     /* a HIP/RCCL call failed                                  */
  DLA_ERR_ORTHO = 5,       /* reference: "catastrophic failure of ortho_vs_x", :3568  */
  DLA_ERR_LAPACK = 6,      /* reference: "dsyev failed", :412-415                     */
  DLA_ERR_COMM = 7
};

/* reference callback shapes, README.md:34-35 (F77 ABI: everything by reference) */
typedef void (*dla_matvec_fn)(const int* n, const int* m, const double* x, double* ax);
typedef void (*dla_precnd_fn)(const int* n, const int* m, const double* fac, const double* x, double* px);
/* linear-response preconditioner lrprec(n,m,fac,xp,xm,yp,ym): reference diaglib.f90:1317, callers main.f90:234-281 */
typedef void (*dla_lrprec_fn)(const int* n, const int* m, const double* fac, const double* xp, const double* xm,
                              double* yp, double* ym);

/* options for dla_set_option */
enum {
  DLA_OPT_CALLBACKS_ON_DEVICE = 1, /* 0 (default, drop-in): callbacks get HOST arrays, staged through pinned
                                      buffers; 1: callbacks get DEVICE addresses (SURVEY 8b "callback residency") */
  DLA_OPT_EVEC_ON_DEVICE = 2,      /* 0 (default): eig/evec of the drivers are host arrays as in the reference;
                                      1: evec is a device address (guess in, Ritz vectors out), eig stays host  */
  DLA_OPT_PROFILE = 3,             /* 1: bracket every kernel launch with HIP events (dla_get_stats)          */
  DLA_OPT_VERBOSE_ORTHO = 4,       /* 1: print ortho_cd/ortho_vs_x pass counts                                 */
  DLA_OPT_CALLBACK_ORDER = 5,      /* ordering contract of DEVICE-mode callbacks against the engine's stream (which is a
                                      non-blocking stream, dla_stream()):
                                      1 (default): host-synchronised -- the engine's stream is drained before the call
                                         and the whole device after it: correct for callbacks on ANY stream (hipfort,
                                         OpenMP target, torch, private streams) that do not synchronise themselves.
                                      0: stream-ordered, no host wait -- before the call the legacy null stream is made
                                         to wait for the engine's pending work, after the call the engine's stream
                                         waits for everything the callback enqueued on the null stream.  For callbacks
                                         that launch on the null stream only.
                                      2: none -- the callback promises to enqueue on dla_stream() only (the built-in
                                         operator does; it is always called this way).                              */
  DLA_OPT_ORTHO_MAXIT = 6,         /* iteration cap of ortho_cd / ortho_vs_x (reference parameter maxit = 10,
                                      diaglib.f90:3224,3521).  TEST knob: a small value makes ortho_cd give up so that
                                      the Householder-QR fallback `ortho` (diaglib.f90:3052-3092, 3534, 3549) runs */
  DLA_OPT_CASLR_ALGORITHM = 7,     /* reduced problem of caslr_driver: 0 (default) the 2 ldu-dimensional pencil (reference
                                      i_alg = 0, dsygv at diaglib.f90:783), 1 the Helmich-Paris route (i_alg = 1, :805-860) */
  DLA_OPT_STAGE_CHUNKS = 8,        /* host-mode callbacks: column chunks a block is cut into for the download | user routine |
                                      upload pipeline.  0 / 1 (default): the caller's routine sees every block once and whole,
                                      like the reference (diaglib.f90:1685, 1786); >= 2: that many chunks (at most 16) = that
                                      many calls per block, whose transfers overlap the routine's work on the neighbouring
                                      chunks -- pays only for an operator without fixed cost per call                       */
  DLA_OPT_P2P_TIMEOUT_MS = 9,      /* peer-to-peer all-reduce (dla_p2p_attach): how long a rank waits INSIDE a kernel for its peers'
                                      contributions, in ms (default 5000; 0 = no limit).  A rank that gives up marks the exchange
                                      as failed in every rank's mailbox: all ranks return DLA_ERR_COMM at their next host wait and
                                      the transport stays down until dla_p2p_detach + a fresh export.  Callers whose ranks can be
                                      further apart than this (host-mode callbacks of unequal length) raise it or use RCCL  */
  DLA_OPT_RUN_AHEAD = 10,          /* dla_expand_project: enqueue the operator and the projection sweep behind the
                                      orthogonalisation chain and read the chain's report at THEIR host wait.  When the chain
                                      takes another route than planned the operator is called a SECOND time on the finished
                                      block and its first output is dropped -- the reference calls matvec exactly once per
                                      block (diaglib.f90:1685, 394-397), so:
                                      1 (default): only for the library's own device operators (dla_synth_*, dla_spmm_matvec, dla_spmm_matvec_t, dla_spmm_bvec, dla_spmm_apbmul .. _smdmul, dla_dense_matvec, dla_dense_matvec_t, dla_dense_bvec, dla_dense_apbmul .. _smdmul),
                                         which are pure functions of their input; a caller's callback is called once, in order;
                                      2: also for the caller's device-mode callbacks (ordering contract 0 or 2) -- the caller
                                         states that the operator keeps no state between calls;
                                      0: never (one call after the other; A/B and debugging)                                  */
  DLA_OPT_PENDING_BLOCKS = 11,     /* dla_expand_project modes 3 / 4 (what the drivers call): 1 (default) the orthogonalisation chain may
                                      leave its closing projection and its last triangular factor to the caller's small matrices
                                      (dla_pending_block); 0: every block is finished in memory (modes 3 / 4 behave like 1 / 0) --
                                      same eigenpairs either way, for A/B runs and tests in one process.  New contexts start
                                      with 0 when $DIAGLIB_AMD_NO_PENDING is set                                              */
  DLA_OPT_TUNE0 = 100              /* 100..107: experiment knobs of the engine for the A/B tools, the fuzz tools and the tests;
                                      0 = the shipped default.  What each value selects: tools/README.md,
                                      "Interleaved A/B tools"                                                    */
};

/* op classes for statistics */
enum {
  DLA_OP_GRAM = 0,      /* C = X^T U                         */
  DLA_OP_GEMM = 1,      /* Z = X C   /  U -= X C             */
  DLA_OP_TRMM = 2,      /* U <- U L^-T                       */
  DLA_OP_RITZ = 3,      /* fused Ritz vectors + residuals    */
  DLA_OP_ELEM = 4,      /* copy / zero / axpy / fill         */
  DLA_OP_MATVEC = 5,    /* built-in operator                 */
  DLA_OP_PRECND = 6,    /* built-in preconditioner           */
  DLA_OP_COUNT = 7
};

typedef struct {
  long long launches[DLA_OP_COUNT];   /* kernel launches per class                          */
  double    alg_bytes[DLA_OP_COUNT];  /* algorithmic (compulsory) HBM bytes, SURVEY 8d      */
  double    flops[DLA_OP_COUNT];      /* reference-schedule flops, SURVEY 8d                */
  double    ms[DLA_OP_COUNT];         /* HIP-event time (only with DLA_OPT_PROFILE)         */
  long long allreduces;               /* cross-rank reductions issued                       */
  long long host_syncs;               /* stream synchronisations for host-visible results   */
  double    ref_flops;                /* reference-schedule flops of the LOGICAL operations the caller asked for (SURVEY 8d:
                                         what the reference's BLAS calls would execute for them), counted at the entry points --
                                         independent of what was launched, fused, left pending or skipped                 */
} dla_stats;

/* per-kernel statistics: name as rocprofv3 prints it (without namespace and argument list), launches,
 * algorithmic bytes and HIP-event time (DLA_OPT_PROFILE) */
typedef struct {
  char      name[96];
  long long launches;
  double    alg_bytes;
  double    ms;
  double    flops;       /* reference-schedule flops of the launches (what the BLAS calls they replace would execute) */
} dla_kernel_stat;

/* ---------------------------------------------------------------- context */
int  dla_create(dla_ctx** ctx, int device);          /* device < 0: $LOCAL_RANK or 0 */
int  dla_destroy(dla_ctx* ctx);
dla_ctx* dla_default_ctx(void);                      /* the context the Fortran drivers use: one per CALLING THREAD, created on
                                                        first use (own stream, scratch, panel cache, statistics and
                                                        options), so two host threads can solve at the same time.  The
                                                        reference cannot: module-level state, diaglib.f90:155-161 */
int  dla_set_option(dla_ctx* ctx, int option, int value);
/* A driver call starts (the Fortran drivers call it first): adaptive choices of the engine -- which sweep schedule the
 * orthogonalisation chains take, decided from what earlier chains of the SAME solve reported -- go back to their initial state, so
 * that a solve's results do not depend on the solves before it (repeated solves are bit-identical). */
int  dla_begin_solve(dla_ctx* ctx);
int  dla_get_option(dla_ctx* ctx, int option);
const char* dla_last_error(dla_ctx* ctx);
const char* dla_backend_name(dla_ctx* ctx);          /* "hip:gfx950" for the product */
int  dla_get_stats(dla_ctx* ctx, dla_stats* out);
int  dla_reset_stats(dla_ctx* ctx);
/* HIP-event time per kernel class since the last reset, ms[DLA_OP_COUNT] in the order of the DLA_OP_* ids (needs DLA_OPT_PROFILE = 1
 * while the work runs).  What the Fortran module's diaglib_amd_timings returns: the reference prints four buckets (matvec,
 * diagonalization, orthogonalization, total; diaglib.f90:1835-1841) and leaves projection / Ritz vectors / residuals un-bucketed. */
int  dla_class_times(dla_ctx* ctx, double* ms);
int  dla_get_kernel_stats(dla_ctx* ctx, dla_kernel_stat* out, int cap);   /* returns the number of entries */
void* dla_stream(dla_ctx* ctx);                      /* hipStream_t the kernels run on */

/* ---------------------------------------------------------------- multi-GPU */
int  dla_comm_unique_id(char id[128]);                                       /* ncclGetUniqueId          */
int  dla_comm_init(dla_ctx* ctx, int nranks, int rank, const char id[128]);  /* ncclCommInitRank         */
int  dla_comm_finalize(dla_ctx* ctx);                                        /* ncclCommDestroy          */
int  dla_comm_info(dla_ctx* ctx, int* nranks, int* rank);
/* One-shot peer-to-peer all-reduce for the small products, an alternative transport to RCCL for buffers
 * of at most 64 KB: every rank writes its contribution into a slot of every peer's mailbox (fine-grained device memory shared
 * through hipIpc), raises a flag and adds the slots of its own mailbox in rank order -- one xGMI hop, a fixed summation order
 * (bit-identical results on all ranks), no host involvement, and it takes part in the device-driven chains.
 *   1. every rank: dla_p2p_export(ctx, nranks, h)   -> 128 bytes (two hipIpcMemHandle_t)
 *   2. the caller's control plane (MPI, torch.distributed, ...) gathers the nranks x 128 bytes in rank order
 *   3. every rank: dla_p2p_attach(ctx, nranks, rank, all)
 * dla_p2p_detach closes the mailboxes and hands the small products back to the RCCL communicator / the hook (rank count and
 * rank stay); dla_comm_finalize detaches too.  Larger buffers and contexts without mailboxes use the communicator / the hook. */
int  dla_p2p_export(dla_ctx* ctx, int nranks, char handles[128]);
int  dla_p2p_attach(dla_ctx* ctx, int nranks, int rank, const char* all_handles);
int  dla_p2p_detach(dla_ctx* ctx);
/* host-buffer reduction hook (op 0 = sum, 1 = max); lets a caller supply the collective
 * (e.g. MPI or torch.distributed/gloo).  Used when no RCCL communicator is attached. */
typedef void (*dla_allreduce_fn)(void* user, double* buf, int count, int op);
int  dla_set_allreduce_hook(dla_ctx* ctx, dla_allreduce_fn fn, void* user, int nranks, int rank);
/* global rows of this rank: the shards are contiguous in rank order, rank r holds rows row0(r) .. row0(r + 1) - 1.  COLLECTIVE
 * once a transport is attached (and attaching a transport after the shard has been announced is collective in the same way):
 * the ranks exchange their row0 through the transport and agree on what schedule decisions may depend on -- a rank whose shard
 * has an odd number of rows would otherwise pick other sweeps than its peers and the exchanges would not pair up. */
int  dla_set_shard(dla_ctx* ctx, long long n_global, long long row0);

/* ---------------------------------------------------------------- device memory
 * replaces allocate/zero/dcopy of the panels: diaglib.f90:1607-1638,1648,1798-1805, 258-287 */
int  dla_alloc(dla_ctx* ctx, size_t bytes, void** dev);
int  dla_free(dla_ctx* ctx, void* dev);
/* Freed panels are kept for reuse (a driver call allocates the same GiB-sized panels every solve and hipMalloc of such
 * blocks costs tens of milliseconds); dla_trim hands the cached blocks back to the runtime (bytes released in *released,
 * may be NULL).  dla_destroy releases everything. */
int  dla_trim(dla_ctx* ctx, size_t* released);
int  dla_zero(dla_ctx* ctx, void* dev, size_t bytes);
int  dla_upload(dla_ctx* ctx, void* dev, const void* host, size_t bytes);
int  dla_download(dla_ctx* ctx, void* host, const void* dev, size_t bytes);
int  dla_copy(dla_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes);   /* dcopy on panels */
int  dla_sync(dla_ctx* ctx);

/* ---------------------------------------------------------------- block algebra */
/* C(l x k) = X(n x l)^T U(n x k), result on the host.  dgemm('t','n') at
 * diaglib.f90:1691 (projection), 3256 (ortho_cd Gram), 3543 (X^T U), 403/313 (LOBPCG S^T AS), 3762. */
int  dla_gram(dla_ctx* ctx, int n, int l, const double* x_dev, int k, const double* u_dev,
              double* c_host, int ldc);
/* Same for two n x l panels when the consumer reads only the LOWER triangle of C (LOBPCG: S^T AS at diaglib.f90:403
 * goes to dsyev('v','l') at :406): entries strictly above the 16 x 16 block diagonal are returned as zero. */
int  dla_gram_lower(dla_ctx* ctx, int n, int l, const double* x_dev, const double* u_dev, double* c_host, int ldc);
/* Z(n x k) = X(n x l) C(l x k).  dgemm('n','n') at diaglib.f90:1717, 420-424, 495-501, 322-324.
 * Z may be a column block of X itself when k <= 48 and 128*l*ceil(k/16) <= 65536 (one output pass, one
 * contraction chunk): every row tile is read completely before it is stored. */
int  dla_panel_gemm(dla_ctx* ctx, int n, int l, const double* x_dev, int k, const double* c_host, int ldc,
                    double* z_dev);
/* U(n x k) -= X(n x l) C(l x k).  dgemm('n','n',-one,...,one) at diaglib.f90:3544, 3633. */
int  dla_panel_update(dla_ctx* ctx, int n, int l, const double* x_dev, int k, const double* c_host, int ldc,
                      double* u_dev);
/* U <- U Linv^T with Linv lower triangular (k x k, host).  dtrmm('r','l','t','n') at diaglib.f90:3327. */
int  dla_trmm_linvt(dla_ctx* ctx, int n, int k, double* u_dev, const double* linv_host, int ld);
/* Fused Ritz step.  evec = V Y(:,1:m), r = AV Y(:,1:m); then for i < n_res with skip[i]==0:
 * r_i -= eig_i evec_i, rnorm[2i] = ||r_i||_2/sqrt(n_global), rnorm[2i+1] = max|r_i|.
 * avy_dev (may be NULL) also receives the uncorrected AV Y (LOBPCG's ax_new).  evec_dev may be NULL: the Ritz vectors are
 * then not written (8 n m bytes less) -- the Davidson driver asks for them only in sweeps after which somebody reads them
 * (convergence in sight, restart, last sweep).
 * diaglib.f90:1717-1732 (Davidson, n_res = n_targ) and 420-442 (LOBPCG, n_res = n_max). */
int  dla_ritz_residual(dla_ctx* ctx, int n, int l, int m, const double* v_dev, const double* av_dev,
                       const double* y_host, int ldy, const double* eig, int n_res, const int* skip,
                       double* evec_dev, double* r_dev, double* avy_dev, double* rnorm);
/* The same sweep with k2 extra products: p_dev = V C2, ap_dev = AV C2 (C2: l x k2, host).  LOBPCG forms its new P block
 * from the same two panels the Ritz step reads (diaglib.f90:495-501: P = S cp, AP = AS cp); with this entry they are read
 * once.  k2 = 0: exactly dla_ritz_residual. */
int  dla_ritz_residual_p(dla_ctx* ctx, int n, int l, int m, const double* v_dev, const double* av_dev,
                         const double* y_host, int ldy, const double* eig, int n_res, const int* skip,
                         double* evec_dev, double* r_dev, double* avy_dev, double* rnorm,
                         int k2, const double* c2_host, int ldc2, double* p_dev, double* ap_dev);
/* The sweep with TWO coefficient sets: e_dev = V Y1, r_dev = AV Y2, then for i < n_res with skip[i]==0: r_i -= eig_i e_i and the
 * norms as above.  The residual blocks of the linear-response drivers are of this shape -- rp = (A+B) vp u+ - w (S-D) vm u-
 * (diaglib.f90:872-889, 1337-1353: two dgemms on two panels with two coefficient blocks, then the daxpy / dnrm2 loop).
 * t_work_dev, junk_dev: n x m scratch blocks (used only for shapes the one-sweep kernel does not take: m > 48). */
int  dla_ritz_residual2(dla_ctx* ctx, int n, int l, int m, const double* v_dev, const double* av_dev,
                        const double* y1_host, int ldy1, const double* y2_host, int ldy2, const double* eig, int n_res,
                        const int* skip, double* e_dev, double* r_dev, double* t_work_dev, double* junk_dev, double* rnorm);
/* dla_ritz_residual that may also form the next Davidson block inside the same sweep, from a PREDICTION of the first open root:
 * u0_dev(:, 1:k) = precnd(r(:, first:m), fac) with k = m - first + 1 (first is 1-based), and [V | u0]^T u0 measured for the
 * orthogonalisation of that block.  The sweep runs fused (*fused = 1) only when precnd is one of the library's diagonal
 * preconditioners on a device-resident diagonal (dla_synth_precnd, dla_spmm_precnd, dla_dense_precnd), callbacks are in device
 * mode, no Ritz vectors and no AV Y are asked for (evec_dev = avy_dev = NULL), the context is not sharded and the shape fits the
 * kernel (even n, 16-byte aligned panels, m <= 16, l <= 112 under the full LDS limit).  r_dev and rnorm come out as from
 * dla_ritz_residual (the same products and the same correction, step by step), u0_dev
 * holds EXACTLY the library's diagonal rule applied to the stored r_dev, and a dla_expand_project / dla_ortho_vs_x that follows on
 * the panel [v_dev | u0_dev] with the same widths, with nothing launched in between, starts from the measured matrices instead of
 * sweeping the basis again.  A caller whose prediction was wrong simply goes on as after dla_ritz_residual (dla_call_precnd on
 * r_dev overwrites the block).  In every other case (*fused = 0) the call is exactly dla_ritz_residual and u0_dev is not
 * touched. */
int  dla_ritz_expand(dla_ctx* ctx, int n, int l, int m, const double* v_dev, const double* av_dev,
                     const double* y_host, int ldy, const double* eig, int n_res, const int* skip,
                     double* evec_dev, double* r_dev, double* avy_dev, double* rnorm,
                     dla_precnd_fn precnd, double fac, int first, int k, double* u0_dev, int* fused);
/* fused sweeps of dla_ritz_expand that ran on this context, and how many of them were discarded (nobody took what they measured:
 * the prediction missed, or another call came between the sweep and the orthogonalisation) */
int  dla_ritz_expand_counts(dla_ctx* ctx, long long* run, long long* discarded);
/* What the last fused sweep measured, while it is still on record: xug(1:m, 1:k) = V^T u0 and xug(m+1:m+k, 1:k) = u0^T u0 (host,
 * leading dimension ld >= m + k), reduced exactly as the orthogonalisation chain reduces them.  The record stays.  For tests. */
int  dla_ritz_expand_measured(dla_ctx* ctx, int m, int k, double* xug, int ld);
/* Expansion step of the Davidson and LOBPCG drivers on the contiguous panels basis = [X | U] (n x (m+k)) and
 * abasis = [AX | AU]:   ortho_vs_x(X, U)  (diaglib.f90:1790, 358-366, 523-529),  AU = A U [+ shift U]  (the caller's matvec,
 * :1685, 394-397; daxpy :397)  and the projection --
 *   mode 0 (Davidson, :1691):  h(1:m+k, 1:k) = [X | U]^T AU, the new columns of the projected matrix;
 *   mode 1 (LOBPCG, :401-403): h = lower triangle of [X | U]^T [AX | AU], (m+k) x (m+k).
 * Same result as dla_ortho_vs_x + dla_call_matvec (+ dla_axpy) + dla_gram / dla_gram_lower.  With device-mode callbacks
 * that need no host wait (DLA_OPT_CALLBACK_ORDER 0 or 2) the three are enqueued back to back and the chain's report is
 * read at the projection's host wait: one wait per expansion instead of two.  When the chain did not end with the planned
 * launches (first call of a shape, or a block that needs more passes than the previous one of its width) the
 * orthogonalisation is completed and the operator and the projection are simply repeated on the finished block -- the
 * operator must therefore be a pure function of its input (it is called a second time for the same block then). */
int  dla_expand_project(dla_ctx* ctx, int mode, int n, int m, int k, double* basis_dev, double* abasis_dev,
                        dla_matvec_fn matvec, double shift, double* h_host, int ldh);
/* mode 3 = mode 1 for a block that is used once and then rebuilt -- LOBPCG's W block (diaglib.f90:518-529, 394-403).  The device
 * chain ends as soon as it holds S = X^T U and G = U^T U MEASURED on the stored block together with the converged factor T of G
 * (T^T G T = I): the reference's closing pass -- U -= X S (:3543-3544), one macro-iteration of ortho_cd with a near-identity factor
 * (:3256-3327) -- is then a matter of coefficients.  The finished block is [X | U_stored] p with p = [E ; T'] ((m + k) x k), formed on
 * the host from what the chain hands over: E = -S T R, T' = T R with the k x k factor R that makes the projected block orthonormal
 * (its Gram matrix is I - (S T)^T (S T): G was measured before the projection).  h_host is the projection for the FINISHED block
 * (D^T H D with D = [I E ; 0 T']); the caller multiplies every coefficient block by D before it forms products with the panel
 * (S [y | cp] = S_stored D [y | cp]).  dla_pending_block returns p of the last mode-3 / mode-4 call ([0 ; I] when nothing stayed
 * pending: host-driven loops, a chain that had to finish in memory); dla_pending_factor returns its T' part.
 * mode 4 = mode 0 for a block that STAYS in the basis (Davidson): the same, but h_host comes back RAW, for the stored block, and
 * dla_pending_block returns the chain's own [-S T ; T] -- the caller keeps the pending blocks of its whole basis in an upper-
 * triangular D and dla_basis_admit completes the closing pass against the FINISHED basis X_stored D (E = -D D^T S T: the stored
 * columns are not orthonormal, X_stored^T X_stored = (D D^T)^-1), records the block in D and turns the raw columns into those of
 * D^T H D; dla_basis_fold multiplies coefficient rows by D.  A block that stays in the basis must keep later device projections
 * against the stored columns effective (the block that comes out of a first projection can be as ill-conditioned as 1e7: what the
 * projection leaves behind has to stay below its smallest directions): the projection part stays pending only for max |S| < 1e-9,
 * the factor only for max |G - I| < 1e-8 -- otherwise the factor is applied in memory (U <- U T, nothing of X is read) or the chain
 * finishes the block there.  (mode 3: max |S| < 1e-4; the block is rebuilt in the next iteration.)  *applied = 1 (mode 4, for
 * 1e-9 <= max |S| < 1e-5): the chain's closing sweep HAS applied [-S T ; T] to the block in memory, without measuring anything behind
 * it -- the block in memory is what h_host belongs to, and dla_basis_admit owes it only the difference to the exact closing pass and
 * the k x k factor of its Gram matrix I - (S T)^T (S T).
 * mode 5 = mode 4 with the caller's D kept on the DEVICE as well (dla_basis_sync after every block, blocks of at most 16 columns, at
 * most 320 basis columns): every projection of the chain is then X (D D^T) X^T U, exact against the finished basis, and the bounds
 * on what may stay pending are those of the host algebra alone -- max |S| < 0.05 with column sums of squares below 0.02, nothing on
 * G (its factor has converged) -- so the chain ends behind the first sweep that has measured S and G on what it stored.  Where the
 * device-driven chain cannot project exactly (an all-reduce hook, the A/B knobs for the host loop, a block wider than 16 columns,
 * an engine whose LDS limit went down after a refused request -- which can happen between two calls of one solve) the block is
 * finished in memory and dla_pending_block answers [0 ; I]: by mode 0 when the copy of D says the m stored columns are finished
 * (D = I there), by the host-driven loop with every X^T U multiplied by D D^T when they are not -- never by a plain projection
 * against unfinished columns.  The call fails (DLA_ERR_ARG) when the copy does not describe the m columns in front of the block.
 * The engine's HOST copy of D has no width limit: a basis with pending blocks that grows beyond the 320 columns of the device copy
 * goes on with blocks finished in memory by the host-driven loop (slower: one host wait per operation; exact).
 * mode 6 = the block is finished in memory against the finished basis X D whatever the device could do (host-driven loop with D D^T),
 * operator and projection on the result, nothing pending: the way out for a caller whose dla_basis_admit answered DLA_ERR_ORTHO (the
 * closing factor I - F^T F of the pending block was not positive definite) -- called on the same block, which is still what the
 * chain stored.  The operator is called a second time for that block.
 * (Mode 4's bounds cost later blocks a projection each time they remove more than 1e-8 from a block -- every chain of such a basis ends
 * on a measured product below that --, so the drivers use mode 5 where it is available and mode 0 elsewhere; mode 4 stays for callers
 * that keep D on the host only.) */
int  dla_pending_factor(dla_ctx* ctx, int k, double* t_host, int ldt);
int  dla_pending_block(dla_ctx* ctx, int m, int k, double* p_host, int ldp, int* applied);
/* Host-size algebra of a basis with pending blocks (no device work; all arrays column-major, leading dimension ld):
 * dla_basis_admit: a block of k columns came in behind m stored ones with the chain's pending block p (in: [-S T ; T], out: the
 * completed [E ; T']); columns m .. m+k-1 of h hold the raw product [X | U]_stored^T A U_stored (reference :1691 on the stored
 * block).  Records them in hraw (both triangles) and p in the upper-triangular dmat, and replaces the columns of h by those of
 * dmat^T hraw dmat.  dla_basis_fold: c <- dmat(0:rows,0:rows) c. */
int  dla_basis_admit(int m, int k, double* p_host, int ldp, int applied, double* hraw, double* dmat, double* h, int ld);
int  dla_basis_fold(int rows, int ncol, const double* dmat, int ld, double* c, int ldc);
/* The engine's copy of the caller's D for dla_expand_project mode 5 (on the device for the first 320 columns, on the host for all of
 * them): columns m .. m+k-1 of dmat (upper triangular, leading dimension ld; rows 0 .. m+k-1 are read) follow the m columns sent so
 * far -- blocks arrive in order, every block of the basis, identity ones included; k <= 0 forgets everything (new solve, restart).
 * Asynchronous: the host array may be changed when the call returns. */
int  dla_basis_sync(dla_ctx* ctx, int m, int k, const double* dmat, int ld);
/* The expansion step with a metric B (gen_david_driver diaglib.f90:2170-2190, lobpcg_driver with gen_eig :523-529): on
 * basis = [X | U], bbasis = [BX | BU], abasis = [AX | AU]:  b_ortho_vs_x(X, BX, U) (:3576-3663),  BU = B U (the caller's bvec),
 * b_ortho(U, BU) (:3094-3183),  AU = A U [+ shift U],  and the projection as in dla_expand_project (mode 0 / 1).  Same result as
 * the separate entry points.  With device-mode callbacks that may run ahead (DLA_OPT_RUN_AHEAD) all of it is enqueued behind
 * the orthogonalisation chain -- the k x k factorisation of b_ortho runs on the device and only behind a chain that ended
 * well -- and one host wait serves the whole step (three with the separate calls).
 * "Same result": the same block as the separate calls up to rounding -- b_ortho's Cholesky-QR gives the same Q for U and for U W
 * (W upper triangular, positive diagonal), so inside this entry the device chain does not apply its last pending factor
 * (16 n k bytes less); dla_b_ortho_vs_x called on its own does.
 * mode 2: b_ortho_vs_x, bvec, b_ortho and nothing else (abasis, matvec, h_host unused, may be NULL): the expansion of
 * caslr_eff_driver, whose new blocks are orthogonalised against the basis in the metric (A+B) resp. (A-B), get their metric
 * image and are made orthonormal in it (diaglib.f90:1397-1424) -- bvec is apbmul resp. ambmul there. */
int  dla_expand_project_metric(dla_ctx* ctx, int mode, int n, int m, int k, double* basis_dev, double* bbasis_dev, double* abasis_dev,
                               dla_matvec_fn matvec, dla_matvec_fn bvec, double shift, double* h_host, int ldh);
/* y += alpha x over len contiguous doubles.  daxpy at diaglib.f90:312,397 (LOBPCG shift). */
int  dla_axpy(dla_ctx* ctx, size_t len, double alpha, const double* x_dev, double* y_dev);
/* sqrt(sum x^2) over len contiguous doubles (all ranks).  dnrm2 at diaglib.f90:3749, 3268. */
int  dla_nrm2(dla_ctx* ctx, size_t len, const double* x_dev, double* out);
/* measurement aid (SURVEY 8d "measured device-triad GB/s as the practical ceiling"): STREAM triad a = b + s c on three
 * scratch arrays of len doubles with the sweeps' access shape, best of reps repetitions, in GB/s (24 bytes per element) */
int  dla_stream_triad(dla_ctx* ctx, size_t len, int reps, double* gbps);
/* fill evec(n x m) with the documented counter-based uniform [0,1) stream (replaces the
 * compiler-specific random_number at diaglib.f90:3754). */
int  dla_random_fill(dla_ctx* ctx, int n, int m, double* evec_dev);
/* evec(i,j) = u01(seed, global row i, j) - 0.5: the "hard" benchmark guess (SURVEY.md 8d guess (b), seed 2); the role of
 * guess_evec mode 4 in the reference harness (main.f90:1362-1367), with a generator that does not depend on the compiler.
 * support_rows > 0 restricts the random entries to the leading support_rows GLOBAL rows (zero below): on the benchmark
 * operator (diagonal 2..n+1) a guess spread over all of n >= 1e6 rows starts at Rayleigh quotients ~n/2 and needs
 * thousands of iterations (measured: 400 iterations at n = 1e7 leave the lowest Ritz value at 4.4e6), so the large
 * restart/locking runs confine it to as many rows as the reference's own toy problem has (main.f90:14: n = 1000..2000). */
int  dla_fill_guess(dla_ctx* ctx, int n, int m, double* evec_dev, unsigned long long seed, long long support_rows);

/* ---------------------------------------------------------------- orthogonalisation */
/* ortho_cd(n,m,u,growth,ok), diaglib.f90:3185-3341: Cholesky-QR with refinement and the level-shift ladder; growth = product of
 * the norm estimates of the inverse factors, ok = 0 when the iteration cap was reached (the reference prints and returns) */
int  dla_ortho_cd(dla_ctx* ctx, int n, int k, double* u_dev, double* growth, int* ok);
/* Fused sweeps of the orthogonalisation loops (one pass over the panel instead of two), as the engine runs them inside
 * ortho_cd / ortho_vs_x; entry points of their own so that each can be checked against the BLAS pair it replaces:
 *   dla_trmm_gram    U <- U W (k x k, general W; dtrmm at diaglib.f90:3327)          and G = U^T U of the result (:3256)
 *   dla_update_gram  U <- U - X C (dgemm at :3544)                                   and G = U^T U of the result
 *   dla_combo_gram   U <- [X | U] C' (C' is (m+k) x k; U follows X in one panel, k <= 48) and G = U^T U of the result:
 *                    the pending triangular factor folded into the projection, X^T (U W) = (X^T U) W
 * G (k x k, host, ld = ldg) comes back complete (symmetric). */
int  dla_trmm_gram(dla_ctx* ctx, int n, int k, double* u_dev, const double* w_host, int ldw, double* g_host, int ldg);
int  dla_update_gram(dla_ctx* ctx, int n, int l, const double* x_dev, int k, const double* c_host, int ldc, double* u_dev,
                     double* g_host, int ldg);
int  dla_combo_gram(dla_ctx* ctx, int n, int m, const double* x_dev, int k, const double* c_host, int ldc, double* u_dev,
                    double* g_host, int ldg);
/* ortho(n,m,u,w), diaglib.f90:3052-3092: Householder QR of a copy (dgeqrf) and U <- U R^-1 (dtrsm) -- the orthonormal factor
 * with LAPACK's sign convention for diag(R).  The reference calls it when ortho_cd gives up (:3534, :3549).  Device path:
 * column-wise Gram-Schmidt for the factor, the Householder recurrence on an isometric 2k x k host matrix for the signs. */
int  dla_ortho_qr(dla_ctx* ctx, int n, int k, double* u_dev);
int  dla_ortho_vs_x(dla_ctx* ctx, int n, int m, int k, const double* x_dev, double* u_dev); /* diaglib.f90:3481-3574 */
int  dla_b_ortho(dla_ctx* ctx, int n, int m, double* u_dev, double* bu_dev);                /* diaglib.f90:3094-3183 */
int  dla_b_ortho_vs_x(dla_ctx* ctx, int n, int m, int k, const double* x_dev, const double* bx_dev,
                      double* u_dev);                                                       /* diaglib.f90:3576-3663 */
int  dla_check_guess(dla_ctx* ctx, int n, int m, double* evec_dev);                         /* diaglib.f90:3734-3786 */
/* host-size coefficient step of LOBPCG, diaglib.f90:3686-3732 (arrays on the host) */
int  dla_get_coeffs(dla_ctx* ctx, int len_a, int len_u, int n_max, int n_act, const double* a_red,
                    double* u_x, double* u_p);

/* ---------------------------------------------------------------- user callbacks
 * call matvec(n,m,x,ax) / precnd(n,m,fac,x,px) on blocks of device panels
 * (diaglib.f90:1685,1786, 309,352,394,518).  Host-callback mode stages through pinned memory. */
int  dla_call_matvec(dla_ctx* ctx, dla_matvec_fn fn, int n, int m, const double* x_dev, double* ax_dev);
int  dla_call_precnd(dla_ctx* ctx, dla_precnd_fn fn, int n, int m, double fac, const double* x_dev, double* px_dev);
/* call lrprec(n,m,fac,xp,xm,yp,ym) (diaglib.f90:1317) on two device blocks, staging through pinned memory in host mode */
int  dla_call_lrprec(dla_ctx* ctx, dla_lrprec_fn fn, int n, int m, double fac, const double* xp_dev, const double* xm_dev,
                     double* yp_dev, double* ym_dev);

/* ---------------------------------------------------------------- small dense, host (LAPACK in the reference) */
int    dla_syev(char uplo, int n, double* a, int lda, double* w);   /* dsyev('v',uplo): :315,406,1708 */
int    dla_syev_lowest(char uplo, int n, double* a, int lda, double* w, int m); /* same call sites: only the m
                                                                       lowest eigenPAIRS are formed (all the drivers use) */
int    dla_potrf_lower(int m, double* a, int lda);                  /* dpotrf('l'): :3261             */
int    dla_trtri_lower(int m, double* a, int lda);                  /* dtrtri('l','n'): :3310         */
double dla_norm_est(int m, const double* a, int lda);               /* norm_est: :3447-3479           */
/* dgeev('v','v') of the non-symmetric driver (:2499): all eigenvalues wr + i wi and the right (vr) and left (vl, u^H A = lambda u^H)
 * eigenvectors of the general n x n matrix a, which is destroyed.  dgeev's conventions: conjugate pairs are consecutive, the one
 * with positive imaginary part first; column j is the vector of a real eigenvalue, columns j and j+1 are the real and imaginary
 * parts of the vector of the first member of a pair (the second member's is its conjugate); every vector has Euclidean norm 1
 * and its component of largest magnitude is real (and, here, positive).  Hessenberg reduction, shifted double-step QR, vectors
 * by back-substitution; no balancing; the left vectors come from a second run on the transpose, its eigenvalues matched to the
 * first run's.  Returns DLA_ERR_LAPACK when an eigenvalue has not deflated after 30 n sweeps, -1 for a bad argument. */
int    dla_geev(int n, double* a, int lda, double* wr, double* wi, double* vl, int ldvl, double* vr, int ldvr);

/* ---------------------------------------------------------------- built-in device operator (bench / tests)
 * A = diag(i+1) + sigma W W^T, W(i,j) = (2 u01(1,i,j)-1)/sqrt(i), i = 1-based global row;
 * preconditioner = main.f90:146-171 (mprec) semantics.  The two callbacks have the reference's shape
 * and expect DEVICE addresses (use with DLA_OPT_CALLBACKS_ON_DEVICE = 1). */
int  dla_synth_setup(dla_ctx* ctx, long long n_global, long long row0, int n_local, int rank_w, double sigma);
void dla_synth_matvec(const int* n, const int* m, const double* x_dev, double* ax_dev);
void dla_synth_precnd(const int* n, const int* m, const double* fac, const double* x_dev, double* px_dev);
/* Sample operators for the linear-response and generalised drivers around the same W (after dla_synth_setup; device addresses,
 * reference callback shapes: apbmul / ambmul / spdmul / smdmul of diaglib.f90:1024-1025, bvec of :1855, lrprec of :1317):
 *   y = d(i) x + W C W^T x :  A+B: d = i+5, C = sigma I;  A-B: d = i+2, C = 0.2 sigma I (the harness' diagonals, main.f90:563,570);
 *   S+D / S-D: d = s(i) = 1 + 0.5/(1 + i mod 7), C = +-0.05 J with J antisymmetric (D = 0.05 W J W^T);  metric: d = s(i), C = 0.1 I.
 * lrprec1 / lrprec2 = the harness' lrprec_1 / lrprec_2 (main.f90:234-281) on the diagonals of these operators. */
void dla_synth_apbmul(const int* n, const int* m, const double* x_dev, double* y_dev);
void dla_synth_ambmul(const int* n, const int* m, const double* x_dev, double* y_dev);
void dla_synth_spdmul(const int* n, const int* m, const double* x_dev, double* y_dev);
void dla_synth_smdmul(const int* n, const int* m, const double* x_dev, double* y_dev);
void dla_synth_metric(const int* n, const int* m, const double* x_dev, double* y_dev);
void dla_synth_lrprec1(const int* n, const int* m, const double* fac, const double* xp_dev, const double* xm_dev, double* yp_dev, double* ym_dev);
void dla_synth_lrprec2(const int* n, const int* m, const double* fac, const double* xp_dev, const double* xm_dev, double* yp_dev, double* ym_dev);

/* ---------------------------------------------------------------- drivers (Fortran, bind(C) twins of the
 * module procedures davidson_driver / gen_david_driver / lobpcg_driver; argument meaning as reference
 * diaglib.f90:1483-1539 and 171-228; logicals as int 0/1) */
void dla_davidson_driver(int verbose, int n, int n_targ, int n_max, int max_iter, double tol, int max_dav,
                         double shift, dla_matvec_fn matvec, dla_precnd_fn precnd,
                         double* eig, double* evec, int* ok);
void dla_gen_david_driver(int verbose, int n, int n_targ, int n_max, int max_iter, double tol, int max_dav,
                          double shift, dla_matvec_fn matvec, dla_precnd_fn precnd, dla_matvec_fn bvec,
                          double* eig, double* evec, int* ok);      /* reference diaglib.f90:1855-2250 */
void dla_lobpcg_driver(int verbose, int gen_eig, int n, int n_targ, int n_max, int max_iter, double tol,
                       double shift, dla_matvec_fn matvec, dla_precnd_fn precnd, dla_matvec_fn bvec,
                       double* eig, double* evec, int* ok);
/* linear-response problem (A B; B A)(Y Z) = w (S D; -D -S)(Y Z): reference diaglib.f90:1024-1481 (caslr_eff_driver).
 * evec is 2n x n_max (Y on top of Z); the four operators have the matvec shape and apply A+B, A-B, S+D, S-D. */
void dla_caslr_eff_driver(int verbose, int n, int n_targ, int n_max, int max_iter, double tol, int max_dav,
                          dla_matvec_fn apbmul, dla_matvec_fn ambmul, dla_matvec_fn spdmul, dla_matvec_fn smdmul,
                          dla_lrprec_fn lrprec, double* eig, double* evec, int* ok);
/* same problem, traditional solver: reference diaglib.f90:558-1022 (caslr_driver, its default algorithm i_alg = 0) */
void dla_caslr_driver(int verbose, int n, int n_targ, int n_max, int max_iter, double tol, int max_dav,
                      dla_matvec_fn apbmul, dla_matvec_fn ambmul, dla_matvec_fn spdmul, dla_matvec_fn smdmul,
                      dla_lrprec_fn lrprec, double* eig, double* evec, int* ok);
/* non-symmetric Davidson: reference diaglib.f90:2252-2943 (nonsym_driver).  matvec applies A, matvec_l its transpose; side is the
 * character code of 'r' (right eigenvectors), 'l' (left), 'c' (right, then left from the right ones; 's' is taken as 'c'); eig is
 * returned with the shift in it; after 'c' the columns of evec_l and evec_r are biorthonormal bases of the two invariant subspaces
 * (L^T R = I), not individual eigenvectors.  The solve report counts both passes. */
void dla_nonsym_driver(int verbose, int n, int n_targ, int n_max, int max_iter, double tol, int max_dav, double shift,
                       dla_matvec_fn matvec, dla_matvec_fn matvec_l, dla_precnd_fn precnd,
                       double* eig, double* evec_r, double* evec_l, int side, int* ok);
/* iteration report of the last driver call (iterations, matvec columns, restarts) */
void dla_last_solve_info(int* iters, int* matvec_cols, int* restarts);
void dla_set_solve_info(int iters, int matvec_cols, int restarts);   /* used by the Fortran drivers */

/* ---------------------------------------------------------------- sample sparse operator
 * A device-resident operator for callers whose matrix is sparse and symmetric: hand A over once in CSR form (host arrays,
 * 0-based, 64-bit row pointers); it is kept on the device as column-major ELLPACK or, on request, as sliced ELLPACK with a CSR
 * tail (below).  dla_spmm_matvec / dla_spmm_precnd have the
 * reference's callback shapes matvec(n,m,x,ax) / precnd(n,m,fac,x,px) (README.md:34-35, main.f90:72-90, 146-171) and expect
 * DEVICE addresses (DLA_OPT_CALLBACKS_ON_DEVICE = 1); the preconditioner is the harness' x / (a_ii + fac).  They act on the
 * operator the calling thread set up last and enqueue on that context's stream.
 * Row shards (dla_spmm_setup_csr_sharded): every rank hands over ITS rows row0 .. row0 + n_local - 1 with GLOBAL 64-bit column
 * indices.  The columns of a shard may reach at most `halo` rows into the two neighbouring shards (a banded matrix; halo is the
 * largest reach of any rank, agreed at setup, at most 4096 and at most a shard's height); each product then exchanges the first
 * and last `halo` rows of every rank's x block through the SAME transport as the small products -- every rank fills its own two
 * slots of a zeroed nranks x 2 x halo x m buffer and the all-reduce sum gathers them (all-reduce only; 2 halo m
 * doubles per rank and call) -- and a matrix with longer-range couplings is refused.  Collective: every rank calls the setup,
 * with shards contiguous in rank order; with one rank it equals dla_spmm_setup_csr.
 * Storage formats (dla_spmm_setup_csr_fmt, single rank): ELLPACK pads every row to the WIDEST one -- ideal for stencils and
 * bands, unusable when a few rows are long (one dense row at n = 20 000 costs 4.8 GB).  DLA_SPMM_SELL stores sliced ELLPACK
 * instead: rows sorted by descending length inside windows of sort_window rows, slices of slice_rows consecutive slots padded to
 * their own longest row, and rows above long_row_threshold entries kept whole in a CSR tail -- storage and traffic follow the
 * non-zeros.  Rows that are not in the tail come out with the same bits as from ELLPACK (same order of accumulation); repeated
 * products are bit-identical in both formats.  DLA_SPMM_AUTO takes ELLPACK while its padding (widest row x n / nnz) is at most
 * 1.25 and SELL otherwise.  The two callbacks serve whichever format was set up last; a refused setup replaces nothing.
 * dla_spmm_setup_csr is always ELLPACK, and dla_spmm_setup_csr_sharded stays ELLPACK plus halo: sharding the sliced format is
 * out of scope here.
 * How a tail row is summed (the contract; SEG = long_segment_entries, a positive multiple of 64).  A tail row with entries
 * [p0, p1) in the caller's order has S = ceil((p1 - p0) / SEG) segments, segment s covering [p0 + s SEG, min(p1, p0 + (s + 1) SEG)),
 * and one wavefront of 64 lanes forms the partial of one segment, per right-hand side: lane l starts from 0.0 and takes the
 * segment's entries l, l + 64, l + 128, ... in that order, one fma(value, x[col], acc) each; then for off = 32, 16, 8, 4, 2, 1 every
 * lane does acc += acc of lane (l xor off); lane 0's value is the partial.  With S = 1 the partial is the row's result (every
 * tail row of up to SEG entries).  With S > 1 the result is ((part_0 + part_1) + part_2) + ..., plain double additions in ascending
 * segment order by one thread per (row, right-hand side), from a workspace of multi_segments x m doubles that belongs to the
 * stored matrix (the operator and the metric each have their own; it grows with m and is not counted in device_bytes).  No
 * atomics and no arrival order anywhere: every element of the result and of the workspace has exactly one writer, so repeated
 * products are bit-identical, and every row stays within (len + 2) eps |A||x| of the exact product.
 * The metric of a generalised problem A x = lambda B x (dla_spmm_setup_metric_csr, single rank): a context keeps a second sparse
 * matrix B beside its operator, handed over the same way and stored in any of the formats above.  dla_spmm_bvec has the shape of
 * the reference's bvec(n,m,x,bx) (diaglib.f90:1855, gen_david_driver; the harness' smult, main.f90:115-144) and goes where a host
 * bvec would go in gen_david_driver and lobpcg_driver(gen_eig = .true.), so that a whole generalised solve stays in HBM.  It runs
 * the kernels dla_spmm_matvec runs: B x comes out with the bits the operator slot gives for the same matrix in the same format.
 * A and B are independent storage with independent formats: setting, replacing or dropping one never touches the other's blocks
 * or results, a refused setup replaces nothing, and dla_spmm_info keeps describing A only (dla_spmm_metric_info describes B).
 * dla_spmm_precnd stays the harness' x / (a_ii + fac), which the reference harness passes for the generalised problem too
 * (main.f90:491-492, 511-512); dla_spmm_precnd_pencil divides by the diagonal of the pencil, a_ii + fac b_ii, instead and needs
 * both matrices with the same n.  A callback that finds its matrix missing, or another n, fails through the status of
 * dla_call_matvec / dla_call_precnd with a message that names it.  A row-sharded metric is out of scope: the metric is refused
 * on a context whose operator came from dla_spmm_setup_csr_sharded, and that setup is refused while a metric is present.
 * Arrays that are already in device memory (dla_spmm_setup_csr_dev, single rank; which = 0: the operator A, 1: the metric B), for
 * callers that assemble on the GPU: the three arrays are DEVICE addresses of the layout above (rowptr n + 1 x int64, colind nnz x
 * int32, values nnz x double, 0-based).  The result is exactly what dla_spmm_setup_csr_fmt / dla_spmm_setup_metric_csr give for the
 * same arrays and format: dla_spmm_info / dla_spmm_metric_info equal field by field, and every later dla_spmm_matvec, dla_spmm_bvec,
 * dla_spmm_precnd and dla_spmm_precnd_pencil returns the same bits; diag[i] is the sum of the (i, i) entries in the caller's order,
 * duplicates and tail rows included.  Only the row pointers travel to the host (8 (n + 1) bytes), where the layout is decided as
 * for host arrays; the entries are checked, rearranged and summed by kernels.  Synchronous: the arrays are read on the context's
 * stream (dla_stream) and the call returns after that stream has been waited for, so the caller may free or overwrite them
 * afterwards; the caller is responsible for its own producer of the arrays having finished before the call (the library does not
 * know the stream they were written on).  Refused (DLA_ERR_ARG, the message names dla_spmm_setup_csr_dev) like the host entries:
 * null pointers, n <= 0, an unknown format, descending row pointers, an empty matrix, a column outside [0, n), which not 0 or 1,
 * and a metric on a row-sharded operator.  Every check that reads the entries has finished before the slot's blocks are written
 * or grown: after a refused call the products of the slot's previous matrix are bit-unchanged.
 * New values for the same pattern (dla_spmm_refresh_values_dev), for callers whose matrix changes per outer iteration while its
 * pattern does not: rewrites only the stored values and the diagonal of slot `which`, in the stored format (AUTO is not decided
 * again; the slot may have been set up from host or device arrays).  Afterwards the slot equals, bit for bit, a fresh set-up of
 * the same arrays in that format.  Refused with DLA_ERR_ARG when the slot is empty, when it is row-sharded, when n or the number
 * of entries differs from the stored one, or when the pattern -- the length of every row and every column index, in the caller's
 * order -- is not the stored one; the pattern is compared in a read-only pass before anything is written, so a refused refresh
 * leaves values and diagonal as they were.  Synchronous like the set-up, with the same rule for the caller's producer.
 * The parts of a linear-response problem (A B; B A)(Y Z) = w (S D; -D -S)(Y Z) (dla_spmm_setup_lr_csr, single rank): a context
 * keeps four more sparse matrices beside A and B -- part DLA_SPMM_LR_APB = A+B, _AMB = A-B, _SPD = S+D, _SMD = S-D -- each handed
 * over like the operator and stored in any of the formats above, with its own diagonal and its own tail workspace.
 * dla_spmm_apbmul / _ambmul / _spdmul / _smdmul have the shape of the reference's apbmul / ambmul / spdmul / smdmul (diaglib.f90:
 * 1024-1025) and dla_spmm_lrprec1 / _lrprec2 the shape of its lrprec (diaglib.f90:1317), so that caslr_eff_driver and caslr_driver
 * run a whole solve in HBM on the caller's matrices.  The four products run the kernels dla_spmm_matvec runs: for the same arrays
 * and format they return the bits the operator slot gives.  No matrix is assumed symmetric, here or in the operator and the metric:
 * every kernel multiplies row i by the entries handed over for row i (S+D and S-D are not symmetric).  dla_spmm_lrprec1 / _lrprec2
 * are the harness' lrprec_1 / lrprec_2 (main.f90:234-281) on the stored diagonals, with aa = 0.5 * (apb_ii + amb_ii) and
 * sg = spd_ii (S-D is not read):
 *   lrprec1: den = -1 / (aa*aa - fac*fac*sg*sg),  yp = den * (aa*xp + fac*sg*xm),      ym = den * (aa*xm + fac*sg*xp)
 *   lrprec2: den =  1 / (fac*fac*aa*aa - sg*sg),  yp = den * (fac*aa*xp + sg*xm),      ym = den * (fac*aa*xm + sg*xp)
 * evaluated in double precision with products taken left to right and no fused multiply-add: the bits a host caller gets from
 * the same expressions.  The parts are independent of each other and of A and B: setting, replacing or dropping one never changes
 * another slot's blocks, its info or the bits of its products, and a refused set-up replaces nothing.  Every rule above for A / B
 * holds for a part: dla_spmm_setup_lr_csr_dev gives the host set-up's result field by field and bit by bit, every check finishes
 * before any write, the calls are synchronous, and dla_spmm_refresh_lr_values_dev is refused while the pattern differs.  A callback
 * that finds a part it needs missing (lrprec: A+B, A-B or S+D), or another n, fails through the status of dla_call_matvec /
 * dla_call_lrprec with a message that names the callback and the part.  Row-sharded parts are out of scope: a part is refused on a
 * context whose operator came from dla_spmm_setup_csr_sharded (the message names the entry), and that set-up is refused while a
 * part is present.  dla_spmm_drop_lr frees all four. */
enum { DLA_SPMM_ELL = 0, DLA_SPMM_SELL = 1, DLA_SPMM_AUTO = 2 };
/* what the calling context's operator occupies (a struct tag only: C keeps tags apart from the function of the same name) */
struct dla_spmm_info {
  int format;                 /* DLA_SPMM_ELL or DLA_SPMM_SELL: what is stored (never AUTO) */
  int n;
  int slice_rows;             /* SELL: rows per slice (64), sorting window (4096) and the row length above which a row goes */
  int sort_window;            /*       to the CSR tail (256); 0 for ELLPACK                                                 */
  int long_row_threshold;
  long long nnz;              /* entries handed over */
  long long stored;           /* padded entries of the ELLPACK or sliced part */
  int slices;                 /* SELL: slices, rows in the tail and their entries; 0 for ELLPACK */
  int long_rows;
  long long long_entries;
  long long device_bytes;     /* bytes of the arrays a product and the preconditioner read (allocations only grow: a smaller
                                 operator after a larger one keeps the larger blocks) */
  int long_segment_entries;   /* SELL: entries per segment of a tail row (SEG above), all segments of the tail, and the segments */
  int long_segments;          /*       of rows with more than one (= rows of the workspace of partial sums); 0 for ELLPACK      */
  int multi_segments;
};
int  dla_spmm_setup_csr(dla_ctx* ctx, int n, const long long* rowptr, const int* colind, const double* values);
int  dla_spmm_setup_csr_fmt(dla_ctx* ctx, int n, const long long* rowptr, const int* colind, const double* values, int format);
int  dla_spmm_info(dla_ctx* ctx, struct dla_spmm_info* out);   /* DLA_ERR_ARG before any setup */
int  dla_spmm_setup_csr_sharded(dla_ctx* ctx, int n_local, long long row0, long long n_global, const long long* rowptr,
                                const long long* colind_global, const double* values);
void dla_spmm_matvec(const int* n, const int* m, const double* x_dev, double* ax_dev);
void dla_spmm_precnd(const int* n, const int* m, const double* fac, const double* x_dev, double* px_dev);
/* a second sparse symmetric matrix B (positive definite: not checked, b_ortho reports a failed Cholesky as it does for any
   metric) beside the operator A of this context; format as in dla_spmm_setup_csr_fmt (ELL / SELL / AUTO), single rank */
int  dla_spmm_setup_metric_csr(dla_ctx* ctx, int n, const long long* rowptr, const int* colind, const double* values, int format);
int  dla_spmm_metric_info(dla_ctx* ctx, struct dla_spmm_info* out);   /* DLA_ERR_ARG while no metric is set */
int  dla_spmm_drop_metric(dla_ctx* ctx);                              /* frees B's device blocks; no-op without one */
void dla_spmm_bvec(const int* n, const int* m, const double* x_dev, double* bx_dev);          /* bx = B x */
void dla_spmm_precnd_pencil(const int* n, const int* m, const double* fac, const double* x_dev, double* px_dev);
                                          /* px = x / (a_ii + fac b_ii) where |a_ii + fac b_ii| > 1e-5, else x */
/* which: 0 = the operator A, 1 = the metric B.  All three arrays are DEVICE addresses: rowptr n+1 x int64, colind nnz x int32,
   values nnz x double; 0-based; format as in dla_spmm_setup_csr_fmt (ELL / SELL / AUTO); single rank. */
int  dla_spmm_setup_csr_dev(dla_ctx* ctx, int which, int n, const long long* rowptr_dev, const int* colind_dev,
                            const double* values_dev, int format);
/* the same matrix pattern with new values: rewrites only the stored values and the diagonal of slot `which` */
int  dla_spmm_refresh_values_dev(dla_ctx* ctx, int which, int n, const long long* rowptr_dev, const int* colind_dev,
                                 const double* values_dev);
/* the four sparse parts of the linear-response pencil beside A and B (part: one of the four below); arrays and format as in
   dla_spmm_setup_csr_fmt (host) and dla_spmm_setup_csr_dev / dla_spmm_refresh_values_dev (device); single rank */
enum { DLA_SPMM_LR_APB = 0, DLA_SPMM_LR_AMB = 1, DLA_SPMM_LR_SPD = 2, DLA_SPMM_LR_SMD = 3 };
int  dla_spmm_setup_lr_csr(dla_ctx* ctx, int part, int n, const long long* rowptr, const int* colind, const double* values, int format);
int  dla_spmm_setup_lr_csr_dev(dla_ctx* ctx, int part, int n, const long long* rowptr_dev, const int* colind_dev,
                               const double* values_dev, int format);
int  dla_spmm_refresh_lr_values_dev(dla_ctx* ctx, int part, int n, const long long* rowptr_dev, const int* colind_dev,
                                    const double* values_dev);
int  dla_spmm_lr_info(dla_ctx* ctx, int part, struct dla_spmm_info* out);   /* DLA_ERR_ARG while that part is empty */
int  dla_spmm_drop_lr(dla_ctx* ctx);                                        /* frees all four; no-op without any */
void dla_spmm_apbmul(const int* n, const int* m, const double* x_dev, double* y_dev);          /* y = (A+B) x */
void dla_spmm_ambmul(const int* n, const int* m, const double* x_dev, double* y_dev);          /* y = (A-B) x */
void dla_spmm_spdmul(const int* n, const int* m, const double* x_dev, double* y_dev);          /* y = (S+D) x */
void dla_spmm_smdmul(const int* n, const int* m, const double* x_dev, double* y_dev);          /* y = (S-D) x */
void dla_spmm_lrprec1(const int* n, const int* m, const double* fac, const double* xp_dev, const double* xm_dev, double* yp_dev, double* ym_dev);
void dla_spmm_lrprec2(const int* n, const int* m, const double* fac, const double* xp_dev, const double* xm_dev, double* yp_dev, double* ym_dev);

/* ---------------------------------------------------------------- y = A^T x from the one stored copy of the sparse operator
 * The left pass of nonsym_driver needs matvec_l = A^T x.  The stored operator keeps its values once: dla_spmm_transpose_prepare
 * builds a TRANSPOSED INDEX of slot A (single rank, any stored format of A, host and device set-ups alike), and dla_spmm_matvec_t
 * forms A^T x by fetching A's stored values through it.  The index holds two int32 per stored entry -- the source row, and the
 * position of the value in A's stored value array (the tail of a sliced A lies behind its `stored` padded entries) -- 8 bytes per
 * entry where a transposed copy would cost 12 and a second refresh: dla_spmm_refresh_values_dev on A is at once a refresh of A^T,
 * and nothing can get out of step.
 * Layout.  The index is laid out by the code that lays out a matrix, applied to the COLUMN lengths of A: `format` is ELL, SELL or
 * AUTO as in dla_spmm_setup_csr_fmt (AUTO: ELLPACK while longest column x n / nnz is at most 1.25), columns above
 * long_row_threshold entries go to the index's tail, in segments of long_segment_entries.  A matrix of short rows with one dense
 * column therefore gets a tail in the index although A itself is ELLPACK, and a matrix with a dense row has positions that point
 * into A's tail values.  A padding entry has position -1 and takes part in no arithmetic.  dla_spmm_transpose_info describes the
 * index in the fields of dla_spmm_info: format is never AUTO, nnz equals A's, stored / slices / long_rows / long_entries / the
 * segment counts describe the index, and device_bytes counts the index arrays only (8 bytes per stored entry plus the tables of a
 * sliced layout).  A set-up whose stored positions do not fit int32 is refused.
 * Order of summation.  The entries of column j are taken in ascending index of the caller's CSR arrays -- ascending source row;
 * duplicates and unsorted columns keep the caller's order.  Outside the index's tail y_j starts from 0.0 and takes one
 * fma(value, x[row], acc) per entry in that order; a tail column follows the tail-row contract above on that list, word for word
 * (lanes striding over a segment, the butterfly with off = 32 .. 1, segments added in ascending order by one thread); a column with
 * no entry gives +0.0.  So dla_spmm_matvec_t returns, bit for bit, what dla_spmm_bvec returns for a metric slot holding the
 * explicitly (stably) transposed CSR arrays in the index's format.  The other guarantees are the forward product's: no atomics,
 * one writer per element of the result and of the workspace of partial sums (which belongs to the index), bit-identical repeats,
 * the same bits from host and device set-ups of A, x unchanged and not overlapping y, nothing outside the n x m result written,
 * every element within (len_j + 2) eps (|A|^T |x|)_j with len_j the column's length, exact on small-integer data.
 * Lifecycle.  The index belongs to the stored PATTERN of A: every accepted set-up of slot A through any entry (the sharded one
 * included) drops it, a refused set-up leaves it and its bits alone, dla_spmm_refresh_values_dev keeps it (the next product uses
 * the new values without another prepare), and preparing again replaces it -- all or nothing: everything is checked and allocated
 * before the index in use is given up.  Preparing never changes what dla_spmm_info answers for A, nor the bits of dla_spmm_matvec,
 * dla_spmm_precnd, the Chebyshev forms or any other slot.  The call is synchronous on dla_stream like the device set-ups; only
 * n + 1 column pointers travel to the host, the entries are sorted (a stable radix sort by column) and scattered by kernels, and
 * the temporaries are freed before it returns.
 * Refusals (DLA_ERR_ARG, the message names the entry and the cause).  dla_spmm_transpose_prepare: no operator stored, a row-sharded
 * operator, an unknown format.  dla_spmm_transpose_info: no index.  dla_spmm_matvec_t fails through the status of dla_call_matvec
 * and writes nothing: no operator, no index ("dla_spmm_matvec_t before dla_spmm_transpose_prepare"), another n.
 * dla_spmm_matvec_t is a pure function of its input (DLA_OPT_RUN_AHEAD = 1 covers it).
 * Statistics.  A product books under DLA_OP_MATVEC alg_bytes = 8 (stored entries of the index) + 8 nnz + 16 n m -- plus, for a
 * sliced index, what the forward product adds: 4 n for the permutation and 16 bytes per partial sum -- and flops = 2 nnz m, under
 * the name of the kernel that walks the ELLPACK or sliced part (ell_spmm_t_kernel<W>, sell_spmm_t_kernel<8>); the tail's kernels
 * (csr_long_segments_t_kernel<4>, long_rows_combine_kernel) book a launch each under their own names. */
int  dla_spmm_transpose_prepare(dla_ctx* ctx, int format);            /* ELL / SELL / AUTO, applied to the TRANSPOSED pattern */
int  dla_spmm_transpose_info(dla_ctx* ctx, struct dla_spmm_info* out); /* layout of the index; DLA_ERR_ARG while none */
int  dla_spmm_drop_transpose(dla_ctx* ctx);                            /* frees the index; no-op without one */
void dla_spmm_matvec_t(const int* n, const int* m, const double* x_dev, double* y_dev);          /* y = A^T x */

/* ---------------------------------------------------------------- Chebyshev polynomial preconditioner on the stored operator
 * dla_spmm_precnd and dla_spmm_precnd_pencil divide by a diagonal, which does nothing for a stencil, FEM or graph matrix whose
 * diagonal is (nearly) constant.  dla_spmm_precnd_cheb has the same shape precnd(n,m,fac,x,px), expects DEVICE addresses, acts on
 * the calling thread's context, enqueues on that context's stream and goes where a precnd goes; it applies d steps of the Chebyshev
 * iteration for M = A + fac I, with A the stored operator (slot A, single rank, any format), d >= 1 the configured number of steps
 * and 0 < f < 1 the configured lo_fraction (dla_spmm_cheb_config).  The contract:
 * Upper bound g of the spectrum (Gershgorin): g = max_i g_i with g_i = diag[i] + sum |v_p| over the entries of row i whose
 * column is not i, in stored order from 0.0; diag[i] is the stored diagonal, which already holds the sum of duplicate (i, i)
 * entries.  Kernels form g from the stored blocks without atomics and in a fixed order of summation (a tail row: lane l of one
 * wavefront takes the row's entries l, l + 64, ... from 0.0, then the butterfly of the tail-row contract above, whatever the
 * number of its segments).  g belongs to the stored matrix: every accepted set-up, refresh or drop of slot A invalidates it, and
 * the next call of the preconditioner or of dla_spmm_cheb_info computes it again.  For the same arrays in the same format it has
 * the same bits whether the matrix came from host arrays or device arrays.
 * Interval: hi = g + fac, lo = f hi.  If hi <= 1e-5 then px = x, bit for bit (the harness' mprec guard, main.f90:161-169, on the
 * interval's upper end).
 * Scalars, on the host, each rounded to double once: theta = (hi + lo) / 2, delta = (hi - lo) / 2, sigma = theta / delta, rho_0 = 1 / sigma,
 * rho_k = 1 / (2 sigma - rho_{k-1}).
 * Recurrence (Saad, Iterative Methods, Algorithm 12.1 with a zero start, written on the iterate):
 *   z_0 = 0,  z_1 = x / theta,
 *   z_{k+1} = z_k + rho_k rho_{k-1} (z_k - z_{k-1}) + (2 rho_k / delta) (x - (A z_k + fac z_k))   for k = 1 .. d - 1,
 *   px = z_d.
 * The residual polynomial of z_d is T_d((theta - lambda) / delta) / T_d(sigma).  d = 1 is the scaled identity x / theta; d steps
 * cost d - 1 sparse products.  Every step is one expression, z_{k+1} = fma(eta, A z_k, fma(gamma, x, fma(beta, z_{k-1}, alpha z_k)))
 * with alpha = 1 + rho_k rho_{k-1} - (2 rho_k / delta) fac, beta = -rho_k rho_{k-1}, gamma = 2 rho_k / delta, eta = -gamma rounded
 * on the host (z_1 is folded into the coefficients of steps 1 and 2, so no scaling sweep runs), and A z_k is accumulated as
 * dla_spmm_matvec accumulates it, in both formats: a matrix stored as ELLPACK and as sliced ELLPACK gives the same bits on every
 * row outside the CSR tail.  x is not changed; x and px must not overlap; repeated calls are bit-identical; every output element
 * has one writer.  The iterates live in two work panels of n x m doubles that belong to the context (a sliced operator with a
 * tail, and the un-fused A/B path, take a third); they grow on demand and are released by steps = 0 and by dla_destroy.
 * Accuracy: px stays within twice the first-order running bound that tests/cheb_ref.py computes beside its long-double reference.
 * Configuration (dla_spmm_cheb_config): a property of the context, independent of the matrix -- it survives set-ups and
 * refreshes -- and deliberately not a dla_set_option option.  steps = 0 switches the preconditioner off; steps < 0 and
 * lo_fraction outside (0, 1) are refused with DLA_ERR_ARG and leave an earlier configuration in force.  dla_spmm_cheb_info answers
 * DLA_ERR_ARG while nothing is configured or no A is stored; upper is g of the stored A.
 * Refusals: the callback fails through the status of dla_call_precnd, with a message that names dla_spmm_precnd_cheb and the
 * cause, when it finds no operator, another n, nothing configured or a row-sharded operator; a refused call writes nothing.
 * Out of scope: the pencil A + fac B (dla_spmm_precnd_cheb_pencil below), the linear-response parts and a row-sharded operator
 * (refused as above); choosing lo_fraction or the number of steps adaptively (the caller passes both); sanitizer runs of code loaded into an interpreter (the
 * host-only scalar recurrence is testable from a stand-alone program); any inspection of kernel assembly. */
struct dla_spmm_cheb_info { int steps; double lo_fraction; double upper; };
int  dla_spmm_cheb_config(dla_ctx* ctx, int steps, double lo_fraction);
int  dla_spmm_cheb_info(dla_ctx* ctx, struct dla_spmm_cheb_info* out);
void dla_spmm_precnd_cheb(const int* n, const int* m, const double* fac, const double* x_dev, double* px_dev);

/* ---------------------------------------------------------------- ... on the diagonally scaled operator
 * The interval [f g, g] of dla_spmm_precnd_cheb is right only while the diagonal is nearly constant.  On a variable-coefficient
 * stencil, an FEM matrix on a graded mesh or a graph with uneven degrees g follows the largest row while the wanted eigenvectors
 * live in the smallest rows, and the diagonal preconditioner has the opposite weakness.  dla_spmm_precnd_cheb_jacobi is the same
 * iteration on D^-1 M with M = A + fac I and D = |diag(A) + fac|, whose spectrum sits in about [0, 2] whatever the coefficients
 * do; the result p(D^-1 M) D^-1 is symmetric, and it contains both others as limits (d = 1 is the diagonal preconditioner up to
 * the factor 1 / theta, a constant diagonal gives the plain polynomial).  Same shape precnd(n,m,fac,x,px), DEVICE addresses, the
 * calling thread's context and stream; it reads the configuration (d, f) of dla_spmm_cheb_config that the plain one reads, and the
 * caller chooses between the two by the function it passes as precnd.  Slot A, single rank, ELLPACK and sliced ELLPACK including
 * the CSR tail.  The contract:
 * 1. Off-diagonal row sums: off_i = sum |v_p| over the entries of row i whose column is not i, in stored order from 0.0 -- the sum
 *    that the Gershgorin kernels form per row; a tail row as described for g above.  The n doubles belong to the stored matrix and
 *    are formed by kernels on first use; every accepted set-up, refresh or drop of slot A invalidates them exactly as it
 *    invalidates g.  Host set-up and device set-up give the same bits.  g itself keeps its bits.
 * 2. Per call, per row: s_i = |diag[i] + fac|; den_i = s_i where s_i > 1e-5, else 1.0 (the harness' mprec guard, per row);
 *    r_i = 1.0 / den_i; q_i = (s_i + off_i) / den_i; hi = max_i q_i bounds the infinity norm of D^-1 (A + fac I); lo = f hi.  If
 *    hi <= 1e-5 then px = x, bit for bit.  One kernel reads diag and off, writes r (n doubles owned by the context) and block
 *    maxima; the host takes the maximum of those, without atomics.  THIS COSTS ONE HOST WAIT PER CALL: the scalars of the
 *    recurrence depend on hi, and hi depends on fac.
 * 3. Scalars: those of dla_spmm_precnd_cheb for the interval [lo, hi] with fac = 0 (fac enters through the product, not through
 *    alpha): alpha = 1 + rho_k rho_{k-1}, beta = -rho_k rho_{k-1}, gamma = 2 rho_k / delta, eta = -gamma.
 * 4. Recurrence: y_i = x_i r_i;  z_0 = 0,  z_1 = y / theta,
 *      z_{k+1} = z_k + rho_k rho_{k-1} (z_k - z_{k-1}) + (2 rho_k / delta) (y - r o (A z_k + fac z_k))   for k = 1 .. d - 1,
 *    px = z_d.
 * 5. Each step is one expression per element, with u = z_k and v = z_{k-1}:
 *      t = fma(fac, u_i, (A u)_i) * r_i,   out = fma(eta, t, fma(gamma, y_i, fma(beta, v_i, alpha u_i)))
 *    where (A u)_i is accumulated as dla_spmm_matvec accumulates it and z_1 is folded into the coefficients of steps 1 and 2 as
 *    in the plain form.  d = 1 is px_i = (x_i r_i) / theta.
 * 6. Bits: ELLPACK and sliced storage give the same bits on every row outside the tail; the un-fused A/B path gives the fused
 *    bits; repeated calls are bit-identical; every output element has one writer; x is unchanged and must not overlap px.
 * 7. dla_spmm_cheb_jacobi_upper returns hi for a given fac (one kernel, one host wait), so that a caller or a test can see the
 *    interval; DLA_ERR_ARG under the conditions of dla_spmm_cheb_info.
 * 8. Refusals: the four of the plain callback -- no operator, another n, nothing configured, a row-sharded operator -- through the
 *    status of dla_call_precnd, with a message that names dla_spmm_precnd_cheb_jacobi and the cause; a refused call writes nothing.
 * Work memory beside the plain form's two or three panels: the panel y (n x m) and the vectors off and r (n each); they belong to
 * the context, grow behind a stream wait and are released by steps = 0 and by dla_destroy.
 * Accuracy: px stays within twice the first-order running bound that tests/cheb_jacobi_ref.py computes beside its long-double
 * reference, wherever that bound is below 1e-9 of the result.
 * Out of scope: the linear-response parts, row shards, choosing d or f adaptively, sanitizer runs of code loaded into an
 * interpreter, any inspection of kernel assembly.  The pencil A + fac B: dla_spmm_precnd_cheb_pencil below. */
int  dla_spmm_cheb_jacobi_upper(dla_ctx* ctx, double fac, double* hi);
void dla_spmm_precnd_cheb_jacobi(const int* n, const int* m, const double* fac, const double* x_dev, double* px_dev);

/* ---------------------------------------------------------------- ... on the scaled pencil A + fac B of a generalised problem
 * A stiffness / mass pair A x = lambda B x is where a diagonal preconditioner does nothing: x / (a_ii + fac b_ii) removes the
 * scaling of the rows and leaves the whole coupling.  dla_spmm_precnd_cheb_pencil is the iteration of the scaled form on D^-1 M
 * with M = A + fac B and D = |diag(A) + fac diag(B)|, where A is slot A and B is slot B, the stored metric.  Same shape
 * precnd(n,m,fac,x,px), DEVICE addresses, the calling thread's context and stream; it reads the configuration (d, f) of
 * dla_spmm_cheb_config that the other two read and goes where a precnd goes (gen_david_driver, lobpcg_driver with gen_eig).
 * Single rank.  Each slot in any format -- ELLPACK, sliced ELLPACK, sliced ELLPACK with the CSR tail -- independently of the
 * other.  The contract:
 * 1. Off-diagonal row sums: offA_i is exactly off_i of the scaled form, the same buffer with the same invalidation.  offB_i is
 *    the same sum over the stored B, formed by the same Gershgorin kernels; it belongs to the stored metric: every accepted
 *    set-up, refresh or drop of slot B invalidates it, and nothing else does.  Host set-up and device set-up give the same bits.
 *    g and off of slot A keep their bits.
 * 2. Per call, per row: den0_i = a_ii + fac * b_ii, the product and the sum each rounded on their own (no contraction: the bits
 *    dla_spmm_precnd_pencil divides by); s_i = |den0_i|; den_i = s_i where s_i > 1e-5, else 1.0; r_i = 1.0 / den_i;
 *    q_i = fma(|fac|, offB_i, s_i + offA_i) / den_i; hi = max_i q_i bounds the infinity norm of D^-1 (A + fac B), because
 *    |a_ij + fac b_ij| <= |a_ij| + |fac| |b_ij| entry by entry, whatever the two patterns are; lo = f hi.  If hi <= 1e-5 then
 *    px = x, bit for bit.  One kernel reads the two diagonals and the two off vectors (40 n bytes with r), writes r and block
 *    maxima; the host takes the maximum of those.  ONE HOST WAIT PER CALL, as in the scaled form and for the same reason.
 * 3. Scalars: those of the scaled form, dla::cheb_coefficients(hi, f hi, 0.0, d); fac enters through the product.
 * 4. Recurrence: y = x o r;  z_0 = 0,  z_1 = y / theta,
 *      z_{k+1} = z_k + rho_k rho_{k-1} (z_k - z_{k-1}) + (2 rho_k / delta) (y - r o (A z_k + fac B z_k))   for k = 1 .. d - 1,
 *    px = z_d.  d steps cost d - 1 products with each matrix.
 * 5. Each step is one expression per element, with u = z_k and v = z_{k-1}:
 *      t = fma(fac, (B u)_i, (A u)_i) * r_i,   out = fma(eta, t, fma(gamma, y_i, fma(beta, v_i, alpha u_i)))
 *    where (A u)_i and (B u)_i are each accumulated as dla_spmm_matvec and dla_spmm_bvec accumulate them in that slot's stored
 *    format (tail rows follow the tail-row contract), and z_1 is folded into the coefficients of steps 1 and 2 as in the other
 *    forms.  d = 1 is px_i = (x_i r_i) / theta.
 * 6. Bits: two ELLPACK matrices share one row loop (both gathers in one kernel); any other pair of formats forms B u by the
 *    metric's own product into a panel; the un-fused A/B path forms both products that way.  All three give the same bits.
 *    ELLPACK and sliced storage of either matrix give the same bits on every row outside that matrix's tail; repeated calls are
 *    bit-identical; every output element has one writer; x is unchanged and must not overlap px.  With B stored as the identity
 *    (one entry 1.0 per row), hi and px have the bits of dla_spmm_cheb_jacobi_upper and dla_spmm_precnd_cheb_jacobi for the same
 *    A, fac and configuration: every formula above reduces to the scaled form's when b_ii = 1 and offB = 0.
 * 7. Refusals, through the status of dla_call_precnd, with a message that names dla_spmm_precnd_cheb_pencil and the cause; a
 *    refused call writes nothing: no operator; no metric; n of the call differs from the operator's; the metric's n differs from
 *    the operator's; nothing configured; a row-sharded operator.  dla_spmm_cheb_pencil_upper returns hi for a given fac (one
 *    kernel, one host wait); DLA_ERR_ARG in the same states and for a null hi, and *hi is left alone.
 * 8. Work memory beside the scaled form's: offB (n doubles, the stored metric's) and one panel for B u (n x m), taken only by the
 *    paths that need it; they belong to the context, grow behind a stream wait and are released by steps = 0 and by dla_destroy.
 * 9. Accuracy: px stays within twice the first-order running bound that tests/cheb_pencil_ref.py computes beside its long-double
 *    reference, wherever that bound is below 1e-9 of the result.
 * Out of scope: the linear-response parts, row shards, a shared gather for two matrices with the same pattern, choosing d or f
 * adaptively, sanitizer runs of code loaded into an interpreter, any inspection of kernel assembly. */
int  dla_spmm_cheb_pencil_upper(dla_ctx* ctx, double fac, double* hi);
void dla_spmm_precnd_cheb_pencil(const int* n, const int* m, const double* fac, const double* x_dev, double* px_dev);

/* ---------------------------------------------------------------- dense device operator and metric
 * The reference's own test problem is a DENSE symmetric matrix (main.f90:311-317: a_ii = i + 1, a_ij = 1 / (i + j)) applied by
 * mmult, preconditioned by mprec and paired with a dense SPD metric (smult).  A caller that holds a(n,n) in memory hands it over
 * once; dla_dense_matvec / dla_dense_bvec / dla_dense_precnd / dla_dense_precnd_pencil then have the reference's callback shapes
 * matvec(n,m,x,ax) / bvec(n,m,x,bx) / precnd(n,m,fac,x,px), expect DEVICE addresses (DLA_OPT_CALLBACKS_ON_DEVICE = 1) and go where
 * the host routines go in davidson_driver, lobpcg_driver, gen_david_driver and lobpcg_driver(gen_eig): the whole solve stays in HBM.
 * Set-up and storage.  a is column-major, n x n, leading dimension lda >= n: the Fortran a(lda, n); which = 0 is the operator A,
 * 1 the metric B.  The library keeps ITS OWN COPY in a layout of its choosing (below), so the caller may free or overwrite the
 * array when the call returns.  The call is synchronous like dla_spmm_setup_csr_dev: a device array is read on the context's
 * stream (dla_stream) and the call returns after that stream has been waited for; the caller is responsible for its own producer
 * of the array having finished before the call.  Host set-up and device set-up of the same values store the same bits, and every
 * later call returns the same bits.  A second set-up of a slot replaces it; allocations only grow; a refused set-up replaces
 * nothing.  dla_dense_info answers DLA_ERR_ARG while the slot is empty.  diag[i] = a(i,i) is stored beside the matrix (n doubles):
 * the two preconditioners are the kernels of dla_spmm_precnd / dla_spmm_precnd_pencil on these vectors -- x / (a_ii + fac) resp.
 * x / (a_ii + fac b_ii) where the magnitude of the denominator exceeds 1e-5, else x (mprec, main.f90:146-171) -- and return the
 * bits a host caller gets from the same expressions (the product fac b_ii rounded before the sum).
 * Layout.  Rows and contraction indices are zero-padded to n_pad = n rounded up to 16.  The matrix is cut into tiles of 16 rows and
 * every tile into groups of 8 contraction indices; a group is 128 doubles in the order of the B operand of v_mfma_f64_16x16x4,
 * lane l = 16 (k mod 4) + (i mod 16) holding the pair [a(i, 8 g + l / 16), a(i, 8 g + 4 + l / 16)]: a wavefront loads a group as
 * 1024 contiguous bytes with no bounds check.  device_bytes = 8 n_pad^2 + 8 n.  row_tile = 64: the rows a wavefront multiplies
 * with one fragment of x (four tiles).
 * No symmetry assumed: row i of the result is row i of what was handed over times x.
 * The product.  One pass takes up to 48 columns of x and reads the matrix once; a wider block takes further passes of up to 48
 * columns each.  A pass may split the contraction into k_chunks chunks of whole groups (boundaries are multiples of 8), chosen
 * by a planner from n, the width of the pass and the number of compute units alone (dense_plan in diaglib_amd/csrc/hip_plans.h
 * states the rule); each chunk is summed in ascending index by the MFMA chain of one wavefront, and with k_chunks > 1 the partials
 * go to a workspace of k_chunks x m x n doubles that belongs to the stored matrix (it grows with m and is not counted in
 * device_bytes) and are added in ascending chunk order, ((p_0 + p_1) + p_2) + ..., by one thread per element -- the rule of the
 * sparse tail's segments.  No atomics; every element of the result and of the workspace has exactly one writer; repeated products
 * are bit-identical.  (The split depends on the width of the pass, so the bits of a column may differ between blocks of different
 * width.)  k_chunks and workspace_bytes of dla_dense_info describe the first pass of the slot's most recent product, and a
 * product of one column before any.
 * Accuracy: every element stays within (n + 2) eps (|A| |x|)_i of the exact product, the bound of the tail-row contract, which
 * holds for any order of summation.
 * Shapes: any n >= 1, any m >= 1.  x and the result must not overlap; x is unchanged; nothing outside the n x m result is written.
 * Independence: A and B are independent of each other and of the six sparse slots -- setting, dropping or replacing one never
 * changes another's blocks, info or bits.  A context may hold a sparse A and a dense A at once; the caller chooses by the function
 * it passes.
 * Callbacks: they act on the context whose dense set-up the calling thread had accepted last (a thread-local binding of their own,
 * cleared by dla_destroy) and enqueue on dla_stream.  A callback that finds its matrix missing, another n, or -- the pencil form --
 * no metric or a metric of another n fails through the status of dla_call_matvec / dla_call_precnd with a message that names it
 * and the cause; a refused call writes nothing.  dla_dense_matvec and dla_dense_bvec are pure functions of their input, so
 * DLA_OPT_RUN_AHEAD = 1 covers them.
 * Refused with DLA_ERR_ARG, the message naming the entry: a null pointer, n <= 0, lda < n, which not 0 or 1.
 * Statistics: a pass books one launch under DLA_OP_MATVEC with alg_bytes = 8 n^2 + 16 n m and flops = 2 n^2 m (m: its columns)
 * under the name of its kernel, dense_mfma_kernel<G> with G accumulator groups of 16 columns; the combining kernel of a split pass
 * books a launch of its own with no algorithmic bytes (the workspace is not compulsory traffic).  The preconditioners book under
 * DLA_OP_PRECND as the sparse ones do.
 * Out of scope (the four linear-response parts as dense matrices: the next block): row shards; aliasing the
 * caller's array instead of copying it; sanitizer runs of code loaded into an interpreter (the layout and the planner are host-only
 * code, testable from a stand-alone program); any inspection of kernel assembly. */
struct dla_dense_info { int n; int n_pad; int row_tile; int k_chunks; long long device_bytes; long long workspace_bytes; };
int  dla_dense_setup    (dla_ctx* ctx, int which, int n, const double* a_host, int lda);   /* which: 0 = operator A, 1 = metric B */
int  dla_dense_setup_dev(dla_ctx* ctx, int which, int n, const double* a_dev,  int lda);
int  dla_dense_info     (dla_ctx* ctx, int which, struct dla_dense_info* out);
int  dla_dense_drop     (dla_ctx* ctx, int which);                                        /* no-op where nothing is stored */
void dla_dense_matvec(const int* n, const int* m, const double* x_dev, double* ax_dev);           /* ax = A x */
void dla_dense_bvec  (const int* n, const int* m, const double* x_dev, double* bx_dev);           /* bx = B x */
/* y = A^T x from the same stored copy of the operator (which = 0): the matvec_l of nonsym_driver, so that a device-mode caller does
 * not store the matrix twice.  Everything dla_dense_matvec says about itself holds with A^T for A: the callback shape, the context
 * it acts on, dla_stream, up to 48 columns per pass with the matrix read once, any n >= 1 and m >= 1, x unchanged and not
 * overlapping y, nothing written outside the n x m result, no atomics, one writer per element, bit-identical repeats, a pure
 * function of its input (DLA_OPT_RUN_AHEAD = 1 covers it).  It reads the existing copy: device_bytes, the set-up entries and what
 * dla_dense_info answers are unchanged by it.  The contraction runs down the rows of the matrix, which are an MFMA output index in
 * the stored order, so a wavefront turns every 16 x 16 block in LDS before it multiplies (dense_t_mfma_kernel<G>).  A wavefront owns
 * 64 output indices and one chunk of whole row tiles (boundaries are multiples of 16) and sums it in ascending row order by one MFMA
 * chain; dense_t_plan in diaglib_amd/csrc/hip_plans.h states how many chunks a pass has.  With more than one, the partials go to
 * the slot's workspace (row_chunks x m x n doubles, grown on demand, not counted in device_bytes) and are added in ascending chunk
 * order, ((p_0 + p_1) + p_2) + ..., by one thread per element (dense_combine_kernel).
 * Accuracy: every element stays within (n + 2) eps (|A|^T |x|)_i of the exact product; exact on small-integer data.
 * Refusals go through the status of dla_call_matvec with a message naming dla_dense_matvec_t and the cause (no dense operator, or
 * another n); a refused call writes nothing.  Statistics: as dla_dense_matvec, under dense_t_mfma_kernel<G>. */
void dla_dense_matvec_t(const int* n, const int* m, const double* x_dev, double* y_dev);         /* y = A^T x */
void dla_dense_precnd(const int* n, const int* m, const double* fac, const double* x_dev, double* px_dev);         /* x / (a_ii + fac), guard 1e-5: mprec */
void dla_dense_precnd_pencil(const int* n, const int* m, const double* fac, const double* x_dev, double* px_dev);  /* x / (a_ii + fac b_ii), same guard */
/* A symmetric operator or metric stored as ONE TRIANGLE.  Every driver that uses these two slots except nonsym_driver works on
 * symmetric matrices; dla_dense_setup_sym stores such a matrix in about half the memory and a product streams each stored byte once.
 * Set-up: the rules of dla_dense_setup -- which = 0 / 1, a column-major with lda >= n, the library's own copy, synchronous, host and
 * device set-up of the same values store the same bits, allocations only grow, a refused set-up replaces nothing.  uplo = 'L' or 'U'
 * (or lower case) names the triangle of the array that is REFERENCED: the other strict triangle is never read, neither on the host
 * nor on the device, inside diagonal blocks either, and may hold anything.  a(i,k) = a(k,i) is assumed, not checked.
 * A slot remembers how it is stored: dla_dense_matvec, dla_dense_bvec, dla_dense_precnd and dla_dense_precnd_pencil keep their names
 * and shapes and dispatch on it, so a caller changes its set-up line and nothing else.  dla_dense_matvec_t on a symmetric slot is
 * the symmetric product (the same bits).  A full set-up of a slot replaces a symmetric one and the reverse; slots stored in full
 * behave bit for bit as before.
 * Layout.  The tile and group format of the full copy, but row tile T (16 rows) keeps only its groups 0 .. 2 T + 1, the column
 * blocks 0 .. T: tile T starts at group T (T + 1) and the copy holds 128 nt (nt + 1) doubles, nt = n_pad / 16 -- n_pad^2 / 2 +
 * 8 n_pad; device_bytes = 8 * 128 nt (nt + 1) + 8 n (at n = 65536: 17 GB instead of 34 GB).  Diagonal blocks are stored whole,
 * mirrored from the referenced triangle; padding is 0.0; diag[i] = a(i,i), so the preconditioners return the bits they return on a
 * full copy.
 * The product.  One pass takes up to 48 columns and loads every stored byte once.  A workgroup owns a panel of 256 rows and one
 * chunk of the column blocks up to the panel's last tile (dense_sym_plan in diaglib_amd/csrc/hip_plans.h states the rule for the
 * chunk length from n, the width of the pass and the number of compute units alone).  A stored 16 x 16 block (T, b) is used twice:
 * as A_Tb x_b (the MFMAs of dense_mfma_kernel) and, for T > b, turned in LDS as in dense_t_mfma_kernel, as A_Tb^T x_T.  The forward
 * partial sums of a (panel, chunk) and the transposed ones of a (panel, column block) -- the four wavefronts' added in wavefront
 * order -- go to the slot's workspace (dense_sym_plan states its layout; it is not counted in device_bytes), and
 * dense_sym_combine_kernel adds the partials of an element with one thread in one order: forward chunks ascending, then transposed
 * partials by ascending panel.  No atomics; every element of the result and of the workspace has one writer; repeated products are
 * bit-identical; 'L' and 'U' of an exactly symmetric array store the same bits.  Accuracy, shapes and callbacks: as dla_dense_matvec
 * ((n + 2) eps (|A| |x|)_i; any n, m >= 1; nothing outside the n x m result is written).
 * The transposed partial sums cost about m / 256 of the copy's bytes per pass in workspace and traffic, whatever the chunking: the
 * format saves memory at every shape and time only where the stored bytes dominate.  Measured against dla_dense_matvec on the full
 * copy (profiles/dense_sym_operator.txt): 0.86-0.88 of its time at n = 32768 for 8-13 columns, 0.97 at n = 8192; it SAVES MEMORY AND
 * COSTS TIME at n = 2048 (1.6-2.0 times the full product) and for blocks of 37 columns (1.6-2.4 times at every size measured).  The
 * panel height and the planner's constants are starting values.
 * Info.  dla_dense_info on a symmetric slot answers n, n_pad, row_tile, device_bytes as above, the workspace of the first pass of the
 * most recent product, and in k_chunks the largest number of chunks of a panel.  dla_dense_sym_info adds the triangle that was
 * referenced ('L' or 'U'), the panels, the chunk length in column blocks and the largest number of partial sums added into one
 * element; it answers DLA_ERR_ARG on an empty slot and on a slot stored in full.
 * Refused with DLA_ERR_ARG, the message naming the entry: what dla_dense_setup refuses, and uplo not one of L l U u.
 * Statistics: a pass books one launch under DLA_OP_MATVEC with alg_bytes = 4 n (n + 1) + 16 n m and flops = 2 n^2 m under
 * dense_sym_mfma_kernel<G>; the combine books a launch of its own with no algorithmic bytes.
 * Out of scope: the four linear-response parts and the pair set-up (A +- B are symmetric, S +- D are not); row shards; symmetric
 * sparse storage. */
struct dla_dense_sym_info { int uplo; int panels; int chunk_blocks; int max_partials; };   /* uplo: 'L' or 'U' */
int  dla_dense_setup_sym    (dla_ctx* ctx, int which, int n, const double* a_host, int lda, char uplo);
int  dla_dense_setup_sym_dev(dla_ctx* ctx, int which, int n, const double* a_dev,  int lda, char uplo);
int  dla_dense_sym_info     (dla_ctx* ctx, int which, struct dla_dense_sym_info* out);

/* ---------------------------------------------------------------- dense linear-response parts
 * The reference harness' linear-response problems are DENSE (main.f90:528-760): A+B, A-B, S+D and S-D of the pencil
 * (A B; B A)(Y Z) = w (S D; -D -S)(Y Z) applied by dgemm in host callbacks.  A context stores four dense parts beside the dense
 * operator and metric; dla_dense_apbmul / ambmul / spdmul / smdmul have the shape of the reference's apbmul / ambmul / spdmul /
 * smdmul (diaglib.f90:1024-1025) and dla_dense_lrprec1 / _lrprec2 the shape of its lrprec (:1317), expect DEVICE addresses
 * (DLA_OPT_CALLBACKS_ON_DEVICE = 1) and go where the host routines go in caslr_eff_driver and caslr_driver: the whole solve stays
 * in HBM.  part: DLA_DENSE_LR_APB .. _SMD, the numbering and the meaning of DLA_SPMM_LR_*.
 * Set-up and storage: every rule of dla_dense_setup holds for a part.  a is column-major, n x n, lda >= n; the library keeps its own
 * copy in the stored layout above (tiles of 16 rows, groups of 8 contraction indices, zero-padded to n_pad) with the diagonal
 * beside it, device_bytes = 8 n_pad^2 + 8 n per part; the call is synchronous like dla_dense_setup_dev; host and device set-up of
 * the same values store the same bits; allocations only grow; a refused set-up replaces nothing.  dla_dense_lr_info answers
 * DLA_ERR_ARG while that part is empty; dla_dense_drop_lr frees all four and does nothing without any.
 * No symmetry assumed (S+D and S-D are not symmetric): row i of the result is row i of what was handed over times x.
 * Set-up from the caller's pairs.  A caller holds A, B, S, D, not their sums: dla_dense_setup_lr_pair takes p(ldp, n) and q(ldq, n)
 * -- pair DLA_DENSE_LR_PAIR_AB: p = A, q = B, fills APB with p + q and AMB with p - q; DLA_DENSE_LR_PAIR_SD: p = S, q = D, fills
 * SPD and SMD -- and forms both while packing: every stored element is ONE rounded addition or ONE rounded subtraction of the two
 * source elements, the padding is 0.0, the two diagonals are formed the same way, and both slots then equal, bit for bit and field
 * by field of dla_dense_lr_info, what dla_dense_setup_lr stores for the host arrays p + q and p - q.  ldp and ldq are independent,
 * both >= n; the sources are only read, each element once.  All or nothing: every check and both allocations happen before either
 * slot is written, so after a refusal or a failed allocation both slots keep their blocks, their info and the bits of their
 * products.
 * Products: the kernels and the plan of dla_dense_matvec (dense_mfma_kernel<G>, dense_combine_kernel, dense_plan), so for the same
 * array a part returns the bits the operator slot returns; each part owns its workspace of partial sums; statistics book as a
 * dense pass does; k_chunks and workspace_bytes of dla_dense_lr_info describe the first pass of that part's most recent product.
 * Preconditioners: dla_dense_lrprec1 / _lrprec2 are the kernel of dla_spmm_lrprec1 / 2 on the stored dense diagonals, with
 * aa = 0.5 * (apb_ii + amb_ii) and sg = spd_ii (S-D is not read), the expressions and the order of operations stated for
 * dla_spmm_lrprec1 / 2 above -- bit for bit what a host caller gets from them -- booked under DLA_OP_PRECND.
 * Independence: the four parts are independent of each other, of the dense operator and metric and of the six sparse slots --
 * blocks, info and product bits alike.
 * Callbacks: they act on the context whose dense set-up (any of dla_dense_setup*, these included) the calling thread had accepted
 * last and enqueue on dla_stream.  A product that finds its part missing or another n, and a preconditioner that finds A+B, A-B
 * or S+D missing or parts of unequal n, fail through the status of dla_call_matvec / dla_call_lrprec with a message that names the
 * callback and the cause; a refused call writes nothing.  The four products are pure functions of their input, so
 * DLA_OPT_RUN_AHEAD = 1 covers them.
 * Refused with DLA_ERR_ARG, the message naming the entry: a null pointer, n <= 0, lda (ldp, ldq) < n, a part outside 0 .. 3, a pair
 * outside 0 and 1.
 * Out of scope: one batched launch for the four independent products of an iteration; storing S-D as the transpose of S+D; row
 * shards; halving the traffic through symmetry; aliasing the caller's arrays; a polynomial preconditioner for the pencil;
 * sanitizer runs of code loaded into an interpreter (the packing twin dense_pack_pair is host-only code, testable from a
 * stand-alone program); any inspection of kernel assembly. */
enum { DLA_DENSE_LR_APB = 0, DLA_DENSE_LR_AMB = 1, DLA_DENSE_LR_SPD = 2, DLA_DENSE_LR_SMD = 3 };
enum { DLA_DENSE_LR_PAIR_AB = 0, DLA_DENSE_LR_PAIR_SD = 1 };
int  dla_dense_setup_lr    (dla_ctx* ctx, int part, int n, const double* a_host, int lda);
int  dla_dense_setup_lr_dev(dla_ctx* ctx, int part, int n, const double* a_dev,  int lda);
int  dla_dense_setup_lr_pair    (dla_ctx* ctx, int pair, int n, const double* p_host, int ldp, const double* q_host, int ldq);
int  dla_dense_setup_lr_pair_dev(dla_ctx* ctx, int pair, int n, const double* p_dev,  int ldp, const double* q_dev,  int ldq);
int  dla_dense_lr_info     (dla_ctx* ctx, int part, struct dla_dense_info* out);   /* DLA_ERR_ARG while that part is empty */
int  dla_dense_drop_lr     (dla_ctx* ctx);                                         /* frees all four; no-op without any */
void dla_dense_apbmul(const int* n, const int* m, const double* x_dev, double* y_dev);          /* y = (A+B) x */
void dla_dense_ambmul(const int* n, const int* m, const double* x_dev, double* y_dev);          /* y = (A-B) x */
void dla_dense_spdmul(const int* n, const int* m, const double* x_dev, double* y_dev);          /* y = (S+D) x */
void dla_dense_smdmul(const int* n, const int* m, const double* x_dev, double* y_dev);          /* y = (S-D) x */
void dla_dense_lrprec1(const int* n, const int* m, const double* fac, const double* xp_dev, const double* xm_dev, double* yp_dev, double* ym_dev);
void dla_dense_lrprec2(const int* n, const int* m, const double* fac, const double* xp_dev, const double* xm_dev, double* yp_dev, double* ym_dev);

#ifdef __cplusplus
}
#endif
#endif
