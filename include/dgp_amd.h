/*
 * dgp_amd.h -- C-ABI of the MI355X-native stochastic-imputation engine.
 *
 * This is the drop-in boundary for dgpsi's SI training / imputed-GP prediction
 * hot path (mingdeyu/DGP).  Each entry point replaces one njit/LAPACK operator
 * of the reference; the reference interface is cited as file:line relative to
 * the reference repository.  A dgpsi maintainer binds these with ctypes (see
 * INTEGRATION.md); dgp_amd/ is the Python host that does exactly that.
 *
 * Conventions
 *   - every array argument is a DEVICE pointer unless its name ends in `_h`
 *     (host) ; f64 row-major (C order) and int64 indices, like numpy's;
 *   - all launches go to the HIP stream given to dgpamd_create(); nothing
 *     synchronises unless documented; workspaces are caller-allocated with the
 *     size returned by the matching *_workspace() query (bytes);
 *   - kernel kind: 0 = 'sexp', 1 = 'matern2.5' (reference passes these strings);
 *   - every function returns 0 on success, DGPAMD_BAD_ARG, or DGPAMD_HIP_ERROR
 *     (message via dgpamd_last_error).  Loss of positive-definiteness is
 *     reported through device-side `info` words (LAPACK convention: 0 = ok,
 *     j>0 = leading minor j not positive) which the host shim turns into
 *     numpy.linalg.LinAlgError (reference: scipy/numpy cholesky raising,
 *     dgp.py:1402, kernel_class.py:749).
 *
 * "Augmented" matrices.  A factorisation buffer is an Np x Np row-major array,
 * Np = dgpamd_padded_dim(n) (a multiple of 64, > n).  Rows/cols [0,n) hold the
 * SPD matrix (lower triangle is referenced), rows [n, n+r) hold r right-hand
 * sides y_q^T in columns [0,n) and the bottom-right corner starts at zero.
 * dgpamd_potrf factors the leading n columns only, so on exit row n+q holds
 * w_q = L^-1 y_q and the corner entry (n+q, n+q') holds -w_q . w_q'
 * (the quadratic forms y^T K^-1 y come out of the trailing update for free).
 */
#ifndef DGP_AMD_H
#define DGP_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGPAMD_OK 0
#define DGPAMD_NOT_PD 1
#define DGPAMD_BAD_ARG 2
#define DGPAMD_HIP_ERROR 3

#define DGPAMD_SEXP 0
#define DGPAMD_MATERN25 1

#define DGPAMD_MAXD 64   /* max columns of [input | global_input] of one GP node */
#define DGPAMD_MAXB 64   /* max matrices in one batched call */

typedef struct dgpamd_ctx dgpamd_ctx;

/* ---- context ------------------------------------------------------------ */
/* stream: a hipStream_t created by the caller (e.g. a torch side stream), or
 * NULL for the device's default (null) stream -- torch's default current stream. */
int dgpamd_create(int device, void *stream, dgpamd_ctx **out);
int dgpamd_destroy(dgpamd_ctx *ctx);
/* The DGPAMD_* environment switches of the library (INTEGRATION.md lists them) are read once, by dgpamd_create: a context
 * keeps the switches it was created under.  *value = what this context runs under for `name` (with or without the
 * "DGPAMD_" prefix), as parsed and clamped; 0 where the switch was unset (or its value not accepted) and the default depends on the call.
 * An unknown name: DGPAMD_BAD_ARG. */
int dgpamd_tuning_get(dgpamd_ctx *ctx, const char *name, int64_t *value);
const char *dgpamd_last_error(const dgpamd_ctx *ctx);
int dgpamd_sync(dgpamd_ctx *ctx);
/* Results to the host: copy `bytes` from device memory through the context's pinned staging buffer, ordered after
 * everything queued on the context's stream, and return when they have landed (one stream synchronisation). */
int dgpamd_fetch(dgpamd_ctx *ctx, const void *device_src, void *host_dst, size_t bytes);
/* The two halves of dgpamd_fetch for results the host does not need yet.  dgpamd_post queues the copy of `bytes` from device
 * memory into mailbox `slot` (0 .. DGPAMD_MAILBOXES-1) behind everything queued so far and returns at once; work queued
 * afterwards does not delay it.  dgpamd_collect waits for that one copy (not for the stream) and hands the bytes over
 * (host_dst NULL: wait and discard).  A mailbox holds one result at a time.  The lock-step M-step keeps two groups of
 * optimisers in flight this way (one group's objective evaluations run while the host advances the other group's
 * optimisers); the I-step's latents travel to the host while the M-step's first evaluations run. */
#define DGPAMD_MAILBOXES 8
int dgpamd_post(dgpamd_ctx *ctx, const void *device_src, size_t bytes, int slot);
int dgpamd_collect(dgpamd_ctx *ctx, int slot, void *host_dst, size_t bytes);
/* A sum over ranks in the middle of a queued sequence.  With the rows of a Vecchia likelihood split over several processes
 * (one per GPU), dgpamd_ess_queue leaves every batch's B x 2 sums of THIS rank's rows in a device buffer and calls
 * hook(user, device_buf, count) -- on the calling thread, while it is queueing, between the launch that produced the sums and
 * the one that reads them.  The hook queues an in-place all-reduce of the count doubles on the context's stream (RCCL:
 * ncclAllReduce on that stream; the Python host passes torch.distributed.all_reduce) and returns 0, or non-zero to abort the
 * call (DGPAMD_BAD_ARG).  Every rank makes the same calls in the same order whatever the accept decisions are (launches of
 * an update that is already closed are predicated away, the hook is not).  NULL: no hook (one process). */
typedef int (*dgpamd_reduce_hook)(void *user, double *device_buf, int count);
int dgpamd_set_reduce_hook(dgpamd_ctx *ctx, dgpamd_reduce_hook hook, void *user);
/* Two device regions (e.g. log-likelihoods and their info words) into one host buffer, back to back, one sync. */
int dgpamd_fetch2(dgpamd_ctx *ctx, const void *src_a, size_t bytes_a, const void *src_b, size_t bytes_b, void *host_dst);
const char *dgpamd_version(void);
int64_t dgpamd_padded_dim(int64_t n); /* Np for an n x n problem (>= n+1, multiple of 64) */

/* Static launch sequences (the ~100 launches of one blocked factorisation / inverse) are captured once per
 * (shape, buffers) and replayed as hipGraphs; enable = 0 turns that off (direct launches).  Graphs need a
 * real stream: with the null stream the library always launches directly.                              */
int dgpamd_set_graphs(dgpamd_ctx *ctx, int enable);

/* Timing on the library's stream (bench.py: HIP events around the timed region). */
int dgpamd_event_create(dgpamd_ctx *ctx, void **ev);
int dgpamd_event_record(dgpamd_ctx *ctx, void *ev);
int dgpamd_event_elapsed_ms(dgpamd_ctx *ctx, void *start, void *stop, float *ms_h); /* syncs on stop */
int dgpamd_event_destroy(dgpamd_ctx *ctx, void *ev);

/* Launch timing of ONE kernel class with HIP events on the launching stream (bench.py's roofline):
 * classes 1 kmatrix, 2 potrf diagonal block, 3 panel TRSM, 4 trailing SYRK, 5 trtri, 6 lauum,
 * 7 grad_reduce, 8 linked-GP J, 9 gp quadratic form.  collect() syncs and returns the number of
 * timed launches, their summed duration and their summed algorithmic work (flops; bytes for 1). */
int dgpamd_prof_enable(dgpamd_ctx *ctx, int kernel_class);
int dgpamd_prof_collect(dgpamd_ctx *ctx, int64_t *launches_h, double *total_ms_h, double *work_h);
int dgpamd_prof_event_overhead_us(dgpamd_ctx *ctx, double *us_h); /* duration an EMPTY event pair reports */

/* ---- a1/a2  kernel-matrix assembly ---------------------------------------
 * kernel.k_matrix()  kernel_class.py:304-359 (pdist/squareform + functions.py:16-34).
 * X = [Xloc[:, colmap] | Xglob]: Xloc is (n x ldloc) with batch stride
 * `stride_loc` (elements) and Dl gathered columns colmap_h[0..Dl); Xglob is
 * (n x Dg), shared by the batch (may be NULL iff Dg == 0).
 * length_h: 1 (shared) or Dl+Dg lengthscales.  Diagonal = 1 + nugget*W[i]
 * (W = NULL -> 1)  kernel_class.py:352-355.
 * Output, per batch b: K + b*stride_k, ld = ldk.
 *   full != 0 : the n x n matrix, both triangles (ldk >= n)            [k_matrix()]
 *   full == 0 : augmented factorisation buffer (ldk = Np): lower tiles of K,
 *               rows [n, n+r) <- Y (r x n, ld = ldy, batch stride stride_y; may
 *               be NULL iff r == 0), zero corner.                                */
int dgpamd_kmatrix(dgpamd_ctx *ctx, int kind, int64_t n,
                   const double *Xloc, int64_t ldloc, int64_t stride_loc, const int32_t *colmap_h, int Dl,
                   const double *Xglob, int Dg,
                   const double *length_h, int nlen, double nugget, const double *W,
                   double *K, int64_t ldk, int64_t stride_k, int full,
                   const double *Y, int64_t ldy, int64_t stride_y, int r,
                   int batch);

/* ---- LAPACK potrf (+ the forward solves and log-determinant it feeds) -----
 * scipy.linalg.cholesky / np.linalg.cholesky call sites kernel_class.py:417,483,746,
 * functions.py:109,119 ; logdet_nb functions.py:220-222 ; cho_solve with y
 * kernel_class.py:423,487.
 * In place on `batch` augmented buffers (see top).  logdet[b] = 2 sum log L_ii;
 * info[b] as LAPACK.  work: dgpamd_potrf_workspace(n,batch) bytes of device memory starting on a
 * 128-byte line (any allocator's base address does; the one-launch kernel's synchronisation words
 * sit on cache lines of their own inside it); it keeps the inverses of the 64x64 diagonal blocks
 * for dgpamd_potri.                                                                            */
size_t dgpamd_potrf_workspace(int64_t n, int batch);
int dgpamd_potrf(dgpamd_ctx *ctx, int64_t n, double *A, int64_t stride_a, int batch,
                 double *logdet, int32_t *info, void *work);
/* How dgpamd_potrf / dgpamd_potrf_inv (and everything built on them) run the blocked factorisation:
 * mode 1 (default): ONE persistent launch -- a pivot-chain workgroup per matrix plus workers that pull tile tasks
 * from a queue, ordered by per-tile version words (csrc/potrf_mega.hpp, potrf_mega_kernel); mode 0: one launch per 64-column
 * block step, replayed as a hipGraph (no waits between workgroups inside a launch: the mode for a device shared with other
 * processes).  The results are bit-identical (every tile applies its panels in the same order).
 * info[b] = -1 reports a lost in-kernel hand-off (a bounded spin gave up), never a numerical failure: the caller
 * rebuilds the matrices and runs the call again in mode 0 (dgp_amd.dgp.train does, once per iteration). */
int dgpamd_set_potrf_mode(dgpamd_ctx *ctx, int mode);

/* Read the quadratic forms out of factored buffers: quad[b*r*r + q*r + q'] =
 * y_q^T K^-1 y_q'  (= -corner).                                               */
int dgpamd_aug_quad(dgpamd_ctx *ctx, int64_t n, const double *A, int64_t stride_a, int batch, int r, double *quad);

/* The closing arithmetic of dgpamd_loglik (kernel_class.py:486-488) for buffers that were assembled with their y row and
 * factored by another call (e.g. as extra matrices of a batched dgpamd_potrf):
 * ll[b] = -0.5 (n log scale + logdet[b] + y'K^-1y / scale). */
int dgpamd_loglik_finish(dgpamd_ctx *ctx, int64_t n, const double *A, int64_t stride_a, int batch, const double *logdet,
                         double scale, double *ll);

/* Dense row-major matrix-vector product out = A x (rows x cols, leading dimension ld): the K alpha + u step of the
 * heteroskedastic exact-posterior draw (likelihood_class.py:184-243), where K is a full kernel matrix. */
int dgpamd_gemv(dgpamd_ctx *ctx, int64_t rows, int64_t cols, const double *A, int64_t ld, const double *x, double *out);

/* ---- a5  ESS target log-likelihood, batched over speculative proposals -----
 * kernel.log_likelihood_func  kernel_class.py:481-492:
 *   ll[b] = -0.5 ( n log(scale) + logdet(K_b) + y^T K_b^-1 y / scale )
 * Fused pipeline: kmatrix (augmented with y) -> potrf -> read-out.  A is scratch
 * for `batch` augmented buffers.  y: (n) shared by the batch.                  */
int dgpamd_loglik(dgpamd_ctx *ctx, int kind, int64_t n,
                  const double *Xloc, int64_t ldloc, int64_t stride_loc, const int32_t *colmap_h, int Dl,
                  const double *Xglob, int Dg,
                  const double *length_h, int nlen, double nugget, const double *W, double scale,
                  const double *y, double *A, int64_t stride_a, int batch,
                  double *ll, int32_t *info, void *work);

/* ---- a3  fmvn: nu = sqrt(scale) * L z  -------------------------------------
 * functions.fmvn  functions.py:113-121 (chol(scale*K) z = sqrt(scale) chol(K) z).
 * L: factored augmented buffers (batch stride stride_a); z, out: (batch x n).   */
int dgpamd_trmv_lower(dgpamd_ctx *ctx, int64_t n, const double *L, int64_t stride_a, const double *scale_h,
                      const double *z, double *out, int batch);

/* ---- a4  ESS proposals: FP[b] = F cos(theta_b) + NU sin(theta_b) -----------
 * functions.update_f  functions.py:203-208.  F, NU: (n x M); FP: (batch x n x M). */
int dgpamd_ess_propose(dgpamd_ctx *ctx, int64_t n, int M, const double *F, const double *NU,
                       const double *theta_h, int batch, double *FP);

/* ---- inverse from the factor (cho_solve(L, I))  kernel_class.py:418,747 -----
 * On entry A holds dgpamd_potrf output (and `work` its workspace).  On exit
 * Ainv (Np x Np buffer) holds K^-1 in BOTH triangles of [0,n)x[0,n) and row n+q
 * of columns [0,n) holds -alpha_q^T = -(K^-1 y_q)^T.  A is overwritten with L^-1. */
int dgpamd_potri(dgpamd_ctx *ctx, int64_t n, double *A, double *Ainv, int r, void *work);
/* Factorisation AND inverse in one sweep (replaces potrf + potri where both are wanted, e.g. kernel.llik
 * kernel_class.py:417-423): the identity rides along as n extra rows, so the right-looking sweep leaves
 *   A: as dgpamd_potrf;   T (Np x Np): L^-T in its first n rows (block upper triangular; column n = -K^-1 y_0);
 *   S (Np x Np): K^-1 in the lower 64x64 tiles of its first n rows/columns (diagonal tiles full), row n = -(K^-1 y_0)^T
 * -- the layout dgpamd_potri leaves in Ainv, minus the strictly upper tiles.  T and S need no initialisation.
 * The inverse's GEMM work runs in the shadow of the factorisation's pivot chain instead of after it. */
int dgpamd_potrf_inv(dgpamd_ctx *ctx, int64_t n, double *A, double *T, double *S, int64_t stride_a, int batch,
                     double *logdet, int32_t *info, void *work);

/* Same on `batch` buffers (A and Ainv share the batch stride stride_a; work = the batched potrf workspace). */
int dgpamd_potri_batched(dgpamd_ctx *ctx, int64_t n, double *A, double *Ainv, int64_t stride_a, int r, int batch,
                         void *work);

/* A GP node as the batched entry points take it (host struct; pointers as commented). */
typedef struct {
    int kind;              /* DGPAMD_SEXP / DGPAMD_MATERN25 */
    int Dl, Dg, nlen;      /* local / global input columns, number of lengthscales */
    int nugget_est;
    int reserved;
    int64_t ldloc;
    const double *Xloc;    /* device, n x ldloc */
    const int32_t *colmap; /* host, Dl entries, or NULL */
    const double *Xglob;   /* device, n x Dg, or NULL */
    const double *length;  /* host, nlen entries */
    double nugget;
    const double *W;       /* device replicate weights or NULL */
    const double *y;       /* device, n */
    /* Vecchia form of the node (read by dgpamd_ess_queue only; vecch_nn == NULL: dense).  kernel.log_likelihood_func_vecch
     * kernel_class.py:494-509 = vecchia_llik (vecchia.py:165-180) on the inputs and outputs permuted by kernel.ord. */
    const int64_t *vecch_ord;   /* device, n: the ordering (row i of the ordered arrays is point vecch_ord[i]) */
    const int64_t *vecch_nn;    /* device, n x (vecch_m + 1): NNarray (ordered coordinates) */
    const double *vecch_nd;     /* device, n: nugget weights in ordered coordinates (ones without replicates) */
    const double *vecch_y;      /* device, n: the outputs in ordered coordinates */
    int vecch_m, reserved2;
    /* This rank's rows of the Vecchia likelihood (dist.split_training(rows=True)): rows vecch_row0 .. vecch_row0 + vecch_rows - 1
     * of vecch_nn; vecch_rows == 0: all n.  The partial sums of a batch are completed by the context's reduce hook
     * (dgpamd_set_reduce_hook) before the accept / shrink decision reads them. */
    int64_t vecch_row0, vecch_rows;
    /* Likelihood node on top of the model (read by dgpamd_ess_queue and dgpamd_lik_loglik only; lik_kind == 0: a GP node).
     * The reference's plugin protocol llik() (likelihood_class.py:30-90 Poisson, :245-292 NegBin, :470-621 ZIP, :624-812 ZINB,
     * the classification likelihood): y = the lik_nobs observations (device; class indices for the categorical kinds),
     * colmap / Dl = the latent columns it reads (one per class for SOFTMAX / ROBUSTMAX), lik_rep = latent row of every
     * observation (device, replicates) or NULL (observation i reads row i), lik_par = robustmax's epsilon. */
    int lik_kind, lik_classes;
    int64_t lik_nobs;
    const int64_t *lik_rep;
    double lik_par;
} dgpamd_node;
enum { DGPAMD_LIK_POISSON = 1, DGPAMD_LIK_NEGBIN = 2, DGPAMD_LIK_ZIP = 3, DGPAMD_LIK_ZINB = 4, DGPAMD_LIK_BIN_LOGIT = 5,
       DGPAMD_LIK_BIN_PROBIT = 6, DGPAMD_LIK_ROBUSTMAX = 7, DGPAMD_LIK_SOFTMAX = 8 };

/* ---- a7  a likelihood node's log-likelihood of `batch` candidate blocks ------------
 * imputation.py:71-78,91-106 -> <likelihood>.llik(): sum_i log p(y_i | f_i) for every block X[b] (n x M, stride_x doubles
 * apart; 0: one block), f_i = row lik_rep[i] (or i), columns colmap.  out (device, batch); work: dgpamd_lik_workspace(batch)
 * bytes.  The sums are formed in a fixed order (the same bits as inside dgpamd_ess_queue). */
size_t dgpamd_lik_workspace(int batch);
int dgpamd_lik_loglik(dgpamd_ctx *ctx, const dgpamd_node *node, int64_t n, int M, const double *X, int64_t stride_x, int batch,
                      double *work, double *out);

/* ---- a7  one elliptical-slice update of a latent block, loop and all ------------
 * imputation.one_sample_block imputation.py:81-119 for the common case of ONE dense GP node upstairs: the
 * shrinking-bracket loop runs here (speculative batches: propose -> batched log-likelihood -> one result copy per
 * batch), so an update costs one library call instead of several host round trips per batch.
 *   F (n x M, device): current latent block, overwritten by the accepted proposal; NU: the prior draw;
 *   node: the upper node (its Xloc / ldloc are ignored: the proposals are its local input through node->colmap);
 *   scale: its variance; log_y: the slice threshold; state[4] = {theta, lo, hi, pending}: the current angle and
 *   bracket (pending != 0: the last batch was rejected and its closing shrink still needs a uniform);
 *   uniforms[nuni]: the next draws of the sampler's uniform stream, consumed exactly as the sequential loop
 *   (imputation.py:115-119) would; batch_first / batch_next: speculative proposals per batch;
 *   FP (batch_first x n x M), A (batch_first x Np x Np), work (dgpamd_potrf_workspace(n, batch_first)),
 *   ll_dev (batch_first doubles), info_dev (batch_first int32): device scratch.
 * out[6] = {status, uniforms consumed, proposals evaluated, batches, accepted log-likelihood, info}: status 0 =
 * accepted, 1 = uniforms used up (call again with more; state is updated), 2 = a proposal's matrix is not positive
 * definite (info = the LAPACK-style index). */
int dgpamd_ess_update(dgpamd_ctx *ctx, int64_t n, int M, double *F, const double *NU, const dgpamd_node *node, double scale,
                      double log_y, double *state, const double *uniforms, int nuni, int batch_first, int batch_next,
                      double *FP, double *A, void *work, double *ll_dev, int32_t *info_dev, double *out);

/* ---- a7  several elliptical-slice updates of a latent block queued without host synchronisation ------------
 * imputation.py:44-119, the accept / shrink loop advanced on the device: after every speculative batch a one-thread
 * kernel compares the batch's log-likelihoods (summed over the `nnodes` dense GP nodes of the layer above) with the
 * threshold, takes the first accepted proposal into F or shrinks the bracket, and moves the cursor into the uniform
 * stream exactly as the sequential loop would; the launches of an update's later batches are predicated on its `done`
 * word.  `nupd` updates (prior draws NU: nupd x n x M) are queued on the context's stream and the call returns at once.
 *   state (device, DGPAMD_ESS_STATE doubles): {theta, lo, hi, pending, cursor, status, info, ll, log_y, proposals,
 *     batches, updates}; the caller zeroes it and sets cursor / ll as needed (compute_ll0 = 1: ll is computed from F first; compute_ll0 = 2 (round 6): the FIRST
 *     update of this call is the update an earlier queue left open -- out of queued batches (status 3) or of uploaded uniforms (1): the caller writes the state back with
 *     status and counters zeroed and the cursor at the start of this call's uniforms, theta / lo / hi / pending / log_y / ll as fetched, and the update goes on where it stopped).
 *     status after the queue: 0 = every update accepted; 1 = uniforms used up; 2 = a proposal the sequential loop reaches
 *     is not positive definite (info); 3 = an update was not accepted within max_batches batches; 4 = uniforms used up
 *     before an update began (nothing of it is in the state).  After a non-zero status
 *     the later updates leave F alone: `updates` tells how many were completed, and {theta, lo, hi, pending, cursor, log_y}
 *     are those of the open update (resume it with dgpamd_ess_update).
 *   uniforms / log_uniforms (device, nuni): the sampler's next uniforms and their logarithms (taken on the host so
 *     that the thresholds are bit-identical to the host loop's).
 *   FP (batch_first x n x M), A (batch_first x Np x Np), work (dgpamd_potrf_workspace(n, batch_first)),
 *   scratch (dgpamd_ess_queue_scratch() bytes): device scratch.
 *   Vecchia nodes upstairs (nodes[k].vecch_nn != NULL, kernel_class.py:494-509): every batch gathers the candidates'
 *     ordered inputs and evaluates vecchia_llik for all of them in one row launch; vwork (dgpamd_ess_queue_vwork(n, max
 *     Dl + Dg, batch_first) bytes, device) holds the gathered inputs and the per-row partials.  A, work may be NULL when
 *     every node upstairs is a Vecchia node; vwork may be NULL when none is.
 *   A likelihood node upstairs (nodes[k].lik_kind != 0; scales_h[k] is ignored): the summed log-density of its observations.
 *   A queue may be continued: a later call on the same `state` that the caller has NOT zeroed carries on from its cursor,
 *     status and counters (ll is recomputed with compute_ll0 when the target changed) -- the layers of a deeper model are
 *     queued one update at a time this way, with one fetch of the state at the end. */
#define DGPAMD_ESS_STATE 16
size_t dgpamd_ess_queue_scratch(void);
size_t dgpamd_ess_queue_vwork(int64_t n, int D, int batch);
int dgpamd_ess_queue(dgpamd_ctx *ctx, int64_t n, int M, double *F, const double *NU, int nupd, const dgpamd_node *nodes,
                     const double *scales_h, int nnodes, double *state, const double *uniforms, const double *log_uniforms,
                     int nuni, int batch_first, int batch_next, int max_batches, int compute_ll0, double *FP, double *A,
                     void *work, void *scratch, void *vwork);
/* Folds the `count` info words of a factorisation queued between two updates of a queue (the prior factors of a deeper
 * layer, imputation.py:54-63) into the queue's state: the first non-zero one stops the queue with status 2. */
int dgpamd_ess_queue_note_info(dgpamd_ctx *ctx, double *state, const int32_t *info, int count);

/* ---- a8  M-step objective pieces -------------------------------------------
 * kernel.llik  kernel_class.py:403-449 restructured:
 *   tr_p   = sum_ij Kinv_ij dK_p,ij          (= trace(K^-1 dK_p))
 *   quad_p = sum_ij alpha_i alpha_j dK_p,ij  (= y^T K^-1 dK_p K^-1 y)
 * with dK_p recomputed in flight (never stored).  p runs over the lengthscales
 * (nlen == 1: the summed derivative) and, iff nugget_est, the nugget last.
 * out (host-visible after sync): out[0..P) = tr_p, out[P..2P) = quad_p.
 * Ainv: from dgpamd_potri (alpha is read from its row n, negated).             */
int dgpamd_grad_reduce(dgpamd_ctx *ctx, int kind, int64_t n,
                       const double *Xloc, int64_t ldloc, const int32_t *colmap_h, int Dl,
                       const double *Xglob, int Dg,
                       const double *length_h, int nlen, double nugget, const double *W, int nugget_est,
                       const double *Ainv, double *out, void *work);

/* kernel.llik's device part (kernel_class.py:403-449) for `batch` GP nodes of the same size n in ONE call -- the
 * lock-step M-step (dgp.py:1391-1398 fits the nodes one after another; their objectives are independent): per node
 * K assembly with its own inputs / hyper-parameters (y as augmented row), ONE batched factorisation and inverse,
 * per-node derivative reductions, ONE device-to-host copy.  The call returns after the results have landed:
 *   host_out[b * stride_out + ...] = { logdet K_b, y' K_b^-1 y, info (0 = PD), tr_p (P_b values), quad_p (P_b values) }
 * with P_b as in dgpamd_grad_reduce; stride_out >= 3 + 2 max P_b.  A, T, Ainv: batch x Np x Np buffers (stride
 * stride_a; see dgpamd_potrf_inv); work: dgpamd_potrf_workspace(n, batch); grad_work: batch x dgpamd_grad_workspace(n, max P_b)
 * (the nodes' reductions run side by side in one launch, like their K assemblies);
 * dev_out: device scratch of batch * (stride_out + 2) doubles. */
int dgpamd_llik_batch(dgpamd_ctx *ctx, int64_t n, int batch, const dgpamd_node *nodes, double *A, double *T, double *Ainv,
                      int64_t stride_a, void *work, void *grad_work, double *dev_out, double *host_out,
                      int64_t stride_out);
/* The same call in two halves (round 6): _launch queues everything and returns, _wait returns when the results have landed in host_out (the layout above).
 * Between the two the caller may do host work that does not touch the evaluations' inputs -- dgp.train's loop refreshes the nodes' numpy attributes from the I-step's
 * device state and runs the R2 diagnostics (dgp.py:1391-1398 would do both BEFORE the first objective evaluation) while the device works on the M-step's first round.
 * One evaluation in flight per context; every other entry point stays usable in between (the results have a pinned staging buffer of their own). */
int dgpamd_llik_batch_launch(dgpamd_ctx *ctx, int64_t n, int batch, const dgpamd_node *nodes, double *A, double *T, double *Ainv,
                             int64_t stride_a, void *work, void *grad_work, double *dev_out, int64_t stride_out);
int dgpamd_llik_batch_wait(dgpamd_ctx *ctx, double *host_out);
size_t dgpamd_grad_workspace(int64_t n, int nparam);

/* ---- a11  GP prediction ------------------------------------------------------
 * functions.gp  functions.py:379-394 (+ K_vec_nb vecchia.py:244-265):
 *   m_t = Rinv_y . r_t ,  v_t = | scale (1 + nugget - r_t^T Rinv r_t) |
 * x: (M x D) test inputs already concatenated [local | global]; Wtr: (n x D)
 * training inputs; Rinv: n x n symmetric with leading dimension ldr.
 * ry: (nry x n) -- several R^-1 y at once: for a first-layer node R^-1 and the
 * variance are identical in every imputation, only y (hence the mean) differs
 * (emulation.py:701-734 recomputes both per imputation).  mean: (nry x M); var: (M).
 * work: dgpamd_gp_workspace(n, M) bytes.                                       */
size_t dgpamd_gp_workspace(int64_t n, int64_t M);
int dgpamd_gp_predict(dgpamd_ctx *ctx, int kind, int64_t n, int64_t M, int D,
                      const double *x, const double *Wtr, const double *length_h, int nlen,
                      const double *Rinv, int64_t ldr, const double *ry, int nry, double scale, double nugget,
                      double *mean, double *var, void *work);

/* ---- joint posterior of test points and sample paths (emulator.sample_paths / gp.sample_paths) ------------------
 * The joint form of functions.gp  functions.py:379-394 (which returns the diagonal only) -- the posterior analogue of
 * the prior paths of path.generate  synthetic.py:20-44.  Item b (batch <= DGPAMD_MAXB) has test inputs x_b (M x D,
 * batch stride stride_x, [local | global]) and a group g = group_h[b] (host; NULL: all 0) < ngroups that selects
 * training inputs W_g (n x D, stride_w), Linv_g = L^-1 of the training correlation matrix R = L L^T (ld = ldl,
 * stride_l; the lower 64x64 tiles of [0,n)^2 are read, entries above the diagonal ignored: what dgpamd_potri leaves
 * in A) and r right-hand-side rows y_g (r x n, stride_y).  With K* = K(W, x_b), V = L^-1 K*, w = L^-1 y^T:
 *   A_b    = Sigma_b = scale (K(x_b, x_b) + nugget I - V^T V): lower tiles of a dgpamd_potrf buffer (ld =
 *            dgpamd_padded_dim(M), batch stride stride_a, padding zero, no right-hand sides);
 *   mean_b = V^T w  (M x r, batch stride M r; may be NULL iff r == 0).
 * diag(Sigma_b) is dgpamd_gp_predict's variance, mean_b its mean.  work: dgpamd_joint_workspace(n, M, r, batch) bytes. */
size_t dgpamd_joint_workspace(int64_t n, int64_t M, int r, int batch);
int dgpamd_joint_cov(dgpamd_ctx *ctx, int kind, int64_t n, int64_t M, int D, int r, int batch,
                     const double *x, int64_t stride_x, const int32_t *group_h, int ngroups,
                     const double *W, int64_t stride_w, const double *Linv, int64_t ldl, int64_t stride_l,
                     const double *y, int64_t stride_y, const double *length_h, int nlen, double scale, double nugget,
                     double *A, int64_t stride_a, double *mean, void *work);
/* Joint draws from the factored covariances: out_b = mean_b(:, q / rep) + L_b E_b, with L_b the factor
 * dgpamd_potrf left in a buffer of dgpamd_joint_cov (ld = dgpamd_padded_dim(M), batch stride stride_l; scale is
 * already inside it), E_b (M x c) standard normals, mean_b (M x c / rep; may be NULL) and out_b (M x c), each with its
 * own batch stride.  c == 1: one wave per row; c > 1: triangular matrix product on f64 MFMA. */
int dgpamd_mvn_paths(dgpamd_ctx *ctx, int64_t M, int c, int rep, int batch, const double *L, int64_t stride_l,
                     const double *mean, int64_t stride_m, const double *E, int64_t stride_e, double *out,
                     int64_t stride_o);

/* ---- a12-a14  linked-GP prediction ------------------------------------------
 * functions.link_gp  functions.py:396-430 with IJ_sexp :432-451 / IJ_matern
 * :453-494 (Jd, Jd0 vecchia.py:915-988), trace_sum :496-506, quad vecchia.py:990:
 *   mean_t = I_t . ry ,  var_t = | ry^T J_t ry - mean_t^2 + scale (1 + nugget - tr(Rinv J_t)) |
 * m, v: (M x Dw) input moments; z: (M x Dz) deterministic global inputs (NULL iff
 * Dz == 0); Wtr: (n x Dw), Wg: (n x Dz).  Psexp/R2sexp are never materialised. */
size_t dgpamd_linkgp_workspace(int64_t n, int64_t M, int Dw);
/* Matern-2.5: by default the J factor is evaluated through its separable form (every erf/exp depends on one
 * training point: Jd = <S(x_min), T(x_max)> + (erf_hi - erf_lo) <S', T'>, csrc/linkfun.hpp), which agrees with the
 * reference's expression to ~1e-11; enable = 1 evaluates the reference's direct expression (vecchia.py:915-959). */
int dgpamd_set_linkgp_direct(dgpamd_ctx *ctx, int enable);

/* Diagnostics: when device_buf (>= 4096 int64 in device memory) is set, the factorisation kernels of matrix 0 write
 * wall_clock64() stamps of their phases into it (16 slots per launch; tools/gpu_potrf_trace.py decodes them).
 * NULL switches it off (the default). */
int dgpamd_debug_trace(dgpamd_ctx *ctx, long long *device_buf);
/* Diagnostics of the one-launch factorisation (tools/gpu_mega_tasklog.py): when device_buf (`words` int64 of device memory) is
 * set, every chain step and every worker task of every matrix writes its wall_clock64() stamps into it -- chain step k of matrix b
 * at 64 + 8 (b nbk + k): start, factored, panel tile staged, diagonal tile seen, solved, updated; task `slot` of matrix b at
 * 64 + 8 batch nbk + 8 (b ntask + slot): pulled, inputs seen, arithmetic done, W_k seen, stored, published, workgroup.  A log that
 * would not fit is not written.  dgpamd_debug_mega_table copies the task table those slots index (8 int32 per task as MTask, then
 * 2 int32 per block: the visits of A[k+1][k] and A[k+1][k+1] the chain waits for) and returns the number of tasks, or a
 * negative status.  NULL switches the log off (the default).  With DGPAMD_JSEP_LOG=1 in the environment the same buffer takes the
 * step log of the next Matern pair-kernel launch of dgpamd_linkgp_predict instead (per workgroup 8 + 48 x 4 x 2 int64 from word 64:
 * start / end on the 100-MHz clock and in shader cycles, HW_ID, XCC_ID, tile, steps; then per step and wave the cycle counts at the
 * arrival at and the departure from the step's barrier, the order class in the top bits: tools/gpu_pair_steplog.py). */
int dgpamd_debug_tasklog(dgpamd_ctx *ctx, long long *device_buf, long long words);
int dgpamd_debug_mega_table(dgpamd_ctx *ctx, int64_t n, int inv, int batch, int32_t *host_out, int64_t cap_words);
int dgpamd_linkgp_predict(dgpamd_ctx *ctx, int kind, int64_t n, int64_t M, int Dw, int Dz,
                          const double *m, const double *v, const double *z,
                          const double *Wtr, const double *Wg, const double *length_h, int nlen,
                          const double *Rinv, int64_t ldr, const double *ry, double scale, double nugget,
                          double *mean, double *var, void *work);
/* Leave-one-out form of the same prediction (emulation.py:90-143 with a dense emulator: vecchia.py:23-26 and
 * kernel_class.py:647-664 hand test row k all training points but row k): drop[t] in [0, n) is the training point
 * left out of the conditioning set of test point t (any index: the kernel does not assume drop[t] == t).  Nothing is refactorised: with u = Rinv[:, d], (R_-d)^-1 = Rinv - u u^T / u_d
 * (embedded), applied inside the pair weights.  Same workspace as dgpamd_linkgp_predict. */
int dgpamd_linkgp_loo(dgpamd_ctx *ctx, int kind, int64_t n, int64_t M, int Dw, int Dz,
                      const double *m, const double *v, const double *z,
                      const double *Wtr, const double *Wg, const double *length_h, int nlen,
                      const double *Rinv, int64_t ldr, const double *ry, const int32_t *drop, double scale,
                      double nugget, double *mean, double *var, void *work);

/* ---- a15  imputation-moment accumulation (emulation.py:846-847) --------------
 * sum_mu += mu ; sum_m2 += mu^2 + var   (count elements).  finalize:
 * mu = sum_mu / S ; var = sum_m2 / S - mu^2.                                   */
int dgpamd_moments_accumulate(dgpamd_ctx *ctx, int64_t count, const double *mu, const double *var,
                              double *sum_mu, double *sum_m2);
int dgpamd_moments_finalize(dgpamd_ctx *ctx, int64_t count, double S, double *sum_mu_to_mu, double *sum_m2_to_var);

/* ---- a17  Vecchia neighbour search --------------------------------------------
 * vecchia.nn  vecchia.py:61-109: NNarray (n x (m+1)) int64, row i = i and its <= m
 * nearest EARLIER points (exact, squared-euclidean on x), sorted by index
 * descending, -1 padded.  vecchia.get_pred_nn  vecchia.py:20-40: (M x m) nearest
 * training points, nearest first.  x, q are already divided by the lengthscales. */
int dgpamd_nn_ordered(dgpamd_ctx *ctx, int64_t n, int D, const double *x, int m, int64_t *NNarray);
int dgpamd_nn_query(dgpamd_ctx *ctx, int64_t M, int64_t n, int D, const double *q, const double *x, int m, int64_t *NN);

/* Debugging aid: fill the LDS of every CU with NaNs (a kernel that reads LDS it has not written then shows it in its results
 * whatever ran before).  DGPAMD_POISON_LDS=1 does this before the Vecchia row / prediction launches, =2 makes the Python
 * engine call this entry point before every library call. */
int dgpamd_debug_poison_lds(dgpamd_ctx *ctx);

/* Testing aid: the library's own device math functions, one lane per element (csrc/mathprobe.hip calls the functions the
 * kernels inline, not copies).  a, out0, out1: `count` doubles each; out1 may be NULL where fn has one result.
 *   fn                              out0                 out1
 *   DGPAMD_FN_EXP_NEGATED           exp(-a)
 *   DGPAMD_FN_EXP_NEGATED_V3        exp(-a)
 *   DGPAMD_FN_EXP_NEGATED_TAB       exp(-a)
 *   DGPAMD_FN_EXP_NEGATED_TAB2      exp(-a)                        (exp_negated_tab_begin + _end)
 *   DGPAMD_FN_COS_REDUCED           cos(a)
 *   DGPAMD_FN_COS_SIN_REDUCED       cos(a)               -sin(a)
 *   DGPAMD_FN_RSQRT                 1/sqrt(a)                      (rsqrt_f64)
 *   DGPAMD_FN_RSQRT_SQRT            1/sqrt(a)            sqrt(a)
 *   DGPAMD_FN_RCP                   1/a                            (rcp_f64)
 *   DGPAMD_FN_DLOG_MATERN25         dlog_factor<matern2.5>(a)
 *   DGPAMD_FN_DLOG_SEXP             dlog_factor<sexp>(a)
 *   DGPAMD_FN_EXP_TABLE             tab[(int)a], the table of exp_negated_tab as the kernels build it in LDS ((int)a taken mod 256)
 *   DGPAMD_FN_TRI_DECODE            bi                   bj        of tri_decode((int)a)
 * An unknown fn, count <= 0 or a null pointer (out1 where fn has two results included): DGPAMD_BAD_ARG. */
#define DGPAMD_FN_EXP_NEGATED 0
#define DGPAMD_FN_EXP_NEGATED_V3 1
#define DGPAMD_FN_EXP_NEGATED_TAB 2
#define DGPAMD_FN_EXP_NEGATED_TAB2 3
#define DGPAMD_FN_COS_REDUCED 4
#define DGPAMD_FN_COS_SIN_REDUCED 5
#define DGPAMD_FN_RSQRT 6
#define DGPAMD_FN_RSQRT_SQRT 7
#define DGPAMD_FN_RCP 8
#define DGPAMD_FN_DLOG_MATERN25 9
#define DGPAMD_FN_DLOG_SEXP 10
#define DGPAMD_FN_EXP_TABLE 11
#define DGPAMD_FN_TRI_DECODE 12
#define DGPAMD_FN_COUNT 13
int dgpamd_debug_mathfn(dgpamd_ctx *ctx, int fn, int64_t count, const double *a, double *out0, double *out1);

/* Testing aid: the Matern-2.5 linked-GP factors of csrc/linkfun.hpp (the functions themselves, not copies), one lane per case.
 * args: count x 5 doubles, rows of (X1, X2, m, v, l): the two points, and the mean, variance and lengthscale of Z ~ N(m, v);
 * out: count doubles.  v == 0 gives the product of point correlations, as in every kernel that calls these functions.
 *   DGPAMD_LINK_I       E[k(X1, Z)]                   matern_I_dim
 *   DGPAMD_LINK_JD      E[k(X1, Z) k(X2, Z)]          matern_Jd
 *   DGPAMD_LINK_JD0     E[k(X1, Z)^2]                 matern_Jd0
 *   DGPAMD_LINK_JSEP    E[k(X1, Z) k(X2, Z)]          matern_role_S(min) . matern_role_T(max), combined as the pair kernels do
 *   DGPAMD_LINK_JSEP0   E[k(X1, Z)^2]                 both roles on X1 (the diagonal of the separable kernels)
 *   DGPAMD_LINK_ERFCX   exp(X1^2) erfc(X1)            the device erfcx those functions call
 * An unknown fn, count <= 0 or a null pointer: DGPAMD_BAD_ARG. */
#define DGPAMD_LINK_I 0
#define DGPAMD_LINK_JD 1
#define DGPAMD_LINK_JD0 2
#define DGPAMD_LINK_JSEP 3
#define DGPAMD_LINK_JSEP0 4
#define DGPAMD_LINK_ERFCX 5
#define DGPAMD_LINK_COUNT 6
int dgpamd_debug_linkfn(dgpamd_ctx *ctx, int fn, int64_t count, const double *args, double *out);

/* ---- a19-a21  Vecchia likelihoods and sampler ---------------------------------
 * vecchia_llik vecchia.py:164-180 ; vecchia_nllik :182-242 (raw sums; the host
 * finishes the scale_est / replicate branches) ; L_matrix :409-424 ;
 * forward_solve_sp :111-120.  X: (n x D) ordered inputs; y: (n); nugget_diag: (n).
 * out_llik (device, 2 doubles): {quad, logdet}.  out_nllik (device, 2+2P
 * doubles): {quad, logdet, dquad[P], dlogdet[P]}, P = nlen (+1 iff nugget_est). */
int dgpamd_vecchia_llik(dgpamd_ctx *ctx, int kind, int64_t n, int D, int m, const double *X, const double *y,
                        const int64_t *NNarray, const double *length_h, int nlen, double nugget,
                        const double *nugget_diag, double *out_llik);
/* The same for `batch` input sets at once (the candidate blocks of one speculative ESS batch, imputation.py:91-106
 * called once per proposal): X holds them x_stride doubles apart, y / NNarray / nugget_diag are shared; out_llik
 * (device, batch x 2 doubles).  One row launch and one reduction for the whole batch. */
int dgpamd_vecchia_llik_batch(dgpamd_ctx *ctx, int kind, int64_t n, int D, int m, const double *X, int64_t x_stride,
                              int batch, const double *y, const int64_t *NNarray, const double *length_h, int nlen,
                              double nugget, const double *nugget_diag, double *out_llik);
int dgpamd_vecchia_nllik(dgpamd_ctx *ctx, int kind, int64_t n, int D, int m, const double *X, const double *y,
                         const int64_t *NNarray, const double *length_h, int nlen, double nugget,
                         const double *nugget_diag, int nugget_est, double *out_nllik);
int dgpamd_vecchia_lmatrix(dgpamd_ctx *ctx, int kind, int64_t n, int D, int m, const double *X,
                           const int64_t *NNarray, const double *length_h, int nlen, double nugget, double *Lmat);
int dgpamd_vecchia_spsolve(dgpamd_ctx *ctx, int64_t n, int m, const double *Lmat, const int64_t *NNarray,
                           double inv_sqrt_scale, const double *b, double *x);
/* The same for nmat matrices (Lmat, NNarray: nmat x n x (m+1); inv_sqrt_scale: nmat, device) with nrhs right-hand
 * sides each (b, x: nmat x nrhs x n): one workgroup per chain -- fmvn_sp (vecchia.py:133-140) for all nodes of a
 * layer and all sweeps of imputer.sample (imputation.py:54-63) in one launch.                                   */
int dgpamd_vecchia_spsolve_batch(dgpamd_ctx *ctx, int64_t n, int m, int nmat, int nrhs, const double *Lmat,
                                 const int64_t *NNarray, const double *inv_sqrt_scale, const double *b, double *x);
/* The same substitution level-scheduled (rows whose dependencies are all solved run side by side: a few hundred steps
 * instead of n).  dgpamd_vecchia_levels builds the schedule of each of the nmat neighbour arrays (it depends on the array
 * only: once per ordering, kernel_class.py:245-277) into sched (device, dgpamd_vecchia_levels_bytes(n, nmat));
 * dgpamd_vecchia_spsolve_levels then solves like dgpamd_vecchia_spsolve_batch (same arguments, same results up to the
 * order of each row's sum: a fixed 32-lane butterfly instead of left to right). */
size_t dgpamd_vecchia_levels_bytes(int64_t n, int nmat);
int dgpamd_vecchia_levels(dgpamd_ctx *ctx, int64_t n, int m, int nmat, const int64_t *NNarray, void *sched);
int dgpamd_vecchia_spsolve_levels(dgpamd_ctx *ctx, int64_t n, int m, int nmat, int nrhs, const double *Lmat,
                                  const int64_t *NNarray, const double *inv_sqrt_scale, const double *b, double *x,
                                  const void *sched);
/* Hetero likelihood under Vecchia: rows of the sparse factor of the latent mean's conditional posterior
 * (vecchia.U_matrix :426-446 / U_matrix_sp :599-610 through kernel.ord_nn(pointer=True) kernel_class.py:268-275;
 * consumer Hetero.post_het_vecch likelihood_class.py:166-182).  X: (n x D) ORDERED inputs; impNN: (n x (m+1))
 * imp_NNarray; gamma, y: (n) ordered noise variances and observations (site-pooled with replicates).
 * Out, in dgpamd_vecchia_spsolve's layout: Lrows (n x (m+1)), NNl (n x (m+1)), and t = U_ol^T y (n):
 * f = -solve(t) + solve(z) is the draw in ordered coordinates.  info (device int32): 0, or 1 + the first row whose
 * block is not positive definite (the reference's np.linalg.cholesky raises LinAlgError there).             */
int dgpamd_vecchia_het_rows(dgpamd_ctx *ctx, int kind, int64_t n, int D, int m, const double *X,
                            const int64_t *impNN, const double *length_h, int nlen, double scale,
                            const double *gamma, const double *y, double *Lrows, int64_t *NNl, double *t, int32_t *info);

/* ---- a22/a23  Vecchia prediction -------------------------------------------------
 * gp_vecch vecchia.py:635-654 ; link_gp_vecch :758-796 (IJ_nb :838-907).
 * NN: (M x pm) conditioning sets, the valid entries first, -1 padded.  Up to 51 (gp; D <= 16) resp. 50 (link_gp, squared
 * exponential, Dw <= 8, Dz <= 8) neighbours run in the register-resident kernels (csrc/vecchia_pred.hip, csrc/vecchia_pred_link_*.hip: one wave per test
 * point, no LDS); larger sets, wider inputs and the Matern link_gp in the one-wave-per-point LDS kernels (csrc/vecchia_gp.hip:
 * conditioning sets up to what fits 160 KiB of LDS).  DGPAMD_VECCHIA_LDS=1 selects the LDS kernels throughout (the tests compare the two). */
int dgpamd_vecchia_gp(dgpamd_ctx *ctx, int kind, int64_t M, int64_t n, int D, int pm, const double *x,
                      const double *w, const int64_t *NN, const double *y, double scale,
                      const double *length_h, int nlen, double nugget, const double *nugget_diag,
                      double *mean, double *var);
int dgpamd_vecchia_linkgp(dgpamd_ctx *ctx, int kind, int64_t M, int64_t n, int Dw, int Dz, int pm,
                          const double *m, const double *v, const double *z, const double *w1, const double *wg,
                          const int64_t *NN, const double *y, double scale, const double *length_h, int nlen,
                          double nugget, const double *nugget_diag, double *mean, double *var);

/* ---- Vecchia joint sample paths (DESIGN I.11) --------------------------------------
 * One GP node, M test rows per path in one order pi.  Position i conditions on c(i): the min(m, n + i) nearest of the n
 * training rows and the path's test rows at positions < i, squared-euclidean on coordinates already divided by the
 * lengthscales, in (distance, combined index) order -- combined index j < n: training row j; n + i': test position i'.
 * dgpamd_vpaths_nn: q (P x M x D) the paths' test rows in order pi; x (G x n x D) training sets; group (device int32, P,
 * or NULL: all 0) picks each path's set.  NN (P x M x m): c(i) nearest first, -1 padded.  m <= 256.
 * dgpamd_vpaths_rows: with A the correlation block over c(i) (diagonal 1 + jitter + nugget * omega_j on training members,
 * omega NULL: 1; 1 + jitter + nugget on test members), a = k(c(i), u_i), b_i = A^-1 a, d_i = scale (1 + jitter + nugget -
 * a^T b_i), the draw  v_i = sum_train b_ij y_j + sum_test b_ij v_j + sqrt(d_i) z_i  is emitted in dgpamd_vecchia_spsolve's
 * layout (unit scale): Lrows / NNl (P x M x (m+1)) = [1/sqrt(d_i), -b_ij/sqrt(d_i) over c(i)'s TEST members in list order,
 * 0..] / [i, their test positions, -1..]; t (P x nrhs x M) = sum over training members of b_ij y[group][r][j] for the nrhs
 * right-hand sides y (G x nrhs x n); sd (P x M) = sqrt(d_i).  The substitution with b = z + t / sd (dgpamd_vecchia_levels,
 * dgpamd_vecchia_spsolve_levels) then gives v.  info (device int32): 0, or 1 + some p*M + i whose block is not positive
 * definite.  m <= 51 with D <= 16 runs register-resident; otherwise one wave per row with the block in LDS, and a block
 * over a CU's 160 KiB returns DGPAMD_BAD_ARG before anything is launched.  DGPAMD_VECCHIA_LDS=1 forces the LDS kernel. */
int dgpamd_vpaths_nn(dgpamd_ctx *ctx, int64_t P, int64_t M, int64_t n, int D, int m, const double *q, const double *x,
                     const int32_t *group, int64_t *NN);
int dgpamd_vpaths_rows(dgpamd_ctx *ctx, int kind, int64_t P, int64_t M, int64_t n, int D, int m, int nrhs, const double *q,
                       const double *x, const int32_t *group, const int64_t *NN, const double *omega, const double *y,
                       double scale, double nugget, double jitter, double *Lrows, int64_t *NNl, double *t, double *sd,
                       int32_t *info);

/* ---- function-valued posterior draws (pathwise conditioning, DESIGN I.12) ---------------------------------
 * One GP node, P paths, M rows.  Path p is the closed-form function
 *   out[p][m] = sqrt(scale) ( sqrt(2/F) sum_f theta[p][f] cos(Omega_f . x_m + b_f) + sum_i v[p][i] c(x_m, W_g(p)[i]) ):
 * a random-Fourier-feature draw of the prior (Omega F x D, b F, theta P x F) plus the update that conditions it on the
 * training set (v P x n; c the node's correlation function with lengthscales length_h, one or D of them).  x is shared by
 * every path (M x D, stride_x == 0: the products run on f64 MFMA against tiles of features and correlations generated on
 * the fly; every path then uses one training set, group_h NULL or constant) or one per path (P x M x D, stride_x >= M D:
 * one lane per row).  group_h (host, P; NULL: all 0) < ngroups picks path p's training inputs W_g (n x D, stride_w between
 * groups).  n == 0 (W, v may be NULL) evaluates the prior draw alone; evaluated at x = W that is the Phi(W) theta the
 * weights v need.  D <= DGPAMD_MAXD, any P and M; neither Phi(x) nor c(x, W) is stored and no workspace is used.  Each
 * out[p][m] is one fixed sequence of operations on row m alone: the same bits whichever rows share the call. */
int dgpamd_pathfun_eval(dgpamd_ctx *ctx, int kind, int64_t n, int64_t M, int D, int64_t F, int P, const double *x,
                        int64_t stride_x, const int32_t *group_h, int ngroups, const double *W, int64_t stride_w,
                        const double *Omega, const double *b, const double *theta, const double *v,
                        const double *length_h, int nlen, double scale, double *out);

/* ---- input gradients of function-valued posterior draws (DESIGN I.13) --------------------------------------
 * dgpamd_pathfun_eval's arguments and a second output: out (P x M) the values, bit for bit dgpamd_pathfun_eval's, and
 *   out_g[p][m][d] = d out[p][m] / d x_md
 *     = sqrt(scale) ( -sqrt(2/F) sum_f theta[p][f] Omega_fd sin(Omega_f . x_m + b_f) + sum_i v[p][i] c(x_m, W_i) q_d(x_m, W_i) ),
 * q_d = d log c / d x_d (sexp: -2 t_d / g_d; matern2.5: -(5/3) t_d (1 + sqrt5 |t_d|) / (1 + sqrt5 |t_d| + (5/3) t_d^2) / g_d with
 * t_d = (x_md - W_id) / g_d: zero and smooth at t_d = 0), in the node's own D input columns (P x M x D), from one pass: the sine
 * comes from the cosine's argument reduction, the correlation and the coefficients are the value's.  Shared x with D <= 10 runs
 * on f64 MFMA with D derivative tiles next to the generated tile; everything else one lane per row (shared x: a zero path
 * stride, and the values from dgpamd_pathfun_eval's own kernel in a launch of its own, to keep its order of summation).  Checks and status codes as dgpamd_pathfun_eval; nothing but the two outputs is stored and no workspace is used.
 * Each out_g[p][m][:] is one fixed sequence of operations on row m alone: the same bits whichever rows share the call. */
int dgpamd_pathfun_grad(dgpamd_ctx *ctx, int kind, int64_t n, int64_t M, int D, int64_t F, int P, const double *x,
                        int64_t stride_x, const int32_t *group_h, int ngroups, const double *W, int64_t stride_w,
                        const double *Omega, const double *b, const double *theta, const double *v,
                        const double *length_h, int nlen, double scale, double *out, double *out_g);

/* ---- function-valued posterior draws by local conditioning (DESIGN I.14) -----------------------------------
 * The pathwise update of a draw through the Vecchia predictor (gp_vecch, vecchia.py:635-654) in place of the dense
 * c(x, W) R^-1 r.  One GP node, R rows.  Row i conditions on N(i), its neighbours NN[i] (R x pm, the valid entries first, -1
 * padded: dgpamd_nn_query's) among the n training rows; with A the correlation block over N(i), diagonal 1 + jitter +
 * nugget * omega_j (omega NULL: 1), and a = c(W_N, x_i):
 *   b_i = A^-1 a,    out = sqrt(scale) (prior + sum_j b_ij r[N_j]).
 * x (R x D) and w (n x D) are coordinates already divided by the lengthscales; prior is dgpamd_pathfun_eval's n = 0 result
 * at scale 1; r the path's residual y / sqrt(scale) - Phi(W) theta - sqrt(nugget omega) * eps.
 *   rows_per_path == 0  shared rows: every row serves all P paths and its block is factored once.  r is NEIGHBOUR-MAJOR
 *       (n x P) and prior and out are ROW-MAJOR OVER PATHS (R x P): the lanes run over the paths, so the 64 residuals of a
 *       training row and the 64 outputs of a row are consecutive doubles (coalesced loads and stores).
 *   rows_per_path = M   per-path rows: R = P * M, row i belongs to path i / M; r is (P x n), prior and out are (P x M).
 *       One call holds one training set: a caller with several (groups of paths) makes one call per group.
 * jitter_h: the ladder of njitter (1 to 4) host doubles, tried in order ROW BY ROW: a block with a non-positive pivot or
 * Schur complement is rebuilt with the next rung by the wave that owns it, so a row's result never depends on the rows that
 * share its call.  info (2 device int32): [0] the number of rows that needed a rung beyond the first; [1] 1 + the smallest
 * row index whose block failed every rung, -1 when none did (an unsigned atomic minimum: deterministic).
 * out is one chain  acc = prior; acc = fma(b_ij, r[N_j], acc), j in list order; out = sqrt(scale) acc  in either form: the
 * same row gives the same bits in any call, block or position.  pm <= 51 with D <= 16 runs register-resident (one wave per
 * row, four per workgroup); otherwise one wave per row with the block in LDS, and a block over a CU's 160 KiB returns
 * DGPAMD_BAD_ARG before anything is launched.  DGPAMD_VECCHIA_LDS=1 forces the LDS kernel. */
int dgpamd_vpathfun_update(dgpamd_ctx *ctx, int kind, int64_t R, int64_t n, int D, int pm, int64_t P, int64_t rows_per_path,
                           const double *x, const double *w, const int64_t *NN, const double *omega, const double *r,
                           const double *prior, double scale, double nugget, const double *jitter_h, int njitter,
                           double *out, int32_t *info);

/* ---- the exact predictive distribution: an equal-weight mixture of S Gaussians per point-output (DESIGN I.15) ----
 * mu, var: (S x count) device doubles, count = M * K point-outputs, component s of entry e at [s * count + e] (the layout of
 * the layer walk's per-imputation moments); weights 1 / S.  A component with var <= 0 is a point mass at mu: its cdf is the
 * right-continuous step 1{y >= mu}, it has no density term, and the log density is -inf where no component has var > 0.
 * With x_s = (y - mu_s) / sqrt(2 var_s):
 *   DGPAMD_MIX_CDF     out = (1/S) sum_s erfc(-x_s) / 2
 *   DGPAMD_MIX_SF      out = (1/S) sum_s erfc(+x_s) / 2           (summed from the upper tails, not 1 - cdf)
 *   DGPAMD_MIX_LOGPDF  out = log (1/S) sum_s exp(-x_s^2) / sqrt(2 pi var_s), a log-sum-exp with the maximum taken first
 * y: thresholds per entry (count x T, y_stride = T) or shared by all entries (T, y_stride = 0); out (count x T).
 * dgpamd_mixture_quantile: out[e, t] = inf{q : F_e(q) >= p[t]}.  p and zp (the standard normal quantiles of p) are T HOST
 * doubles, T <= DGPAMD_MIX_MAXT, 0 < p < 1.  Start bracket [min_s, max_s] of mu_s + zp sigma_s; Newton steps on the log of
 * the smaller tail (lower for p <= 1/2, upper above) taken only inside the bracket, else its midpoint; stops when the
 * bracket is 2^-52 max(|q|, max_s |mu_s|) wide, after at most 400 iterations.  info (1 device int32): the number of (e, t)
 * that reached the iteration limit (expected 0).  With S = 1, or S equal components, out = fma(zp, sqrt(var), mu).
 * dgpamd_mixture_crps: with A(m, v) = 2 sqrt(v) phi(m / sqrt(v)) + m (2 Phi(m / sqrt(v)) - 1), A(m, 0) = |m|,
 *   out[e] = (1/S) sum_s A(y_e - mu_s, var_s) - (1 / 2S^2) [sum_s A(0, 2 var_s) + 2 sum_{s<t} A(mu_s - mu_t, var_s + var_t)],
 * y, out: count doubles.
 * Every output is one fixed sequence of operations on its own entry's components: any slice of a call gives the same bits.
 * path (quantile, crps): 0 -- the kernel that stages an entry's components in LDS (64 entries x S x 2 doubles per wave)
 * while eight such waves fit a CU (S <= 20), the one that re-reads global memory above that; 1 / 2 ask for the LDS kernel
 * (S <= 160) / the global kernel: the same arithmetic on the same numbers.  count = 0 returns DGPAMD_OK without a launch.  DGPAMD_BAD_ARG before any launch: S < 1,
 * T < 1, a p outside (0, 1), a null pointer.  (mu is device memory: a NaN in it is refused by the Python front,
 * PredictiveMixture; the kernels pass it through as NaN and never loop on it.) */
#define DGPAMD_MIX_CDF 0
#define DGPAMD_MIX_SF 1
#define DGPAMD_MIX_LOGPDF 2
#define DGPAMD_MIX_MAXT 32
int dgpamd_mixture_eval(dgpamd_ctx *ctx, int what, int S, int64_t count, int T, const double *mu, const double *var,
                        const double *y, int64_t y_stride, double *out);
int dgpamd_mixture_quantile(dgpamd_ctx *ctx, int S, int64_t count, int T, const double *mu, const double *var,
                            const double *p, const double *zp, int path, double *out, int32_t *info);
int dgpamd_mixture_crps(dgpamd_ctx *ctx, int S, int64_t count, const double *mu, const double *var, const double *y,
                        int path, double *out);

/* ---- pick-freeze sums for Sobol' indices of function-valued draws (DESIGN I.16) ----
 * fA, fB, fAB: the values of P paths at M design rows with K outputs, (P x M x K) device doubles, K fastest: at the rows of
 * the base sample A, of B, and of AB_i (A with column i taken from B).  shift: (P x K) device doubles; every value enters as
 * g = f - shift[p, k], one IEEE subtraction (the indices do not depend on the shift: the caller passes f_A at the first row
 * of the whole design, which takes the cancellation out of sum g^2 for a path with a large mean).
 * dgpamd_sobol_tiles: a tile is 64 consecutive rows (the last one may be short), ntiles = ceil(M / 64).
 *   fAB == NULL:  partial[t, p, k, 0..3] = sum g_A, sum g_B, sum g_A^2, sum g_B^2
 *   otherwise:    partial[t, p, k, 0..1] = sum g_B (g_AB - g_A)   (Saltelli 2010, first-order numerator),
 *                                          sum (g_A - g_AB)^2     (Jansen, total-order numerator)
 * over the rows of tile t; partial: (ntiles x P x K x 4 or 2) device doubles.  One row per lane; every product is rounded once
 * and the 64 terms are added by one fixed tree (lanes past the end of a short tile add +0).
 * dgpamd_sobol_add: sums[c] = (((sums[c] + partial[0, c]) + partial[1, c]) + ...), c < count, in tile order, in place: the
 * running sum continues across calls, so a design split at any multiple of 64 rows gives the bits of one call.
 * No atomics.  DGPAMD_BAD_ARG before any launch: P, M, K, ntiles or count < 1, a null pointer other than fAB.  A NaN value
 * makes the sums of its own path and output NaN; nothing loops on data. */
int dgpamd_sobol_tiles(dgpamd_ctx *ctx, int64_t P, int64_t M, int K, const double *fA, const double *fB, const double *fAB,
                       const double *shift, double *partial);
int dgpamd_sobol_add(dgpamd_ctx *ctx, int64_t ntiles, int64_t count, const double *partial, double *sums);

/* ---- second moments of the input gradient of function-valued draws (DESIGN I.18) ----
 * f (P x M x K), J (P x M x K x Dx, Dx fastest), shift (P x K): device doubles, the values and the Jacobian of P paths at M
 * design rows with K outputs, and the shift of the values (g = f - shift[p, k], as dgpamd_sobol_tiles).  1 <= Dx <= 64.
 * A tile is 64 consecutive rows (the last one may be short), ntiles = ceil(M / 64), NC = 2 + Dx + Dx (Dx + 1) / 2:
 *   partial[t, p, k, 0..1]       = sum g, sum g^2
 *   partial[t, p, k, 2 + d]      = sum J_d,      d < Dx
 *   partial[t, p, k, 2 + Dx + ..] = sum J_d J_e,  d <= e < Dx, the upper triangle packed row-major
 * over the rows of tile t; partial: (ntiles x P x K x NC) device doubles.  Rows past M contribute +0.  The products are formed
 * and added by v_mfma_f64_16x16x4 over the 64 rows of the tile: their order inside a tile is the instruction's, and it is the
 * same for every tile, path and launch.  dgpamd_sobol_add adds the tiles onto running sums (P x K x NC) in tile order, so a
 * design split at any multiple of 64 rows gives the bits of one call.  No atomics.  A column of J that is zero gives +0 in its
 * sum and in every product it takes part in.  DGPAMD_BAD_ARG before any launch: P, M or K < 1, Dx outside 1 .. 64, a null
 * pointer, ntiles * P * K beyond 2^31 - 1. */
int dgpamd_gradmom_tiles(dgpamd_ctx *ctx, int64_t P, int64_t M, int K, int Dx, const double *f, const double *J,
                         const double *shift, double *partial);

/* ---- batched box-constrained minimisation of function-valued draws (DESIGN I.17) ----
 * A projected L-BFGS for Q independent problems min phi_q(x), lo <= x <= hi, D <= DGPAMD_MAXD columns, driven by reverse
 * communication: a call takes the objective and its gradient at the current trial points, advances every problem's state
 * machine by one transition and writes the next trial points.  Nothing goes to the host.
 * f (Q x K), J (Q x K x D): device doubles, the values and the Jacobian of the walk at x_trial, q = p R + r; the kernel reads
 * column k alone and forms phi = sign f[q, k], grad = sign J[q, k, :] (sign +1 minimises the draw, -1 maximises it).
 * lo, hi: D device doubles; lo_h, hi_h: host copies, for the checks below.  history 1 .. DGPAMD_BOXMIN_MAXHIST stored pairs.
 * work: dgpamd_boxmin_workspace(Q, D, history) bytes (a host-side formula, no GPU; 0 for sizes the step refuses), opaque, kept
 * by the caller between the calls of one minimisation.  x_trial (Q x D): read as the point just evaluated, overwritten with the
 * next one; first != 0 initialises the state from it (and status, n_iter, n_eval, running).
 * Results, written when a problem finishes: x (Q x D), fun (Q) the value of the draw (sign undone), status (Q) int32 one of
 * DGPAMD_BOXMIN_*; n_iter, n_eval (Q) int32 accepted steps and evaluations so far; running: one int32, the problems whose
 * status is DGPAMD_BOXMIN_RUNNING after the call (the only atomic: an integer count does not depend on order).
 * Per problem (tests/boxmin_ref.py restates it):
 *   INIT       (x, f, g) <- trial; phi or g not finite: NAN.  Then DIRECTION (after its GTOL test: MAXEVAL if max_eval is 1).
 *   DIRECTION  B = {i: (x_i <= lo_i and g_i > 0) or (x_i >= hi_i and g_i < 0) or lo_i == hi_i}; pg = g off B, 0 on B.
 *              max |P(x - g) - x| <= gtol: GTOL.  d = -H pg by the two-loop recursion, the components of B of q, s, y taken as
 *              zero and d = 0 on B; a pair with s^T y <= 0 over the free components is skipped; gamma = s^T y / y^T y of the
 *              newest pair over the free components (1 if it is skipped or there is none).  No pair, or pg^T d >= 0 or not
 *              finite: d = -pg and t = min(1, 1 / max|pg|) 2^grow; else t = 1.  trial = P(x + t d).  grow (at most 30) counts
 *              the accepted steps just before that stored no pair and needed no halving: without positive curvature the
 *              steps along -pg double, and a linear objective overshoots its corner and is projected onto it exactly.
 *   SEARCH     delta = trial - x; accept if phi_t and g_t are finite, phi_t <= f + 1e-4 g^T delta and g^T delta < 0.  Else
 *              MAXEVAL at max_eval (x kept); after 20 halvings a quasi-Newton direction drops the pairs and restarts along
 *              -pg, and -pg ends with LINESEARCH (x kept); else t <- t / 2, trial = P(x + t d).  A NaN is a failed test.
 *   ACCEPT     s = delta, y = g_t - g enter the ring if s^T y > 1e-10 |s| |y| (grow <- 0; else grow <- grow + 1 after a search
 *              without halvings, 0 after one with); (x, f, g) <- trial; n_iter += 1; GTOL as above;
 *              FTOL if f_old - f <= ftol max(|f_old|, |f|, 1); MAXITER at maxiter; MAXEVAL at max_eval; else DIRECTION.
 * A finished problem writes x_trial = x and changes nothing more.  One lane per problem and no cross-lane operation: any
 * slice of the problems, run alone, gives the same bits.  Products are not fused into sums (the file is built without
 * contraction).  DGPAMD_BAD_ARG before any launch: Q < 1, D < 1 or D > DGPAMD_MAXD, K < 1, k outside [0, K), sign not +-1,
 * history outside 1 .. DGPAMD_BOXMIN_MAXHIST, maxiter or max_eval < 1, a null pointer, lo_h[i] > hi_h[i] or a NaN bound, a
 * negative or NaN tolerance. */
#define DGPAMD_BOXMIN_RUNNING 0
#define DGPAMD_BOXMIN_GTOL 1
#define DGPAMD_BOXMIN_FTOL 2
#define DGPAMD_BOXMIN_MAXITER 3
#define DGPAMD_BOXMIN_MAXEVAL 4
#define DGPAMD_BOXMIN_LINESEARCH 5
#define DGPAMD_BOXMIN_NAN 6
#define DGPAMD_BOXMIN_COUNT 7
#define DGPAMD_BOXMIN_MAXHIST 16
size_t dgpamd_boxmin_workspace(int64_t Q, int D, int history);
int dgpamd_boxmin_step(dgpamd_ctx *ctx, int64_t Q, int D, int K, int k, double sign, const double *f, const double *J,
                       const double *lo, const double *hi, const double *lo_h, const double *hi_h, int history, int maxiter,
                       int max_eval, double gtol, double ftol, int first, void *work, double *x_trial, double *x, double *fun,
                       int32_t *status, int32_t *n_iter, int32_t *n_eval, int32_t *running);

/* ---- batched chains over a box: the input posterior of function-valued draws (DESIGN I.19, I.20) ----
 * What dgpamd_boxmala_step and dgpamd_boxhmc_step below share (csrc/boxchain.hpp holds it once for both kernels).
 * Q independent chains, q = p R + r, D <= DGPAMD_MAXD columns, driven by reverse communication: a call takes the walk's values
 * and Jacobian at the current trial points, advances every chain's state machine and writes the next trial points.  Nothing
 * goes to the host; no atomics, no cross-lane operation.  The target of a chain, on the box lo <= x <= hi:
 *   lp(x) = -1/2 sum_k w_k (ybar_k - f_k(x))^2 - 1/2 sum_d pv_d (x_d - pm_d)^2
 *   g_d   = sum_k w_k (ybar_k - f_k) J_kd - pv_d (x_d - pm_d)
 * f (Q x K), J (Q x K x D, D fastest): device doubles, as the walk leaves them.  par: 2 K + 5 D device doubles, w (K), ybar (K),
 * pv (D), pm (D), s (D), lo (D), hi (D) in this order; par_h: a host copy, for the checks below.  An output with w_k = 0 and a
 * column with pv_d = 0 are not read (their f, J, ybar, pm may hold NaN).  z (Q x D) standard normal and logu (Q) log-uniform
 * draws of this call, device doubles: the kernels have no generator.  work: dgpamd_box*_workspace(Q, D) bytes (a host-side
 * formula, no GPU; 0 for sizes the step refuses), opaque, kept between the calls of one run.  x_trial (Q x D): read as the point
 * just evaluated, overwritten with the next one; on the first call it holds the starts, which must lie in the box.
 * State the caller may read: h (Q) the steps, logr (Q) the log acceptance ratio of the last decision, status (Q) int32 (the
 * two steps' DGPAMD_BOX*_OK and _NAN are the same numbers), n_prop, n_acc (Q) int32 decisions and acceptances.  xs (n_slots x
 * D x Q), lps (n_slots x Q): the samples, chain fastest.  A FIXED column (s_d = 0 or lo_d = hi_d) keeps x_d and is left out of
 * every sum over d of a step's own phases; the others are free.  The phases both steps run, per chain:
 *   TARGET   (chains with status OK, or first != 0) (lp', g') at x_trial, the sums in index order, a product rounded before it
 *            enters a sum: a += (w_k r_k) r_k, r_k = ybar_k - f_k; b += (pv_d e_d) e_d, e_d = x'_d - pm_d;
 *            lp' = -0.5 a - 0.5 b; c_d += (w_k r_k) J_kd over k, then g'_d = c_d - pv_d e_d.
 *   INIT     (first != 0) (x, lp, g) <- trial's; h <- h0; logr 0; counts 0; lp' or g' not finite: status NAN, else OK.
 *   TALLY    of a decision: accept if logu < logr (a NaN comparison rejects): (x, lp, g) <- trial's.  n_prop += 1,
 *            n_acc += accepted.  adapt != 0: h <- min(max(h (accepted ? up : down), hmin), hmax), h the step decided with.
 *   STORE    slot >= 0: xs[slot, :, q] = x, lps[slot, q] = lp (in any call).
 * A chain with status NAN writes x_trial = x, so that the walk evaluates a finite point, stores, and changes nothing more.
 * One lane per chain: any slice of the chains, run alone with its slice of z and logu, gives the same bits.  Products are not
 * fused into sums (both files are built without contraction).  DGPAMD_BAD_ARG before any launch: Q < 1, D < 1 or
 * D > DGPAMD_MAXD, K < 1, a null pointer, lo > hi or a NaN bound, a negative or NaN w, pv or s, h0, hmin, hmax, up or down not
 * positive and finite, hmin > hmax, slot outside -1 .. n_slots - 1.
 *
 * ---- batched MALA over a box (DESIGN I.19) ----
 * Metropolis-adjusted Langevin chains: a call decides every chain's pending proposal and proposes the next.  work:
 * dgpamd_boxmala_workspace(Q, D) = Q (8 (3 D + 1) + 4) bytes -- x, g, g' (D x Q doubles each), lp (Q doubles), the int32
 * out-of-box flag (Q).  Per chain and call, in this order (tests/boxmala_ref.py restates it): TARGET; INIT or DECIDE; STORE;
 * PROPOSE.
 *   DECIDE   (first = 0; chains with status OK) the out-of-box flag set: logr = -inf; else lp' or g' not finite: logr = NaN; else
 *            logr = (lp' - lp) + (0.5 qf - 0.5 qb), qf = sum_d u_d^2, qb = sum_d v_d^2 over the free columns,
 *            u_d = ((x'_d - x_d) - c_d g_d) / (h s_d), v_d = ((x_d - x'_d) - c_d g'_d) / (h s_d), c_d = (0.5 (h h)) (s_d s_d).
 *            Then TALLY.
 *   PROPOSE  (status OK) x'_d = (x_d + c_d g_d) + (h s_d) z_d on the free columns, x'_d = x_d on a fixed one; any x'_d outside
 *            [lo_d, hi_d] or not finite: the flag is set and x_trial = x, so that the walk evaluates a finite point and the
 *            next call rejects it.
 * A proposal outside the box has target density zero: rejecting it is a valid Metropolis-Hastings step for a target supported
 * on the box (no reflection, no projection). */
#define DGPAMD_BOXMALA_OK 0
#define DGPAMD_BOXMALA_NAN 1
#define DGPAMD_BOXMALA_COUNT 2
size_t dgpamd_boxmala_workspace(int64_t Q, int D);
int dgpamd_boxmala_step(dgpamd_ctx *ctx, int64_t Q, int D, int K, const double *f, const double *J, const double *par,
                        const double *par_h, const double *z, const double *logu, double h0, double hmin, double hmax, double up,
                        double down, int adapt, int first, int slot, int n_slots, void *work, double *x_trial, double *h,
                        double *logr, double *xs, double *lps, int32_t *status, int32_t *n_prop, int32_t *n_acc);

/* ---- batched HMC over a box with reflecting walls (DESIGN I.20) ----
 * Hamiltonian Monte Carlo chains on the shared contract above.  A trajectory of L leapfrog steps takes L calls, of which only
 * the L-th has last != 0; a run is one call with first != 0 and then the calls of its trajectories, 1 + sum L walk evaluations.
 * z and logu are read only by a call that starts a trajectory (z: INIT, DECIDE) or closes one (logu: DECIDE).  The walls of
 * the box reflect (Neal 2011, 5.5.1): the map of a trajectory stays reversible and volume preserving.  A fixed column has
 * momentum 0.  work: dgpamd_boxhmc_workspace(Q, D) = Q (8 (4 D + 2) + 4) bytes -- x, g, g', p (D x Q doubles each), lp, H0
 * (Q doubles), the int32 flag `bad` (Q).  Per chain and call, in this order (tests/boxhmc_ref.py restates it): TARGET; INIT,
 * MID or DECIDE; STORE; after INIT and DECIDE, START.
 *   INIT     (first != 0; last is not read) as above.
 *   else     lp' or g' not finite and bad = 0: bad <- NONFINITE.
 *   MID      (first = 0, last = 0) bad = 0: on every free column p_d <- p_d + (h s_d) g'_d, then DRIFT from y = x_trial.
 *            bad != 0 (before or after): x_trial = x.  Then STORE; nothing more.
 *   DECIDE   (first = 0, last != 0) bad = WALL: logr = -inf; bad = NONFINITE: logr = NaN; else
 *            ke += p'_d p'_d over the free columns in index order, p'_d = p_d + (0.5 (h s_d)) g'_d;
 *            logr = (lp' - 0.5 ke) - H0.  Then TALLY, STORE and START.
 *   START    (status OK) with the chain's h as it is now, which every call of the trajectory uses: bad <- 0; on a free column
 *            kz += z_d z_d, p_d <- z_d + (0.5 (h s_d)) g_d, then DRIFT from y = x; p_d = 0 on a fixed one.
 *            H0 = lp - 0.5 kz.  bad != 0: x_trial = x.
 *   DRIFT    of a free column: y_d <- y_d + (h s_d) p_d; then at most DGPAMD_BOXHMC_NREFL times, while y_d lies outside:
 *            y_d > hi_d: y_d <- hi_d - (y_d - hi_d), p_d <- -p_d; else y_d < lo_d: y_d <- lo_d + (lo_d - y_d), p_d <- -p_d.
 *            y_d then outside [lo_d, hi_d] or not finite: bad <- WALL.  Else x_trial_d = y_d.
 * With bad set the walk evaluates x, a finite point, and the remaining calls of the trajectory change nothing but
 * x_trial = x; DECIDE rejects it.  A drift reflects as often forwards as backwards, so the cap keeps detailed balance.  With
 * L = 1 (every call DECIDE + START) the proposal and the acceptance ratio are the MALA step's in exact arithmetic.
 * DGPAMD_BAD_ARG before any launch: the shared cases; first and last together are accepted. */
#define DGPAMD_BOXHMC_OK 0
#define DGPAMD_BOXHMC_NAN 1
#define DGPAMD_BOXHMC_COUNT 2
#define DGPAMD_BOXHMC_NREFL 8
size_t dgpamd_boxhmc_workspace(int64_t Q, int D);
int dgpamd_boxhmc_step(dgpamd_ctx *ctx, int64_t Q, int D, int K, const double *f, const double *J, const double *par,
                       const double *par_h, const double *z, const double *logu, double h0, double hmin, double hmax, double up,
                       double down, int adapt, int first, int last, int slot, int n_slots, void *work, double *x_trial, double *h,
                       double *logr, double *xs, double *lps, int32_t *status, int32_t *n_prop, int32_t *n_acc);

/* ---- tempered sequential Monte Carlo over a box: evidence and multimodal input posteriors (DESIGN I.21) ----
 * P draws with R particles each, 1 <= R <= DGPAMD_BOXSMC_MAXR, lane q = p R + r, P R < 2^31.  Draw p's particles sample
 * pi_beta(x) proportional to prior(x) exp(beta_p ll(x)) on the box, ll(x) = -1/2 sum_k w_k (ybar_k - f_k(x))^2 and
 * lprior(x) = -1/2 sum_d pv_d (x_d - pm_d)^2, the two parts of the chains' lp above; only the likelihood is tempered.
 * f, J, par, par_h, z, logu, x_trial, h, logr, n_prop, n_acc and the fixed columns: as for the chains.  State tensors the
 * caller owns and may read: x (D x Q, particle fastest), ll, lprior (Q), status (Q) int32 per particle (DGPAMD_BOXSMC_OK,
 * _NAN); beta (P), and h (Q), which no call resets: the caller fills it before the first one.
 *
 * dgpamd_boxsmc_move: one call of every particle's tempered MALA state machine, one lane per particle, beta read from
 * beta[q / R].  work: dgpamd_boxsmc_workspace(P, R, D) = P R (16 D + 4) bytes -- g, g' (D x Q doubles each) and the int32
 * out-of-box flag (Q); 0 for sizes the calls refuse.  Per particle and call, in this order (tests/boxsmc_ref.py restates it):
 *   TARGET   (status OK, or first != 0) the chains' sums in their order: ll' = -0.5 a, lprior' = -0.5 b,
 *            g'_d = beta c_d, then g'_d - pv_d e_d where pv_d > 0.
 *   INIT     (first != 0: a stage starts at the gathered particles) (x, g, ll, lprior) <- the trial's under this beta; logr 0;
 *            counts 0; the flag down; ll', lprior' or g' not finite: status NAN, else OK.  h stays.
 *   DECIDE   (first = 0, status OK) the flag set: logr = -inf; else a non-finite trial: logr = NaN; else
 *            logr = ((beta ll' + lprior') - (beta ll + lprior)) + (0.5 qf - 0.5 qb), qf and qb as in the MALA step's DECIDE.
 *            Then TALLY as above (an accepted trial also commits ll and lprior).
 *   HOLD     status NAN, or last != 0 (the stage ends): x_trial = x, and nothing more.
 *   PROPOSE  else, as the MALA step's.
 * Products are not fused into sums.  DGPAMD_BAD_ARG: the chains' cases, R outside 1 .. DGPAMD_BOXSMC_MAXR, a null pointer.
 *
 * dgpamd_boxsmc_temper: one workgroup per draw.  With d_i = m - ll_i, m the largest finite ll of the draw (a particle whose
 * ll is not finite is dead: weight 0, never an ancestor), a_i(delta) = exp_negated(delta d_i) and
 * ESS(delta) = (sum a)^2 / sum a^2: delta = 1 - beta if ESS(1 - beta) >= ess_frac R_live, then beta' = 1 exactly; else
 * the lower end of [0, 1 - beta] after 52 halvings, which keeps ESS >= the target, and beta' = beta + delta.  Then
 *   log_evidence[p] += delta m + log(sum a / R), stage_ess[p] = ESS(delta), dbeta[p] = delta, beta[p] = beta';
 *   C_i the inclusive scan of a_i / sum a, clamped to 1 and exactly 1 from the last particle of positive weight on; particle i
 *   is the ancestor of the slots ceil(R C_{i-1} - u_p) .. ceil(R C_i - u_p) - 1 of anc[p, :] (systematic resampling with the
 *   one uniform u_p in [0, 1)); x_trial[p, j, :] = x[:, p R + anc[p, j]].
 * Every sum runs in an order that R alone fixes: a draw's outputs do not depend on P or on the draws beside it.
 * A draw with beta = 1 or status not OK, and one for which no delta > 0 keeps the target: delta = 0, anc the identity,
 * x_trial = x, stage_ess NaN, log_evidence as it was.  A draw with status OK and no live particle: status NAN (P) and
 * log_evidence NaN.  status (P) int32 per draw; DGPAMD_BOXSMC_MAX_STAGES is the driver's.  running (1) int32: set to the
 * count of draws with status OK and beta' < 1.  DGPAMD_BAD_ARG: the sizes above, ess_frac outside (0, 1), a null pointer. */
#define DGPAMD_BOXSMC_OK 0
#define DGPAMD_BOXSMC_NAN 1
#define DGPAMD_BOXSMC_MAX_STAGES 2
#define DGPAMD_BOXSMC_COUNT 3
#define DGPAMD_BOXSMC_MAXR 8192
size_t dgpamd_boxsmc_workspace(int64_t P, int64_t R, int D);
int dgpamd_boxsmc_move(dgpamd_ctx *ctx, int64_t P, int64_t R, int D, int K, const double *f, const double *J, const double *par,
                       const double *par_h, const double *beta, const double *z, const double *logu, double hmin, double hmax,
                       double up, double down, int adapt, int first, int last, void *work, double *x_trial, double *x, double *ll,
                       double *lprior, double *h, double *logr, int32_t *status, int32_t *n_prop, int32_t *n_acc);
int dgpamd_boxsmc_temper(dgpamd_ctx *ctx, int64_t P, int64_t R, int D, double ess_frac, const double *ll, const double *x,
                         const double *u, double *beta, double *dbeta, double *log_evidence, double *stage_ess, int32_t *status,
                         int32_t *anc, double *x_trial, int32_t *running);

/* ---- the whitening fold of field calibration: known control inputs, correlated errors (DESIGN I.24) ----
 * Q chains, each evaluated at T sites, 1 <= T <= DGPAMD_BOXSITES_MAXT: f (Q, T, K) and J (Q, T, K, Dx) are the walk's values and
 * Jacobian at the chain's T rows, W_k (T, T) the lower-triangular whitening matrix of output k (the inverse of the Cholesky
 * factor of the error covariance across sites; a site that was not observed has a zero row and a zero column), cols the Dt
 * columns of the walk's input that are calibrated.  The fold writes the pseudo-outputs j = t K + k that the chain steps and
 * dgpamd_boxsmc_move take as their K = T K outputs and D = Dt columns, in their layouts:
 *   ft[q, t K + k]    = sum_{s = 0 .. t} W[k, t, s] f[q, s, k]                  ft (Q, T K)
 *   Jt[q, t K + k, d] = sum_{s = 0 .. t} W[k, t, s] J[q, s, k, cols[d]]         Jt (Q, T K, Dt)
 * Each sum starts from 0.0 and runs in the order of s; products are not fused into sums (the file is built without contraction);
 * a term whose W[k, t, s] is exactly 0 is skipped, not multiplied, so a NaN in f or J at a site that was not observed reaches
 * nothing, and that site's own outputs are 0.  tests/boxsites_ref.py restates it.  W is passed transposed, Wt[k, s, t] =
 * W[k, t, s], (K, T, T) contiguous: the thread that owns row t reads addresses consecutive in t.  Entries with s > t are not read.
 * cols: Dt int32 on the device; cols_h: their host copy, which the checks read.  Dt = 0: the values alone -- cols, cols_h, J and
 * Jt are not read and may be null.  One workgroup per (chain, output); 16 KiB of LDS; no atomics, no workspace: an element
 * depends on its own chain's inputs alone, not on Q or on what shares the launch.
 * DGPAMD_BAD_ARG before any launch: Q < 1 or Q >= 2^31, T outside 1 .. DGPAMD_BOXSITES_MAXT, K outside 1 .. 65535, Dx < 1,
 * Dt < 0, Dt > DGPAMD_MAXD or Dt > Dx, Q T K Dx over 2^60, a column outside 0 .. Dx - 1 or named twice, a null pointer. */
#define DGPAMD_BOXSITES_MAXT 256
int dgpamd_boxsites_fold(dgpamd_ctx *ctx, int64_t Q, int T, int K, int Dx, int Dt, const int32_t *cols, const int32_t *cols_h,
                         const double *Wt, const double *f, const double *J, double *ft, double *Jt);

/* ---- subset simulation over a box: the probability of a rare event of a function draw (DESIGN I.22) ----
 * P draws with R particles each, 1 <= R <= DGPAMD_BOXSUS_MAXR (a level needs R >= 2), lane q = p R + r, P R < 2^31, 1 <= D <= 64.
 *   score = sign (f[q, output] - threshold) + 0.0 (the + 0.0 turns -0 into +0), sign = +1 or -1; the event is F = {score >= 0}.
 * A particle whose score is NaN is dead: never a survivor, and the divisor stays R.  n_s = max(1, floor(level_prob R)) is the
 * caller's, 1 <= n_s < R.  The driver (reliability.failure_probability; tests/boxsus_ref.py restates both calls and the
 * schedule): particles from the prior on the box, one walk evaluation and MOVE(first, last); sd (P, D) filled by the caller
 * with the prior particles' spread per column; then stages of LEVEL and n_moves + 1 walk evaluations with MOVE behind each,
 * first on the first and last on the last; after a stage lam[p] <- clamp(lam[p] exp(acceptance rate - target), 1e-3, 1e2).
 * State the caller owns and may read: x (D x Q, particle fastest), score (Q), moved, status, n_prop, n_acc (Q) int32 per
 * particle (status DGPAMD_BOXSUS_OK or _NAN); per draw prob (P, ones at first), level, lam (P), sd (P, D), nsurv, done, status
 * (P) int32, anc (P, R) int32; running (1) int32.  par and its host copy par_h: pv (D), pm (D), lo (D), hi (D), the prior
 * prop. to exp(-1/2 sum_d pv_d (x_d - pm_d)^2) on the box, pv_d = 0 flat.
 *
 * dgpamd_boxsus_level: one workgroup per draw.  A draw with done = 0: k = min(n_s, live count), b = the k-th largest live
 * score.  b >= 0: the level is +0.0 and this is the draw's final stage; else the level is b.  Survivors: the live particles
 * with score >= level, in increasing particle index; n_b their count (ties at the level all survive).  Then
 *   prob[p] <- prob[p] * ((double)n_b / (double)R); nsurv[p] = n_b; level[p] = the level;
 *   done[p] <- 1 in the final stage, else when prob[p] < min_prob, with status DGPAMD_BOXSUS_BELOW_MIN;
 *   anc[p, j] = the (j mod n_b)-th survivor; x_trial[p, j, :] = x[:, p R + anc[p, j]];
 *   sd[p, d] = sqrt(sum_surv (x_d - mean_d)^2 / n_b), mean_d = sum_surv x_d / n_b, every sum in an order that R alone fixes
 *   (thread t of T = min(1024, R rounded up to 64) adds its particles t, t + T, ... in order, the 64 lanes of a wave combine
 *   by an xor butterfly 32, 16, .. 1, the wave totals add in index order); a column whose new value is 0 or not finite keeps
 *   its old sd.
 * No live particle: status DGPAMD_BOXSUS_NAN, prob NaN, nsurv 0, done 1, the particles stay.  A draw with done = 1: anc the
 * identity, x_trial = x, nothing else touched.  running[0] = the number of draws with done = 0 after the call.
 * A draw's outputs do not depend on P or on the draws beside it.  DGPAMD_BOXSUS_MAX_STAGES is the driver's.
 * DGPAMD_BAD_ARG: the sizes above, n_s outside 1 .. R - 1, min_prob outside [0, 1), a null pointer.
 *
 * dgpamd_boxsus_move: the component-wise modified Metropolis move of Au and Beck (2001), one lane per particle.  f (Q, K): the
 * walk's values at x_trial (Q, D), of which column `output` alone is read; z, logu (Q, D): this call's normal draws and
 * logarithms of uniform draws, logu read only where pv_d > 0.  Per particle and call, in this order:
 *   SCORE    score' as above.
 *   INIT     (first != 0) (x, score) <- the trial's; counts 0; the moved flag down; score' NaN: status NAN, else OK.
 *   DECIDE   (first = 0, status OK) accept iff the moved flag is set and score' >= level[p] (a NaN comparison rejects); on
 *            acceptance (x, score) <- the trial's.  n_prop += 1, n_acc += accepted.
 *   HOLD     status NAN, or last != 0: x_trial = x, and nothing more.
 *   PROPOSE  else, on every free column (a column with lo_d = hi_d or sd[p, d] = 0 is fixed: it keeps x_d):
 *            c = x_d + (lam_p sd_pd) z_d, kept iff lo_d <= c <= hi_d and either pv_d = 0 or
 *            logu_qd < ((-0.5 (pv_d e')) e') - ((-0.5 (pv_d e)) e), e' = c - pm_d, e = x_d - pm_d;
 *            a column not kept stays at x_d.  The moved flag is set iff any column was kept (x_trial = x otherwise, and the
 *            next DECIDE counts a rejection).
 * Products are not fused into sums; the kernel has no generator and needs no workspace.  DGPAMD_BAD_ARG: the sizes above,
 * K < 1, output outside 0 .. K - 1, sign not +1 or -1, a threshold that is not finite, a pv that is negative or NaN, a bound
 * with lo > hi or NaN, a null pointer. */
#define DGPAMD_BOXSUS_OK 0
#define DGPAMD_BOXSUS_NAN 1
#define DGPAMD_BOXSUS_MAX_STAGES 2
#define DGPAMD_BOXSUS_BELOW_MIN 3
#define DGPAMD_BOXSUS_COUNT 4
#define DGPAMD_BOXSUS_MAXR 8192
int dgpamd_boxsus_move(dgpamd_ctx *ctx, int64_t P, int64_t R, int D, int K, int output, double sign, double threshold,
                       const double *f, const double *par, const double *par_h, const double *level, const double *lam,
                       const double *sd, const double *z, const double *logu, int first, int last, double *x_trial, double *x,
                       double *score, int32_t *moved, int32_t *status, int32_t *n_prop, int32_t *n_acc);
int dgpamd_boxsus_level(dgpamd_ctx *ctx, int64_t P, int64_t R, int D, int n_s, double min_prob, const double *score,
                        const double *x, double *prob, double *level, int32_t *nsurv, int32_t *done, int32_t *status, int32_t *anc,
                        double *x_trial, double *sd, int32_t *running);

/* ---- counter-based random streams on the device: Philox4x64-10 (DESIGN I.23) ----
 * dgpamd_philox_fill fills out, a contiguous (rounds, P, R, D) array of 8-byte entries, with the numbers of one stream.  The
 * generator is Philox4x64-10 of Salmon et al. (2011), the function of numpy.random.Philox: multipliers 0xD2E7470EE14C6C93 and
 * 0xCA5A826395121157, key increments 0x9E3779B97F4A7C15 and 0xBB67AE8584CAA73B, ten rounds, the key bumped before rounds
 * 2 to 10.  The key (key0, key1) is the caller's; the drivers use numpy.random.SeedSequence(seed).generate_state(2, uint64).
 * The counter contract: entry [i, p, r, e] is word e mod 4 of the block of the counter
 *   c0 = 1 + e div 4,  c1 = (p << 32) | r,  c2 = c2_first + i,  c3 = stream,
 * a pure function of (key, stream, c2, p, r, e): it does not depend on rounds, P, R, D or on how the rounds are split over
 * calls.  With the 1 + it is the e-th output of numpy.random.Philox(counter=[0, c1, c2, c3], key=key).random_raw().
 * Kinds, w the word:
 *   DGPAMD_PHILOX_BITS         w itself (out is int64 / uint64);
 *   DGPAMD_PHILOX_UNIFORM      (w >> 11) 2^-53 in [0, 1), numpy's mapping, bit for bit;
 *   DGPAMD_PHILOX_LOG_UNIFORM  log of that uniform by the device library's log; a zero uniform gives -inf;
 *   DGPAMD_PHILOX_NORMAL       Box and Muller on the pairs of words (0, 1) and (2, 3) of a block: u1 = ((w_a >> 11) + 1) 2^-53 in
 *                              (0, 1], u2 = (w_b >> 11) 2^-53, rho = sqrt(-2 log u1); elements 4 j + 2 q and 4 j + 2 q + 1 are
 *                              rho cos(2 pi u2) and rho sin(2 pi u2), by the device library's log and sincospi(2 u2).
 * One lane per block of four elements; stores are guarded at a partial last block.  No workspace, no LDS, no atomics.
 * DGPAMD_BAD_ARG, before anything is launched: an unknown kind; rounds, P or R < 1; D outside 1 .. DGPAMD_MAXD; P >= 2^31 or
 * R >= 2^32; c2_first + rounds wrapping; rounds P R > 2^56; a null out. */
#define DGPAMD_PHILOX_BITS 0
#define DGPAMD_PHILOX_UNIFORM 1
#define DGPAMD_PHILOX_LOG_UNIFORM 2
#define DGPAMD_PHILOX_NORMAL 3
#define DGPAMD_PHILOX_COUNT 4
int dgpamd_philox_fill(dgpamd_ctx *ctx, int kind, uint64_t key0, uint64_t key1, uint64_t stream, uint64_t c2_first,
                       int64_t rounds, int64_t P, int64_t R, int D, void *out);

#ifdef __cplusplus
}
#endif
#endif /* DGP_AMD_H */
