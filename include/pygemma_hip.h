/*
 * pygemma_hip.h — C ABI of the MI355X-native pyGEMMA hot path (libpygemma_hip.so).
 *
 * The reference (rlangefe/pygemma) has NO C ABI: its operator boundary is the Python call
 * calculate((eigenVals, Y, W, X_block, grid)) -> list[dict]  (lmm/lmm.py:461-495) plus two
 * third-party calls, scipy.linalg.eigh(K) (lmm/lmm.py:152,197) and U.T @ X (lmm/lmm.py:244-246).
 * This header DEFINES the boundary a maintainer would bind with ctypes (INTEGRATION.md shows the
 * stub).  Plain C: pointers + sizes, no C++/torch types.
 *
 * Conventions
 *  - every function returns 0 on success, a negative PG_E* code on failure; never throws, never
 *    calls exit(); pg_last_error() returns a thread-local message for the last failure.
 *  - "_dev" entry points take DEVICE pointers (hipMalloc'd, or torch tensors' data_ptr()) and
 *    enqueue on the context's stream; they return after enqueueing (call pg_ctx_sync).
 *    Entry points without "_dev" take HOST pointers, copy in/out and return when done.
 *  - the caller owns every buffer it passes; the library owns only what hangs off pg_ctx.
 *  - layouts: "SNP-major" Xr[g*ldx + i] (row g = rotated genotype vector of SNP g, ldx >= n);
 *    "reference layout" X[i*p + g] (NumPy C-order (n,p), lmm/lmm.py:121-122).
 */
#ifndef PYGEMMA_HIP_H
#define PYGEMMA_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PG_OK 0
#define PG_EINVAL (-22)     /* bad argument (shape, NULL, unsupported c)               */
#define PG_ENOMEM (-12)     /* device allocation failed                                */
#define PG_EHIP (-5)        /* a HIP runtime call or kernel launch failed               */
#define PG_ENOTSUP (-95)    /* configuration not supported by this build                */
#define PG_ENODEV (-19)     /* no usable GPU                                            */

#define PG_MAX_COVARIATES 30 /* c supported by the register-resident Gram kernels (reference benchmark: up to 26) */

typedef struct pg_ctx pg_ctx; /* one per (process, GPU): device id, stream, scratch      */

const char *pg_last_error(void);
const char *pg_version(void);
int pg_device_count(void);                      /* GPUs visible to HIP (0 if none)       */
int pg_ctx_create(int device, pg_ctx **out);    /* binds a device, creates a stream       */
int pg_ctx_create_on_stream(int device, void *hip_stream, pg_ctx **out); /* caller's stream */
void pg_ctx_destroy(pg_ctx *ctx);
int pg_ctx_sync(pg_ctx *ctx);
int pg_ctx_device(const pg_ctx *ctx);

/* device memory helpers for callers without their own allocator (Python/ctypes hosts) */
int pg_malloc(pg_ctx *ctx, size_t bytes, void **dptr);
int pg_free(pg_ctx *ctx, void *dptr);
int pg_mem_info(pg_ctx *ctx, size_t *free_bytes, size_t *total_bytes);   /* of ctx's device (how much of X may be prefetched) */
int pg_memcpy_h2d(pg_ctx *ctx, void *dst, const void *src, size_t bytes);
int pg_memcpy_d2h(pg_ctx *ctx, void *dst, const void *src, size_t bytes);
int pg_memset(pg_ctx *ctx, void *dst, int value, size_t bytes);
/* strided host -> device copy: `height` rows of `width` bytes (a column window of a row-major host matrix) */
int pg_memcpy2d_h2d(pg_ctx *ctx, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height);

/* ---- S1: pinned host memory + asynchronous copies: streaming SNP batches and precomputed eigenvectors from the host
 * (BASELINE configs 4-5).  The reference's eigen=False caller reads raw float32 .bin files and hands the whole pre-rotated X
 * over (experiments/large_gwas/run_pygemma.py:33-65); here X is read straight out of pinned memory by the DMA engines, batch
 * by batch, while the previous batch computes.
 *   pg_host_alloc/free        : hipHostMalloc'd (portable) buffer — e.g. the array a caller np.fromfile()s its .bin into
 *   pg_host_register/unregister: pin a caller-owned range in place
 *   pg_memcpy*_async          : enqueue on the context's stream and return (host side should be pinned; pageable memory
 *                               makes the runtime stage the copy and blocks)
 *   pg_stage_rows             : host-side gather of a column window into a (pinned) staging buffer with nthreads threads —
 *                               the pageable -> pinned leg for callers whose X is an ordinary NumPy array */
int pg_host_alloc(pg_ctx *ctx, size_t bytes, void **hptr);
int pg_host_free(pg_ctx *ctx, void *hptr);
int pg_host_register(pg_ctx *ctx, void *hptr, size_t bytes);
int pg_host_unregister(pg_ctx *ctx, void *hptr);
int pg_memcpy_h2d_async(pg_ctx *ctx, void *dst, const void *src, size_t bytes);
int pg_memcpy_d2h_async(pg_ctx *ctx, void *dst, const void *src, size_t bytes);
int pg_memcpy_d2d_async(pg_ctx *ctx, void *dst, const void *src, size_t bytes);
int pg_memcpy2d_h2d_async(pg_ctx *ctx, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height);
int pg_stage_rows(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, int nthreads);

/* HIP events on the context's stream (kernel timing for bench.py's roofline leg) */
int pg_event_create(pg_ctx *ctx, void **event);
int pg_event_destroy(pg_ctx *ctx, void *event);
int pg_event_record(pg_ctx *ctx, void *event);
int pg_event_elapsed_ms(pg_ctx *ctx, void *start, void *stop, float *ms); /* synchronises on `stop` */
int pg_event_sync(pg_ctx *ctx, void *event);            /* host waits for the event                         */
int pg_stream_wait_event(pg_ctx *ctx, void *event);     /* the context's stream waits for it (no host wait) */

/* ---- H3 / SURVEY 8e: the one exchange step of the path, RCCL over xGMI called directly (librccl is dlopen'ed on first
 * use; no PyTorch).  Replaces Pool(nproc).imap + the ordered concatenation of the per-block lists (lmm/lmm.py:378-403):
 * a SNP block lives on one GPU; U/d/rotated y,W travel once (broadcast from the GPU that ran the eigensolver), the 32-byte
 * result rows once at the end (all-gather in rank order = SNP order, blocks padded to ceil(p/G) rows like SampleIter's).
 *   pg_comm_unique_id + pg_comm_init_rank : one process per GPU; rank 0 makes the 128-byte id and passes it to the other
 *                                           ranks over any host channel (pygemma_amd/dist.py: file or TCP rendezvous)
 *   pg_comm_init_all                      : one process, ndev GPUs, one host thread per GPU issuing the collectives
 * Collectives are enqueued on the stream of the context the communicator was made with. */
typedef struct pg_comm pg_comm;
#define PG_COMM_ID_BYTES 128
int pg_comm_unique_id(void *id128);
int pg_comm_init_rank(pg_ctx *ctx, int nranks, int rank, const void *id128, pg_comm **out);
int pg_comm_init_all(int ndev, pg_ctx *const *ctxs, pg_comm **out /* [ndev] */);
int pg_comm_destroy(pg_comm *comm);
int pg_comm_size(const pg_comm *comm);
int pg_comm_rank(const pg_comm *comm);
int pg_comm_broadcast_dev(pg_comm *comm, void *buf, size_t bytes, int root);                      /* in place */
int pg_comm_allgather_dev(pg_comm *comm, const void *send, void *recv, size_t bytes_per_rank);
int pg_comm_allreduce_f64_dev(pg_comm *comm, double *buf, size_t count, int op_max);              /* in place; sum or max */
int pg_comm_barrier(pg_comm *comm);                                                               /* + stream sync */
int pg_comm_group_start(void);
int pg_comm_group_end(void);

/* ---- H3-H10: the per-SNP operator -------------------------------------------------------
 * Replaces calculate() (lmm/lmm.py:461-495) and everything under it: calc_lambda_restricted
 * (pygemma_model.pyx:64-194, grid :99-132 / decade-scan+brentq+newton :135-194), precompute_mat
 * (:880-1053), newton (:1349-1416), the *_overload scalars (:1656-1698, :1813-1830),
 * calc_beta_vg_ve_restricted_overload (:1514-1537) and scipy.stats.f.sf (lmm/lmm.py:482).
 *
 * Inputs are in the eigenbasis (the reference's eigen=False boundary, lmm/lmm.py:164-167):
 *   d   (n)      eigenvalues, already clamped >= 0
 *   Wr  (n x c)  rotated covariates, row-major (NumPy C-order)
 *   yr  (n)      rotated phenotype
 *   Xr  (p rows) rotated genotypes, SNP-major, row stride ldx >= n
 * Outputs (length p, caller-allocated, SNP order preserved): beta, se_beta, tau, lambda as
 * float32; F_wald, p_wald as float64 (lmm/lmm.py:476-483; lambda is the f32 value the reference
 * widens to a Python float).  pval may be NULL.  grid != 0 selects calc_lambda_restricted's grid
 * branch.  stats (may be NULL) receives [fast evaluations, full (Newton) evaluations] summed over SNPs.
 */
int pg_assoc_dev(pg_ctx *ctx, int64_t n, int c, int64_t p, const float *d, const float *Wr, const float *yr,
                 const float *Xr, int64_t ldx, int grid, float *beta, float *se, float *tau, float *lambda,
                 double *F, double *pval, unsigned long long *stats_dev);

/* Work-per-SNP trace (tail analysis of the data-dependent Brent/Newton path, pygemma_model.pyx:1349-1416): the following
 * pg_assoc_dev calls on this context write, per SNP, fast evaluations | full (Newton) evaluations << 16 into trace_dev
 * (device, >= p entries, caller-owned); NULL switches the trace off. */
int pg_assoc_set_eval_trace(pg_ctx *ctx, unsigned *trace_dev);
/* Which passes over the n elements the SNP-specific evaluations (Brent, Newton, the one at the root) took: the following
 * pg_assoc_dev calls on this context add, summed over their SNPs, to dev4[0..3] (device, caller-owned, caller-zeroed) the passes
 * that produced the Gram power P, those that produced Q, those that produced R — a fused pass counts once for each power it
 * produces, the decade scan is not counted — and the Newton starts that reused Brent's P and Q; NULL switches it off.  The
 * evaluation counts of pg_assoc_dev's stats do not depend on it: those count evaluations, not passes. */
int pg_assoc_set_pass_stats(pg_ctx *ctx, unsigned long long *dev4);
/* Optional: what the FIRST pg_assoc_dev / pg_assoc_lrt_dev call of a context does on the host before it can enqueue its kernels (the
 * float32-sum plan of numpy's add.reduce for length n: built on the host, uploaded after a stream drain; scratch allocations for c
 * covariates) — ahead of time.  A streaming caller (lmm/lmm.py:461-495's per-SNP loop cut into batches) calls it while its first batch is
 * still on the host link.  No reference counterpart: the reference has no device. */
int pg_assoc_warm(pg_ctx *ctx, int64_t n, int c);

/* Several phenotypes over one SNP block (the reference's callers loop lmm.pygemma over phenotype columns with the same X, W, K:
 * experiments/wtccc/run_pygemma_imputed.py:516-532, experiments/animal_gwas/run_gwas.py:167-175).  For every phenotype k the six
 * outputs are bit-identical to pg_assoc_dev(..., yr = Yr + k ldy, ...): the decade scan's Gram entries that do not involve y (x'HW,
 * x'Hx at the 11 decade lambdas) are accumulated once per SNP for a chunk of up to 8 phenotypes, x'Hy_k once per phenotype, in the
 * per-element order of pg_assoc_dev's scan; the lambda search then runs one wavefront per (SNP, phenotype).
 *   Yr   t rotated phenotypes, phenotype-major: phenotype k is Yr[k ldy .. k ldy + n), ldy >= n
 *   outputs: t x p, phenotype-major (phenotype k's SNP g at [k p + g]); pval may be NULL; stats as pg_assoc_dev (summed)
 * Same argument checks as pg_assoc_dev, plus t >= 1 and ldy >= n. */
int pg_assoc_pheno_dev(pg_ctx *ctx, int64_t n, int c, int64_t p, int t, const float *d, const float *Wr,
                       const float *Yr, int64_t ldy, const float *Xr, int64_t ldx, int grid,
                       float *beta, float *se, float *tau, float *lambda, double *F, double *pval,
                       unsigned long long *stats_dev);
/* Optional, like pg_assoc_warm: the host-side set-up of a first pg_assoc_pheno_dev call with t phenotypes and up to p SNPs. */
int pg_assoc_pheno_warm(pg_ctx *ctx, int64_t n, int c, int t, int64_t p);

/* ---- N2: the same operator plus the likelihood-ratio test the reference sketches and leaves commented out
 * ("Fix these calculations later", lmm/lmm.py:137-141, 277-300), built from its own ML functions: lambda_alt =
 * calc_lambda(eigenVals, Y, [W, x]) (lmm/lmm.py:22-84: decade scan of dlogL/dlambda, brentq(rtol=0.1) + scipy newton),
 * l_alt = likelihood_lambda(lambda_alt, ...) (pygemma_model.pyx:1542-1562; derivatives :1567-1603), l_null the same for the
 * covariates alone, D_lrt = 2 (l_alt - l_null) on float32 scalars, p_lrt = chi2(1).sf(D_lrt).  The first six outputs are
 * bit-identical to pg_assoc_dev's.  l_alt, l_null (the same value in every row), D_lrt: float32 values widened to float64
 * (like the frame's lambda column); p_lrt float64.  The reference evaluates the quadratic forms of its ML functions with
 * float32 NumPy helpers (pyx:2045-2180); here they come from the same float64 sweeps as the REML path, so agreement with the
 * reference is at its float32 noise (l within 2 ulp, D within 2.5e-4: tests/golden/lrt_panels.npz), not bit-for-bit. */
int pg_assoc_lrt_dev(pg_ctx *ctx, int64_t n, int c, int64_t p, const float *d, const float *Wr, const float *yr,
                     const float *Xr, int64_t ldx, int grid, float *beta, float *se, float *tau, float *lambda,
                     double *F, double *pval, double *l_alt, double *l_null, double *D_lrt, double *p_lrt);

/* ---- The score test (GEMMA's -lmm 3: the score statistic at the null model's ML lambda), a first screen over a whole genome:
 * lambda is fitted once, on y ~ W, and every SNP is evaluated at it — no per-SNP search, one pass over the rotated X.
 *   pg_score_null_dev : lambda0 = the ML lambda of y ~ W, calc_lambda(eigenVals, Y, W) (lmm/lmm.py:22-84); the null search of
 *                       pg_assoc_lrt_dev (Brent); one float32 into lambda0_dev (device)
 *   pg_score_dev      : with h = 1/(lambda0 d + 1), G = W'HW, P0 = H - HW G^-1 W'H (all fp64; Cholesky of G):
 *                       P_xx = x'P0x, P_xy = x'P0y, P_yy = y'P0y, Px_yy = P_yy - P_xy^2 / P_xx, df = n - c - 1;
 *                       beta = P_xy / P_xx, se = sqrt(Px_yy / (df P_xx)), tau = df / Px_yy, lambda = lambda0 (float32 each),
 *                       F = n P_xy^2 / (P_yy P_xx), pval = F(1, df).sf(F) (float64; pval may be NULL).
 *                       A SNP with P_xx <= 1e-10 x'Hx (constant, in span(W)) or a non-finite x gets NaN in every column but lambda;
 *                       so does every SNP when the Cholesky of G fails (W rank-deficient).  A row depends only on its SNP.
 * Same argument checks as pg_assoc_dev. */
int pg_score_null_dev(pg_ctx *ctx, int64_t n, int c, const float *d, const float *Wr, const float *yr, float *lambda0_dev);
int pg_score_dev(pg_ctx *ctx, int64_t n, int c, int64_t p, const float *d, const float *Wr, const float *yr, float lambda0,
                 const float *Xr, int64_t ldx, float *beta, float *se, float *tau, float *lambda, double *F, double *pval);

/* ---- The plain linear model (GEMMA's -lm 1; the per-SNP OLS loop of experiments/1000G/run_lin_reg.py): the K-free baseline a
 * mixed-model scan is read against, straight from RAW genotypes — no eigensolver, no rotation (csrc/lm.hip).  For phenotype k
 * (k < t), SNP x and covariates W (n x c, full rank):  y_k = W alpha + x beta + eps,  df = n - c - 1.
 *   pg_lm_work_bytes : bytes of the device work area for (n, c, t); 0 for a shape the entries refuse
 *   pg_lm_setup_dev  : once per (W, Y), all in fp64: W'W = L L' (Cholesky), Q = W L^-T, Y~ = Y - Q Q'Y, syy_k = y~_k'y~_k; the panel
 *                      [Q | Y~] (columns padded to a multiple of 16) goes into work.  W n x c row-major, Y phenotype-major
 *                      (phenotype k is Y[k ldy .. k ldy + n), ldy >= n), float32 each.
 *   pg_lm_x_dev      : pb SNPs of an (n x pb) sample-major (snp_major = 0, row stride ldX >= pb) or (pb x n) SNP-major (ldX >= n)
 *                      block of dtype PG_DTYPE_*; values as the reference's X.astype(np.float32) (float64 rounded per element).
 *   pg_lm_bed_dev    : pb packed .bed records (row stride ldb >= ceil(n/4) bytes), code convention and count_a1 of
 *                      pg_rotate_bed_dev; a missing call takes the fp64 mean of the called genotypes of its SNP rounded to float32.
 *                      Per SNP, fp64 on v_mfma_f64_16x16x4_f64:  sxx = x'x - |Q'x|^2,  sxy_k = x'y~_k,  rss_k = syy_k - sxy_k^2 / sxx;
 *                      beta = sxy / sxx, se = sqrt(rss / (df sxx)), tau = df / rss (float32 each), F = df sxy^2 / (sxx rss),
 *                      pval = F(1, df).sf(F) (float64; pval may be NULL).  There is no lambda.
 *                      Outputs are phenotype-major windows: phenotype k's SNP g at [k ldo + g], ldo >= pb.
 *                      A SNP with sxx <= 1e-10 x'x (constant, in span(W)), a NaN or Inf, or an all-missing .bed record gets NaN in all
 *                      five columns for every phenotype; a rank-deficient or non-finite W (the Cholesky fails) gives NaN everywhere; a
 *                      non-finite phenotype NaN in its own rows only.  A row depends only on its SNP and on (W, Y).
 * PG_ENOTSUP for c outside 1..PG_MAX_COVARIATES or c + t > 64; PG_EINVAL for NULL pointers (but pval), t < 1, n - c - 1 <= 0 or strides
 * too small: a refused call enqueues nothing. */
size_t pg_lm_work_bytes(int64_t n, int c, int t);
int pg_lm_setup_dev(pg_ctx *ctx, int64_t n, int c, int t, const float *W, const float *Y, int64_t ldy, void *work);
int pg_lm_x_dev(pg_ctx *ctx, int64_t n, int c, int t, int64_t pb, const void *X, int dtype, int64_t ldX, int snp_major, const void *work,
                float *beta, float *se, float *tau, double *F, double *pval, int64_t ldo);
int pg_lm_bed_dev(pg_ctx *ctx, int64_t n, int c, int t, int64_t pb, const unsigned char *bed, int64_t ldb, int count_a1, const void *work,
                  float *beta, float *se, float *tau, double *F, double *pval, int64_t ldo);

/* ---- Per-SNP quality control from RAW genotypes (csrc/snp_stats.hip): what GEMMA's n_miss / af columns and its -miss / -maf / -hwe
 * filters are made of, read once from the block as it is stored.  Block conventions of pg_lm_x_dev / pg_lm_bed_dev: an (n x pb)
 * sample-major (snp_major = 0, ldX >= pb) or (pb x n) SNP-major (ldX >= n) block of dtype PG_DTYPE_*, or pb packed .bed records
 * (ldb >= ceil(n/4) bytes; code convention and count_a1 of pg_rotate_bed_dev).  An element is first rounded to float32.
 *   counts  : pb x 4 int64 {n_miss, n0, n1, n2}.  n_miss: .bed code 01, or a non-finite float element (an 8-bit block has no missing
 *             code); n0, n1, n2: observed elements that are exactly 0, 1 or 2 (-0.0 is 0).  The .bed pad bits after sample n - 1 are
 *             never counted.
 *   moments : pb x 4 fp64 {mean, var, min, max} over the n_obs = n - n_miss observed values, var the population variance (ddof = 0);
 *             all NaN with n_obs = 0.  A hard-call SNP (n0 + n1 + n2 == n_obs) takes them from the integers: S1 = n1 + 2 n2,
 *             S2 = n1 + 4 n2, mean = (double)S1 / (double)n_obs, var = (double)(n_obs S2 - S1^2) / (double)(n_obs^2) — one correctly
 *             rounded division each, the same bits from every storage.  Any other SNP takes fp64 two-pass moments (sum, then
 *             sum of (x - mean)^2) in a fixed order, without floating-point atomics.
 *             A row depends only on its SNP: not on pb, the row pitch, the batch boundaries or the run.
 *   work    : device scratch of pg_snp_stats_work_bytes(n, pb) bytes (the chunk partials of a sample-major block); 0 for a refused shape.
 *   pg_hwe_exact_dev : the exact Hardy-Weinberg test of Wigginton, Cutler and Abecasis (2005), two-sided, fp64, on p rows of counts of
 *             n samples.  N = n0 + n1 + n2, nr = 2 min(n0, n2) + n1, nc = 2N - nr; the probabilities P(h) of h = nr mod 2, ..., nr
 *             (step 2) heterozygotes are built unnormalised from the mode nr nc / 2N (raised by one to nr's parity) outward:
 *             P(h - 2) = P(h) h (h - 1) / (4 (a + 1)(b + 1)), P(h + 2) = P(h) 4 a b / ((h + 2)(h + 1)), a = (nr - h) / 2, b = N - h - a;
 *             pval = sum{P(h) : P(h) <= P(n1) (1 + 2^-30)} / sum P(h), at most 1 (the factor makes mathematically tied terms count
 *             whichever way they were reached).  N = 0 -> NaN; monomorphic -> 1.0; a row with n_miss + n0 + n1 + n2 != n (not
 *             hard-call) or a negative count -> NaN.
 * PG_EINVAL for NULL pointers, n < 1, n >= 2^30, pb < 0, pb > 2^25 (p >= 2^31 for pg_hwe_exact_dev), a sample-major block of 2^24 or
 * more workgroups (ceil(n / 256) chunks x ceil(pb / 256) column groups, ceil(pb / 128) for float64) or strides too small; PG_ENOTSUP
 * for an unknown dtype: a refused call enqueues nothing.  pg_snp_stats_bed_dev and a SNP-major pg_snp_stats_x_dev do not touch work
 * (any non-NULL pointer will do); only a sample-major block needs its pg_snp_stats_work_bytes. */
size_t pg_snp_stats_work_bytes(int64_t n, int64_t pb);
int pg_snp_stats_bed_dev(pg_ctx *ctx, int64_t n, int64_t pb, const unsigned char *bed, int64_t ldb, int count_a1, void *work, int64_t *counts,
                         double *moments);
int pg_snp_stats_x_dev(pg_ctx *ctx, int64_t n, int64_t pb, const void *X, int dtype, int64_t ldX, int snp_major, void *work, int64_t *counts,
                       double *moments);
int pg_hwe_exact_dev(pg_ctx *ctx, int64_t n, int64_t p, const int64_t *counts, double *pval);

/* ---- Linkage disequilibrium between hard-call SNPs on the int8 matrix pipe (csrc/ld.hip): the pairwise-complete Pearson r (PLINK's
 * --r) that LD pruning, clumping and a region's LD matrix are made of.  Block conventions of pg_snp_stats_x_dev / pg_snp_stats_bed_dev.
 * A SNP is hard-call when every non-missing value (in the element's own precision, nothing is rounded) is exactly 0, 1 or 2; missing is .bed code
 * 01, NaN or +-Inf (an 8-bit block has no missing code); any other SNP counts as ALL missing.  With m_a[i] in {0, 1} "sample i is
 * called" and x_a[i] its code (0 where missing), a pair (a, b) has six int32 sums over the n samples,
 *     N = sum m_a m_b   Sa = sum x_a m_b   Sb = sum m_a x_b   Sab = sum x_a x_b   Saa = sum x_a^2 m_b   Sbb = sum m_a x_b^2
 * then exactly in int64  ca = N Saa - Sa^2, cb = N Sbb - Sb^2, cab = N Sab - Sa Sb,  and
 *     r = clamp((double)cab / sqrt((double)ca (double)cb), -1, 1)  rounded once to float32;  NaN when ca <= 0 or cb <= 0
 * (no jointly called sample, or either SNP monomorphic among them).  A SNP against a copy gives exactly 1, against 2 - x exactly -1.
 *   image   : pg_ld_image_bytes(n, pe) device bytes on a 16-byte boundary, opaque: int8 planes x, m, x^2 of pe SNP-major rows (n padded
 *             with zeros to the K-tile of 128 samples) and per-SNP totals.  pg_ld_encode_{bed,x}_dev write the pb SNPs of a block to
 *             the SNP positions [at, at + pb) of an image for pe; pg_ld_shift_dev moves SNPs [from, from + count) to [0, count) —
 *             overlap-safe, the carry of a stream (4 ceil(count / from) device-to-device copies).  Positions never encoded hold whatever the memory held.
 *   pg_ld_block_dev : r[ia ldr + ib] = r(a0 + ia of image A, b0 + ib of image B), ia < na, ib < nb (A and B may be the same image).
 *   pg_ld_band_dev  : band[(j - j0) ldo + k] = r(j, j + 1 + k) for rows j in [j0, j0 + rows), k in [0, w), SNPs [0, have) of one image
 *             encoded; a partner j + 1 + k >= have gives NaN.  Only the tiles that meet the band run.
 *   sums    : or NULL; the six int32 of every pair, pair at element o of r / band at sums[6 o + t], t in the order N, Sa, Sb, Saa, Sbb,
 *             Sab; zeros where the band has no partner.  Nothing outside the na x nb (rows x w) window of r and sums is written.
 * A pair of 252-SNP tiles without a missing call takes one int8 product (N = n, the other sums from the per-SNP totals), any other
 * nine products over the three planes: the same integers either way (PG_LD_PLANES=1 in the environment sends every tile the second
 * way; tests and A/B timing only).
 * PG_EINVAL for NULL pointers, an image off 16 bytes, n < 1, n >= 2^28 (every sum fits int32), negative counts, windows outside the
 * image (at + pb > pe, a0 + na > pea, j0 + rows > have, have > pe, ...), w < 1 or strides too small; PG_ENOTSUP for an unknown dtype:
 * a refused call enqueues nothing.  pg_ld_image_bytes is 0 for n or pe out of range (pe < 1, pe >= 2^31). */
size_t pg_ld_image_bytes(int64_t n, int64_t pe);
int pg_ld_encode_bed_dev(pg_ctx *ctx, int64_t n, int64_t pb, const unsigned char *bed, int64_t ldb, int count_a1, void *image, int64_t pe,
                         int64_t at);
int pg_ld_encode_x_dev(pg_ctx *ctx, int64_t n, int64_t pb, const void *X, int dtype, int64_t ldX, int snp_major, void *image, int64_t pe,
                       int64_t at);
int pg_ld_shift_dev(pg_ctx *ctx, int64_t n, void *image, int64_t pe, int64_t from, int64_t count);
int pg_ld_block_dev(pg_ctx *ctx, int64_t n, const void *A, int64_t pea, int64_t a0, int64_t na, const void *B, int64_t peb, int64_t b0,
                    int64_t nb, float *r, int64_t ldr, int *sums);
int pg_ld_band_dev(pg_ctx *ctx, int64_t n, const void *image, int64_t pe, int64_t j0, int64_t rows, int64_t have, int64_t w, float *band,
                   int64_t ldo, int *sums);

/* ---- LD scores (csrc/ld.hip): l_j = sum over a window of r^2(j, k), the regressor of LD score regression, from the
 * pairs of pg_ld_band_dev without their band.  Image, rows, have and w as there, with a width per row:
 *   pairs   : rows j in [j0, j0 + rows) against j + 1 + k, 0 <= k < min(w, reach[j]) (reach NULL: w for every row); a partner at or
 *             past `have` is skipped.  reach, sum, npairs and nobs are indexed by image position (a stream passes ptr + base).
 *   value   : with the pair's exact int64 ca, cb, cab (above) the pair is DEFINED when ca > 0 and cb > 0 and, with adjust != 0, N > 2;
 *             then in fp64, every operation rounded once,  r2 = min(((double)cab (double)cab) / ((double)ca (double)cb), 1),  with adjust
 *             r2 = r2 - (1 - r2) / (double)(N - 2)  (the ldsc bias correction with the pair's own N),  q = rint(r2 2^32) to nearest even.
 *   sum, npairs : a defined pair ADDS q to sum[j] and to sum[partner] and 1 to npairs[j] and to npairs[partner]; an undefined pair adds
 *             nothing.  Accumulated in integer atomics (the caller zeroes them once): the same bits in any order, whatever the batch
 *             boundaries, the tile order or PG_LD_PLANES.  l_j = 1 + sum[j] / 2^32.
 *   nobs    : WRITTEN for the rows: n - missing calls when the SNP's own variance term (n - miss) sum x^2 - (sum x)^2 is positive, else 0
 *             (monomorphic, all missing, not hard-call).  Nothing else of nobs is touched.
 * PG_EINVAL for what pg_ld_band_dev refuses, a NULL sum, npairs or nobs, w >= 2^28 (2 w 2^32 stays inside int64) and a sum off 8 bytes:
 * a refused call enqueues nothing. */
int pg_ld_score_dev(pg_ctx *ctx, int64_t n, const void *image, int64_t pe, int64_t j0, int64_t rows, int64_t have, int64_t w,
                    const int32_t *reach, int adjust, int64_t *sum, int32_t *npairs, int32_t *nobs);

/* ---- Pairwise SNP x SNP interaction (epistasis) on the int8 matrix pipe (csrc/epistasis.hip): the allele-table odds-ratio
 * test of PLINK's --fast-epistasis over every pair of two windows of SNPs, reduced on the device to the pairs above a chi2 cut and a
 * per-SNP summary.  Samples carry a group: 1 case, 0 control, any other value in neither.  With x, m of a SNP as LD defines them (hard
 * calls only; a SNP that is not hard-call is all missing) a pair (a, b) has per group G four int32 sums over the samples of G,
 *     N = sum m_a m_b   Sa = sum x_a m_b   Sb = sum m_a x_b   Sab = sum x_a x_b
 * then exactly in int64 the allele table  A = 4 N - 2 Sa - 2 Sb + Sab,  B = 2 Sb - Sab,  C = 2 Sa - Sab,  D = Sab.  The group is DEFINED
 * for the pair when A + B, C + D, A + C and B + D are all positive.  Doubled cells t = 2 cell + z with z = 1 when any of the four cells is
 * 0 (1/2 added to every cell), else 0; in fp64, every operation rounded once,
 *     L = log(((double)tA (double)tD) / ((double)tB (double)tC))      v = (2 / tA + 2 / tD) + (2 / tB + 2 / tC)
 * PG_EPI_CASE_CONTROL: z = (L1 - L0) / sqrt(v1 + v0), defined when both groups are; PG_EPI_CASE_ONLY: z = L1 / sqrt(v1), defined when
 * the cases are.  chi2 = z z on 1 df.  z(a, b) and z(b, a) are the same bits.
 *   image   : pg_epi_image_bytes(n, pe) device bytes on a 16-byte boundary, opaque: six int8 planes x [g=1], x [g=0], m [g=1], m [g=0],
 *             x [g>=0], m [g>=0] of pe SNP-major rows with the LD image's row pitch, zero past sample n; per SNP {sum x in cases, sum x
 *             in controls, called cases, called controls} and a flag "a missing call among the cases and controls"; the group sizes.
 *   pg_epi_split_dev : writes the SNP positions [from, from + count) of an epistasis image for pe from the same positions of an LD
 *             image for pe (pg_ld_encode_{bed,x}_dev) and the int8 group[n] (device memory).  Every SNP of an image, and both images of a
 *             pg_epi_block_dev call, must have been split with the same group vector.
 *   pg_epi_block_dev : visits the pairs (a0 + ia of image A, b0 + ib of image B), ia < na, ib < nb (A and B may be the same image).
 *             The pair's SNPs carry the GLOBAL indices ga0 + ia and gb0 + ib (32-bit): the hit records, `best` and the per-SNP arrays
 *             speak in them (with ga0 = a0, gb0 = b0 that is the image position, as in pg_ld_score_dev).  upper != 0: only the pairs
 *             with ga0 + ia < gb0 + ib are visited; tile pairs wholly on or below the diagonal return at once.
 *   count, hits, cap : a visited, defined pair with chi2 >= chi2_min takes the next slot of the 64-bit counter *count (the caller
 *             zeroes it; it counts every hit) and, while slot < cap, is written as the 16-byte record {int32 a, int32 b, double z}
 *             at hits[slot], in no particular order.  Nothing is written at or past cap; hits may be NULL when cap = 0.
 *   n_tot, n_sig, best : each or NULL; indexed by global index, accumulated with integer atomics (the caller zeroes them once): a
 *             defined pair adds 1 to n_tot of both of its SNPs, a hit 1 to n_sig of both, and best[s] becomes the maximum of
 *             (float32 bits of (float)chi2) << 32 | ~partner (32 bits) over the defined pairs of s: the same bits in any order, ties
 *             to the smaller partner.
 *   sums    : or NULL; eight int32 of every VISITED pair at sums[8 (ia nb + ib) + t], t in the order N, Sa, Sb, Sab of the cases, then
 *             of the controls.  Nothing outside the na x nb window is written.
 * A tile pair (128 SNPs of A, 256 of B) without a missing call among the cases and controls takes one int8 product (N the group's
 * size, Sa and Sb from the per-SNP totals), any other four products over the masked planes: the same integers either way
 * (PG_EPI_PLANES=1 in the environment sends every tile pair the second way; tests and A/B timing only).
 * PG_EINVAL for NULL pointers (ctx, images, group, count, hits with cap > 0), an image or hits off 16 bytes, count or best off 8, n < 1,
 * n >= 2^28, negative counts or indices, windows outside their images, a global index of 2^31 or more, cap < 0, chi2_min negative
 * or not finite; PG_ENOTSUP for an unknown mode: a refused call enqueues nothing.  pg_epi_image_bytes is 0 for n or pe out of range. */
#define PG_EPI_CASE_CONTROL 0
#define PG_EPI_CASE_ONLY 1
size_t pg_epi_image_bytes(int64_t n, int64_t pe);
int pg_epi_split_dev(pg_ctx *ctx, int64_t n, const void *ld_image, int64_t pe, int64_t from, int64_t count, const signed char *group,
                     void *epi_image);
int pg_epi_block_dev(pg_ctx *ctx, int64_t n, const void *A, int64_t pea, int64_t a0, int64_t na, int64_t ga0, const void *B, int64_t peb,
                     int64_t b0, int64_t nb, int64_t gb0, int mode, int upper, double chi2_min, uint64_t *count, void *hits, int64_t cap,
                     int32_t *n_tot, int32_t *n_sig, uint64_t *best, int32_t *sums);

/* ---- Polygenic scores from RAW genotypes on the fp64 matrix pipe (csrc/prs.hip): S = G W, PLINK's --score, accumulated over
 * the SNP batches of a stream.  Block conventions of pg_snp_stats_x_dev / pg_snp_stats_bed_dev: an (n x pb) sample-major (snp_major = 0,
 * ldX >= pb) or (pb x n) SNP-major (ldX >= n) block of dtype PG_DTYPE_*, or pb packed .bed records (ldb >= ceil(n/4) bytes; code
 * convention and count_a1 of pg_rotate_bed_dev).  An element is first rounded to float32; missing is .bed code 01 or a non-finite float
 * element (an 8-bit block has no missing code); pad bits and pad elements are never read into a result.
 *   Wt      : t <= PG_PRS_MAX_T weight columns, score-major: the weight of the block's SNP g in column k at Wt[k ldw + g], ldw >= pb.
 *   score   : t rows of lds >= n doubles, called the same shape in int64 or NULL; both accumulated in place (the caller zeroes them
 *             before the first batch); nothing outside [k lds, k lds + n) is written.
 *   values  : x_gi = the stored value widened to fp64; a missing call is 0 (impute = 0) or mu_g (impute != 0), bit for bit the mean
 *             pg_snp_stats_*_dev reports for the SNP (the exact division of a hard-call SNP, else the fixed-order two-pass mean: those
 *             kernels run as a pre-pass over the batch); every call of an all-missing SNP is 0.
 *             score[k][i] += sum_g x_gi w_gk;   called[k][i] += #{g : sample i called at g and w_gk != 0}, whatever impute.
 *   order   : the block's SNPs are cut into chunks of PG_PRS_CHUNK from its first SNP; a chunk's partial is accumulated from zero on
 *             v_mfma_f64_16x16x4_f64 (K = SNPs) in an order that depends only on the position inside the chunk; the partials are added
 *             to score in ascending chunk order; no floating-point atomics.  A row depends only on the inputs and on where the batch
 *             boundaries fall — not on pitches, alignment, the device or the run — and not on the batch sizes at all when every batch
 *             but the last holds a multiple of PG_PRS_CHUNK SNPs.  The counts are exact.
 *   work    : device scratch of pg_prs_work_bytes(n, pb, t) bytes: the pre-pass's outputs and the per-chunk partials (split-K: one
 *             workgroup per chunk and 256 samples, 12 t n bytes per chunk, added in order by a second kernel); 0 for a refused shape.
 * PG_EINVAL for NULL pointers (but called), n < 1, n >= 2^30, pb < 0, pb > 2^25, t < 1, a block of 2^31 or more workgroups
 * (ceil(n / 256) sample groups x ceil(pb / 256) chunks), strides too small, or a pre-pass that pg_snp_stats_x_dev refuses; PG_ENOTSUP for t > PG_PRS_MAX_T or an unknown dtype: a refused call enqueues nothing.  pb = 0 is a no-op. */
#define PG_PRS_CHUNK 256      /* SNPs per summation chunk */
#define PG_PRS_MAX_T 64       /* weight columns per call: four 16-column tiles */
size_t pg_prs_work_bytes(int64_t n, int64_t pb, int t);      /* 0 for a refused shape */
int pg_prs_bed_acc_dev(pg_ctx *ctx, int64_t n, int64_t pb, const unsigned char *bed, int64_t ldb, int count_a1, int t, const double *Wt,
                       int64_t ldw, int impute, void *work, double *score, int64_t *called, int64_t lds);
int pg_prs_x_acc_dev(pg_ctx *ctx, int64_t n, int64_t pb, const void *X, int dtype, int64_t ldX, int snp_major, int t, const double *Wt,
                     int64_t ldw, int impute, void *work, double *score, int64_t *called, int64_t lds);

/* ---- Principal components from RAW genotypes on the fp64 matrix pipe (csrc/pca.hip): the two skinny products of a
 * randomised block subspace iteration against the standardised genotypes Z (pb x n), T = Z'Q and Y += Z T.  Block conventions of
 * pg_prs_*_acc_dev / pg_snp_stats_*_dev: an (n x pb) sample-major (snp_major = 0, ldX >= pb) or (pb x n) SNP-major (ldX >= n) block of
 * dtype PG_DTYPE_*, or pb packed .bed records (ldb >= ceil(n/4) bytes; code convention and count_a1 of pg_rotate_bed_dev).  An element is
 * first rounded to float32; missing is .bed code 01 or a non-finite float element (an 8-bit block has no missing code); pad bits and
 * pad elements never reach a result and are never read.
 *   stat    : pb x 2 doubles {mu_g, isd_g}.  pg_pca_stat_* runs pg_snp_stats_*_dev over the block as a pre-pass and writes mu_g = the
 *             mean it reports, bit for bit (0 for a SNP without a called sample), and with v = var_g ((double)n_obs / (double)n)
 *             isd_g = v > 0 ? 1.0 / sqrt(v) : 0.0 (IEEE division and square root): the population sd over all n samples after mean
 *             imputation, lmm.kinship(standardize=True)'s; a constant or all-missing SNP contributes zeros.  A row depends only on
 *             its SNP.  stat is an INPUT of proj and back: new samples are projected with the training panel's moments.
 *   values  : z_gi = fl(fl(x_gi - mu_g) isd_g), two fp64 roundings; 0 for a missing call, a sample >= n and a SNP >= pb.
 *   Q, Y, T : component-major, like the scores of pg_prs: component k of sample i at Q[k ldq + i] (ldq >= n), of SNP g at T[k ldt + g]
 *             (ldt >= pb); l <= PG_PCA_MAX_L components.  The output of back is the input of proj.
 *   proj    : T[k][g] = sum_i z_gi Q[k][i] on v_mfma_f64_16x16x4_f64 with the samples as K.  An output is one fixed chain that depends
 *             only on the SNP, its stat and Q — not on the SNP's slot, tile, batch, pitch, alignment or storage; no split over samples,
 *             no atomics.  Nothing outside [k ldt, k ldt + pb), k < l, is written.
 *   back    : Y[k][i] += sum_g z_gi T[k][g] (the caller zeroes Y before the first batch), the SNPs as K.  The ordering contract of
 *             pg_prs_*_acc_dev: the block's SNPs are cut into chunks of PG_PCA_CHUNK from its first SNP; a chunk's partial is accumulated
 *             from zero in an order that depends only on the position inside the chunk; a second kernel adds the partials to Y in
 *             ascending chunk order; no floating-point atomics.  Y does not depend on the batch sizes when every batch but the last
 *             holds a multiple of PG_PCA_CHUNK SNPs.  Nothing outside [k ldy, k ldy + n), k < l, is written.
 *   work    : device scratch of pg_pca_work_bytes(n, pb, l) bytes: the pre-pass's outputs (stat; any l will do) and the per-chunk
 *             partials (back: 8 l n bytes per chunk); 0 for a refused shape.
 * PG_EINVAL for NULL pointers, n < 1, n >= 2^30, pb < 0, pb > 2^25, l < 1, strides too small, a block of 2^31 or more workgroups
 * (ceil(n / 256) sample groups x ceil(pb / 256) chunks) or a pre-pass that pg_snp_stats_x_dev refuses; PG_ENOTSUP for l > PG_PCA_MAX_L or
 * an unknown dtype: a refused call enqueues nothing.  pb = 0 is a no-op. */
#define PG_PCA_CHUNK 256      /* SNPs per summation chunk of the back-product */
#define PG_PCA_MAX_L 64       /* columns of the iterated block: four 16-column tiles */
size_t pg_pca_work_bytes(int64_t n, int64_t pb, int l);      /* 0 for a refused shape */
int pg_pca_stat_bed_dev(pg_ctx *ctx, int64_t n, int64_t pb, const unsigned char *bed, int64_t ldb, int count_a1, void *work, double *stat);
int pg_pca_stat_x_dev(pg_ctx *ctx, int64_t n, int64_t pb, const void *X, int dtype, int64_t ldX, int snp_major, void *work, double *stat);
int pg_pca_proj_bed_dev(pg_ctx *ctx, int64_t n, int64_t pb, const unsigned char *bed, int64_t ldb, int count_a1, const double *stat, int l,
                        const double *Q, int64_t ldq, double *T, int64_t ldt);
int pg_pca_proj_x_dev(pg_ctx *ctx, int64_t n, int64_t pb, const void *X, int dtype, int64_t ldX, int snp_major, const double *stat, int l,
                      const double *Q, int64_t ldq, double *T, int64_t ldt);
int pg_pca_back_bed_dev(pg_ctx *ctx, int64_t n, int64_t pb, const unsigned char *bed, int64_t ldb, int count_a1, const double *stat, int l,
                        const double *T, int64_t ldt, void *work, double *Y, int64_t ldy);
int pg_pca_back_x_dev(pg_ctx *ctx, int64_t n, int64_t pb, const void *X, int dtype, int64_t ldX, int snp_major, const double *stat, int l,
                      const double *T, int64_t ldt, void *work, double *Y, int64_t ldy);

/* ---- SNP-by-environment interaction (GEMMA's -gxe): for SNP g with rotated genotype x = U'x_g and rotated interaction
 * xe = U'(x_g o e), the REML Wald test of xe in  y ~ W' + x + xe,  W' = the c shared covariates (the caller's W and U'e).
 * Row g is by definition calculate(d, yr, [W', x], xe) of pg_assoc_dev's arithmetic with c + 1 covariates (decade scan,
 * brentq + Newton, no grid): beta = beta_gxe, se, tau, lambda (float32), F (float64), pval = F(1, n - c - 2).sf(F) (may be NULL).
 * Degenerate rows (constant x, xe in span([W', x]), a non-finite SNP, rank-deficient W') get NaN where calculate() does.
 *   Wr n x c row-major, yr n, d n;  xr: p rows of n floats at row stride ldx >= n;  xer the same at ldxe >= n.
 *   c = 1..PG_MAX_COVARIATES - 1 (else PG_ENOTSUP); n - c - 2 > 0 and non-NULL pointers (but pval, stats_dev), else PG_EINVAL.
 *   pg_assoc_gxe_warm  : as pg_assoc_warm, for pg_assoc_gxe_dev with c shared covariates.
 *   pg_gxe_scale_u_dev : Ue[i n + k] = e_i U[i ldU + k] (one float32 rounding; Ue dense n x n): U'(x o e) = Ue' x, so x o e is
 *                        rotated by any rotation path of x with Ue (and its pg_geno_prep_dev image) in U's place. */
int pg_assoc_gxe_dev(pg_ctx *ctx, int64_t n, int c, int64_t p, const float *d, const float *Wr, const float *yr,
                     const float *xr, int64_t ldx, const float *xer, int64_t ldxe, float *beta, float *se, float *tau,
                     float *lambda, double *F, double *pval, unsigned long long *stats_dev);
int pg_assoc_gxe_warm(pg_ctx *ctx, int64_t n, int c);
int pg_gxe_scale_u_dev(pg_ctx *ctx, int64_t n, const float *U, int64_t ldU, const float *e, float *Ue);

/* host-pointer convenience: X in the REFERENCE layout (n x p row-major, already rotated), as
 * calculate() receives it; transposed to SNP-major on the device. */
int pg_assoc(pg_ctx *ctx, int64_t n, int c, int64_t p, const float *d, const float *Wr, const float *yr,
             const float *X_n_by_p, int grid, float *beta, float *se, float *tau, float *lambda, double *F,
             double *pval, unsigned long long *stats2);

/* pg_assoc over several GPUs of the node: contiguous blocks of ceil(p/ngpu) SNP columns like the reference's
 * SampleIter (lmm/lmm.py:427-434) — one host thread and one context per GPU; the 32-byte result rows of all blocks are
 * all-gathered over RCCL (pg_comm_*) and leave the node's GPU 0 in SNP order with one copy per column. */
int pg_assoc_multi(int ngpu, int64_t n, int c, int64_t p, const float *d, const float *Wr, const float *yr,
                   const float *X_n_by_p, int grid, float *beta, float *se, float *tau, float *lambda, double *F, double *pval);

/* scipy.stats.f.sf(F, 1, dfd) (lmm/lmm.py:482) for a device vector */
int pg_fdist_sf_dev(pg_ctx *ctx, int64_t count, const double *F, double dfd, double *pval);

/* (n x p row-major, row stride ldX >= p) -> SNP-major (p x ldx), pad columns [n, ldx) zero-filled */
int pg_transpose_dev(pg_ctx *ctx, int64_t n, int64_t p, const float *X_n_by_p, int64_t ldX, float *Xr, int64_t ldx);

/* ---- H2: rotation  X <- U' X  (lmm/lmm.py:243-246, OpenBLAS sgemm in the reference) ---------
 * U (n x n, row stride ldU) row-major with eigenvector j in COLUMN j (scipy.linalg.eigh's convention); X in
 * the reference layout (n x p, row stride ldX >= p: a column window of a wider matrix is fine); output
 * SNP-major Xr (p x ldx): Xr[g*ldx + k] = sum_i U[i*ldU + k] * X[i*ldX + g], pad columns [n, ldx) zeroed.
 * fp32 MFMA (v_mfma_f32_32x32x2_f32), fp32 accumulate in sample order i = 0..n-1 — the reference's precision. */
int pg_rotate_dev(pg_ctx *ctx, int64_t n, int64_t p, const float *U, int64_t ldU, const float *X_n_by_p, int64_t ldX,
                  float *Xr, int64_t ldx);

/* ---- N4: rotation fast path for GENOTYPE columns (each column of the block takes <= 3 equally spaced
 * values: hard calls 0/1/2, raw or centred/standardised).  U'x = v0 (U'1) + dx (U'code): the codes are exact in int8,
 * U is held once as a 24-bit fixed point per eigenvector in three int8 digit planes (|error| <= 2^-24 * 2 max_i |U[i][k]|:
 * float32's own rounding for entries within a factor two of the column's largest), products and sums are EXACT on the int8
 * MFMA pipe, and the three partial sums meet in fp64 with one rounding to float32 (error below pg_rotate_dev's / the
 * reference's sgemm's fp32 accumulation on delocalised eigenvectors, within 3x of it on the adversarial ones of
 * tests/test_gpu_rotate.py; 1/7 of its time).  PG_GENO_I8=0 selects the r2-r3 kernel instead: U split into two fp16 planes by
 * round-to-nearest (residual <= 2^-23 |U|), fp32 accumulation on the fp16 MFMA pipe.  A column may also hold ONE other
 * value anywhere (missing calls imputed with the column mean, experiments/benchmarks/benchmarks.py:243-244): such blocks
 * take a second, accumulating pass of the SAME kernel on the 0/1 indicator plane — int8 like the codes, exact like them:
 * Xr = float32(fma(delta_g 2^(E_k - 22), U'ind, Xr)) for every row of the block (the fp16 kernel's with PG_GENO_I8=0).  The whole
 * genotype path is integer sums, one fp64 fma and one rounding per pass: tests/test_gpu_rotate_i8_exact.py predicts every bit.
 * Finite blocks that are not genotype-valued (imputed dosages, any float X) take the same GEMM with X itself split into two
 * fp16 planes (per-column power-of-two scale, residual <= 2^-23 |x|): two passes, still 3x faster than pg_rotate_dev.
 *   pg_geno_prep_dev   : once per U -> Uprep (pg_geno_prep_bytes(n) bytes, device)
 *   pg_rotate_geno_dev : per SNP block; Xr written (same layout as pg_rotate_dev) and *is_geno = 1 (genotype-valued block)
 *                        or 2 (general finite block, split path); *is_geno = 0 and Xr untouched when the block holds a NaN
 *                        or Inf (call pg_rotate_dev: its propagation is the reference's).  Synchronises the stream. */
size_t pg_geno_prep_bytes(int64_t n);
size_t pg_geno_work_bytes(int64_t n, int64_t p);
/* The detect pass in front of these rotations reads X ONCE (extremes, codes and flags from one kernel, 2-bit tags of every element of
 * a 32-SNP strip held in LDS) when n <= pg_geno_onepass_max_n(LDS bytes one workgroup may use), and in two passes above that;
 * pg_geno_onepass_limit is that bound on the context's device.  Same outputs either way; PG_GENO_ONEPASS=0 forces the two passes. */
int64_t pg_geno_onepass_max_n(int64_t lds_bytes);
int64_t pg_geno_onepass_limit(pg_ctx *ctx);
int pg_geno_prep_dev(pg_ctx *ctx, int64_t n, const float *U, int64_t ldU, void *Uprep);
int pg_rotate_geno_dev(pg_ctx *ctx, int64_t n, int64_t p, const void *Uprep, const float *X_n_by_p, int64_t ldX, float *Xr,
                       int64_t ldx, void *work, int *is_geno);
/* pg_rotate_geno_dev + the caller's fallback to pg_rotate_dev in ONE enqueue, with the path chosen on the device: every candidate
 * kernel is launched predicated on the flags of the detect pass, so the stream is never synchronised (the flag read-back of
 * pg_rotate_geno_dev idles the GPU for ~0.7 ms per 16 384-SNP block at n = 10 000).  float32 X only.  U (row stride ldU) is the
 * operand of the fp32-MFMA fallback; path_dev (device int, may be NULL) receives 1 / 2 / 0 like *is_geno. */
int pg_rotate_auto_dev(pg_ctx *ctx, int64_t n, int64_t p, const float *U, int64_t ldU, const void *Uprep, const float *X_n_by_p, int64_t ldX,
                       float *Xr, int64_t ldx, void *work, int *path_dev);
int pg_rotate_auto_i8_dev(pg_ctx *ctx, int64_t n, int64_t p, const void *Uprep, const void *X8_n_by_p, int is_unsigned, int64_t ldX,
                          float *Xr, int64_t ldx, void *work, int *path_dev);   /* int8/uint8 X (always finite): genotype or split path */
/* The same for X stored as 8-bit integers (int8 / uint8 genotype matrices; the reference casts any dtype to float32,
 * lmm/lmm.py:121-122, so the values are identical): 4x fewer bytes to upload and to scan.  pg_cast_i8_f32_dev makes the
 * float32 image a block needs when it does not qualify (then pg_rotate_dev as usual). */
int pg_rotate_geno_i8_dev(pg_ctx *ctx, int64_t n, int64_t p, const void *Uprep, const void *X8_n_by_p, int is_unsigned, int64_t ldX,
                          float *Xr, int64_t ldx, void *work, int *is_geno);
int pg_cast_i8_f32_dev(pg_ctx *ctx, int64_t n, int64_t p, const void *X8_n_by_p, int is_unsigned, int64_t ldX, float *Xf, int64_t ldXf);
/* ... and for float64 X (numpy's default): the reference's X.astype(np.float32) is a per-element round-to-nearest, which the
 * kernels apply as they read the block — no host-side float32 copy of the matrix. */
int pg_rotate_geno_f64_dev(pg_ctx *ctx, int64_t n, int64_t p, const void *Uprep, const double *X_n_by_p, int64_t ldX, float *Xr,
                           int64_t ldx, void *work, int *is_geno);
int pg_cast_f64_f32_dev(pg_ctx *ctx, int64_t n, int64_t p, const double *X_n_by_p, int64_t ldX, float *Xf, int64_t ldXf);
/* The same rotation straight from a PLINK .bed block (the format the reference's callers read with pysnptools.Bed,
 * experiments/benchmarks/benchmarks.py:233-239): bed = device copy of p SNP records of ldb >= ceil(n/4) bytes (SNP-major,
 * 2 bits per sample: 00 hom A1, 01 missing, 10 het, 11 hom A2).  Dosage = copies of A2 (count_a1 = 0, pysnptools
 * count_A1=False) or of A1; missing calls take the mean of the called genotypes of their SNP (SimpleImputer 'mean',
 * benchmarks.py:243-244).  16x fewer input bytes than float32 X.  work: pg_geno_work_bytes(n, p). */
int pg_rotate_bed_dev(pg_ctx *ctx, int64_t n, int64_t p, const void *Uprep, const unsigned char *bed, int64_t ldb, int count_a1,
                      float *Xr, int64_t ldx, void *work);

/* ---- N3: relatedness matrix from standardised genotypes, K = G G' / p_k
 * (experiments/animal_gwas/run_gwas.py:45-55, tests/test_pygemma.py:184-192).  Gt is the SNP-major (p_k x ldg)
 * image of the standardised G (n x p_k), e.g. from pg_transpose_dev; K (n x n, row-major) float32, both triangles written
 * (computed as a syrk: tiles on or below the diagonal only). */
int pg_kinship_dev(pg_ctx *ctx, int64_t n, int64_t p_k, const float *Gt, int64_t ldg, float *K);
/* The same straight from the (n x p) genotype matrix G (row-major, row stride ldG), as calculate_genetic_relatedness_matrix
 * builds it (run_gwas.py:46-56): standardize != 0 centres every column and divides by its population standard deviation
 * (fp64 statistics, sd == 0 -> 1) on the device; then a lower-triangle syrk on the fp32 MFMA pipe (the upper triangle is the
 * mirror, bit-symmetric).  K can go straight into pg_syevd_dev. */
int pg_kinship_geno_dev(pg_ctx *ctx, int64_t n, int64_t p, const float *G, int64_t ldG, int standardize, float *K);

/* ---- The same K accumulated over SNP batches (csrc/kinship.hip): host and device memory bounded at any p.
 * acc: device buffer of pg_kinship_acc_bytes(n, pb) bytes for the largest batch pb used — an fp64 n x n accumulator (its first
 *      8 n^2 bytes, zeroed by the caller before the first batch; lower triangle used) followed by the batch work area.
 * pg_kinship_bed_acc_dev : pb packed .bed records (row stride ldb >= ceil(n/4) bytes), code convention and count_a1 of
 *      pg_rotate_bed_dev; a missing call takes the mean of the called genotypes of its SNP; an all-missing SNP contributes zeros.
 * pg_kinship_x_acc_dev   : an (n x pb) sample-major (snp_major = 0, row stride ldX >= pb) or (pb x n) SNP-major (ldX >= n) block of
 *      dtype PG_DTYPE_*.  8-bit values and .bed codes go through the fp16 matrix pipe (exact operand, the other in two fp16 planes,
 *      fp32 accumulation per batch); float blocks, and every block when the environment has PG_KINSHIP_FP32=1, through the fp32 syrk.
 *      Per SNP: fp64 mean and population variance over all n samples after imputation; standardize != 0 centres and scales by 1/sd
 *      (sd == 0 -> 1), else X X'.
 * pg_kinship_finish_dev  : K = acc / p as float32 (n x n, row-major), both triangles, bit-symmetric; p = the total number of SNPs.
 * Batches are summed in call order on the context's stream; the result depends only on the inputs and the batch boundaries. */
enum { PG_DTYPE_INT8 = 0, PG_DTYPE_UINT8 = 1, PG_DTYPE_FLOAT32 = 2, PG_DTYPE_FLOAT64 = 3 };
size_t pg_kinship_acc_bytes(int64_t n, int64_t pb);
int pg_kinship_bed_acc_dev(pg_ctx *ctx, int64_t n, int64_t pb, const unsigned char *bed, int64_t ldb, int count_a1, int standardize,
                           double *acc);
int pg_kinship_x_acc_dev(pg_ctx *ctx, int64_t n, int64_t pb, const void *X, int dtype, int64_t ldX, int snp_major, int standardize,
                         double *acc);
int pg_kinship_finish_dev(pg_ctx *ctx, int64_t n, int64_t p, const double *acc, float *K);

/* ---- KING-robust relatedness, IBS similarity and per-sample QC counts on the int8 matrix pipe (csrc/king.hip), accumulated
 * over the SNP batches of a stream.  Block conventions of pg_kinship_x_acc_dev / pg_kinship_bed_acc_dev; elements and hard calls as for
 * LD above: missing is .bed code 01, NaN or +-Inf (an 8-bit block has no missing code), a SNP with a non-missing value other than
 * exactly 0, 1, 2 counts as ALL missing for every sample.  Sample i at a SNP has m (called), h (called and 1), a (called and 0),
 * b (called and 2); a pair (i, j) has the int32 sums over all SNPs of all batches
 *     N = sum m_i m_j   HH = sum h_i h_j   IBS0 = sum (a_i b_j + b_i a_j)   Hij = sum h_i m_j   (Hij is not symmetric: Hji = Hij')
 *     IBS1 = Hij + Hji - 2 HH,  IBS2 = N - IBS0 - IBS1,  all exact;
 *     phi = float32((double)(HH - 2 IBS0) / (double)(Hij + Hji)), NaN when Hij + Hji == 0   (what plink2 --make-king prints)
 *     ibs = float32(1 - (double)(IBS1 + 2 IBS0) / (double)(2 N)),  NaN when N == 0.
 * A sample against itself or an exact copy gives phi = 0.5 exactly; phi does not depend on count_a1.
 *   acc     : pg_king_acc_bytes(n, pb) device bytes on a 16-byte boundary for the largest batch pb used, opaque.  Its first
 *             pg_king_zero_bytes(n) bytes (four n x n int32 accumulators, the totals of the batches without a missing call, the
 *             per-sample counts) are zeroed by the caller before the first batch; the rest (flags and the int8 planes c = b - a, h, m
 *             of one batch, n sample-major rows of pb rounded up to the K-tile of 128 SNPs) is rewritten by every batch.
 *   pg_king_{bed,x}_acc_dev : add one batch of pb SNPs.  A batch without a missing call takes two int8 products per pair of 256-sample
 *             tiles (c c', h h'; N and Hij grow by per-batch totals), any other five (c c', h h', m m', h m' and its transpose); the
 *             same integers either way (PG_KING_PLANES=1 in the environment sends every batch the second way; tests and A/B timing).
 *             "Without a missing call" is about the calls of hard-call SNPs: a SNP of an array that is not hard-call has all-zero
 *             planes and does not count in the batch's N, on either path.  With PG_KING_TIMING=1 in the environment every batch
 *             is bracketed by events and waited for, and pg_king_last_batch_ms gives the milliseconds of the calling thread's
 *             last batch: encode (flags, screen, encode, totals) and pair kernel; same results (tools/bench_king.py).
 *   pg_king_finish_dev : out (n x n float32, row-major, both triangles, bit-symmetric) = phi (what = 0) or ibs (what = 1).
 *   pg_king_counts_dev : counts5 = five n x n int32 matrices one after the other, every entry of both triangles: N, HH, IBS0,
 *             Hij (row i, column j: i's het calls where j is called) and IBS1; sample5 = n x 5 int64, row i = n_obs, n_miss, n0, n1, n2
 *             of sample i (count_a1 swaps n0 and n2; a SNP that is not hard-call adds 1 to every n_miss).
 *   pg_sample_stats_{bed,x}_acc_dev : the count kernel alone: ADDS the batch's n x 5 counts (the layout above) to sample5, which the
 *             caller zeroes before the first batch.  Scratch comes from the context.
 * Batches are summed in call order on the context's stream; every count is an integer, so the result does not depend on the batch
 * boundaries.  The total number of SNPs over all batches must stay below 2^31 (every count fits int32).
 * PG_EINVAL for NULL pointers, an accumulator off 16 bytes, n < 1, n >= 2^20, pb < 1, pb >= 2^31, `what` other than 0 or 1 or strides
 * too small; PG_ENOTSUP for an unknown dtype: a refused call enqueues nothing.  pg_king_acc_bytes and pg_king_zero_bytes are 0 for a
 * refused shape. */
size_t pg_king_acc_bytes(int64_t n, int64_t pb);
size_t pg_king_zero_bytes(int64_t n);
int pg_king_last_batch_ms(float *encode_ms, float *pair_ms);
int pg_king_bed_acc_dev(pg_ctx *ctx, int64_t n, int64_t pb, const unsigned char *bed, int64_t ldb, int count_a1, void *acc);
int pg_king_x_acc_dev(pg_ctx *ctx, int64_t n, int64_t pb, const void *X, int dtype, int64_t ldX, int snp_major, void *acc);
int pg_king_finish_dev(pg_ctx *ctx, int64_t n, const void *acc, int what, float *out);
int pg_king_counts_dev(pg_ctx *ctx, int64_t n, const void *acc, int32_t *counts5, int64_t *sample5);
int pg_sample_stats_bed_acc_dev(pg_ctx *ctx, int64_t n, int64_t pb, const unsigned char *bed, int64_t ldb, int count_a1, int64_t *sample5);
int pg_sample_stats_x_acc_dev(pg_ctx *ctx, int64_t n, int64_t pb, const void *X, int dtype, int64_t ldX, int snp_major, int64_t *sample5);

/* ---- lmm/lmm.py:124-125: K <- Z K Z' for the optional design matrix Z (n x q) of the random effect, K (q x q).  Z and K may each be
 * float32 or float64 (z_is_f64 / k_is_f64), row-major with row strides ldz / ldk, on the device; out = float32 (n x n, row stride ldo),
 * what lmm.py:127-128 hands to the eigensolver.  Two fp64-MFMA products and one rounding. */
int pg_zkzt_dev(pg_ctx *ctx, int64_t n, int64_t q, const void *Z, int z_is_f64, int64_t ldz, const void *K, int k_is_f64, int64_t ldk,
                float *out, int64_t ldo);

/* ---- H1: eigendecomposition of K (lmm/lmm.py:151-162 / :196-207, scipy.linalg.eigh = LAPACK ssyevr)
 * Reads the LOWER triangle of row-major K (n x n, float32, device).  Computes in fp64; delivers ascending
 * eigenvalues clamped at 0 (lmm/lmm.py:157) as float32, and U (column j = eigenvector j) as float32
 * (and optionally fp64 for the invariant checks: U64/evals64 may be NULL).
 * Two reductions to tridiagonal form behind this one entry point: from n = 768 on, dense -> band (fp64 MFMA GEMMs) -> tridiagonal
 * (persistent bulge-chasing kernel) with two blocked back-transformations (csrc/sb2.hip); below that, and for a K whose panels the
 * band reduction cannot factor (rank-deficient K: decided on the device), the one-stage Householder reduction (csrc/syevd.hip).
 * Environment, for tests and A/B timing only: PG_SYEVD_STAGES=1|2 forces a path, PG_SYEVD_TIMING=1 prints phase times.
 * Work space ~ 10 n^2 doubles on the two-stage path (200 GB at n = 50 000; when the device cannot give it the one-stage path is taken),
 * ~ 8 n^2 on the one-stage path. */
int pg_syevd_dev(pg_ctx *ctx, int64_t n, const float *K, float *evals, float *U, double *evals64, double *U64);

/* ---- Inspection surface: the model-level functions the reference's tests call directly
 * (tests/test_pygemma.py:256-294).  One wavefront each; for fixture-level parity, not for throughput.
 * All pointers are device pointers.  ctot = columns of Wx = the reference's np.c_[W, x] (SNP last), m = ctot + 1.
 *
 * pg_precompute_mat_dev : precompute_mat(lam, eigenVals, W, Y, full) (pygemma_model.pyx:880-1053).
 *     P3/Q3/R3 : m*m*m float32 each, indexed [row][level][col] like wjt_Pi_wk / wjt_Pi_Pi_wk / wjt_Pi_Pi_Pi_wk;
 *                entries the reference leaves undefined (np.empty) are NaN; R3 all NaN unless full.
 *     vecs     : [5][m] = yt_Pi_y, yt_Pi_Pi_y, yt_Pi_Pi_Pi_y, tr_Pi, tr_Pi_Pi per level.
 *     scal     : 8 floats = logdet_Wt_H_inv_W, logdet_H, then d1, d2 (NaN unless full), logL at the last level, sum h, sum h^2
 *                (NaN unless full): the un-projected traces the ML functions use.
 * pg_newton_dev         : newton(lam, eigenVals, Y, W, precompute=True, lambda_min, lambda_max) (pyx:1349-1416) -> *root.
 * pg_reml_scalars_dev   : args8 = {lam, yPy, yPPy, yPPPy, trP, trPP, logdet_H, logdet_Wt_H_inv_W} ->
 *     out3 = {likelihood_restricted_lambda_overload (pyx:1813), likelihood_derivative1_..._overload (pyx:1656),
 *             likelihood_derivative2_..._overload (pyx:1675)} with n and c = ctot as the reference passes them. */
int pg_precompute_mat_dev(pg_ctx *ctx, int64_t n, int ctot, float lam, const float *d, const float *Wx, const float *y,
                          int full, float *P3, float *Q3, float *R3, float *vecs, float *scal);
int pg_newton_dev(pg_ctx *ctx, int64_t n, int ctot, float lam, float lam_min, float lam_max, const float *d,
                  const float *Wx, const float *y, float *root);
int pg_reml_scalars_dev(pg_ctx *ctx, int64_t n, int ctot, const float *args8, float *out3);
/* pg_ml_scalars_dev     : args7 = {lam, yPy, yPPy, yPPPy, sum h, sum h^2, logdet_H} -> out3 = {likelihood_lambda (pyx:1542),
 *     likelihood_derivative1_lambda (pyx:1567), likelihood_derivative2_lambda (pyx:1586)}: the ML scalars of the LRT (N2). */
int pg_ml_scalars_dev(pg_ctx *ctx, int64_t n, const float *args7, float *out3);

/* ---- Test hooks of the eigensolver's stages (tests/test_gpu_syevd.py, tools/bench_dgemm.py): not part of the drop-in
 * surface, exported so that each stage can be checked against host LAPACK on its own.
 * pgx_dgemm_dev : C = alpha op(A) B + beta C in fp64 on v_mfma_f64_16x16x4_f64 (row-major; transA: A is K x M)
 * pgx_sytrd_dev : Householder tridiagonalisation of the lower triangle of float32 K -> d, e, tau, reflectors (device)
 * pgx_stedc_dev : divide & conquer on a tridiagonal given on the host -> eigenvalues (host), eigenvectors Z (device) */
int pgx_dgemm_dev(pg_ctx *ctx, int transA, int64_t M, int64_t N, int64_t K, double alpha, const double *A, int64_t lda,
                  const double *B, int64_t ldb, double beta, double *C, int64_t ldc);
/* pgx_dgemm_ex_dev: every mode of that GEMM: flags bit 0 transA, bit 1 transB (B stored N x K), bit 2 lower triangle of C only,
 * bit 3 A symmetric (lower triangle + full diagonal tiles valid), bit 4 no split-K; kxorB: B's k index XOR-ed (multiple of 8) */
int pgx_dgemm_ex_dev(pg_ctx *ctx, int flags, int kxorB, int64_t M, int64_t N, int64_t K, double alpha, const double *A, int64_t lda,
                     const double *B, int64_t ldb, double beta, double *C, int64_t ldc);
/* pgx_ring_stamps: in-kernel time stamps one workgroup of the ring GEMM left when PG_DGEMM_TUNE has bit 3 set (diagnostics) */
int pgx_ring_stamps(long long *out64);
int pgx_sytrd_dev(pg_ctx *ctx, int64_t n, const float *K, double *d, double *e, double *tau, double *Vall);
int pgx_stedc_dev(pg_ctx *ctx, int64_t n, const double *d_host, const double *e_host, double *evals_host, double *Z_dev);
/* The two-stage tridiagonalisation of pg_syevd_dev (csrc/sb2.hip), one stage at a time (all matrices n x n fp64 row-major on the device):
 * pgx_sb2_stage1_dev : lower triangle of float32 K -> Aband (the band |i - j| <= 64 of the result is the band matrix Q1' K Q1);
 *                      Z, if given, is replaced by Q1 Z.  flags (host, 4 ints): [0] a panel needed the one-stage fallback.
 * pgx_sb2_stage2_dev : band |i - j| <= 64 of Aband (lower part read) -> tridiagonal d (n), e (n - 1) on the device by bulge chasing;
 *                      Z, if given, is replaced by Q2 Z.  flags: [1] a wait inside the bulge-chasing kernel expired. */
int pgx_sb2_stage1_dev(pg_ctx *ctx, int64_t n, const float *K, double *Aband, double *Z, int *flags);
int pgx_sb2_stage2_dev(pg_ctx *ctx, int64_t n, const double *Aband, double *d, double *e, double *Z, int *flags);
/* debugging aid: host-mapped memory (pg_host_alloc, >= 4 ints) in which the bulge-chasing kernel records (sweep, step, phase); NULL = off */
int pgx_sb2_set_debug(void *host_mapped);

#ifdef __cplusplus
}
#endif
#endif /* PYGEMMA_HIP_H */
