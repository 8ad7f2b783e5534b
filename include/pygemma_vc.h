/*
 * pygemma_vc.h — C ABI of the variance-component unit (libpygemma_vc.so, csrc/vc.hip): a library of its own beside
 * libpygemma_hip.so, which it needs (contexts, errors and scratch are that library's: every call takes its pg_ctx and reports
 * through pg_last_error()).  It is loaded when lmm.reml or lmm.vc_kinship is first called, not with the package: a process that
 * never fits variance components runs the association path from exactly the code and the device images it ran before.
 * Conventions as in pygemma_hip.h.
 */
#ifndef PYGEMMA_VC_H
#define PYGEMMA_VC_H
#include "pygemma_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- Variance components for several kinship matrices (lmm.reml; csrc/vc.hip): dense fp64 linear algebra on
 * V = sum_i s_i K_i + s_k I.  Every matrix is row-major on the device; of a symmetric or triangular matrix only the LOWER triangle
 * (with the diagonal) is read or written: the strict upper triangle and the pad of a pitched row stay as they were, bit for bit.
 * K, k_is_f64, ldk and s are HOST arrays (k <= 64 entries; s: k + 1, the identity's coefficient last); K[i] is a device pointer to a
 * float32 (k_is_f64[i] = 0) or float64 matrix of row stride ldk[i].
 * pg_vc_combine_dev   : V = sum_i s_i K_i + s_k I, the terms added in this order.
 * pg_potrf_dev        : A = L L' in place, blocked (64-column panels, the trailing update on the fp64 matrix pipe).  *info_dev
 *                       (device) = 0, or 1 + the index of the first pivot that is not a positive finite number; the call then still
 *                       runs to its end inside A and returns PG_OK — the factor is unusable, the host decides.
 * pg_potrf_logdet_dev : *out (device) = 2 sum_j log L[j][j], one kernel.
 * pg_potri_dev        : Ainv = (L L')^-1 from the factor; work: pg_potri_work_bytes(n) bytes, 16-byte aligned.
 * pg_sym_trdot_dev    : *out (device) = tr(A B) = sum_i a_ii b_ii + 2 sum_{i>j} a_ij b_ij; B float32 or float64.  No atomics:
 *                       the same bits on every run.
 * pg_symv_dev         : Y (n x m, row stride ldy) = A X for symmetric A (float32 or float64) and X (n x m, row stride ldx), m <= 32.
 * pg_vc_eval_dev      : one evaluation of the REML objective at sigma (HOST, k + 1) for Wy = [W y] (device, n x (c + 1), row stride
 *                       c + 1; c <= 30 < n): chains the above on the context's stream in work (device, pg_vc_work_bytes(n, k) bytes,
 *                       256-byte aligned: three n x n matrices and a few panels), waits, and fills out (HOST, pg_vc_out_len(k, c)
 *                       doubles; kk = k + 1, K_k = I):
 *                         [0] logL = -1/2 (log|V| + log|W'V^-1 W| + y'Py)   [1] log|V|   [2] log|W'V^-1 W|   [3] y'Py
 *                         score[kk]: -1/2 (tr(P K_i) - y'P K_i P y)         AI[kk][kk]: 1/2 y'P K_i P K_j P y
 *                         beta[c] (GLS)    (W'V^-1 W)^-1 [c][c]             tr(P K_i)[kk]     y'P K_i P y[kk]
 *                       Py (device, n; may be NULL) receives P y.  *info (HOST) = pg_potrf_dev's: when it is not 0, out holds NaN
 *                       and the call returns PG_OK.  Nothing of size n^2 leaves the device. */
int pg_vc_combine_dev(pg_ctx *ctx, int64_t n, int k, const void *const *K, const int *k_is_f64, const int64_t *ldk, const double *s,
                      double *V, int64_t ldv);
int pg_potrf_dev(pg_ctx *ctx, int64_t n, double *A, int64_t lda, int *info_dev);
int pg_potrf_logdet_dev(pg_ctx *ctx, int64_t n, const double *A, int64_t lda, double *out);
size_t pg_potri_work_bytes(int64_t n);
int pg_potri_dev(pg_ctx *ctx, int64_t n, const double *L, int64_t ldl, double *Ainv, int64_t ldi, double *work);
int pg_sym_trdot_dev(pg_ctx *ctx, int64_t n, const double *A, int64_t lda, const void *B, int b_is_f64, int64_t ldb, double *out);
int pg_symv_dev(pg_ctx *ctx, int64_t n, const void *A, int a_is_f64, int64_t lda, int m, const double *X, int64_t ldx, double *Y,
                int64_t ldy);
size_t pg_vc_work_bytes(int64_t n, int k);
int pg_vc_out_len(int k, int c);
int pg_vc_eval_dev(pg_ctx *ctx, int64_t n, int k, int c, const void *const *K, const int *k_is_f64, const int64_t *ldk,
                   const double *sigma, const double *Wy, void *work, double *out, double *Py, int *info);

#ifdef __cplusplus
}
#endif
#endif /* PYGEMMA_VC_H */
