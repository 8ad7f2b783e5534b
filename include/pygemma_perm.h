/*
 * pygemma_perm.h — C ABI of the permutation unit (libpygemma_perm.so, csrc/perm.hip): a library of its own beside
 * libpygemma_hip.so, which it needs (contexts and errors are that library's: every call takes its pg_ctx and reports through
 * pg_last_error()).  It is loaded when lmm.case_control_perm is first called, not with the package: a process that never calls it
 * runs every other path from exactly the code and the device images it ran before.  Conventions as in pygemma_hip.h.
 */
#ifndef PYGEMMA_PERM_H
#define PYGEMMA_PERM_H
#include "pygemma_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- max(T) permutation tests of a case/control trait on the int8 matrix pipe (csrc/perm.hip): what PLINK computes with --assoc
 * --mperm B and --model trend --mperm B.  Samples carry a study flag s in {0, 1} (0: no status or no stratum); a labelling l is a 0/1
 * vector with l <= s: the samples it calls cases.  For a hard-call SNP with x, m as the LD image holds them (csrc/ld.hip) the per-SNP
 * totals over the study samples are At = sum x s, Nc = sum m s, Q = sum x^2 s, and per labelling a = sum x l, R = sum m l: int32 sums,
 * everything derived from them exact in int64.  The statistic of (SNP, labelling), in fp64 with one rounding per operation
 * ((double)(...) is the one conversion of an exact int64), in the operation order of csrc/case_control.hip:
 *   test PG_PERM_ALLELIC: the table a, b = 2 R - a / c = At - a, d = 2 (Nc - R) - c with margins r1 = a + b, r2 = c + d, c1 = a + c,
 *                         c2 = b + d, T = r1 + r2:  chi2 = ((double)T * (D * D)) / ((double)(r1 r2) * (double)(c1 c2)), D = (double)(a d - b c);
 *                         NaN when a margin is 0
 *   test PG_PERM_TREND  : N = Nc, S' = Nc - R, U = (double)(N a - R At), V = (double)(N Q - At^2):
 *                         chi2 = ((double)N * (U * U)) / ((double)(R S') * V);  NaN when V = 0
 *   both NaN when R = 0 or R = Nc.
 * With l the observed status the value is lmm.case_control's chi2_allelic / chi2_trend, bit for bit.
 *   Label rows : labellings, and the study flags s, are rows of int8 0/1 on the device at pitch ldk = ceil(n / 128) * 128, zero past
 *             sample n and zero where s = 0; the host writes them, they are uploaded as they are.  pg_perm_label_bytes(n, nb): the
 *             bytes of nb rows (0 for a refused shape).  The tile reads no row past the last (a row past the window repeats it).
 *   pg_perm_label_counts_dev : counts[k] = sum of row k of `labels`, k < nb: the cases of every labelling (int32).
 *   pg_perm_totals_dev : SNPs [from, from + count) of an LD image for pe SNPs (pg_ld_image_bytes, pg_ld_encode_*_dev) and the row
 *             `study` -> totals[k] = {At, Nc, Q, flag} of SNP from + k (int32 x 4, on 16 bytes); flag bit 0: a study sample is
 *             uncalled (Nc < sum s), bit 1: the SNP is not hard-call (its planes are zero: Nc = 0).  A bandwidth kernel: 3 n bytes in.
 *   pg_perm_block_dev : SNPs a0 + ia, ia < na, of the LD image with totals[ia] (as pg_perm_totals_dev wrote them from `a0`), against
 *             the labellings b0 + ib, ib < nb, of `labels` with lab_counts[b0 + ib].  Three outputs, each may be NULL:
 *               dense    dense[ia * ldo + ib] = the statistic (fp64, NaN included); nothing outside the na x nb window is written
 *               n_ge     with obs (na fp64, required then): n_ge[ia] += #{ib: statistic >= obs[ia]} (uint32; a NaN on either side
 *                        never counts), one integer atomic add per SNP and workgroup
 *               max_null max_null[ib] = max(max_null[ib], bits of the largest non-NaN statistic over ia) as the uint64 pattern of
 *                        a non-negative double under an integer atomic max; the caller zeroes it before the first call
 *             Both reductions are order-independent integers: the result does not depend on tiling, on how the SNPs or the
 *             labellings are split over calls, or on the run.  A workgroup owns 256 SNPs x 256 labellings on the int8 pair tile
 *             (csrc/i8_pair.hpp): one product (256 SNPs x plane x, R = the labelling's case count) when every SNP's flag is 0, else
 *             two of 128 SNPs x {x, m}; the same integers either way.  PG_PERM_PLANES=1 in the environment (read at each call) sends
 *             every tile down the second path: tests and A/B timing.
 * PG_EINVAL for NULL pointers (but the outputs of pg_perm_block_dev; obs with n_ge), an image, labels or totals off 16 bytes, dense,
 * obs or max_null off 8, n < 1, n >= 2^28 (every sum fits int32), negative counts, windows outside the image (from + count > pe,
 * a0 + na > pe), nb >= 2^31, ldo < nb; PG_ENOTSUP for an unknown test: a refused call enqueues nothing.  count = 0, na = 0 and nb = 0
 * are no-ops. */
#define PG_PERM_ALLELIC 0
#define PG_PERM_TREND 1
size_t pg_perm_label_bytes(int64_t n, int64_t nb);
int pg_perm_label_counts_dev(pg_ctx *ctx, int64_t n, const signed char *labels, int64_t nb, int32_t *counts);
int pg_perm_totals_dev(pg_ctx *ctx, int64_t n, const void *image, int64_t pe, int64_t from, int64_t count, const signed char *study, int32_t *totals);
int pg_perm_block_dev(pg_ctx *ctx, int64_t n, const void *image, int64_t pe, int64_t a0, int64_t na, const int32_t *totals, const signed char *labels,
                      const int32_t *lab_counts, int64_t b0, int64_t nb, int test, double *dense, int64_t ldo, const double *obs, uint32_t *n_ge,
                      uint64_t *max_null);

#ifdef __cplusplus
}
#endif
#endif /* PYGEMMA_PERM_H */
