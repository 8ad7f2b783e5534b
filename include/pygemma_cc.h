/*
 * pygemma_cc.h — C ABI of the case/control unit (libpygemma_cc.so, csrc/case_control.hip): a library of its own beside
 * libpygemma_hip.so, which it needs (contexts and errors are that library's: every call takes its pg_ctx and reports through
 * pg_last_error()).  It is loaded when lmm.case_control is first called, not with the package: a process that never calls it runs
 * every other path from exactly the code and the device images it ran before.  Conventions as in pygemma_hip.h.
 */
#ifndef PYGEMMA_CC_H
#define PYGEMMA_CC_H
#include "pygemma_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- Per-SNP case/control tests on contingency tables (csrc/case_control.hip): what PLINK prints with --assoc, --model, --fisher and
 * --mh, every statistic a function of exact integer counts read from packed .bed records.  The samples fall into 2 S groups, (stratum
 * k, case) and (stratum k, control), S = 1..PG_CC_MAX_STRATA; a sample with status -1, or with a stratum outside 0..S-1, is in no group
 * and is counted nowhere.
 *   pg_cc_setup_dev  : status (n int8 on the device: 1 case, 0 control, anything else neither) and stratum (n int32 on the device, or NULL:
 *             everyone in stratum 0) -> work, pg_cc_work_bytes(n, S) device bytes on a 16-byte boundary (0 for a refused shape): the
 *             members of every group and one mask word per group and 16-sample .bed word, a subset of 0x55555555 with the bits of the
 *             samples >= n clear.
 *   pg_cc_pack_x_dev : an (n x pb) sample-major (snp_major = 0, ldX >= pb) or (pb x n) SNP-major (ldX >= n) block of dtype PG_DTYPE_* ->
 *             pb records in .bed coding at pitch ldb >= ceil(n/4): 0 -> 00, missing (NaN, +-Inf) -> 01, 1 -> 10, 2 -> 11, the pad calls of
 *             the last byte 00; bytes beyond ceil(n/4) of a row are not written.  hard (pb bytes) becomes 1, or 0 for a SNP that holds
 *             an observed value other than 0, 1, 2 in the element's own precision (the hard-call rule of pg_ld_encode_x_dev; such a
 *             value is packed as 01).  X, rec and hard do not overlap.
 *   pg_cc_count_dev  : pb records (code convention and count_a1 of pg_rotate_bed_dev; the pad bits after sample n - 1 are cleared by the
 *             masks, never read for what they hold) -> counts, pb x 8 int64 {case0, case1, case2, case_miss, ctrl0, ctrl1, ctrl2,
 *             ctrl_miss} pooled over the strata, and cmh, pb x 4 fp64 {u, v, sum a d / T, sum b c / T} of the Cochran-Mantel-Haenszel
 *             test over the strata's allelic 2 x 2 tables (a, b the counted and the other allele among the called cases, c, d among
 *             the called controls; row1 = a + b, col1 = a + c, T the table's total), added in stratum order 0..S-1:
 *               u += (double)(a T - row1 col1) / (double)T,   v += ((double)(row1 row2) (double)(col1 col2)) / ((double)(T T) (double)(T - 1)),
 *             a stratum without a called case or a called control adds nothing; all four NaN when the SNP has no called case or no
 *             called control.  With hard non-NULL a SNP whose hard byte is 0 has no call counted: its counts are 0.  No atomics: a row
 *             depends on its SNP and the groups alone.
 *   pg_cc_stats_dev  : p rows of counts (and of cmh, or NULL) -> stat, p x PG_CC_NSTAT fp64 {af_case, af_ctrl, or, chi2_allelic,
 *             chi2_trend, chi2_geno, chi2_dom, chi2_rec, p_fisher, chi2_cmh, or_mh}: allele frequencies and odds ratio a d / (b c) of
 *             the pooled allelic table (+inf when b c = 0 < a d, NaN when both are 0), the 1-df chi2 of the allelic table, the
 *             Cochran-Armitage trend test (weights 0, 1, 2), the 2-df chi2 of the 2 x 3 table (NaN when a genotype is unseen), the 1-df
 *             dominant (1 + 2 against 0) and recessive (2 against 0 + 1) tests, the two-sided Fisher exact test of the allelic table
 *             (hypergeometric terms from the mode outward in two sweeps, tail = the terms <= P(obs) (1 + 2^-30), at most 1; NaN with
 *             fisher = 0), chi2_cmh = u u / v (NaN when v = 0) and or_mh = sum a d / T / sum b c / T (NaN when the divisor is 0; both
 *             NaN without cmh).  A 2 x 2 chi2 is NaN when a margin is 0; every column is NaN when the row has no called case or no
 *             called control, or a count outside 0..2^30-1.  Each cross-difference is exact in int64 and converted once; the
 *             operation order is written at the head of csrc/case_control.hip.
 * PG_EINVAL for NULL pointers (but stratum, hard, cmh), n < 1, n >= 2^30, pb < 0, pb > 2^25, p >= 2^31, a work area off 16 bytes, a
 * sample-major block of 2^24 or more workgroups (ceil(n / 256) x ceil(pb / 256), ceil(pb / 128) for float64) or strides too small;
 * PG_ENOTSUP for S outside 1..PG_CC_MAX_STRATA or an unknown dtype: a refused call enqueues nothing.  pb = 0 and p = 0 are no-ops. */
#define PG_CC_MAX_STRATA 16
#define PG_CC_NSTAT 11
size_t pg_cc_work_bytes(int64_t n, int S);
int pg_cc_setup_dev(pg_ctx *ctx, int64_t n, int S, const signed char *status, const int *stratum, void *work);
int pg_cc_pack_x_dev(pg_ctx *ctx, int64_t n, int64_t pb, const void *X, int dtype, int64_t ldX, int snp_major, unsigned char *rec, int64_t ldb,
                     unsigned char *hard);
int pg_cc_count_dev(pg_ctx *ctx, int64_t n, int64_t pb, const unsigned char *rec, int64_t ldb, int count_a1, int S, const void *work,
                    const unsigned char *hard, int64_t *counts, double *cmh);
int pg_cc_stats_dev(pg_ctx *ctx, int64_t p, const int64_t *counts, const double *cmh, int fisher, double *stat);

#ifdef __cplusplus
}
#endif
#endif /* PYGEMMA_CC_H */
