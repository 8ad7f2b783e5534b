// assoc.hip — the per-SNP LMM association operator on gfx950 (MI355X).
//
// Replaces, per SNP g, everything under calculate() in the reference (lmm/lmm.py:461-495):
//   calc_lambda_restricted (pygemma_model.pyx:64-194) -> precompute_mat (:880-1053), newton (:1349-1416),
//   scipy.optimize.brentq (:176-182), the *_overload scalars (:1656-1698, :1813-1830),
//   calc_beta_vg_ve_restricted_overload (:1514-1537), F = (beta/se)^2 and scipy.stats.f.sf (lmm.py:471,482).
//
// Mapping: ONE 64-lane wavefront per SNP.  Lane l owns elements i = l, l+64, ... of the n-vectors
// (coalesced reads of the SNP-major genotype row and of the packed fixed rows {d_i, w_i*, y_i});
// every Gram entry is a per-lane fma chain followed by a 64-lane xor-butterfly (strides 1,2,..,32),
// so all lanes hold the same f64 sums and run the O(m^3) sweeps / Brent / Newton logic uniformly.
// Precision follows SURVEY.md Appendix A: h = 1/(lam*d+1) in three separately rounded f32 ops,
// Grams and sweeps in f64, every exported quadratic form rounded to f32, f32 lambda iterates.
// The arithmetic order is mirrored exactly by oracle/pygemma_oracle.c (order=1) so that GPU and
// oracle agree bit-for-bit; compile with -ffp-contract=off (every fma below is explicit).
//
// What is shared between SNPs is hoisted: the decade lambdas 10^-5..10^5 are the same for every SNP,
// so h tables, the SNP-independent Gram entries (W,y block), trace terms and log|H| at those 11
// lambdas are computed once (setup kernel); per SNP the scan only accumulates the 2(c+2) entries
// that involve x, and of the sweeps at those lambdas the c covariate pivots on the (W,y) block are the
// setup kernel's too (the decade table): a SNP updates its x row only, several lambdas side by side on
// the lanes (decade_lanes).  Evaluations at SNP-specific lambdas (Brent, Newton, final) need the full Grams.
// The scan itself reads its SNP-independent operands from a table of its own, one packed row per element (the scan rows,
// assoc_srow_layout: w, y and h at the 11 decade lambdas, copied from the fixed rows and the h table once per call), a few 16-byte
// loads at immediate offsets from one 32-bit row offset, through a two-slot ring whose loads are pinned a whole element ahead of
// their use.  The Gram passes, the multi-phenotype scan and the GxE scan read the fixed rows and the h table as before, and so does
// the scan at c = 19..22, which measured slower on the rows (assoc_scan_packed).
#include "common.hpp"

#include <cmath>

namespace pg {

constexpr int NLAM = 11;  // decade lambdas 10^-5 .. 10^5
#ifndef PG_ASSOC_WPB
#define PG_ASSOC_WPB 2    // wavefronts (= SNPs) per workgroup
#endif
// Two wavefronts per workgroup (r3; it was 4).  A SNP whose Newton iteration runs to the reference's 100-step cap (pyx:1411) keeps its
// whole workgroup's slots and LDS until it is done: in a 4-SNP workgroup three finished wavefronts idled behind each straggler.
// Measured on one box, same inputs (weak-signal phenotype, 43 Newton evaluations per SNP on average, max 106 | default phenotype,
// 6 evaluations for every SNP):   4 per workgroup 0.381 of the fp64 roof | 33.75 ms;   2: 0.464 | 33.8 ms;   1: 0.469 | 34.16 ms.
// A persistent work queue inside the kernel (wavefronts pulling SNP indices from an atomic counter) reaches 0.479 on the weak-signal
// phenotype too, but its loop costs registers (VGPR spills 58 -> 90 at c = 5) and 9 % on the default one: the hardware dispatcher
// refilling small workgroups does the same job for free.
constexpr int WPB = PG_ASSOC_WPB;
#define PG_MINV 1e-35f    // pygemma_model.pyx:39
// tuning knobs (overridable with -D for A/B builds)
#ifndef PG_FUSE_PQ_MAX
#define PG_FUSE_PQ_MAX 36   // fuse the P and Q powers in one pass while (c+2)(c+3)/2 <= this
#endif
#ifndef PG_FUSE_PQR_MAX
#define PG_FUSE_PQR_MAX 28  // fuse all three powers (Newton evaluations)
#endif
#ifndef PG_PFD
#define PG_PFD 2            // prefetch ring depth
#endif
#ifndef PG_CHUNK_MIN_NP
#define PG_CHUNK_MIN_NP 80   // more Gram entries than this (c >= 11): slot-chunked passes (measured: c=10 is still faster un-chunked)
#endif
#ifndef PG_SCAN_NV
#define PG_SCAN_NV 96        // decade-scan accumulators per pass (x-entries of as many lambdas as fit)
#endif
#ifndef PG_SCAN_PFD
#define PG_SCAN_PFD 2        // prefetch ring depth of the decade scan (its slots are the packed scan rows, see assoc_srow_layout)
#endif
#ifndef PG_SWEEP_LDS_MIN_SLOTS
#define PG_SWEEP_LDS_MIN_SLOTS 3   // lanes owning this many Gram entries or more exchange the sweeps' pivot column through LDS
#endif
#ifndef PG_PHENO_SPLIT_XE
#define PG_PHENO_SPLIT_XE 26   // multi-phenotype scan: rows of more entries (c + 1 + chunk width) accumulate P and Q in separate passes
#endif
#ifndef PG_WAVES
#define PG_WAVES 2          // waves per SIMD the register allocation is held to
#endif
// Gram powers the result does not need (each its own switch, so that a stage can be timed and dropped alone):
#ifndef PG_ASSOC_FINAL_P
#define PG_ASSOC_FINAL_P 1        // the evaluation at the root feeds logL, beta and se only: P alone, no Q
#endif
#ifndef PG_ASSOC_NEWTON_REUSE
#define PG_ASSOC_NEWTON_REUSE 1   // Newton's first evaluation takes P, Q and t1 from Brent when it starts at a lambda Brent evaluated: R alone
#endif
#ifndef PG_REUSE_MAX_SLOTS
#define PG_REUSE_MAX_SLOTS 4      // ... while a lane owns at most this many Gram entries per power (c <= 20): 9 KiB of LDS per wave at 4
#endif
// Work repeated for nothing:
#ifndef PG_ASSOC_DECADE_HOIST
#define PG_ASSOC_DECADE_HOIST 1   // the covariate pivots of the decade sweeps once per call (setup_tabs_kernel), the x rows of the decades side by side on the lanes
#endif

// The decade table, per lambda — ONE definition for setup_tabs_kernel, decade_lanes and the host's allocation: c (c + 2) records of 4
// doubles {ia, ba2, P(r_k, q), Q(r_k, q)} [step q][x-row entry k], then 8 doubles {trP, ld, P(y,y), Q(y,y) after the c covariate
// pivots, t1, log|H|, lambda, 0}.
__host__ __device__ constexpr size_t assoc_dtab_doubles(int c) { return (size_t)c * (c + 2) * 4 + 8; }

// The scan rows — ONE definition for build_scan_rows_kernel, scan_accumulate and the host's allocation.  The decade scan reads, per
// element, the c + 1 columns w_0..w_{c-1}, y and h at the pass's decade lambdas, and nothing else (not d): srow[npad][rowf] packs them
// as [w_0..w_{c-1}, y | zeros up to hoff | h_0..h_10 | zeros up to rowf], rows i >= n all zero.  A pass over the lambdas
// [t0, t0 + gg) loads the 16-byte vectors of the row that hold any of its floats (assoc_srow_mask), each at an immediate offset from
// the one row address; hoff in [c + 1, c + 4] is the one at which the passes of assoc_scan_lams(c) lambdas read the fewest vectors
// in all (c = 5: hoff 6, rows of 20 floats, 3 vectors for the lambdas 0..5 and 4 for 6..10, where htab and fixed took 8 and 7 loads).
// Accumulators per decade-scan pass — ONE rule for the three scans (2 VGPRs each; measured: PG_SCAN_NV = 96 is best for c >= 3, 64
// for c <= 2 where one more lambda per pass starts to spill).  `wald`: assoc_kernel's own scan (scan_all) — at c = 14 it takes 64, two
// lambdas per pass: with 96 beside rows of 16 columns its loop spills and the ring does not hold (measured: 9.5 % faster at 64, at
// n = 4 000 and n = 10 000).  The multi-phenotype and GxE scans (!wald) budget their lambdas from this number by their own formulas.
__host__ __device__ constexpr int assoc_scan_nv(int c, bool wald)
{
    return (PG_SCAN_NV > 64 && (c + 2 <= 4 || (wald && c == 14))) ? 64 : PG_SCAN_NV;
}
// Which instantiations of scan_all read the scan rows.  c = 19..22 (84 to 96 values in 96 accumulators beside rows of 21 to 24 columns)
// stay on htab and fixed (scan_accumulate_tabs): c = 20..22 spill inside the scan loop whichever way they load, and the spill reloads
// drain the ring; c = 19 does not spill there but measured 8 % slower on the rows, c = 20 13 %.
__host__ __device__ constexpr bool assoc_scan_packed(int c) { return c < 19 || c > 22; }
__host__ __device__ constexpr int assoc_scan_lams(int c)   // decade lambdas per pass of scan_all (Shape<C>::G)
{
    const int g = assoc_scan_nv(c, true) / (2 * (c + 2));
    return g < 1 ? 1 : (g > NLAM ? NLAM : g);
}
__host__ __device__ constexpr unsigned assoc_srow_mask(int c, int hoff, int t0, int gg)
{
    unsigned m = 0;
    for (int f = 0; f <= c; f++) m |= 1u << (f / 4);
    for (int t = t0; t < t0 + gg; t++) m |= 1u << ((hoff + t) / 4);
    return m;
}
struct SrowLayout { int hoff, rowf; };   // floats: h_t at hoff + t, row stride rowf (a multiple of 4: rows are 16-byte aligned)
__host__ __device__ constexpr SrowLayout assoc_srow_layout(int c)
{
    const int G = assoc_scan_lams(c);
    int best = 0, best_vecs = 1 << 30;
    for (int hoff = c + 1; hoff <= c + 4; hoff++) {
        int vecs = 0;
        for (int t0 = 0; t0 < NLAM; t0 += G)
            for (unsigned m = assoc_srow_mask(c, hoff, t0, (NLAM - t0) < G ? (NLAM - t0) : G); m; m &= m - 1) vecs++;
        if (vecs < best_vecs) { best_vecs = vecs; best = hoff; }
    }
    return SrowLayout{best, (best + NLAM + 3) / 4 * 4};
}

// Per-wave dynamic LDS of assoc_kernel — ONE definition for the kernel's carve-up and the host's launch size, so the two
// cannot drift apart: [piv: 3 M doubles when the sweeps exchange their pivot column through LDS] | [sav: Brent's last two
// evaluations, every lane's P[slots], Q[slots] and t1, where Newton reuses them (sav_slots = 0: nowhere)] | xent[NLAM][2M] doubles |
// evs[NLAM] | d1s[NLAM] | lls[NLAM] | vals[n_vals], rounded up to 16 bytes.
__host__ __device__ constexpr size_t assoc_sav_doubles(int sav_slots) { return sav_slots ? (size_t)2 * (2 * sav_slots + 1) * 64 : 0; }
__host__ __device__ constexpr size_t assoc_per_wave_bytes(int M, bool sweep_lds, int sav_slots, size_t evalout_bytes, int n_vals)
{
    return (((sweep_lds ? (size_t)3 * M * 8 : 0) + assoc_sav_doubles(sav_slots) * 8 + (size_t)NLAM * 2 * M * 8 + NLAM * evalout_bytes + 2 * NLAM * 4 +
             (size_t)n_vals * 4) + 15) & ~(size_t)15;
}

struct AssocParams {
    int n, npad, c, niter, nu, grid, rowf;  // nu = n - (c+1); rowf = floats per fixed row (multiple of 4)
    long long p, ldx;
    const float *xr;
    const float *fixed;    // [npad][rowf]: d, w_0..w_{c-1}, y, zero pad; rows >= n all zero
    float *htab;           // [NLAM][npad]   (0 for i >= n)
    float *srow;           // [npad][assoc_srow_layout(c).rowf]  the decade scan's rows: w, y and h at the 11 decade lambdas, copied from fixed
                           // and htab (build_scan_rows_kernel); not built where scan_all does not read it (assoc_scan_packed(c)), 0 for the
                           // callers whose kernels do not run scan_all
    double *fixg;          // [NLAM][2][NP]  level-0 P,Q over all columns with x := 0
    double *t1tab;         // [NLAM]
    float *ldHtab;         // [NLAM]
    double *dtab;          // [NLAM][assoc_dtab_doubles(c)]  the decade table (0: not built; the callers whose kernels sweep every decade themselves)
    float lam11[NLAM];
    float logl_c;          // f32(f32(.5nu*ln(.5nu/pi)) - .5nu)   (pyx:1821-1822)
    const int *leaf, *node, *level, *chunk;
    int n_leaf, n_level, n_chunk, n_vals;
    float *beta, *se, *tau, *lam;
    double *F;
    unsigned long long *stats;
    unsigned *trace;       // optional: per SNP, fast evaluations | full (Newton) evaluations << 16 (pg_assoc_set_eval_trace)
    unsigned long long *passes;   // optional: passes over n that produced P | Q | R, Newton starts on Brent's P and Q (pg_assoc_set_pass_stats)
    // N2 (LRT instantiations only): ML lambda and log-likelihood per SNP; ml_c = f32(f32((n/2) ln(n/2pi)) - (n/2)) (pyx:1552-1554)
    int lrt, nhalf;
    float ml_c;
    float *lalt, *lamalt;
    // pg_assoc_pheno_dev (PHENO instantiations only): the x-entries of the decade scan come from scan_pheno_kernel's buffer
    // xbuf [p][NLAM][2][xe] (xe = c + 1 shared entries + the chunk's padded phenotype count); this launch's phenotype is column xcol
    const double *xbuf;
    int xe, xcol;
};

// quadratic forms of one evaluation; sh, shh = the level-0 (un-projected) traces sum h, sum h^2 the ML functions use
struct EvalOut { float yPy, yPPy, yPPPy, trP, trPP, ld, Pxx_c, Pyx_c, sh, shh; };

// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float hinv_f32(float lam, float d)
{   // pyx:903  1.0/(lam*eigenVals + 1.0) on float32 arrays: three separately rounded f32 operations.
    // The reciprocal: v_rcp_f32 plus ONE Newton step in fma form is the correctly rounded 1/x for every normal x whose
    // reciprocal is normal (checked exhaustively against __fdiv_rn over all 2^23 mantissas, tools/rcpcheck.hip) — 3
    // instructions instead of the 11 of the IEEE division expansion; anything else (x >= 2^126, inf, NaN; x >= 1 here)
    // takes the full division.
    const float x = __fadd_rn(__fmul_rn(lam, d), 1.0f);
    const float r0 = __builtin_amdgcn_rcpf(x);
    float r = __builtin_fmaf(__builtin_fmaf(-x, r0, 1.0f), r0, r0);
    if (__builtin_expect(!(x < 0x1p126f), 0)) r = __fdiv_rn(1.0f, x);
    return r;
}

// numpy's SIMD float32 log (see oracle/pygemma_oracle.c: orc_np_logf) — bit-exact restatement
__device__ __forceinline__ float np_logf(float x)
{
    const float p1 = 9.999999999999998702752e-01f, p2 = 2.112677543073053063722e+00f,
                p3 = 1.480000633576506585156e+00f, p4 = 3.808837741388407920751e-01f,
                p5 = 2.589979117907922693523e-02f;
    const float q1 = 2.612677543073109236779e+00f, q2 = 2.453006071784736363091e+00f,
                q3 = 9.864942958519418960339e-01f, q4 = 1.546476374983906719538e-01f,
                q5 = 5.875095403124574342950e-03f;
    // anything but a positive finite argument (an eigenvalue handed over as inf / NaN / negative): numpy's special values
    if (__builtin_expect(!(x > 0.0f) || x == INFINITY, 0)) return (x != x) ? x : (x < 0.0f ? NAN : (x == 0.0f ? -INFINITY : x));
    unsigned u = __float_as_uint(x);
    int e = (int)((u >> 23) & 0xff) - 126;
    float m = __uint_as_float((u & 0x007fffffu) | 0x3f000000u);
    float ef = (float)e;
    if (m <= 0.70710678118f) { m = __fadd_rn(m, m); ef = __fsub_rn(ef, 1.0f); }
    float t = __fsub_rn(m, 1.0f);
    float den = fmaf(q5, t, q4);
    den = fmaf(den, t, q3); den = fmaf(den, t, q2); den = fmaf(den, t, q1); den = fmaf(den, t, 1.0f);
    float num = fmaf(p5, t, p4);
    num = fmaf(num, t, p3); num = fmaf(num, t, p2); num = fmaf(num, t, p1); num = fmaf(num, t, 0.0f);
    float poly = __fdiv_rn(num, den);
    return fmaf(ef, 0.693147180559945309417232121458176568f, poly);
}

__device__ __forceinline__ double bfly(double v)
{
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// log|H| = float(np.log(lam*eigenVals + 1.0).sum())  (pyx:972): numpy's float32 pairwise sum
// (8-accumulator leaves of <= 128 elements, binary recursion, sequential across 8192-element
// chunks) reproduced with the host-built plan: 8 lanes per leaf, tree levels in parallel.
// vals: per-wave LDS scratch of n_vals floats.  All lanes return the same value.
__device__ float device_logdet_H(const AssocParams &pr, float lam, int lane, float *vals)
{
    const int sub = lane & 7, grp = lane >> 3;
    auto elem = [&](int i) -> float {
        float d = pr.fixed[(size_t)i * pr.rowf];
        return np_logf(__fadd_rn(__fmul_rn(lam, d), 1.0f));
    };
    for (int l0 = 0; l0 < pr.n_leaf; l0 += 8) {
        const int lf = l0 + grp;
        int start = 0, len = 0;
        if (lf < pr.n_leaf) { start = pr.leaf[2 * lf]; len = pr.leaf[2 * lf + 1]; }
        float res = 0.0f;
        if (len >= 8) {
            const int body = len - (len & 7);
            float r = elem(start + sub);
            for (int i = 8; i < body; i += 8) r = __fadd_rn(r, elem(start + i + sub));
            // ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) : xor butterfly inside the 8-lane group
            r = __fadd_rn(r, __shfl_xor(r, 1, 64));
            r = __fadd_rn(r, __shfl_xor(r, 2, 64));
            r = __fadd_rn(r, __shfl_xor(r, 4, 64));
            res = r;
            for (int i = body; i < len; i++) res = __fadd_rn(res, elem(start + i));
        } else {
            // the shuffles above must be executed by whole groups only; groups are uniform in `len`
            for (int i = 0; i < len; i++) res = __fadd_rn(res, elem(start + i));
        }
        if (lf < pr.n_leaf && sub == 0) vals[lf] = res;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int h = 0; h < pr.n_level; h++) {
        const int b = pr.level[h], e = pr.level[h + 1];
        for (int k = b + lane; k < e; k += 64) {
            float a = vals[pr.node[2 * k]], c = vals[pr.node[2 * k + 1]];
            vals[pr.n_leaf + k] = __fadd_rn(a, c);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    float tot = vals[pr.chunk[0]];
    for (int k = 1; k < pr.n_chunk; k++) tot = __fadd_rn(tot, vals[pr.chunk[k]]);
    return tot;
}

// ------------------------------------------------------------------------------------------------
// scalar REML functions — same statements, same widths as the C Cython generates
__device__ __forceinline__ float logl_f(const AssocParams &pr, float yPy, float ldH, float ld)
{   // pyx:1813-1830 (first two statements folded into pr.logl_c on the host; logdet_Wt_W = 0.0)
    float r = pr.logl_c;
    r = (float)((double)r + (0.5 * (double)0.0f));
    r = (float)((double)r - (0.5 * (double)ldH));
    r = (float)((double)r - (0.5 * (double)ld));
    r = (float)((double)r - ((0.5 * (double)pr.nu) * log((double)yPy)));
    return r;
}
__device__ __forceinline__ float d1_f(const AssocParams &pr, float lam, float yPy, float yPPy, float trP)
{   // pyx:1656-1669
    float yT = (PG_MINV > yPy) ? PG_MINV : yPy;
    float nc_tr = __fsub_rn((float)pr.nu, trP);
    float r = (float)(-0.5 * (double)__fdiv_rn(nc_tr, lam));
    float t = (0.0f > yPPy) ? 0.0f : yPPy;
    float g = __fdiv_rn(__fsub_rn(yT, t), lam);
    r = (float)((double)r + ((0.5 * (double)pr.nu) * (double)g) / (double)yT);
    return r;
}
__device__ __forceinline__ float d2_f(const AssocParams &pr, float lam, float yPy, float yPPy, float yPPPy,
                                      float trP, float trPP)
{   // pyx:1675-1698
    float a = (PG_MINV > yPy) ? PG_MINV : yPy;
    float b = (PG_MINV > yPPy) ? PG_MINV : yPPy;
    float e = (PG_MINV > yPPPy) ? PG_MINV : yPPPy;
    double lam2 = (double)lam * (double)lam;           // pow(lam, 2.0): exact product of two f32
    float ae = __fadd_rn(a, e);
    float G2 = (float)(((double)ae - 2.0 * (double)b) / lam2);
    float G1 = __fdiv_rn(__fsub_rn(a, b), lam);
    float nct = __fadd_rn((float)pr.nu, trPP);
    float r = (float)((0.5 * ((double)nct - 2.0 * (double)trP)) / lam2);
    float G2a = __fmul_rn(G2, a);
    r = (float)((double)r - ((double)pr.nu * ((double)G2a - (0.5 * (double)G1) * (double)G1)) / ((double)a * (double)a));
    return r;
}

// N2: the ML (non-restricted) scalars — likelihood_lambda pyx:1542-1562, likelihood_derivative1_lambda pyx:1567-1581,
// likelihood_derivative2_lambda pyx:1586-1603 — same statements and widths as oracle orc_ml_logl / orc_ml_d1 / orc_ml_d2
// (the reference takes the quadratic forms from float32 NumPy helpers; here they come from the sweeps: tolerance parity,
// see oracle/pygemma_oracle.c).
__device__ __forceinline__ float ml_logl_f(const AssocParams &pr, float yPy, float ldH)
{
    float r = pr.ml_c;                                                       // pyx:1552-1554 folded on the host
    r = __fsub_rn(r, __fmul_rn(0.5f, ldH));                                  // pyx:1556
    const float t = (PG_MINV > yPy) ? PG_MINV : yPy;
    r = (float)((double)r - (double)pr.nhalf * log((double)t));              // pyx:1558
    return r;
}
__device__ __forceinline__ float ml_d1_f(const AssocParams &pr, float lam, float yPy, float yPPy, float sh)
{
    float r = __fmul_rn(-0.5f, __fdiv_rn(__fsub_rn((float)pr.n, sh), lam));  // pyx:1574
    const float num = (PG_MINV > yPPy) ? PG_MINV : yPPy, den = (PG_MINV > yPy) ? PG_MINV : yPy;
    r = (float)((double)r + ((double)pr.nhalf * (1.0 - (double)__fdiv_rn(num, den))) / (double)lam);   // pyx:1579
    return r;
}
__device__ __forceinline__ float ml_d2_f(const AssocParams &pr, float lam, float yPy, float yPPy, float yPPPy, float sh, float shh)
{
    const float a = (PG_MINV > yPy) ? PG_MINV : yPy, b = (PG_MINV > yPPy) ? PG_MINV : yPPy, e = (PG_MINV > yPPPy) ? PG_MINV : yPPPy;
    const float G2 = (float)(((double)__fadd_rn(a, e) - 2.0 * (double)b) / (double)__fmul_rn(lam, lam));   // pyx:1597
    const float G1 = __fdiv_rn(__fsub_rn(a, b), lam);                                                    // pyx:1598
    const float t = __fmul_rn(0.5f, __fsub_rn(__fadd_rn((float)pr.n, shh), __fmul_rn(2.0f, sh)));        // pyx:1600
    float r = (float)((double)t / ((double)lam * (double)lam));
    r = (float)((double)r - ((0.5 * (double)pr.n) * ((2.0 * (double)G2) - (double)__fdiv_rn(__fmul_rn(G1, G1), a))) / (double)a);   // pyx:1601
    return r;
}

// ------------------------------------------------------------------------------------------------
template <int C> struct Shape {
    static constexpr int M = C + 2;             // columns of W* = [W | x | y]
    static constexpr int NP = M * (M + 1) / 2;  // lower-triangle entries
    static constexpr int SLOTS = (NP + 63) / 64;               // Gram entries owned per lane
    static constexpr int NV0 = NP < 64 ? NP : 64, NV1 = NP > 64 ? NP - 64 : 0;
    // entries of slot sl: [64 sl, 64 sl + slot_nv(sl)).  CHUNKED: one slot and one power per pass over n (64 accumulators),
    // which fits 2 waves/SIMD at any c; below PG_CHUNK_MIN_NP all entries of one or more powers share a pass.
    static constexpr int slot_nv(int sl) { return (NP - 64 * sl) < 64 ? (NP - 64 * sl) : 64; }
    static constexpr bool CHUNKED = NP > PG_CHUNK_MIN_NP;
    static constexpr bool SWEEP_LDS = SLOTS >= PG_SWEEP_LDS_MIN_SLOTS;   // pivot column of the sweeps through per-wave LDS (3 M doubles)
    // scans: the per-pass accumulator budget (assoc_scan_nv; two reduce-scatters of <= 64 and <= 32 values).  G: decade lambdas per
    // pass of assoc_kernel's scan (scan_all); SCAN_NV: the budget the multi-phenotype and GxE scans derive their own lambda counts from
    static constexpr int SCAN_NV = assoc_scan_nv(C, false);
    static constexpr int G = assoc_scan_lams(C);
    static constexpr bool SCAN_PACKED = assoc_scan_packed(C);   // scan_all reads the scan rows (else htab and fixed)
    // powers accumulated per pass over n: fused while the accumulators fit the register budget of 2 waves/SIMD
    static constexpr bool FUSE_PQ = NP <= PG_FUSE_PQ_MAX, FUSE_PQR = NP <= PG_FUSE_PQR_MAX;
    // Newton's first evaluation on Brent's P and Q, kept in the wave's LDS (2 SLOTS + 1 doubles per lane and evaluation): up to
    // PG_REUSE_MAX_SLOTS, beyond which the two kept evaluations would cost the 8 waves of a CU more than half of its LDS
    static constexpr bool NEWTON_REUSE = PG_ASSOC_NEWTON_REUSE && SLOTS <= PG_REUSE_MAX_SLOTS;
    static constexpr int SAV_SLOTS = NEWTON_REUSE ? SLOTS : 0, SAV_STRIDE = (2 * SLOTS + 1) * 64;   // doubles per kept evaluation
};
// the powers of an evaluation, as the MASK of gram_pass: P | Q | R
constexpr int PW_P = 1, PW_PQ = 3, PW_R = 4, PW_PQR = 7;
__host__ __device__ constexpr int tri(int r, int c) { return r * (r + 1) / 2 + c; }  // r >= c
__host__ __device__ constexpr int next_pow2(int v) { int p = 1; while (p < v) p <<= 1; return p; }

__device__ __forceinline__ double dmaxf(double a, float b) { return ((double)b > a) ? (double)b : a; }

// 64-lane sums of NVP per-lane partials, one value index per lane ("reduce-scatter"): recursive halving with
// ascending strides 1,2,4,.. — lane l keeps the values whose index agrees with its low bits and adds its
// partner's partials of them — then plain butterfly steps for the strides >= NVP.  Every value goes through
// exactly the additions of the xor-butterfly (strides 1..32) the oracle's order=1 mode performs, so the bits
// are the same, at ~1/6 of the adds and shuffles.  Returns the total of value index (lane % NVP).
template <int NVP>
__device__ __forceinline__ double reduce_scatter(double (&v)[NVP], int lane)
{
    static_assert(NVP >= 1 && NVP <= 64 && (NVP & (NVP - 1)) == 0, "power of two");
#pragma unroll
    for (int s = 1; s < NVP; s <<= 1) {
        const bool b = (lane & s) != 0;
#pragma unroll
        for (int m = 0; m < NVP / (2 * s); m++) {
            const double keep = b ? v[2 * m + 1] : v[2 * m];
            const double send = b ? v[2 * m] : v[2 * m + 1];
            v[m] = keep + __shfl_xor(send, s, 64);
        }
    }
    double x = v[0];
#pragma unroll
    for (int s = NVP; s < 64; s <<= 1) x += __shfl_xor(x, s, 64);
    return x;
}

// NP per-lane partials (lower-triangle entries) -> one owned entry per lane and slot: slot 0 holds entry
// (lane % NVP0) of entries [0,64), slot 1 entry 64 + (lane % NVP1).
template <int C, int SL = 0>
__device__ __forceinline__ void scatter_entries(const double (&acc)[Shape<C>::NP], int lane, double (&out)[Shape<C>::SLOTS])
{
    constexpr int NV = Shape<C>::slot_nv(SL), NVP = next_pow2(NV);
    double t[NVP];
#pragma unroll
    for (int k = 0; k < NVP; k++) t[k] = (k < NV) ? acc[64 * SL + k] : 0.0;
    out[SL] = reduce_scatter<NVP>(t, lane);
    if constexpr (SL + 1 < Shape<C>::SLOTS) scatter_entries<C, SL + 1>(acc, lane, out);
}

// which Gram entries a lane owns
template <int C> struct Own {
    int e[Shape<C>::SLOTS], r[Shape<C>::SLOTS], c[Shape<C>::SLOTS];
    bool valid[Shape<C>::SLOTS];
    __device__ __forceinline__ void init(int lane)
    {
#pragma unroll
        for (int sl = 0; sl < Shape<C>::SLOTS; sl++) {
            const int nv = Shape<C>::slot_nv(sl), k = lane % next_pow2(nv);
            valid[sl] = k < nv;
            e[sl] = valid[sl] ? 64 * sl + k : 0;
            int rr = 0;
            while ((rr + 1) * (rr + 2) / 2 <= e[sl]) rr++;
            r[sl] = rr; c[sl] = e[sl] - rr * (rr + 1) / 2;
        }
    }
};

// value of Gram entry `es` (per-lane index) / `eq` (wave-uniform index) from its owning lane
template <int SLOTS>
__device__ __forceinline__ double gather(const double (&X)[SLOTS], int es)
{
    double v = __shfl(X[0], es & 63, 64);
#pragma unroll
    for (int sl = 1; sl < SLOTS; sl++) { const double w = __shfl(X[sl], es & 63, 64); v = ((es >> 6) == sl) ? w : v; }
    return v;
}

__device__ __forceinline__ void wave_lds_sync();

// The c_tot sweeps of precompute_mat (pyx:947-963 / :1007-1036) with the Gram entries spread over the lanes:
// every lane updates the entry (r,c) it owns, fetching the pivot-column operands from their owners; arithmetic per
// entry identical to oracle sweeps(order=1).  Scalars (traces, pivots) are wave-uniform.
// PW: the powers swept (PW_P, PW_PQ or PW_PQR).  Every power's update reads itself and the lower powers only, and the pivots,
// their logs and the clamps of P are P's own: sweeping fewer powers leaves the bits of those swept as they are.  PW_P exports
// yPy, ld, Pxx_c, Pyx_c and sh; the fields of a power that is not swept are 0 and must not be read.
// REC (setup_tabs_kernel, PW_PQ): the sweeps stop after the C covariate pivots and leave in rec what decade_lanes applies to a SNP's
// x row — per step q and x-row entry k the record {ia, ba2, P(r_k, q), Q(r_k, q)} (r_k = k, the (y, x) entry reads row y; zeros
// where the entry is not updated at that step), then {trP, ld, P(y,y), Q(y,y)} after the C steps.  Nothing of o is set.
template <int C, int PW, bool REC = false>
__device__ __forceinline__ void lane_sweeps(double (&P)[Shape<C>::SLOTS], double (&Q)[Shape<C>::SLOTS], double (&R)[Shape<C>::SLOTS],
                                            const Own<C> &own, double t1, double t2, int lane, EvalOut &o, double *piv, double *rec = nullptr)
{
    constexpr int M = Shape<C>::M, NP = Shape<C>::NP, SLOTS = Shape<C>::SLOTS;
    static_assert(PW == PW_P || PW == PW_PQ || PW == PW_PQR, "powers");
    static_assert(!REC || PW == PW_PQ, "the decade table holds P and Q");
    constexpr bool DQ = (PW & 2) != 0, FULL = (PW & 4) != 0;
    // With three or more slots per lane (c >= 14) the pivot column goes through the wave's LDS (piv: 3 M doubles) instead of
    // lane shuffles: a shuffle-gather costs SLOTS permutes per operand, 6 SLOTS^2 per step — pure data movement either way.
    constexpr bool VIA_LDS = Shape<C>::SWEEP_LDS;
    if (own.valid[0] && own.e[0] == 0) P[0] = dmaxf(P[0], PG_MINV);
    double trP = t1, trPP = t2, apiv = 1.0;
    for (int i = 1; i < (REC ? M - 1 : M); i++) {
        const int q = i - 1, eqq = tri(q, q);
        double a, b = 0.0, e = 0.0;
        double ur[SLOTS], uc[SLOTS], vr[SLOTS], vc[SLOTS], wr[SLOTS], wc[SLOTS];
        bool act[SLOTS];
        if constexpr (VIA_LDS) {
#pragma unroll
            for (int sl = 0; sl < SLOTS; sl++)
                if (own.valid[sl] && own.c[sl] == q) {       // owners of column q publish it (replicas write the same value)
                    piv[own.r[sl]] = P[sl];
                    if (DQ) piv[M + own.r[sl]] = Q[sl];
                    if (FULL) piv[2 * M + own.r[sl]] = R[sl];
                }
            wave_lds_sync();
            a = piv[q];
            if (DQ) b = piv[M + q];
            if (FULL) e = piv[2 * M + q];
#pragma unroll
            for (int sl = 0; sl < SLOTS; sl++) {
                act[sl] = own.valid[sl] && own.c[sl] >= i;
                const int rr = act[sl] ? own.r[sl] : q, cc = act[sl] ? own.c[sl] : q;
                ur[sl] = piv[rr]; uc[sl] = piv[cc];
                if (DQ) { vr[sl] = piv[M + rr]; vc[sl] = piv[M + cc]; }
                if (FULL) { wr[sl] = piv[2 * M + rr]; wc[sl] = piv[2 * M + cc]; }
            }
            wave_lds_sync();                                  // all reads done before the next step's writes
        } else {
            a = gather<SLOTS>(P, eqq);
            if (DQ) b = gather<SLOTS>(Q, eqq);
            if (FULL) e = gather<SLOTS>(R, eqq);
#pragma unroll
            for (int sl = 0; sl < SLOTS; sl++) {
                act[sl] = own.valid[sl] && own.c[sl] >= i;       // r >= c >= i
                const int er = act[sl] ? tri(own.r[sl], q) : 0, ec = act[sl] ? tri(own.c[sl], q) : 0;
                ur[sl] = gather<SLOTS>(P, er); uc[sl] = gather<SLOTS>(P, ec);
                if (DQ) { vr[sl] = gather<SLOTS>(Q, er); vc[sl] = gather<SLOTS>(Q, ec); }
                if (FULL) { wr[sl] = gather<SLOTS>(R, er); wc[sl] = gather<SLOTS>(R, ec); }
            }
        }
        if (lane == q) apiv = a;
        const double a2 = a * a, ia = -1.0 / a, ba2 = b / a2;
        if constexpr (REC) {   // column q is not updated at its own step: every location is written once (replicas write the same value)
            double *rq = rec + (size_t)q * M * 4;
            if (lane < M) { rq[4 * lane] = ia; rq[4 * lane + 1] = ba2; }
            if (lane <= q) { rq[4 * lane + 2] = 0.0; rq[4 * lane + 3] = 0.0; }
#pragma unroll
            for (int sl = 0; sl < SLOTS; sl++)
                if (own.valid[sl] && own.c[sl] == q && own.r[sl] > q) { rq[4 * own.r[sl] + 2] = P[sl]; rq[4 * own.r[sl] + 3] = Q[sl]; }
        }
        if constexpr (FULL) {
            const double ba = b / a;
            trPP = (trPP + ba * ba) - 2 * (e / a);
            const double a3 = a2 * a, b2 = b * b;
            const double cR = (e / a2) - (b2 / a3);
#pragma unroll
            for (int sl = 0; sl < SLOTS; sl++)
                if (act[sl]) {
                    double s1 = fma(cR * uc[sl], ur[sl], R[sl]);
                    double s2 = fma(ia * uc[sl], wr[sl], 0.0); s2 = fma(ia * wc[sl], ur[sl], s2);
                    double s3 = fma(ia * vc[sl], vr[sl], 0.0);
                    double s4 = fma(ba2 * uc[sl], vr[sl], 0.0); s4 = fma(ba2 * vc[sl], ur[sl], s4);
                    double rn = ((s1 + s2) + s3) + s4;
                    if (own.r[sl] == i && own.c[sl] == i) rn = dmaxf(rn, PG_MINV);
                    R[sl] = rn;
                }
        }
        if constexpr (DQ) {
            trP = trP - b / a;
#pragma unroll
            for (int sl = 0; sl < SLOTS; sl++)
                if (act[sl]) {
                    double s1 = fma(ba2 * uc[sl], ur[sl], Q[sl]);
                    double s2 = fma(ia * uc[sl], vr[sl], 0.0); s2 = fma(ia * vc[sl], ur[sl], s2);
                    double qn = s1 + s2;
                    double pn = fma(ia * uc[sl], ur[sl], P[sl]);
                    if (own.r[sl] == i && own.c[sl] == i) { qn = dmaxf(qn, PG_MINV); pn = dmaxf(pn, PG_MINV); }
                    Q[sl] = qn; P[sl] = pn;
                }
        } else {
#pragma unroll
            for (int sl = 0; sl < SLOTS; sl++)
                if (act[sl]) {
                    double pn = fma(ia * uc[sl], ur[sl], P[sl]);
                    if (own.r[sl] == i && own.c[sl] == i) pn = dmaxf(pn, PG_MINV);
                    P[sl] = pn;
                }
        }
        if (i == M - 2) { o.Pxx_c = (float)gather<SLOTS>(P, tri(M - 2, M - 2)); o.Pyx_c = (float)gather<SLOTS>(P, tri(M - 1, M - 2)); }
    }
    // logdet_Wt_H_inv_W (pyx:957/1029): f32 accumulator += log(pivot), pivots in order; the M-1 logs are taken
    // at once (lane q holds pivot q), the f32 accumulation stays sequential
    const double lg = log(apiv);
    float ld = 0.0f;
    for (int q = 0; q < (REC ? M - 2 : M - 1); q++) ld = (float)((double)ld + __shfl(lg, q, 64));
    if constexpr (REC) {
        const double pyy = gather<SLOTS>(P, NP - 1), qyy = gather<SLOTS>(Q, NP - 1);
        double *tail = rec + (size_t)C * M * 4;
        if (lane == 0) { tail[0] = trP; tail[1] = (double)ld; tail[2] = pyy; tail[3] = qyy; }
        return;
    }
    o.yPy = (float)gather<SLOTS>(P, NP - 1);
    o.yPPy = DQ ? (float)gather<SLOTS>(Q, NP - 1) : 0.0f;
    o.yPPPy = FULL ? (float)gather<SLOTS>(R, NP - 1) : 0.0f;
    o.trP = DQ ? (float)trP : 0.0f;
    o.trPP = FULL ? (float)trPP : 0.0f;
    o.ld = ld;
    o.sh = (float)t1;
    o.shh = FULL ? (float)t2 : 0.0f;
}

// One element's operands: the packed fixed row (d, w_0..w_{C-1}, y) as 16-byte vectors plus x_i.
// Loads are unconditional so that the next element's loads can be issued before the current element's arithmetic, and no value
// is selected afterwards: rows >= n of the table hold w = y = 0 and d = +inf, which makes h = 1/(lam d + 1) exactly 0 there
// (x = inf takes the division fallback of hinv_f32: 1/inf = 0), so every product of a pad element is 0 whatever x is read
// (the x index is clamped to n-1: a caller's row need not have a pad).
template <int C> struct Elem {
    static constexpr int S4 = (C + 2 + 3) / 4;
    float4 row[S4];
    float x;
};
template <int C, bool HASX = true>
__device__ __forceinline__ void load_elem(const AssocParams &pr, const float *xrow, int i, Elem<C> &e)
{
    const float4 *src = reinterpret_cast<const float4 *>(pr.fixed + (size_t)i * pr.rowf);
#pragma unroll
    for (int k = 0; k < Elem<C>::S4; k++) e.row[k] = src[k];
    const int ic = min(i, pr.n - 1);
    e.x = HASX ? xrow[ic] : 0.0f;
}
// software pipeline with a ring of PFD register sets (compile-time slots: no register copies, no scratch)
// PIN: nothing is scheduled across the point where a slot's loads are issued, so they go out right behind the body that freed the slot
// and stay in flight for the whole body of the other one (the decade scan: left alone, the scheduler sinks them to their first use)
constexpr int PFD = PG_PFD;
template <class E, int PF = PFD, bool PIN = false, class LoadF, class BodyF>
__device__ __forceinline__ void pipelined(int niter, LoadF &&ld, BodyF &&body)
{
    E buf[PF];
#pragma unroll
    for (int d = 0; d < PF; d++) {
        ld(buf[d], d < niter ? d : niter - 1);
        if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);   // slot by slot here too: the loop's waits count the loads behind a slot's
    }
    for (int it = 0; it < niter; it += PF) {
#pragma unroll
        for (int d = 0; d < PF; d++) {
            if (it + d < niter) body(buf[d], it + d);
            const int nx = it + d + PF;
            if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
            ld(buf[d], nx < niter ? nx : niter - 1);
            if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
        }
    }
}
template <int C>
__device__ __forceinline__ void unpack_elem(const AssocParams &pr, const Elem<C> &e, int i, float &d, float (&col)[C + 2])
{
    float buf[4 * Elem<C>::S4];
#pragma unroll
    for (int k = 0; k < Elem<C>::S4; k++) {
        buf[4 * k] = e.row[k].x; buf[4 * k + 1] = e.row[k].y; buf[4 * k + 2] = e.row[k].z; buf[4 * k + 3] = e.row[k].w;
    }
    d = buf[0];
#pragma unroll
    for (int j = 0; j < C; j++) col[j] = buf[1 + j];
    col[C] = e.x;
    col[C + 1] = buf[C + 1];
}
// The operands of one element as the Gram passes read them: EL::E (the element's registers), EL::Row (what addresses the SNP's
// per-SNP columns), EL::load / EL::unpack.  WaldElem: the packed fixed row plus the SNP's x; the GxE scan has its own (GxeElem).
template <int C> struct WaldElem {
    using E = Elem<C>;
    using Row = const float *;
    template <bool HASX>
    static __device__ __forceinline__ void load(const AssocParams &pr, Row xrow, int i, E &e) { load_elem<C, HASX>(pr, xrow, i, e); }
    static __device__ __forceinline__ void unpack(const AssocParams &pr, const E &e, int i, float &d, float (&col)[C + 2]) { unpack_elem<C>(pr, e, i, d, col); }
};

// One pass over the n elements accumulating the level-0 Gram powers selected by MASK (1: P = W*'H^-1 W*,
// 2: Q = W*'H^-2 W*, 4: R = W*'H^-3 W*; t1 rides with P, t2 with R), then the reduce-scatter to the owning lanes.
template <int C, int MASK, bool HASX, class EL = WaldElem<C>>
__device__ __forceinline__ void gram_pass(const AssocParams &pr, typename EL::Row xrow, float lam, int lane, float *htab_out,
                                          double (&Po)[Shape<C>::SLOTS], double (&Qo)[Shape<C>::SLOTS], double (&Ro)[Shape<C>::SLOTS],
                                          double &t1, double &t2)
{
    constexpr int M = Shape<C>::M, NP = Shape<C>::NP;
    constexpr bool DP = (MASK & 1) != 0, DQ = (MASK & 2) != 0, DR = (MASK & 4) != 0;
    double P[DP ? NP : 1], Q[DQ ? NP : 1], R[DR ? NP : 1];
#pragma unroll
    for (int k = 0; k < NP; k++) { if constexpr (DP) P[k] = 0.0; if constexpr (DQ) Q[k] = 0.0; if constexpr (DR) R[k] = 0.0; }
    double s1 = 0.0, s2 = 0.0;
    using E = typename EL::E;
    pipelined<E>(pr.niter, [&](E &e, int it) { EL::template load<HASX>(pr, xrow, it * 64 + lane, e); },
                       [&](const E &cur, int it) {
        const int i = it * 64 + lane;
        float d, colf[M];
        EL::unpack(pr, cur, i, d, colf);
        const float h = hinv_f32(lam, d);        // pad rows: d = +inf -> h = 0
        if (htab_out) htab_out[i] = h;
        const double hd = (double)h;
        double col[M], a[M];
#pragma unroll
        for (int j = 0; j < M; j++) { col[j] = (double)colf[j]; a[j] = hd * col[j]; }
        if (DP || DQ) {
#pragma unroll
            for (int j = 0; j < M; j++)
#pragma unroll
                for (int k = 0; k <= j; k++) {
                    if constexpr (DP) P[tri(j, k)] = fma(a[j], col[k], P[tri(j, k)]);
                    if constexpr (DQ) Q[tri(j, k)] = fma(a[j], a[k], Q[tri(j, k)]);
                }
        }
        if (DP) s1 += hd;
        if constexpr (DR) {
            const double h2 = hd * hd;
#pragma unroll
            for (int j = 0; j < M; j++) {
                const double gj = h2 * col[j];
#pragma unroll
                for (int k = 0; k <= j; k++) R[tri(j, k)] = fma(gj, a[k], R[tri(j, k)]);
            }
            s2 = fma(hd, hd, s2);
        }
    });
    if constexpr (DP) { scatter_entries<C>(P, lane, Po); t1 = bfly(s1); }
    if constexpr (DQ) scatter_entries<C>(Q, lane, Qo);
    if constexpr (DR) { scatter_entries<C>(R, lane, Ro); t2 = bfly(s2); }
}

// One pass over the n elements for the entries of ONE slot and ONE power (PW = 1: P, 2: Q, 3: R): the per-entry arithmetic
// and summation order are those of gram_pass (every entry is its own fma chain), only the grouping into passes differs.
template <int C, int PW, int SL, bool HASX, class EL = WaldElem<C>>
__device__ __forceinline__ void gram_pass_slot(const AssocParams &pr, typename EL::Row xrow, float lam, int lane, float *htab_out, double &out, double &tsum)
{
    constexpr int M = Shape<C>::M, E0 = 64 * SL, NV = Shape<C>::slot_nv(SL), NVP = next_pow2(NV);
    double acc[NVP];
#pragma unroll
    for (int k = 0; k < NVP; k++) acc[k] = 0.0;
    double s = 0.0;
    // wide rows (c > 20): one register set in flight instead of two, the element ring would push the slot's 64 accumulators to scratch
    using E = typename EL::E;
    pipelined<E, (M > 22 ? 1 : PFD)>(pr.niter, [&](E &e, int it) { EL::template load<HASX>(pr, xrow, it * 64 + lane, e); },
                       [&](const E &cur, int it) {
        const int i = it * 64 + lane;
        float d, colf[M];
        EL::unpack(pr, cur, i, d, colf);
        const float h = hinv_f32(lam, d);        // pad rows: d = +inf -> h = 0
        if (htab_out) htab_out[i] = h;
        const double hd = (double)h, h2 = hd * hd;
        double col[M], a[M], g[PW == 3 ? M : 1];
#pragma unroll
        for (int j = 0; j < M; j++) { col[j] = (double)colf[j]; a[j] = hd * col[j]; if constexpr (PW == 3) g[j] = h2 * col[j]; }
#pragma unroll
        for (int j = 0; j < M; j++)
#pragma unroll
            for (int k = 0; k <= j; k++) {
                const int e = tri(j, k);
                if (e >= E0 && e < E0 + NV) {
                    if constexpr (PW == 1) acc[e - E0] = fma(a[j], col[k], acc[e - E0]);
                    else if constexpr (PW == 2) acc[e - E0] = fma(a[j], a[k], acc[e - E0]);
                    else acc[e - E0] = fma(g[j], a[k], acc[e - E0]);
                }
            }
        if constexpr (SL == 0 && PW == 1) s += hd;
        if constexpr (SL == 0 && PW == 3) s = fma(hd, hd, s);
    });
    out = reduce_scatter<NVP>(acc, lane);
    if constexpr (SL == 0 && (PW == 1 || PW == 3)) tsum = bfly(s);
}
template <int C, int PW, bool HASX, int SL = 0, class EL = WaldElem<C>>
__device__ __forceinline__ void slot_passes(const AssocParams &pr, typename EL::Row xrow, float lam, int lane, float *htab_out,
                                            double (&X)[Shape<C>::SLOTS], double &tsum)
{
    gram_pass_slot<C, PW, SL, HASX, EL>(pr, xrow, lam, lane, SL == 0 ? htab_out : nullptr, X[SL], tsum);
    if constexpr (SL + 1 < Shape<C>::SLOTS) slot_passes<C, PW, HASX, SL + 1, EL>(pr, xrow, lam, lane, htab_out, X, tsum);
}

// Level-0 Grams of the powers in MASK at an arbitrary lambda, as they leave the reduce-scatter: P and t1, Q, R and t2.  Which
// powers share a pass over n follows Shape<C>; every entry is its own fma chain, so its bits do not depend on that grouping.
template <int C, int MASK, class EL = WaldElem<C>>
__device__ __forceinline__ void gram_powers(const AssocParams &pr, typename EL::Row xrow, float lam, int lane,
                                            double (&P)[Shape<C>::SLOTS], double (&Q)[Shape<C>::SLOTS], double (&R)[Shape<C>::SLOTS],
                                            double &t1, double &t2)
{
    constexpr bool DP = (MASK & 1) != 0, DQ = (MASK & 2) != 0, DR = (MASK & 4) != 0;
    if constexpr (Shape<C>::CHUNKED) {
        double tq = 0.0;
        if constexpr (DP) slot_passes<C, 1, true, 0, EL>(pr, xrow, lam, lane, nullptr, P, t1);
        if constexpr (DQ) slot_passes<C, 2, true, 0, EL>(pr, xrow, lam, lane, nullptr, Q, tq);
        if constexpr (DR) slot_passes<C, 3, true, 0, EL>(pr, xrow, lam, lane, nullptr, R, t2);
    } else if constexpr (MASK == PW_PQR && Shape<C>::FUSE_PQR) {
        gram_pass<C, 7, true, EL>(pr, xrow, lam, lane, nullptr, P, Q, R, t1, t2);
    } else if constexpr (DP && DQ && Shape<C>::FUSE_PQ) {
        gram_pass<C, 3, true, EL>(pr, xrow, lam, lane, nullptr, P, Q, R, t1, t2);
        if constexpr (DR) gram_pass<C, 4, true, EL>(pr, xrow, lam, lane, nullptr, P, Q, R, t1, t2);
    } else {
        if constexpr (DP) gram_pass<C, 1, true, EL>(pr, xrow, lam, lane, nullptr, P, Q, R, t1, t2);
        if constexpr (DQ) gram_pass<C, 2, true, EL>(pr, xrow, lam, lane, nullptr, P, Q, R, t1, t2);
        if constexpr (DR) gram_pass<C, 4, true, EL>(pr, xrow, lam, lane, nullptr, P, Q, R, t1, t2);
    }
}

// Level-0 Grams at an arbitrary lambda, then the sweeps, for the powers PW (PW_P, PW_PQ or PW_PQR).
template <int C, int PW, class EL = WaldElem<C>>
__device__ __forceinline__ void eval_specific(const AssocParams &pr, typename EL::Row xrow, float lam, int lane, const Own<C> &own, EvalOut &o,
                                              double *piv)
{
    constexpr int SLOTS = Shape<C>::SLOTS;
    double P[SLOTS], Q[SLOTS], R[SLOTS], t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int sl = 0; sl < SLOTS; sl++) { Q[sl] = 0.0; R[sl] = 0.0; }
    gram_powers<C, PW, EL>(pr, xrow, lam, lane, P, Q, R, t1, t2);
    lane_sweeps<C, PW>(P, Q, R, own, t1, t2, lane, o, piv);
}

// ------------------------------------------------------------------------------------------------
// setup: one wavefront per decade lambda t — h table, SNP-independent level-0 Gram entries (x := 0),
// t1 and log|H| at lam11[t].
template <int C>
__global__ __launch_bounds__(64) void setup_tabs_kernel(AssocParams pr)
{
    constexpr int NP = Shape<C>::NP, SLOTS = Shape<C>::SLOTS;
    extern __shared__ float smem_f[];
    const int t = blockIdx.x, lane = threadIdx.x;
    const float lam = pr.lam11[t];
    Own<C> own;
    own.init(lane);
    double P[SLOTS], Q[SLOTS], R[SLOTS], t1 = 0.0, t2 = 0.0;
    if constexpr (Shape<C>::CHUNKED) {
        double tq = 0.0;
        slot_passes<C, 1, false>(pr, nullptr, lam, lane, pr.htab + (size_t)t * pr.npad, P, t1);
        slot_passes<C, 2, false>(pr, nullptr, lam, lane, nullptr, Q, tq);
    } else if constexpr (Shape<C>::FUSE_PQ) {
        gram_pass<C, 3, false>(pr, nullptr, lam, lane, pr.htab + (size_t)t * pr.npad, P, Q, R, t1, t2);
    } else {
        gram_pass<C, 1, false>(pr, nullptr, lam, lane, pr.htab + (size_t)t * pr.npad, P, Q, R, t1, t2);
        gram_pass<C, 2, false>(pr, nullptr, lam, lane, nullptr, P, Q, R, t1, t2);
    }
#pragma unroll
    for (int sl = 0; sl < SLOTS; sl++)
        if (own.valid[sl]) {   // replicas write the same value
            pr.fixg[((size_t)t * 2 + 0) * NP + own.e[sl]] = P[sl];
            pr.fixg[((size_t)t * 2 + 1) * NP + own.e[sl]] = Q[sl];
        }
    float ldH = device_logdet_H(pr, lam, lane, smem_f);
    if (lane == 0) { pr.t1tab[t] = t1; pr.ldHtab[t] = ldH; }
    // the decade table: the C covariate pivots on the block [W | y] by lane_sweeps' own statements (the x row is 0 here and is not
    // recorded), and the scalars of this lambda decade_lanes reads per lane
    if constexpr (PG_ASSOC_DECADE_HOIST && C >= 1) {
        __shared__ double piv_s[Shape<C>::SWEEP_LDS ? 3 * Shape<C>::M : 1];
        if (pr.dtab) {
            double *rec = pr.dtab + (size_t)t * assoc_dtab_doubles(C);
            EvalOut e;
            lane_sweeps<C, PW_PQ, true>(P, Q, R, own, t1, 0.0, lane, e, piv_s, rec);
            double *tail = rec + (size_t)C * Shape<C>::M * 4;
            if (lane == 0) { tail[4] = t1; tail[5] = (double)ldH; tail[6] = (double)lam; tail[7] = 0.0; }
        }
    }
}

// The 64-lane totals of a scan pass's NV per-lane partials (the x-entries of NV / 2M lambdas from t0) into xent: two reduce-scatters
// of <= 64 and <= 32 values.
template <int M, int NV, int NACC>
__device__ __forceinline__ void scan_totals(const double (&acc)[NACC], int t0, int lane, double *xent)
{
    constexpr int NV0 = NV < 64 ? NV : 64, NV1 = NV > 64 ? NV - 64 : 0;
    constexpr int NVP0 = next_pow2(NV0), NVP1 = next_pow2(NV1 > 0 ? NV1 : 1);
    {
        double t[NVP0];
#pragma unroll
        for (int k = 0; k < NVP0; k++) t[k] = acc[k];
        const double tot = reduce_scatter<NVP0>(t, lane);
        const int idx = lane % NVP0;
        if (idx < NV0 && lane < NVP0) xent[t0 * 2 * M + idx] = tot;
    }
    if constexpr (NV1 > 0) {
        double t[NVP1];
#pragma unroll
        for (int k = 0; k < NVP1; k++) t[k] = acc[64 + k];
        const double tot = reduce_scatter<NVP1>(t, lane);
        const int idx = lane % NVP1;
        if (idx < NV1 && lane < NVP1) xent[t0 * 2 * M + 64 + idx] = tot;
    }
}

// The scan rows (assoc_srow_layout), one thread per element, behind build_fixed_kernel and setup_tabs_kernel: copies of the fixed row's
// w and y and of the h that setup_tabs_kernel wrote for the element at each decade lambda — the bits the scan read from the two tables.
// Rows >= n hold zeros in both, so they are all zero here.
template <int C>
__global__ __launch_bounds__(256) void build_scan_rows_kernel(AssocParams pr)
{
    constexpr SrowLayout L = assoc_srow_layout(C);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pr.npad) return;
    const float *fx = pr.fixed + (size_t)i * pr.rowf;
    float *row = pr.srow + (size_t)i * L.rowf;
#pragma unroll
    for (int k = 0; k < L.rowf; k++) {
        float v = 0.0f;
        if (k <= C) v = fx[1 + k];
        else if (k >= L.hoff && k < L.hoff + NLAM) v = pr.htab[(size_t)(k - L.hoff) * pr.npad + i];
        row[k] = v;
    }
}

// scan accumulation: only the Gram entries that involve x, for the GG decade lambdas from T0 at once; the totals go to
// xent[t][2M] in the wave's LDS (entry k <= C: P(x,k); C+1: P(y,x); M+k likewise for Q).
// Operands: the element's scan row (assoc_srow_layout) and x.  Both addresses are a wave-uniform base (xrow must be one) plus a 32-bit
// lane offset, so a slot of the ring is NVEC 16-byte loads at immediate offsets and one dword, on two offset registers; the host checks
// that the table is below 4 GiB.  x is read at min(i, n - 1) as load_elem reads it, so a pad element multiplies the same x by the same zeros.
template <int C, int T0, int GG>
__device__ __forceinline__ void scan_accumulate(const AssocParams &pr, const float *xrow, int lane, double *xent)
{
    constexpr int M = Shape<C>::M, NV = GG * 2 * M;
    constexpr int NV0 = NV < 64 ? NV : 64, NV1 = NV > 64 ? NV - 64 : 0;      // values reduced by the first / second reduce-scatter
    constexpr int NVP0 = next_pow2(NV0), NVP1 = next_pow2(NV1 > 0 ? NV1 : 1);
    static_assert(NV <= 128, "scan group too large");
    constexpr SrowLayout L = assoc_srow_layout(C);
    constexpr unsigned MASK = assoc_srow_mask(C, L.hoff, T0, GG);
    constexpr int NVEC = __builtin_popcount(MASK);
    double acc[NV0 == 64 ? 64 + NVP1 : NVP0];
#pragma unroll
    for (int k = 0; k < (NV0 == 64 ? 64 + NVP1 : NVP0); k++) acc[k] = 0.0;
    typedef float v4f __attribute__((ext_vector_type(4)));
    struct SE { v4f v[NVEC]; float x; };
    const char *rows = reinterpret_cast<const char *>(pr.srow), *xs = reinterpret_cast<const char *>(xrow);
    constexpr unsigned ROWB = L.rowf * 4;
    const unsigned xlast = (unsigned)(pr.n - 1) * 4u, lane_row = (unsigned)lane * ROWB, lane_x = (unsigned)lane * 4u;
    pipelined<SE, PG_SCAN_PFD, true>(pr.niter, [&](SE &q, int it) {
        const char *row = rows + (lane_row + (unsigned)it * (64u * ROWB));   // one vector add per element: the lane's part does not change
        // vector k of the row, where the pass reads it, is the slot's vector number popcount(MASK below bit k)
#pragma unroll
        for (int k = 0; k < 32; k++)
            if (MASK >> k & 1) q.v[__builtin_popcount(MASK & ((1u << k) - 1))] = *reinterpret_cast<const v4f *>(row + 16 * k);
        q.x = *reinterpret_cast<const float *>(xs + min(lane_x + (unsigned)it * 256u, xlast));
    }, [&](const SE &q, int it) {
        // each loaded vector stays one register tuple from its load to this point: carried round the loop as single floats, the
        // components get registers of their own and are copied out of the tuple right behind the load, which waits for it there
        v4f qv[NVEC];
#pragma unroll
        for (int k = 0; k < NVEC; k++) { qv[k] = q.v[k]; asm volatile("" : "+v"(qv[k])); }
        auto rf = [&](int f) -> float {      // float f of the row
            return qv[__builtin_popcount(MASK & ((1u << (f / 4)) - 1))][f & 3];
        };
        float colf[M];
#pragma unroll
        for (int k = 0; k < C; k++) colf[k] = rf(k);
        colf[C] = q.x;
        colf[C + 1] = rf(C);
        // z_k = x * col_k (k <= C: the covariates and x itself) and z_{C+1} = y * x are exact in f64 (24 x 24 bits) and do not
        // depend on lambda: P(x,k) += h z_k and Q(x,k) += h^2 z_k add the same exact products (h x)(w_k), (h x)(h w_k) that
        // the Gram pass of a specific lambda forms from a_j = h col_j — same bits, 6 multiplies fewer per lambda.
        const double xd = (double)colf[C];
        double z[M];
#pragma unroll
        for (int k = 0; k <= C; k++) z[k] = xd * (double)colf[k];
        z[C + 1] = (double)colf[C + 1] * xd;
#pragma unroll
        for (int g = 0; g < GG; g++) {
            const double hd = (double)rf(L.hoff + T0 + g);
            const double h2 = hd * hd;                       // exact
            // row x (index C): columns k <= C ; row y (index C+1): column x
#pragma unroll
            for (int k = 0; k <= C + 1; k++) {
                acc[g * 2 * M + k] = fma(hd, z[k], acc[g * 2 * M + k]);
                acc[g * 2 * M + M + k] = fma(h2, z[k], acc[g * 2 * M + M + k]);
            }
        }
    });
    scan_totals<M, NV>(acc, T0, lane, xent);
}
// The same accumulation from the fixed rows and the h table (one load per lambda, each with its own address), for the instantiations
// that do not read the scan rows (!Shape<C>::SCAN_PACKED): same operands, same chains, same reduce-scatters as scan_accumulate.
template <int C, int GG>
__device__ __forceinline__ void scan_accumulate_tabs(const AssocParams &pr, const float *xrow, int t0, int lane, double *xent)
{
    constexpr int M = Shape<C>::M, NV = GG * 2 * M;
    constexpr int NV0 = NV < 64 ? NV : 64, NV1 = NV > 64 ? NV - 64 : 0;
    constexpr int NVP0 = next_pow2(NV0), NVP1 = next_pow2(NV1 > 0 ? NV1 : 1);
    static_assert(NV <= 128, "scan group too large");
    double acc[NV0 == 64 ? 64 + NVP1 : NVP0];
#pragma unroll
    for (int k = 0; k < (NV0 == 64 ? 64 + NVP1 : NVP0); k++) acc[k] = 0.0;
    struct SE { Elem<C> e; float h[GG]; };
    pipelined<SE>(pr.niter, [&](SE &q, int it) {
        const int i = it * 64 + lane;
        load_elem<C>(pr, xrow, i, q.e);
#pragma unroll
        for (int g = 0; g < GG; g++) q.h[g] = pr.htab[(size_t)(t0 + g) * pr.npad + i];
    }, [&](const SE &q, int it) {
        const int i = it * 64 + lane;
        float d, colf[M];
        unpack_elem<C>(pr, q.e, i, d, colf);
        const double xd = (double)colf[C];
        double z[M];
#pragma unroll
        for (int k = 0; k <= C; k++) z[k] = xd * (double)colf[k];
        z[C + 1] = (double)colf[C + 1] * xd;
#pragma unroll
        for (int g = 0; g < GG; g++) {
            const double hd = (double)q.h[g];
            const double h2 = hd * hd;                       // exact
#pragma unroll
            for (int k = 0; k <= C + 1; k++) {
                acc[g * 2 * M + k] = fma(hd, z[k], acc[g * 2 * M + k]);
                acc[g * 2 * M + M + k] = fma(h2, z[k], acc[g * 2 * M + M + k]);
            }
        }
    });
    scan_totals<M, NV>(acc, t0, lane, xent);
}
template <int C, int T0>
__device__ __forceinline__ void scan_all(const AssocParams &pr, const float *xrow, int lane, double *xent)
{
    constexpr int G = Shape<C>::G;
    if constexpr (T0 < NLAM) {
        constexpr int GG = (NLAM - T0) < G ? (NLAM - T0) : G;
        if constexpr (Shape<C>::SCAN_PACKED) scan_accumulate<C, T0, GG>(pr, xrow, lane, xent);
        else scan_accumulate_tabs<C, GG>(pr, xrow, T0, lane, xent);
        scan_all<C, T0 + GG>(pr, xrow, lane, xent);
    }
}

// Multi-phenotype decade scan (pg_assoc_pheno_dev): the x-entries of TC phenotypes at once.  P(x,k) and Q(x,k), k <= C, do not involve
// y and are accumulated once; P(y_j,x), Q(y_j,x) once per phenotype j: C + 1 + TC values per lambda and power instead of TC (C + 2).
// Every value is the per-lane fma chain of scan_accumulate (same products z, same element order) and goes through reduce_scatter,
// whose additions do not depend on how the values are grouped: the totals are scan_accumulate's bits.  Phenotypes j >= tcn (the pad
// of a chunk up to TC) read y = 0.  out: this SNP's [NLAM][2][XE] row of the scan buffer.  PWS powers per pass from PW0 (2, 0: P and Q;
// 1, pw: one of them, for wide rows: the products z are then used once each and need not stay in registers).
template <int C, int TC, int GG, int PWS, int PW0>
__device__ __forceinline__ void scan_pheno_accumulate(const AssocParams &pr, const float *xrow, const float *Y, long long ldy, int tcn,
                                                      int t0, int lane, double *out)
{
    constexpr int M = Shape<C>::M, XE = C + 1 + TC, NV = GG * PWS * XE;
    // accumulator v -> lambda t0 + v / (PWS XE), power PW0 + (v % (PWS XE)) / XE, entry v % XE of the [NLAM][2][XE] row
    auto dest = [&](int v) { const int gg = v / (PWS * XE), r = v - gg * PWS * XE; return (t0 + gg) * 2 * XE + PW0 * XE + r; };
    constexpr int NV0 = NV < 64 ? NV : 64, NV1 = NV > 64 ? NV - 64 : 0;
    constexpr int NVP0 = next_pow2(NV0), NVP1 = next_pow2(NV1 > 0 ? NV1 : 1);
    static_assert(NV <= 128, "scan group too large");
    double acc[NV0 == 64 ? 64 + NVP1 : NVP0];
#pragma unroll
    for (int k = 0; k < (NV0 == 64 ? 64 + NVP1 : NVP0); k++) acc[k] = 0.0;
    struct SE { Elem<C> e; float y[TC]; float h[GG]; };
    pipelined<SE>(pr.niter, [&](SE &q, int it) {
        const int i = it * 64 + lane;
        load_elem<C>(pr, xrow, i, q.e);
#pragma unroll
        for (int j = 0; j < TC; j++) q.y[j] = (i < pr.n && j < tcn) ? Y[(size_t)j * ldy + i] : 0.0f;   // pad rows: y = 0 as in the fixed rows
#pragma unroll
        for (int g = 0; g < GG; g++) q.h[g] = pr.htab[(size_t)(t0 + g) * pr.npad + i];
    }, [&](const SE &q, int it) {
        const int i = it * 64 + lane;
        float d, colf[M];
        unpack_elem<C>(pr, q.e, i, d, colf);
        const double xd = (double)colf[C];
        double z[XE];
#pragma unroll
        for (int k = 0; k <= C; k++) z[k] = xd * (double)colf[k];
#pragma unroll
        for (int j = 0; j < TC; j++) z[C + 1 + j] = (double)q.y[j] * xd;
#pragma unroll
        for (int g = 0; g < GG; g++) {
            const double hd = (double)q.h[g];
            const double h2 = hd * hd;
#pragma unroll
            for (int k = 0; k < XE; k++) {
                if constexpr (PWS == 2) {
                    acc[g * 2 * XE + k] = fma(hd, z[k], acc[g * 2 * XE + k]);
                    acc[g * 2 * XE + XE + k] = fma(h2, z[k], acc[g * 2 * XE + XE + k]);
                } else {
                    acc[g * XE + k] = fma(PW0 == 0 ? hd : h2, z[k], acc[g * XE + k]);
                }
            }
        }
    });
    {
        double t[NVP0];
#pragma unroll
        for (int k = 0; k < NVP0; k++) t[k] = acc[k];
        const double tot = reduce_scatter<NVP0>(t, lane);
        const int idx = lane % NVP0;
        if (idx < NV0 && lane < NVP0) out[dest(idx)] = tot;
    }
    if constexpr (NV1 > 0) {
        double t[NVP1];
#pragma unroll
        for (int k = 0; k < NVP1; k++) t[k] = acc[64 + k];
        const double tot = reduce_scatter<NVP1>(t, lane);
        const int idx = lane % NVP1;
        if (idx < NV1 && lane < NVP1) out[dest(64 + idx)] = tot;
    }
}
template <int C, int TC, int T0>
__device__ __forceinline__ void scan_pheno_all(const AssocParams &pr, const float *xrow, const float *Y, long long ldy, int tcn, int lane,
                                               double *out)
{
    // lambdas per pass: the 2 XE accumulators of each plus the XE products z held across them within the SCAN_NV budget; rows wider
    // than PG_PHENO_SPLIT_XE take one pass per power and lambda (the register report: from c = 23 on hundreds of VGPRs spilled otherwise)
    constexpr int XE = C + 1 + TC, PWS = XE > PG_PHENO_SPLIT_XE ? 1 : 2;
    constexpr int G0 = PWS == 1 ? 1 : (Shape<C>::SCAN_NV - XE) / (PWS * XE), G = G0 < 1 ? 1 : (G0 > NLAM ? NLAM : G0);
    if constexpr (T0 < NLAM) {
        constexpr int GG = (NLAM - T0) < G ? (NLAM - T0) : G;
        if constexpr (PWS == 2) {
            scan_pheno_accumulate<C, TC, GG, 2, 0>(pr, xrow, Y, ldy, tcn, T0, lane, out);
        } else {
            scan_pheno_accumulate<C, TC, GG, 1, 0>(pr, xrow, Y, ldy, tcn, T0, lane, out);
            scan_pheno_accumulate<C, TC, GG, 1, 1>(pr, xrow, Y, ldy, tcn, T0, lane, out);
        }
        scan_pheno_all<C, TC, T0 + GG>(pr, xrow, Y, ldy, tcn, lane, out);
    }
}
constexpr int SCAN_WPB = 4;   // SNPs (wavefronts) per workgroup of scan_pheno_kernel: no LDS, no barrier, no straggler
// One wavefront per SNP: the rows [NLAM][2][C + 1 + TC] of xbuf for pr.p SNPs of pr.xr; Y: tcn rotated phenotypes, row stride ldy.
template <int C, int TC>
__global__ __launch_bounds__(64 * SCAN_WPB, PG_WAVES) void scan_pheno_kernel(AssocParams pr, const float *Y, long long ldy, int tcn, double *xbuf)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * SCAN_WPB + wave;
    if (g >= pr.p) return;
    scan_pheno_all<C, TC, 0>(pr, pr.xr + (size_t)g * pr.ldx, Y, ldy, tcn, lane, xbuf + (size_t)g * NLAM * 2 * (C + 1 + TC));
}

__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// scipy.optimize.brentq (scipy/optimize/Zeros/brentq.c), xtol=2e-12, rtol=0.1, maxiter=100 (pyx:176-182).
// f(a), f(b) are the decade-scan values (the reference re-evaluates them: same inputs, same results).
template <class Fn>
__device__ __forceinline__ double brentq_dev(Fn &&f, double xa, double xb, double fa, double fb, int maxiter = 100)
{
    const double xtol = 2e-12, rtol = 0.1;
    double xpre = xa, xcur = xb, xblk = 0., fpre = fa, fcur = fb, fblk = 0., spre = 0., scur = 0., sbis, delta, stry, dpre, dblk;
    if (fpre == 0) return xpre;
    if (fcur == 0) return xcur;
    for (int i = 0; i < maxiter; i++) {
        if (fpre != 0 && fcur != 0 && (__builtin_signbit(fpre) != __builtin_signbit(fcur))) {
            xblk = xpre; fblk = fpre; spre = scur = xcur - xpre;
        }
        if (fabs(fblk) < fabs(fcur)) {
            xpre = xcur; xcur = xblk; xblk = xpre;
            fpre = fcur; fcur = fblk; fblk = fpre;
        }
        delta = (xtol + rtol * fabs(xcur)) / 2;
        sbis = (xblk - xcur) / 2;
        if (fcur == 0 || fabs(sbis) < delta) return xcur;
        if (fabs(spre) > delta && fabs(fcur) < fabs(fpre)) {
            if (xpre == xblk) {
                stry = -fcur * (xcur - xpre) / (fcur - fpre);
            } else {
                dpre = (fpre - fcur) / (xpre - xcur);
                dblk = (fblk - fcur) / (xblk - xcur);
                stry = -fcur * (fblk * dblk - fpre * dpre) / (dblk * dpre * (fblk - fpre));
            }
            double lim = 3 * fabs(sbis) - delta;
            double mn = fabs(spre) < lim ? fabs(spre) : lim;
            if (2 * fabs(stry) < mn) { spre = scur; scur = stry; }
            else { spre = sbis; scur = sbis; }
        } else { spre = sbis; scur = sbis; }
        xpre = xcur; fpre = fcur;
        if (fabs(scur) > delta) xcur += scur;
        else xcur += (sbis > 0 ? delta : -delta);
        fcur = f(xcur);
    }
    return xcur;
}

// newton (pyx:1349-1416), all f32: root <- root - d1/d2; stops on the sign test (:1392), on leaving [l0, l1] (returns the
// previous iterate, :1398-1404), on NaN/Inf (:1406), on r_eps < 1e-5 or iteration > 100 (:1411).  eval(lam, e) fills the
// full (three-power) quadratic forms at lam.
template <class Eval>
__device__ __forceinline__ float newton_dev(const AssocParams &pr, float lroot, float l0, float l1, Eval &&eval)
{
    int iteration = 0;
    for (;;) {
        EvalOut e;
        eval(lroot, e);
        const float d1 = d1_f(pr, lroot, e.yPy, e.yPPy, e.trP);
        const float d2 = d2_f(pr, lroot, e.yPy, e.yPPy, e.yPPPy, e.trP, e.trPP);
        const float ratio = __fdiv_rn(d1, d2);
        // np.sign(ratio)*np.sign(d1)*np.sign(d2) <= 0.0   (NaN compares False)
        const bool any_nan = (ratio != ratio) || (d1 != d1) || (d2 != d2);
        const float sr = (float)((ratio > 0) - (ratio < 0)), s1 = (float)((d1 > 0) - (d1 < 0)), s2 = (float)((d2 > 0) - (d2 < 0));
        if (!any_nan && sr * s1 * s2 <= 0.0f) break;
        const float lnew = __fsub_rn(lroot, ratio);
        const float r_eps = (float)(fabs((double)__fsub_rn(lnew, lroot)) / fabs((double)lroot));
        if (lnew < l0) break;
        if (lnew > l1) break;
        if (isnan(lnew) || isinf(lnew)) break;
        lroot = lnew;
        if ((double)r_eps < 1e-5 || iteration > 100) break;
        iteration++;
    }
    return lroot;
}

#if defined(PG_ASSOC_STAMPS) && !defined(PG_ASSOC_PART)   // tools/assoc_decade_stamps.py: s_memtime at wave entry, before and after the
// decade sweeps and at wave exit, for 1024 SNPs spread evenly over the launch (this unit's kernels only: Wald, c <= 15)
__device__ long long g_assoc_stamps[1024 * 4];
#define ASSOC_STAMP(slot)                                                                                       \
    do {                                                                                                        \
        const long long sq_ = pr.p >= 1024 ? pr.p / 1024 : 1, sr_ = g / sq_;                                    \
        if (lane == 0 && sr_ < 1024 && g == sr_ * sq_)                                                          \
            g_assoc_stamps[sr_ * 4 + slot] = (long long)__builtin_amdgcn_s_memtime();                           \
    } while (0)
#else
#define ASSOC_STAMP(slot) do { } while (0)
#endif

// The sweeps at the 11 decade lambdas, side by side on the lanes.  At a decade lambda the block [W | y] of P and Q is the same for every
// SNP, and an update of entry (r, c) on the pivot q reads (r, q), (c, q) and the pivot only: the C covariate pivots, their
// reciprocals, trP and the first C terms of ld are setup_tabs_kernel's (the decade table), and a SNP owns just its x row — the xent
// entries k < C: (x, w_k), C: (x, x), C + 1: (y, x).  Lane (g, k) of 64 / M lambdas per round holds P and Q of entry k and applies
// step q with the operand roles lane_sweeps gives that entry (ur, vr: the entry's row at column q; uc, vc: its column's), the x
// row's own (x, q) by one shuffle inside the lambda's lanes; then every lane of the lambda does the pivot on x — (y, y), trP, the
// last term of ld — and the scalars.  Each value is formed by lane_sweeps' expression from operands of the same bits.
template <int C>
__device__ __forceinline__ void decade_lanes(const AssocParams &pr, const double *xent, int lane, EvalOut *evs, float *d1s, float *lls)
{
    constexpr int M = Shape<C>::M, G = 64 / M;
    static_assert(C >= 1 && G >= 2, "decade_lanes: one covariate step at least, two lambdas per round at least");
    const int tl = lane / M, k = lane - tl * M;
    for (int t0 = 0; t0 < NLAM; t0 += G) {
        const bool on = tl < G && t0 + tl < NLAM;     // lanes past the round's lambdas repeat its first one and write nothing
        const int g = on ? tl : 0, t = t0 + g, base = g * M;
        const double2 *tab = reinterpret_cast<const double2 *>(pr.dtab + (size_t)t * assoc_dtab_doubles(C));
        double P = xent[t * 2 * M + k], Q = xent[t * 2 * M + M + k];
#pragma unroll
        for (int q = 0; q < C; q++) {
            const double2 s = tab[(q * M + k) * 2], w = tab[(q * M + k) * 2 + 1];
            const double ia = s.x, ba2 = s.y;
            const double xp = __shfl(P, base + q, 64), xq = __shfl(Q, base + q, 64);
            const double ur = (k == C + 1) ? w.x : xp, uc = (k < C) ? w.x : xp;
            const double vr = (k == C + 1) ? w.y : xq, vc = (k < C) ? w.y : xq;
            double s1 = fma(ba2 * uc, ur, Q);
            double s2 = fma(ia * uc, vr, 0.0); s2 = fma(ia * vc, ur, s2);
            double qn = s1 + s2;
            double pn = fma(ia * uc, ur, P);
            if (q == C - 1 && k == C) { qn = dmaxf(qn, PG_MINV); pn = dmaxf(pn, PG_MINV); }
            if (k > q) { Q = qn; P = pn; }
        }
        // the pivot on x: only (y, y) is left to update
        const double a = __shfl(P, base + C, 64), b = __shfl(Q, base + C, 64);
        const double u = __shfl(P, base + C + 1, 64), v = __shfl(Q, base + C + 1, 64);
        const double2 z0 = tab[C * M * 2], z1 = tab[C * M * 2 + 1], z2 = tab[C * M * 2 + 2], z3 = tab[C * M * 2 + 3];
        const double t1 = z2.x;
        const float ldH = (float)z2.y, lam = (float)z3.x;
        EvalOut e;
        e.Pxx_c = (float)a; e.Pyx_c = (float)u;
        const double a2 = a * a, ia = -1.0 / a, ba2 = b / a2;
        const double trP = z0.x - b / a;
        double s1 = fma(ba2 * u, u, z1.y);
        double s2 = fma(ia * u, v, 0.0); s2 = fma(ia * v, u, s2);
        const double qn = dmaxf(s1 + s2, PG_MINV);
        const double pn = dmaxf(fma(ia * u, u, z1.x), PG_MINV);
        e.yPy = (float)pn; e.yPPy = (float)qn; e.yPPPy = 0.0f;
        e.trP = (float)trP; e.trPP = 0.0f;
        e.ld = (float)((double)(float)z0.y + log(a));
        e.sh = (float)t1; e.shh = 0.0f;
        if (on && k == 0) {
            evs[t] = e;
            d1s[t] = d1_f(pr, lam, e.yPy, e.yPPy, e.trP);
            lls[t] = logl_f(pr, e.yPy, ldH, e.ld);
        }
    }
}

template <int C, bool LRT, bool PHENO = false>
// PHENO (pg_assoc_pheno_dev; never with LRT): the decade scan's x-entries are read from pr.xbuf; one launch per phenotype, so that
// every (SNP, phenotype) is one wavefront and a workgroup holds WPB of them, as in a single-phenotype launch.
// two waves per SIMD for EVERY c (PG_WAVES = 2): a lone wave cannot issue fp64 VALU at the pipe's rate (measured 2.3x faster at 2 than at
// 1).  From c = 4 on the instantiations are capped at 256 VGPRs with spills to scratch (c = 5: 76 VGPR + 36 SGPR spills, 228 B; c = 10:
// 125, 360 B; c = 14: 178, 544 B) — all of them in the per-evaluation outer loops; the Gram loops themselves are scratch-free (checked on
// the shipped code object: VERDICT r3), and so are the scan loops except at c = 20..22
__global__ __launch_bounds__(64 * WPB, PG_WAVES) void assoc_kernel(AssocParams pr)
{
    constexpr int M = Shape<C>::M, NP = Shape<C>::NP, SLOTS = Shape<C>::SLOTS;
    extern __shared__ unsigned char smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    static_assert(!(PHENO && LRT), "the multi-phenotype search has no LRT");
    const long long g = (long long)blockIdx.x * WPB + wave;
    if (g >= pr.p) return;  // whole wavefront leaves; no workgroup barrier is used anywhere in this kernel
    ASSOC_STAMP(0);
    // per-wave LDS: [piv] | [sav] | xent[NLAM][2M] doubles | evs[NLAM] | d1s[NLAM] | lls[NLAM] | vals[n_vals]
    constexpr size_t piv_bytes = Shape<C>::SWEEP_LDS ? (size_t)3 * M * 8 : 0;
    constexpr bool REUSE = Shape<C>::NEWTON_REUSE;
    unsigned char *base = smem + (size_t)wave * assoc_per_wave_bytes(M, Shape<C>::SWEEP_LDS, Shape<C>::SAV_SLOTS, sizeof(EvalOut), pr.n_vals);
    double *piv = reinterpret_cast<double *>(base);          // pivot column exchange of the sweeps (c >= 14 only)
    base += piv_bytes;
    double *sav = reinterpret_cast<double *>(base) + lane;   // Brent's last two evaluations: this lane's P[SLOTS], Q[SLOTS], t1, 64 doubles apart
    base += assoc_sav_doubles(Shape<C>::SAV_SLOTS) * 8;
    double *xent = reinterpret_cast<double *>(base);
    EvalOut *evs = reinterpret_cast<EvalOut *>(base + (size_t)NLAM * 2 * M * 8);
    float *d1s = reinterpret_cast<float *>(evs + NLAM);
    float *lls = d1s + NLAM;
    float *vals = lls + NLAM;
    const float *xrow = pr.xr + (size_t)g * pr.ldx;

    Own<C> own;
    own.init(lane);
    // ---- decade scan: x-dependent Gram entries at the 11 shared lambdas
    if constexpr (PHENO) {   // from the scan buffer: xent[t][pw][k] = row (t, pw) entry k (k <= C) or this phenotype's (k = C + 1)
        const double *src = pr.xbuf + (size_t)g * NLAM * 2 * pr.xe;
        for (int j = lane; j < NLAM * 2 * M; j += 64) {
            const int tp = j / M, k = j - tp * M;
            xent[j] = src[(size_t)tp * pr.xe + (k <= C ? k : pr.xcol)];
        }
    } else {
        // the scan wants the SNP's row as a wave-uniform base: every lane of a wave has the same `wave`, which the compiler cannot see
        const long long gu = (long long)blockIdx.x * WPB + __builtin_amdgcn_readfirstlane(wave);
        scan_all<C, 0>(pr, pr.xr + (size_t)gu * pr.ldx, lane, xent);
    }
    wave_lds_sync();
    ASSOC_STAMP(1);
    // the decade sweeps: lane-parallel on the decade table, or — the multi-phenotype search, c = 0, rows too wide for two lambdas
    // per round — every lambda's whole sweep in turn
    constexpr bool HOIST = PG_ASSOC_DECADE_HOIST && !PHENO && C >= 1 && 64 / M >= 2;
    if constexpr (HOIST) decade_lanes<C>(pr, xent, lane, evs, d1s, lls);
    else for (int t = 0; t < NLAM; t++) {
        double P[SLOTS], Q[SLOTS], R[SLOTS];
        const double *fp = pr.fixg + ((size_t)t * 2 + 0) * NP, *fq = pr.fixg + ((size_t)t * 2 + 1) * NP;
        const double *xe = xent + t * 2 * M;
#pragma unroll
        for (int sl = 0; sl < SLOTS; sl++) {
            const int r = own.r[sl], c = own.c[sl];
            const bool isx = (r == C) || (r == C + 1 && c == C);
            const int k = (r == C) ? c : C + 1;
            P[sl] = isx ? xe[k] : fp[own.e[sl]];
            Q[sl] = isx ? xe[M + k] : fq[own.e[sl]];
            R[sl] = 0.0;
        }
        EvalOut e;
        lane_sweeps<C, PW_PQ>(P, Q, R, own, pr.t1tab[t], 0.0, lane, e, piv);
        if (lane == 0) {
            evs[t] = e;
            d1s[t] = d1_f(pr, pr.lam11[t], e.yPy, e.yPPy, e.trP);
            lls[t] = logl_f(pr, e.yPy, pr.ldHtab[t], e.ld);
        }
    }
    ASSOC_STAMP(2);
    wave_lds_sync();
    // ---- candidate selection (pyx:109-117 / :144-152): start from the two boundaries
    float best_l = lls[0], best_lambda;
    EvalOut best_e;
    if (best_l < lls[NLAM - 1]) { best_l = lls[NLAM - 1]; best_lambda = pr.lam11[NLAM - 1]; best_e = evs[NLAM - 1]; }
    else { best_lambda = pr.lam11[0]; best_e = evs[0]; }
    // n_fast / n_full count evaluations (two-power | three-power quadratic forms asked for), whatever passes they took; n_ponly:
    // evaluations that made P alone, n_reuse: Newton evaluations that made R alone on Brent's P and Q
    unsigned n_fast = 0, n_full = 0, n_ponly = 0, n_reuse = 0;
    constexpr int PW_FINAL = PG_ASSOC_FINAL_P ? PW_P : PW_PQ;   // at the root only yPy, ld, Pxx_c and Pyx_c are read
    if (pr.grid) {
        for (int t = 0; t < NLAM - 1; t++)   // pyx:119-130, k = -5..4, strict '>'
            if (lls[t] > best_l) { best_l = lls[t]; best_lambda = pr.lam11[t]; best_e = evs[t]; }
    } else {
        for (int k = 0; k < NLAM - 1; k++) {  // pyx:154-192
            const float f0 = d1s[k], f1 = d1s[k + 1];
            if (__builtin_signbit(f0) == __builtin_signbit(f1)) continue;   // copysignf product < 0 (pyx:174)
            const float l0 = pr.lam11[k], l1 = pr.lam11[k + 1];
            // Brent returns one of the lambdas it evaluated, mostly one of the last two (not always the last: the bracket's other
            // end when that has the smaller |f|), and Newton starts there: the level-0 P, Q and t1 of Brent's last two evaluations
            // are kept as they leave the reduce-scatter (the sweeps overwrite them), this lane's entries in the wave's LDS.
            float sav_lam0 = NAN, sav_lam1 = NAN;
            unsigned sav_next = 0;
            double root = brentq_dev(
                [&](double x) -> double {
                    EvalOut e;
                    const float lf = (float)x;      // pyx:1631: np.float32_t lam
                    if constexpr (REUSE) {
                        double P[SLOTS], Q[SLOTS], R[SLOTS], t1 = 0.0, t2 = 0.0;
#pragma unroll
                        for (int sl = 0; sl < SLOTS; sl++) R[sl] = 0.0;
                        gram_powers<C, PW_PQ>(pr, xrow, lf, lane, P, Q, R, t1, t2);
                        double *sv = sav + sav_next * Shape<C>::SAV_STRIDE;
#pragma unroll
                        for (int sl = 0; sl < SLOTS; sl++) { sv[64 * sl] = P[sl]; sv[64 * (SLOTS + sl)] = Q[sl]; }
                        sv[64 * 2 * SLOTS] = t1;
                        if (sav_next) sav_lam1 = lf; else sav_lam0 = lf;
                        sav_next ^= 1u;
                        lane_sweeps<C, PW_PQ>(P, Q, R, own, t1, t2, lane, e, piv);
                    } else {
                        eval_specific<C, PW_PQ>(pr, xrow, lf, lane, own, e, piv);
                    }
                    n_fast++;
                    return (double)d1_f(pr, lf, e.yPy, e.yPPy, e.trP);
                },
                (double)l0, (double)l1, (double)f0, (double)f1);
            // newton (pyx:1349-1416), all f32.  Its first evaluation, at a lambda bit-equal to a kept one, needs only the R pass;
            // anything else (a decade endpoint, an older Brent point, NaN) and every later evaluation takes all three powers.
            bool first = true;
            const float lroot = newton_dev(pr, (float)root, l0, l1, [&](float lf, EvalOut &e) {
                if constexpr (REUSE) {
                    const unsigned lb = __float_as_uint(lf);
                    const int hit = !(first && lf == lf) ? -1 : (lb == __float_as_uint(sav_lam0)) ? 0 : (lb == __float_as_uint(sav_lam1)) ? 1 : -1;
                    first = false;
                    double P[SLOTS], Q[SLOTS], R[SLOTS], t1 = 0.0, t2 = 0.0;
                    if (hit >= 0) {
                        const double *sv = sav + hit * Shape<C>::SAV_STRIDE;
#pragma unroll
                        for (int sl = 0; sl < SLOTS; sl++) { P[sl] = sv[64 * sl]; Q[sl] = sv[64 * (SLOTS + sl)]; }
                        t1 = sv[64 * 2 * SLOTS];
                        gram_powers<C, PW_R>(pr, xrow, lf, lane, P, Q, R, t1, t2);
                        n_reuse++;
                    } else {
                        gram_powers<C, PW_PQR>(pr, xrow, lf, lane, P, Q, R, t1, t2);
                    }
                    lane_sweeps<C, PW_PQR>(P, Q, R, own, t1, t2, lane, e, piv);
                } else {
                    eval_specific<C, PW_PQR>(pr, xrow, lf, lane, own, e, piv);
                }
                n_full++;
            });
            EvalOut e;
            eval_specific<C, PW_FINAL>(pr, xrow, lroot, lane, own, e, piv);   // pyx:186
            n_fast++;
            if (PW_FINAL == PW_P) n_ponly++;
            const float ldH = device_logdet_H(pr, lroot, lane, vals);
            const float ll = logl_f(pr, e.yPy, ldH, e.ld);       // pyx:188
            if (ll > best_l) { best_l = ll; best_lambda = lroot; best_e = e; }
        }
    }
    if constexpr (LRT) {
        // ---- N2: lambda_ML = calc_lambda(eigenVals, Y, [W, x]) (lmm/lmm.py:22-84) and likelihood_lambda at it (pyx:1542-1562).
        // Candidates in the reference's order: 1e-5, 1e5, then per decade with a sign change of d logL / d lambda one root by
        // brentq(rtol = 0.1, maxiter = 5000) + scipy.optimize.newton(fprime = d2, rtol = 1e-5, tol = 1.48e-8, maxiter = 10);
        // np.argmax keeps the first maximum (a NaN wins).  The decade values reuse the scan's quadratic forms.
        float ml_l = ml_logl_f(pr, evs[0].yPy, pr.ldHtab[0]), ml_lam = pr.lam11[0];
        {
            const float l1 = ml_logl_f(pr, evs[NLAM - 1].yPy, pr.ldHtab[NLAM - 1]);
            if (ml_l == ml_l && (l1 != l1 || l1 > ml_l)) { ml_l = l1; ml_lam = pr.lam11[NLAM - 1]; }
        }
        for (int k = 0; k < NLAM - 1; k++) {
            const float f0 = ml_d1_f(pr, pr.lam11[k], evs[k].yPy, evs[k].yPPy, evs[k].sh);
            const float f1 = ml_d1_f(pr, pr.lam11[k + 1], evs[k + 1].yPy, evs[k + 1].yPPy, evs[k + 1].sh);
            if (f0 != f0 || f1 != f1) continue;
            const float s0 = (float)((f0 > 0) - (f0 < 0)), s1 = (float)((f1 > 0) - (f1 < 0));
            if (!(s0 * s1 < 0.0f)) continue;                                 // np.sign(f0) * np.sign(f1) < 0
            double p0 = brentq_dev(
                [&](double x) -> double {
                    EvalOut e;
                    const float lf = (float)x;
                    eval_specific<C, PW_PQ>(pr, xrow, lf, lane, own, e, piv);
                    n_fast++;
                    return (double)ml_d1_f(pr, lf, e.yPy, e.yPPy, e.sh);
                },
                (double)pr.lam11[k], (double)pr.lam11[k + 1], (double)f0, (double)f1, 5000);
            double pn = p0;
            for (int itr = 0; itr < 10; itr++) {
                EvalOut e;
                const float lf = (float)p0;
                eval_specific<C, PW_PQR>(pr, xrow, lf, lane, own, e, piv);
                n_full++;
                const float fval = ml_d1_f(pr, lf, e.yPy, e.yPPy, e.sh);
                if (fval == 0.0f) { pn = p0; break; }
                const float fder = ml_d2_f(pr, lf, e.yPy, e.yPPy, e.yPPPy, e.sh, e.shh);
                if (fder == 0.0f) { pn = p0; break; }
                pn = p0 - (double)__fdiv_rn(fval, fder);
                if (fabs(pn - p0) <= 1.48e-8 + 1e-5 * fabs(p0)) break;
                p0 = pn;
            }
            if (ml_l == ml_l) {
                EvalOut e;
                const float lf = (float)pn;
                eval_specific<C, PW_FINAL>(pr, xrow, lf, lane, own, e, piv);   // the ML logL reads yPy only
                n_fast++;
                if (PW_FINAL == PW_P) n_ponly++;
                const float l = ml_logl_f(pr, e.yPy, device_logdet_H(pr, lf, lane, vals));
                if (l != l || l > ml_l) { ml_l = l; ml_lam = lf; }
            }
        }
        if (lane == 0) { pr.lalt[g] = ml_l; pr.lamalt[g] = ml_lam; }
    }
    // ---- beta, se, tau, F (pyx:1529-1537, lmm.py:471)
    if (lane == 0) {
        const float b = __fdiv_rn(best_e.Pyx_c, best_e.Pxx_c);
        const float pxx = (PG_MINV > best_e.Pxx_c) ? PG_MINV : best_e.Pxx_c;
        const float sb = (float)(__dsqrt_rn((double)best_e.yPy) / ((double)sqrtf(pxx) * __dsqrt_rn((double)(pr.nu))));
        const float ta = __fdiv_rn((float)pr.nu, best_e.yPy);
        const double t = (double)__fdiv_rn(b, sb);
        pr.beta[g] = b; pr.se[g] = sb; pr.tau[g] = ta; pr.lam[g] = best_lambda; pr.F[g] = t * t;
        if (pr.stats) { atomicAdd(&pr.stats[0], (unsigned long long)n_fast); atomicAdd(&pr.stats[1], (unsigned long long)n_full); }
        if (pr.trace) pr.trace[g] = n_fast | (n_full << 16);
        if (pr.passes) {   // every evaluation passes over n once per power it makes: all make P but the reusing ones, all Q but those and the P-only ones
            const unsigned long long np = (unsigned long long)(n_fast + n_full - n_reuse);
            atomicAdd(&pr.passes[0], np); atomicAdd(&pr.passes[1], np - n_ponly);
            atomicAdd(&pr.passes[2], (unsigned long long)n_full); atomicAdd(&pr.passes[3], (unsigned long long)n_reuse);
        }
    }
    ASSOC_STAMP(3);
}

// ------------------------------------------------------------------------------------------------
// GxE (pg_assoc_gxe_dev): the REML Wald test of x o e with the SNP's own x among the covariates.  The full model has C = CS + 1
// covariates — the CS shared ones W' = [W, e] of the packed fixed rows and the per-SNP x — and the tested column xe, so the Gram
// matrices are those of Shape<CS + 1> over the columns [W' | x | xe | y], swept by lane_sweeps<CS + 1> exactly as the Wald kernel
// sweeps [W | x | y] with CS + 1 covariates: a row is what oracle calculate(d, y, [W', x], xe) gives in the kernels' order.
// The fixed block [W', y] at the decade lambdas is setup_tabs_kernel<CS>'s output on the same fixed rows (its row y is row CS + 1
// there); per SNP the decade scan accumulates only the NE = 2 CS + 5 entries per power that involve x or xe.
#if defined(PG_ASSOC_PART) && (PG_ASSOC_PART == 6 || PG_ASSOC_PART == 7)
struct GxeRows { const float *x, *xe; };   // the SNP's rotated x and x o e
template <int CS> struct GxeVals {
    static constexpr int S4 = (CS + 2 + 3) / 4;
    float4 row[S4];
    float x, xe;
};
// element operands of the Gram passes at the C = CS + 1 covariates of the full model: columns w_0..w_{CS-1}, x, xe, y
template <int C> struct GxeElem {
    static constexpr int CS = C - 1;
    using E = GxeVals<CS>;
    using Row = GxeRows;
    template <bool HASX>
    static __device__ __forceinline__ void load(const AssocParams &pr, Row r, int i, E &e)
    {   // as load_elem: unconditional loads, pad rows have d = +inf (h = 0), the per-SNP index clamped to n - 1
        const float4 *src = reinterpret_cast<const float4 *>(pr.fixed + (size_t)i * pr.rowf);
#pragma unroll
        for (int k = 0; k < E::S4; k++) e.row[k] = src[k];
        const int ic = min(i, pr.n - 1);
        e.x = r.x[ic];
        e.xe = r.xe[ic];
    }
    static __device__ __forceinline__ void unpack(const AssocParams &pr, const E &e, int i, float &d, float (&col)[C + 2])
    {
        float buf[4 * E::S4];
#pragma unroll
        for (int k = 0; k < E::S4; k++) {
            buf[4 * k] = e.row[k].x; buf[4 * k + 1] = e.row[k].y; buf[4 * k + 2] = e.row[k].z; buf[4 * k + 3] = e.row[k].w;
        }
        d = buf[0];
#pragma unroll
        for (int j = 0; j < CS; j++) col[j] = buf[1 + j];
        col[CS] = e.x;
        col[CS + 1] = e.xe;
        col[CS + 2] = buf[CS + 1];
    }
};
template <int CS> struct GxeShape {
    static constexpr int C = CS + 1, NE = 2 * CS + 5;   // scan entries per power: x.w_k, x.x, xe.w_k, xe.x, xe.xe, y.x, y.xe
    // lambdas per scan pass as in the multi-phenotype scan: the accumulators plus the NE products held across them within SCAN_NV;
    // rows wider than PG_PHENO_SPLIT_XE (CS >= 11) take one power per pass
    static constexpr int PWS = NE > PG_PHENO_SPLIT_XE ? 1 : 2;
    static constexpr int G0 = (Shape<C>::SCAN_NV - NE) / (PWS * NE), G = G0 < 1 ? 1 : (G0 > NLAM ? NLAM : G0);
};
// per-wave dynamic LDS of assoc_gxe_kernel: [piv: 3 M doubles when the sweeps go through LDS] | xent[NLAM][2][NE] doubles |
// evs[NLAM] | d1s[NLAM] | lls[NLAM] | vals[n_vals]
__host__ __device__ constexpr size_t gxe_per_wave_bytes(int M, bool sweep_lds, int NE, size_t evalout_bytes, int n_vals)
{
    return (((sweep_lds ? (size_t)3 * M * 8 : 0) + (size_t)NLAM * 2 * NE * 8 + NLAM * evalout_bytes + 2 * NLAM * 4 + (size_t)n_vals * 4) + 15) & ~(size_t)15;
}

// GG decade lambdas, PWS powers from PW0 (2, 0: P and Q; 1, pw: one of them) of the NE x / xe entries into xent [NLAM][2][NE].
// z_k are exact f64 products of two f32 columns, so fma(h, z_k) and fma(h^2, z_k) add what the Gram pass of a specific lambda adds
// for the same entry (see scan_accumulate); every value goes through reduce_scatter: same bits as a full Gram pass.
template <int CS, int GG, int PWS, int PW0>
__device__ __forceinline__ void gxe_scan_accumulate(const AssocParams &pr, GxeRows xr, int t0, int lane, double *out)
{
    using EL = GxeElem<CS + 1>;
    constexpr int M = CS + 3, NE = GxeShape<CS>::NE, NV = GG * PWS * NE;
    auto dest = [&](int v) { const int gg = v / (PWS * NE), r = v - gg * PWS * NE; return (t0 + gg) * 2 * NE + PW0 * NE + r; };
    constexpr int NV0 = NV < 64 ? NV : 64, NV1 = NV > 64 ? NV - 64 : 0;
    constexpr int NVP0 = next_pow2(NV0), NVP1 = next_pow2(NV1 > 0 ? NV1 : 1);
    static_assert(NV <= 128, "scan group too large");
    double acc[NV0 == 64 ? 64 + NVP1 : NVP0];
#pragma unroll
    for (int k = 0; k < (NV0 == 64 ? 64 + NVP1 : NVP0); k++) acc[k] = 0.0;
    struct SE { typename EL::E e; float h[GG]; };
    pipelined<SE>(pr.niter, [&](SE &q, int it) {
        const int i = it * 64 + lane;
        EL::template load<true>(pr, xr, i, q.e);
#pragma unroll
        for (int g = 0; g < GG; g++) q.h[g] = pr.htab[(size_t)(t0 + g) * pr.npad + i];
    }, [&](const SE &q, int it) {
        const int i = it * 64 + lane;
        float d, colf[M];
        EL::unpack(pr, q.e, i, d, colf);
        const double xd = (double)colf[CS], ed = (double)colf[CS + 1], yd = (double)colf[CS + 2];
        double z[NE];
#pragma unroll
        for (int k = 0; k < CS; k++) { z[k] = xd * (double)colf[k]; z[CS + 1 + k] = ed * (double)colf[k]; }
        z[CS] = xd * xd;
        z[2 * CS + 1] = ed * xd;
        z[2 * CS + 2] = ed * ed;
        z[2 * CS + 3] = yd * xd;
        z[2 * CS + 4] = yd * ed;
#pragma unroll
        for (int g = 0; g < GG; g++) {
            const double hd = (double)q.h[g];
            const double h2 = hd * hd;
#pragma unroll
            for (int k = 0; k < NE; k++) {
                if constexpr (PWS == 2) {
                    acc[g * 2 * NE + k] = fma(hd, z[k], acc[g * 2 * NE + k]);
                    acc[g * 2 * NE + NE + k] = fma(h2, z[k], acc[g * 2 * NE + NE + k]);
                } else {
                    acc[g * NE + k] = fma(PW0 == 0 ? hd : h2, z[k], acc[g * NE + k]);
                }
            }
        }
    });
    {
        double t[NVP0];
#pragma unroll
        for (int k = 0; k < NVP0; k++) t[k] = acc[k];
        const double tot = reduce_scatter<NVP0>(t, lane);
        const int idx = lane % NVP0;
        if (idx < NV0 && lane < NVP0) out[dest(idx)] = tot;
    }
    if constexpr (NV1 > 0) {
        double t[NVP1];
#pragma unroll
        for (int k = 0; k < NVP1; k++) t[k] = acc[64 + k];
        const double tot = reduce_scatter<NVP1>(t, lane);
        const int idx = lane % NVP1;
        if (idx < NV1 && lane < NVP1) out[dest(64 + idx)] = tot;
    }
}
template <int CS, int T0>
__device__ __forceinline__ void gxe_scan_all(const AssocParams &pr, GxeRows xr, int lane, double *xent)
{
    constexpr int G = GxeShape<CS>::G;
    if constexpr (T0 < NLAM) {
        constexpr int GG = (NLAM - T0) < G ? (NLAM - T0) : G;
        if constexpr (GxeShape<CS>::PWS == 2) {
            gxe_scan_accumulate<CS, GG, 2, 0>(pr, xr, T0, lane, xent);
        } else {
            gxe_scan_accumulate<CS, GG, 1, 0>(pr, xr, T0, lane, xent);
            gxe_scan_accumulate<CS, GG, 1, 1>(pr, xr, T0, lane, xent);
        }
        gxe_scan_all<CS, T0 + GG>(pr, xr, lane, xent);
    }
}

// One wavefront per SNP, WPB per workgroup; the REML search of assoc_kernel (Brent + Newton, no grid) on the full model's Grams.
template <int CS>
__global__ __launch_bounds__(64 * WPB, PG_WAVES) void assoc_gxe_kernel(AssocParams pr, const float *xer, long long ldxe)
{
    constexpr int C = CS + 1, M = Shape<C>::M, SLOTS = Shape<C>::SLOTS, NE = GxeShape<CS>::NE, NPS = Shape<CS>::NP;
    using EL = GxeElem<C>;
    extern __shared__ unsigned char smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * WPB + wave;
    if (g >= pr.p) return;  // whole wavefront leaves; no workgroup barrier is used anywhere in this kernel
    constexpr size_t piv_bytes = Shape<C>::SWEEP_LDS ? (size_t)3 * M * 8 : 0;
    unsigned char *base = smem + (size_t)wave * gxe_per_wave_bytes(M, Shape<C>::SWEEP_LDS, NE, sizeof(EvalOut), pr.n_vals);
    double *piv = reinterpret_cast<double *>(base);
    base += piv_bytes;
    double *xent = reinterpret_cast<double *>(base);
    EvalOut *evs = reinterpret_cast<EvalOut *>(base + (size_t)NLAM * 2 * NE * 8);
    float *d1s = reinterpret_cast<float *>(evs + NLAM);
    float *lls = d1s + NLAM;
    float *vals = lls + NLAM;
    const GxeRows xr{pr.xr + (size_t)g * pr.ldx, xer + (size_t)g * ldxe};

    Own<C> own;
    own.init(lane);
    // ---- decade scan: the x / xe entries at the 11 shared lambdas
    gxe_scan_all<CS, 0>(pr, xr, lane, xent);
    wave_lds_sync();
    for (int t = 0; t < NLAM; t++) {
        double P[SLOTS], Q[SLOTS], R[SLOTS];
        const double *fp = pr.fixg + ((size_t)t * 2 + 0) * NPS, *fq = pr.fixg + ((size_t)t * 2 + 1) * NPS;
        const double *xe = xent + t * 2 * NE;
#pragma unroll
        for (int sl = 0; sl < SLOTS; sl++) {
            const int r = own.r[sl], c = own.c[sl];
            // rows x (CS) and xe (CS + 1) and the entries (y, x), (y, xe) come from the scan; W' and y from setup_tabs_kernel<CS>,
            // whose row y is row CS + 1
            const int k = (r == CS) ? c : (r == CS + 1) ? CS + 1 + c : (r == CS + 2 && c == CS) ? 2 * CS + 3 : (r == CS + 2 && c == CS + 1) ? 2 * CS + 4 : -1;
            const int f = (r < CS) ? tri(r, c) : tri(CS + 1, c < CS ? c : CS + 1);
            const int kk = k >= 0 ? k : 0;
            P[sl] = k >= 0 ? xe[kk] : fp[f];
            Q[sl] = k >= 0 ? xe[NE + kk] : fq[f];
            R[sl] = 0.0;
        }
        EvalOut e;
        lane_sweeps<C, PW_PQ>(P, Q, R, own, pr.t1tab[t], 0.0, lane, e, piv);
        if (lane == 0) {
            evs[t] = e;
            d1s[t] = d1_f(pr, pr.lam11[t], e.yPy, e.yPPy, e.trP);
            lls[t] = logl_f(pr, e.yPy, pr.ldHtab[t], e.ld);
        }
    }
    wave_lds_sync();
    // ---- candidate selection, Brent + Newton: assoc_kernel's (pyx:144-192)
    float best_l = lls[0], best_lambda;
    EvalOut best_e;
    if (best_l < lls[NLAM - 1]) { best_l = lls[NLAM - 1]; best_lambda = pr.lam11[NLAM - 1]; best_e = evs[NLAM - 1]; }
    else { best_lambda = pr.lam11[0]; best_e = evs[0]; }
    unsigned n_fast = 0, n_full = 0;
    for (int k = 0; k < NLAM - 1; k++) {
        const float f0 = d1s[k], f1 = d1s[k + 1];
        if (__builtin_signbit(f0) == __builtin_signbit(f1)) continue;
        const float l0 = pr.lam11[k], l1 = pr.lam11[k + 1];
        double root = brentq_dev(
            [&](double x) -> double {
                EvalOut e;
                const float lf = (float)x;
                eval_specific<C, PW_PQ, EL>(pr, xr, lf, lane, own, e, piv);
                n_fast++;
                return (double)d1_f(pr, lf, e.yPy, e.yPPy, e.trP);
            },
            (double)l0, (double)l1, (double)f0, (double)f1);
        const float lroot = newton_dev(pr, (float)root, l0, l1, [&](float lf, EvalOut &e) {
            eval_specific<C, PW_PQR, EL>(pr, xr, lf, lane, own, e, piv);
            n_full++;
        });
        EvalOut e;
        eval_specific<C, PW_PQ, EL>(pr, xr, lroot, lane, own, e, piv);
        n_fast++;
        const float ldH = device_logdet_H(pr, lroot, lane, vals);
        const float ll = logl_f(pr, e.yPy, ldH, e.ld);
        if (ll > best_l) { best_l = ll; best_lambda = lroot; best_e = e; }
    }
    // ---- beta_gxe, se, tau, F (pyx:1529-1537, lmm.py:471): the tested column is xe, the last one before y
    if (lane == 0) {
        const float b = __fdiv_rn(best_e.Pyx_c, best_e.Pxx_c);
        const float pxx = (PG_MINV > best_e.Pxx_c) ? PG_MINV : best_e.Pxx_c;
        const float sb = (float)(__dsqrt_rn((double)best_e.yPy) / ((double)sqrtf(pxx) * __dsqrt_rn((double)(pr.nu))));
        const float ta = __fdiv_rn((float)pr.nu, best_e.yPy);
        const double t = (double)__fdiv_rn(b, sb);
        pr.beta[g] = b; pr.se[g] = sb; pr.tau[g] = ta; pr.lam[g] = best_lambda; pr.F[g] = t * t;
        if (pr.stats) { atomicAdd(&pr.stats[0], (unsigned long long)n_fast); atomicAdd(&pr.stats[1], (unsigned long long)n_full); }
    }
}

template <int CS>
static int launch_gxe(pg_ctx *ctx, AssocParams &pr, const float *xer, long long ldxe)
{
    constexpr int C = CS + 1;
    const size_t lds = (size_t)WPB * gxe_per_wave_bytes(Shape<C>::M, Shape<C>::SWEEP_LDS, GxeShape<CS>::NE, sizeof(EvalOut), pr.n_vals);
    PG_REQUIRE(pr.n_vals >= 0 && lds <= 160 * 1024, "assoc_gxe: c = %d, n_vals = %d need %zu bytes of LDS per workgroup", CS, pr.n_vals, lds);
    setup_tabs_kernel<CS><<<NLAM, 64, (size_t)pr.n_vals * 4 + 16, ctx->stream>>>(pr);
    PG_HIP(hipGetLastError());
    if (lds > 64 * 1024)
        PG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&assoc_gxe_kernel<CS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const long long nblk = (pr.p + WPB - 1) / WPB;
    assoc_gxe_kernel<CS><<<dim3((unsigned)nblk), 64 * WPB, lds, ctx->stream>>>(pr, xer, ldxe);
    PG_HIP(hipGetLastError());
    return PG_OK;
}
#endif

// ------------------------------------------------------------------------------------------------
// host side
template <int C, bool LRT = false>
static int launch_assoc(pg_ctx *ctx, AssocParams &pr)
{
    // launch size from the instantiation's own Shape (the same constexpr the kernel indexes with), checked on the host
    // against the device limit before anything is launched
    const size_t lds = (size_t)WPB * assoc_per_wave_bytes(Shape<C>::M, Shape<C>::SWEEP_LDS, Shape<C>::SAV_SLOTS, sizeof(EvalOut), pr.n_vals);
    static_assert(Shape<C>::M == C + 2, "Shape<C>::M");
    PG_REQUIRE(pr.n_vals >= 0 && lds <= 160 * 1024, "assoc: c = %d, n_vals = %d need %zu bytes of LDS per workgroup", C, pr.n_vals, lds);
    // the scan addresses its rows with 32-bit byte offsets
    if constexpr (Shape<C>::SCAN_PACKED)
        PG_REQUIRE(pr.srow && (size_t)pr.npad * assoc_srow_layout(C).rowf * 4 < ((size_t)1 << 32), "assoc: n = %d, c = %d: scan rows of %zu bytes",
                   pr.n, C, (size_t)pr.npad * assoc_srow_layout(C).rowf * 4);
    setup_tabs_kernel<C><<<NLAM, 64, (size_t)pr.n_vals * 4 + 16, ctx->stream>>>(pr);
    PG_HIP(hipGetLastError());
    if constexpr (Shape<C>::SCAN_PACKED) {
        build_scan_rows_kernel<C><<<(pr.npad + 255) / 256, 256, 0, ctx->stream>>>(pr);
        PG_HIP(hipGetLastError());
    }
    if (lds > 64 * 1024)
        PG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&assoc_kernel<C, LRT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const long long nblk = (pr.p + WPB - 1) / WPB;
    assoc_kernel<C, LRT><<<dim3((unsigned)nblk), 64 * WPB, lds, ctx->stream>>>(pr);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

// The kernels of pg_assoc_pheno_dev, one launch per call: SETUP = setup_tabs_kernel for one phenotype (pr.fixed / pr.fixg are its own),
// SCAN = scan_pheno_kernel over pr.p SNPs for a chunk of tcn phenotypes padded to tpad (1, 2, 4 or 8), SEARCH = the lambda search of
// assoc_kernel for one phenotype (pr.fixed, pr.fixg, pr.xcol and the outputs are its own), one wavefront per SNP.
struct PhenoLaunch {
    enum { SETUP, SCAN, SEARCH } phase;
    const float *Y; long long ldy;
    int tcn, tpad;
    double *xbuf;
};
constexpr int PHENO_CHUNK = 8;   // phenotypes per scan pass: C + 1 + 8 entries per lambda and power (47 at c = 30) keep 1 - 3 lambdas per pass
template <int C>
static int launch_pheno(pg_ctx *ctx, AssocParams &pr, const PhenoLaunch &pl)
{
    if (pl.phase == PhenoLaunch::SETUP) {
        setup_tabs_kernel<C><<<NLAM, 64, (size_t)pr.n_vals * 4 + 16, ctx->stream>>>(pr);
    } else if (pl.phase == PhenoLaunch::SCAN) {
        const unsigned nblk = (unsigned)((pr.p + SCAN_WPB - 1) / SCAN_WPB);
        switch (pl.tpad) {
            case 1: scan_pheno_kernel<C, 1><<<nblk, 64 * SCAN_WPB, 0, ctx->stream>>>(pr, pl.Y, pl.ldy, pl.tcn, pl.xbuf); break;
            case 2: scan_pheno_kernel<C, 2><<<nblk, 64 * SCAN_WPB, 0, ctx->stream>>>(pr, pl.Y, pl.ldy, pl.tcn, pl.xbuf); break;
            case 4: scan_pheno_kernel<C, 4><<<nblk, 64 * SCAN_WPB, 0, ctx->stream>>>(pr, pl.Y, pl.ldy, pl.tcn, pl.xbuf); break;
            case 8: scan_pheno_kernel<C, 8><<<nblk, 64 * SCAN_WPB, 0, ctx->stream>>>(pr, pl.Y, pl.ldy, pl.tcn, pl.xbuf); break;
            default: set_error("assoc_pheno: chunk width %d", pl.tpad); return PG_EINVAL;
        }
    } else {
        const size_t lds = (size_t)WPB * assoc_per_wave_bytes(Shape<C>::M, Shape<C>::SWEEP_LDS, Shape<C>::SAV_SLOTS, sizeof(EvalOut), pr.n_vals);
        PG_REQUIRE(pr.n_vals >= 0 && lds <= 160 * 1024, "assoc_pheno: c = %d, n_vals = %d need %zu bytes of LDS per workgroup", C, pr.n_vals, lds);
        if (lds > 64 * 1024)
            PG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&assoc_kernel<C, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        const long long nblk = (pr.p + WPB - 1) / WPB;
        assoc_kernel<C, false, true><<<dim3((unsigned)nblk), 64 * WPB, lds, ctx->stream>>>(pr);
    }
    PG_HIP(hipGetLastError());
    return PG_OK;
}


// The association kernel is instantiated per covariate count (and once more with the LRT search, N2); the instantiations
// are split over translation units so that they compile in parallel:
//   assoc.hip          c = 1..15            assoc_hi.hip      c = 16..PG_MAX_COVARIATES
//   assoc_lrt.hip      LRT, c = 0..15       assoc_lrt_hi.hip  LRT, c = 16..PG_MAX_COVARIATES
// (c = 0 exists for the LRT's null model at c = 1: the covariates alone, run as "c - 1 covariates + the last one as the SNP").
int launch_assoc_hi(pg_ctx *ctx, AssocParams &pr);
int launch_assoc_lrt(pg_ctx *ctx, AssocParams &pr);
int launch_assoc_lrt_hi(pg_ctx *ctx, AssocParams &pr);
//   assoc_pheno.hip    multi-phenotype kernels (pg_assoc_pheno_dev), c = 1..15     assoc_pheno_hi.hip  c = 16..PG_MAX_COVARIATES
int launch_assoc_pheno(pg_ctx *ctx, AssocParams &pr, const PhenoLaunch &pl);
int launch_assoc_pheno_hi(pg_ctx *ctx, AssocParams &pr, const PhenoLaunch &pl);
//   assoc_gxe.hip      GxE kernels (pg_assoc_gxe_dev), shared c = 1..15            assoc_gxe_hi.hip    c = 16..PG_MAX_COVARIATES - 1
int launch_assoc_gxe(pg_ctx *ctx, AssocParams &pr, const float *xer, long long ldxe);
int launch_assoc_gxe_hi(pg_ctx *ctx, AssocParams &pr, const float *xer, long long ldxe);
#define PG_CASE(CC) case CC: return launch_assoc<CC, PG_CASE_LRT>(ctx, pr);
#define PG_PCASE(CC) case CC: return launch_pheno<CC>(ctx, pr, pl);
#define PG_GCASE(CC) case CC: return launch_gxe<CC>(ctx, pr, xer, ldxe);
#if defined(PG_ASSOC_PART) && PG_ASSOC_PART == 6
int launch_assoc_gxe(pg_ctx *ctx, AssocParams &pr, const float *xer, long long ldxe)
{
    switch (pr.c) {
        PG_GCASE(1) PG_GCASE(2) PG_GCASE(3) PG_GCASE(4) PG_GCASE(5) PG_GCASE(6) PG_GCASE(7) PG_GCASE(8) PG_GCASE(9) PG_GCASE(10)
        PG_GCASE(11) PG_GCASE(12) PG_GCASE(13) PG_GCASE(14) PG_GCASE(15)
        default: return launch_assoc_gxe_hi(ctx, pr, xer, ldxe);
    }
}
// Ue[i, k] = e_i U[i, k] (one f32 rounding): U'(e o x) = (diag(e) U)' x, so every rotation path of x gives x o e from Ue
__global__ __launch_bounds__(256) void gxe_scale_u_kernel(long long n, const float *U, long long ldU, const float *e, float *Ue)
{
    const long long i = blockIdx.y, k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && k < n) Ue[i * n + k] = __fmul_rn(e[i], U[i * ldU + k]);
}
extern "C" int pg_gxe_scale_u_dev(pg_ctx *ctx, int64_t n, const float *U, int64_t ldU, const float *e, float *Ue)
{
    PG_REQUIRE(ctx && U && e && Ue, "pg_gxe_scale_u_dev: NULL argument");
    PG_REQUIRE(n >= 1 && n < (1LL << 30) && ldU >= n, "pg_gxe_scale_u_dev: bad shape n=%lld ldU=%lld", (long long)n, (long long)ldU);
    PG_HIP(hipSetDevice(ctx->device));
    gxe_scale_u_kernel<<<dim3((unsigned)((n + 255) / 256), (unsigned)n), 256, 0, ctx->stream>>>(n, U, ldU, e, Ue);
    PG_HIP(hipGetLastError());
    return PG_OK;
}
#elif defined(PG_ASSOC_PART) && PG_ASSOC_PART == 7
int launch_assoc_gxe_hi(pg_ctx *ctx, AssocParams &pr, const float *xer, long long ldxe)
{
    switch (pr.c) {
        PG_GCASE(16) PG_GCASE(17) PG_GCASE(18) PG_GCASE(19) PG_GCASE(20) PG_GCASE(21) PG_GCASE(22) PG_GCASE(23) PG_GCASE(24) PG_GCASE(25)
        PG_GCASE(26) PG_GCASE(27) PG_GCASE(28) PG_GCASE(29)
        default: return PG_ENOTSUP;
    }
}
#elif defined(PG_ASSOC_PART) && PG_ASSOC_PART == 4
int launch_assoc_pheno(pg_ctx *ctx, AssocParams &pr, const PhenoLaunch &pl)
{
    switch (pr.c) {
        PG_PCASE(1) PG_PCASE(2) PG_PCASE(3) PG_PCASE(4) PG_PCASE(5) PG_PCASE(6) PG_PCASE(7) PG_PCASE(8) PG_PCASE(9) PG_PCASE(10)
        PG_PCASE(11) PG_PCASE(12) PG_PCASE(13) PG_PCASE(14) PG_PCASE(15)
        default: return launch_assoc_pheno_hi(ctx, pr, pl);
    }
}
#elif defined(PG_ASSOC_PART) && PG_ASSOC_PART == 5
int launch_assoc_pheno_hi(pg_ctx *ctx, AssocParams &pr, const PhenoLaunch &pl)
{
    switch (pr.c) {
        PG_PCASE(16) PG_PCASE(17) PG_PCASE(18) PG_PCASE(19) PG_PCASE(20) PG_PCASE(21) PG_PCASE(22) PG_PCASE(23) PG_PCASE(24) PG_PCASE(25)
        PG_PCASE(26) PG_PCASE(27) PG_PCASE(28) PG_PCASE(29) PG_PCASE(30)
        default: return PG_ENOTSUP;
    }
}
#elif defined(PG_ASSOC_PART) && PG_ASSOC_PART == 1
#define PG_CASE_LRT false
int launch_assoc_hi(pg_ctx *ctx, AssocParams &pr)
{
    switch (pr.c) {
        PG_CASE(16) PG_CASE(17) PG_CASE(18) PG_CASE(19) PG_CASE(20) PG_CASE(21) PG_CASE(22) PG_CASE(23) PG_CASE(24) PG_CASE(25)
        PG_CASE(26) PG_CASE(27) PG_CASE(28) PG_CASE(29) PG_CASE(30)
        default: return PG_ENOTSUP;
    }
}
#elif defined(PG_ASSOC_PART) && PG_ASSOC_PART == 2
#define PG_CASE_LRT true
int launch_assoc_lrt(pg_ctx *ctx, AssocParams &pr)
{
    switch (pr.c) {
        PG_CASE(0) PG_CASE(1) PG_CASE(2) PG_CASE(3) PG_CASE(4) PG_CASE(5) PG_CASE(6) PG_CASE(7) PG_CASE(8) PG_CASE(9) PG_CASE(10)
        PG_CASE(11) PG_CASE(12) PG_CASE(13) PG_CASE(14) PG_CASE(15)
        default: return launch_assoc_lrt_hi(ctx, pr);
    }
}
#elif defined(PG_ASSOC_PART) && PG_ASSOC_PART == 3
#define PG_CASE_LRT true
int launch_assoc_lrt_hi(pg_ctx *ctx, AssocParams &pr)
{
    switch (pr.c) {
        PG_CASE(16) PG_CASE(17) PG_CASE(18) PG_CASE(19) PG_CASE(20) PG_CASE(21) PG_CASE(22) PG_CASE(23) PG_CASE(24) PG_CASE(25)
        PG_CASE(26) PG_CASE(27) PG_CASE(28) PG_CASE(29) PG_CASE(30)
        default: return PG_ENOTSUP;
    }
}
#else
#define PG_CASE_LRT false
static int launch_assoc_any(pg_ctx *ctx, AssocParams &pr)
{
    if (pr.lrt) return launch_assoc_lrt(ctx, pr);
    switch (pr.c) {
#ifdef PG_ONLY_C
        PG_CASE(PG_ONLY_C)
#else
        PG_CASE(1) PG_CASE(2) PG_CASE(3) PG_CASE(4) PG_CASE(5) PG_CASE(6) PG_CASE(7) PG_CASE(8) PG_CASE(9) PG_CASE(10)
        PG_CASE(11) PG_CASE(12) PG_CASE(13) PG_CASE(14) PG_CASE(15)
#endif
        default: return launch_assoc_hi(ctx, pr);
    }
}
#ifdef PG_ONLY_C   // single-c development builds (A/B timing): the LRT pair c, c-1 in this translation unit, nothing else
#undef PG_CASE_LRT
#define PG_CASE_LRT true
int launch_assoc_lrt(pg_ctx *ctx, AssocParams &pr)
{
    switch (pr.c) { PG_CASE(PG_ONLY_C) case PG_ONLY_C - 1: return launch_assoc<PG_ONLY_C - 1, true>(ctx, pr); default: return PG_ENOTSUP; }
}
int launch_assoc_hi(pg_ctx *, AssocParams &) { return PG_ENOTSUP; }
int launch_assoc_pheno(pg_ctx *, AssocParams &, const PhenoLaunch &) { return PG_ENOTSUP; }
#endif
#endif
#undef PG_CASE
#undef PG_PCASE
#undef PG_GCASE

#ifndef PG_ASSOC_PART
// ------------------------------------------------------------------------------------------------
// scipy.stats.f.sf(F, 1, dfd) (lmm.py:482): I_{w}(dfd/2, 1/2), w = dfd/(dfd+F) — same statements as
// oracle orc_fdist_sf (continued fraction, modified Lentz).
__device__ double betacf_dev(double a, double b, double x)
{
    const double FPMIN = 1e-300, EPS = 1e-16;
    double qab = a + b, qap = a + 1.0, qam = a - 1.0, c = 1.0, dd = 1.0 - qab * x / qap, h;
    if (fabs(dd) < FPMIN) dd = FPMIN;
    dd = 1.0 / dd; h = dd;
    for (int m = 1; m <= 2000; m++) {
        int m2 = 2 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        dd = 1.0 + aa * dd; if (fabs(dd) < FPMIN) dd = FPMIN;
        c = 1.0 + aa / c; if (fabs(c) < FPMIN) c = FPMIN;
        dd = 1.0 / dd; h *= dd * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        dd = 1.0 + aa * dd; if (fabs(dd) < FPMIN) dd = FPMIN;
        c = 1.0 + aa / c; if (fabs(c) < FPMIN) c = FPMIN;
        dd = 1.0 / dd;
        double del = dd * c;
        h *= del;
        if (fabs(del - 1.0) < EPS) break;
    }
    return h;
}
__global__ void fdist_sf_kernel(long long count, const double *F, double dfd, double *pval)
{
    long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= count) return;
    double f = F[g], r;
    if (f != f) r = f;
    else if (f <= 0.0) r = 1.0;
    else if (isinf(f)) r = 0.0;
    else {
        double a = 0.5 * dfd, b = 0.5;
        double x = dfd / (dfd + f), omx = 1.0 - x;
        double lbeta = lgamma(a) + lgamma(b) - lgamma(a + b);
        double lbt = a * log(x) + b * log(omx) - lbeta;
        if (x < (a + 1.0) / (a + b + 2.0)) r = exp(lbt) * betacf_dev(a, b, x) / a;
        else r = 1.0 - exp(lbt) * betacf_dev(b, a, omx) / b;
    }
    pval[g] = r;
}

// packed fixed rows: d, w_0..w_{c-1}, y, zero pad; rows [n, npad) zero
__global__ void build_fixed_kernel(int n, int npad, int c, int ldw, int rowf, const float *d, const float *Wr, const float *yr, float *fixed)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npad) return;
    float *row = fixed + (size_t)i * rowf;
    for (int k = 0; k < rowf; k++) row[k] = 0.0f;
    if (i >= n) row[0] = INFINITY;      // h = 1/(lam*inf + 1) = 0: pad elements contribute exact zeros without any select
    if (i < n) {
        row[0] = d[i];
        for (int j = 0; j < c; j++) row[1 + j] = Wr[(size_t)i * ldw + j];
        row[c + 1] = yr[i];
    }
}

// (n x p row-major) -> SNP-major (p x ldx), 32x32 LDS tile transpose, pad zeroed
__global__ __launch_bounds__(256) void transpose_kernel(long long n, long long p, const float *X, long long ldX, float *Xr, long long ldx)
{
    __shared__ float tile[32][33];
    const long long g0 = (long long)blockIdx.x * 32, i0 = (long long)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        long long i = i0 + r, g = g0 + tx;
        tile[r][tx] = (i < n && g < p) ? X[(size_t)i * ldX + g] : 0.0f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        long long g = g0 + r, i = i0 + tx;
        if (g < p && i < ldx) Xr[(size_t)g * ldx + i] = tile[tx][r];
    }
}

// ------------------------------------------------------------------------------------------------
// Inspection surface (the functions tests/test_pygemma.py:256-294 calls directly): precompute_mat (pyx:880) with
// every level exported, the *_overload scalars, newton.  One wavefront, any m = ctot+1 <= PG_MAX_COVARIATES + 2,
// written for checking, not for speed: level-0 Gram entries one at a time with exactly the arithmetic of
// gram_pass (per-lane fma chain over i = lane, lane+64, .., xor butterfly 1..32), then the sweeps run serially.
constexpr int IM = PG_MAX_COVARIATES + 2;

struct InspectParams {
    AssocParams pr;          // n, nu = n - ctot, logl_c, fixed = d (rowf = 1), the pairwise-sum plan
    int ctot, m, full;
    float lam, lam_min, lam_max;
    const float *d, *Wx, *y; // Wx: n x ctot row-major (the reference's np.c_[W, x]); y: n
    float *P3, *Q3, *R3;     // [m][m][m] indexed [row][level][col]; undefined entries NaN
    float *vecs;             // [5][m]: yt_Pi_y, yt_Pi_Pi_y, yt_Pi_Pi_Pi_y, tr_Pi, tr_Pi_Pi per level
    float *scal;             // logdet_Wt_H_inv_W, logdet_H, d1, d2 (full only), logL at the last level
    float *out;              // newton: the root
};

__device__ __forceinline__ float inspect_col(const InspectParams &ip, int j, int i)
{
    return (j < ip.ctot) ? ip.Wx[(size_t)i * ip.ctot + j] : ip.y[i];
}

// level-0 Grams into G[3][IM][IM] (lower triangles) + traces; all lanes hold the same values afterwards
__device__ void inspect_gram0(const InspectParams &ip, float lam, bool full, int lane, double (*G)[IM][IM], double *tr)
{
    const int n = ip.pr.n, m = ip.m;
    for (int j = 0; j < m; j++)
        for (int k = 0; k <= j; k++) {
            double P = 0.0, Q = 0.0, R = 0.0;
            for (int i = lane; i < n; i += 64) {
                const double hd = (double)hinv_f32(lam, ip.d[i]);
                const double cj = (double)inspect_col(ip, j, i), ck = (double)inspect_col(ip, k, i);
                const double aj = hd * cj, ak = hd * ck;
                P = fma(aj, ck, P);
                Q = fma(aj, ak, Q);
                if (full) { const double gj = (hd * hd) * cj; R = fma(gj, ak, R); }
            }
            P = bfly(P); Q = bfly(Q); R = bfly(R);
            if (lane == 0) { G[0][j][k] = P; G[1][j][k] = Q; G[2][j][k] = full ? R : 0.0; }
        }
    double s1 = 0.0, s2 = 0.0;
    for (int i = lane; i < n; i += 64) {
        const double hd = (double)hinv_f32(lam, ip.d[i]);
        s1 += hd;
        s2 = fma(hd, hd, s2);
    }
    s1 = bfly(s1); s2 = bfly(s2);
    if (lane == 0) { tr[0] = s1; tr[1] = full ? s2 : 0.0; }
    wave_lds_sync();
}

// the c_tot sweeps (pyx:947-963 / :1007-1036) on lane 0, statement for statement the oracle's sweeps(order=1);
// exp: optional export of every level.  Returns the last level's forms in o.
__device__ void inspect_sweeps(const InspectParams &ip, bool full, double (*G)[IM][IM], const double *tr, bool exp, EvalOut &o)
{
    const int m = ip.m;
    double (*P)[IM] = G[0], (*Q)[IM] = G[1], (*R)[IM] = G[2];
    double trP = tr[0], trPP = tr[1];
    float ld = 0.0f;
    P[0][0] = dmaxf(P[0][0], PG_MINV);
    auto level_out = [&](int lv) {
        if (!exp) return;
        for (int r = lv; r < m; r++)
            for (int c = lv; c <= r; c++) {
                const size_t idx = ((size_t)r * m + lv) * m + c;
                ip.P3[idx] = (float)P[r][c]; ip.Q3[idx] = (float)Q[r][c];
                if (full) ip.R3[idx] = (float)R[r][c];
            }
        ip.vecs[0 * m + lv] = (float)P[m - 1][m - 1];
        ip.vecs[1 * m + lv] = (float)Q[m - 1][m - 1];
        if (full) ip.vecs[2 * m + lv] = (float)R[m - 1][m - 1];
        ip.vecs[3 * m + lv] = (float)trP;
        ip.vecs[4 * m + lv] = (float)trPP;
    };
    level_out(0);
    for (int i = 1; i < m; i++) {
        const int q = i - 1;
        const double a = P[q][q], b = Q[q][q], e = R[q][q];
        double u[IM], v[IM], w[IM];
        for (int r = i; r < m; r++) { u[r] = P[r][q]; v[r] = Q[r][q]; w[r] = R[r][q]; }
        if (full) {
            const double ba = b / a;
            trPP = trPP + ba * ba - 2 * (e / a);
            const double a2 = a * a, a3 = a2 * a, b2 = b * b;
            const double cR = (e / a2) - (b2 / a3), ia = -1.0 / a, ba2 = b / a2;
            for (int r = i; r < m; r++)
                for (int c = i; c <= r; c++) {
                    const double t1 = fma(cR * u[c], u[r], R[r][c]);
                    double t2 = fma(ia * u[c], w[r], 0.0); t2 = fma(ia * w[c], u[r], t2);
                    const double t3 = fma(ia * v[c], v[r], 0.0);
                    double t4 = fma(ba2 * u[c], v[r], 0.0); t4 = fma(ba2 * v[c], u[r], t4);
                    R[r][c] = ((t1 + t2) + t3) + t4;
                }
            R[i][i] = dmaxf(R[i][i], PG_MINV);
        }
        trP = trP - b / a;
        {
            const double a2 = a * a, al1 = b / a2, ia = -1.0 / a;
            for (int r = i; r < m; r++)
                for (int c = i; c <= r; c++) {
                    const double t1 = fma(al1 * u[c], u[r], Q[r][c]);
                    double t2 = fma(ia * u[c], v[r], 0.0); t2 = fma(ia * v[c], u[r], t2);
                    Q[r][c] = t1 + t2;
                }
            Q[i][i] = dmaxf(Q[i][i], PG_MINV);
        }
        ld = (float)((double)ld + log(a));
        {
            const double ia = -1.0 / a;
            for (int r = i; r < m; r++)
                for (int c = i; c <= r; c++) P[r][c] = fma(ia * u[c], u[r], P[r][c]);
            P[i][i] = dmaxf(P[i][i], PG_MINV);
        }
        if (!full) trPP = 0.0;
        level_out(i);
    }
    o.yPy = (float)P[m - 1][m - 1]; o.yPPy = (float)Q[m - 1][m - 1]; o.yPPPy = (float)R[m - 1][m - 1];
    o.trP = (float)trP; o.trPP = (float)trPP; o.ld = ld;
    o.Pxx_c = (m >= 2) ? (float)P[m - 2][m - 2] : 0.0f; o.Pyx_c = (m >= 2) ? (float)P[m - 1][m - 2] : 0.0f;
}

__global__ __launch_bounds__(64) void precompute_kernel(InspectParams ip)
{
    __shared__ double G[3][IM][IM];
    __shared__ double tr[2];
    __shared__ EvalOut eo;
    extern __shared__ float vals_dyn[];
    const int lane = threadIdx.x, m = ip.m;
    for (int idx = lane; idx < m * m * m; idx += 64) { ip.P3[idx] = NAN; ip.Q3[idx] = NAN; ip.R3[idx] = NAN; }
    for (int idx = lane; idx < 5 * m; idx += 64) ip.vecs[idx] = NAN;
    for (int idx = lane; idx < 3 * IM * IM; idx += 64) (&G[0][0][0])[idx] = 0.0;
    wave_lds_sync();
    inspect_gram0(ip, ip.lam, ip.full != 0, lane, G, tr);
    if (lane == 0) inspect_sweeps(ip, ip.full != 0, G, tr, true, eo);
    wave_lds_sync();
    const float ldH = device_logdet_H(ip.pr, ip.lam, lane, vals_dyn);
    if (lane == 0) {
        ip.scal[0] = eo.ld; ip.scal[1] = ldH;
        ip.scal[2] = d1_f(ip.pr, ip.lam, eo.yPy, eo.yPPy, eo.trP);
        ip.scal[3] = ip.full ? d2_f(ip.pr, ip.lam, eo.yPy, eo.yPPy, eo.yPPPy, eo.trP, eo.trPP) : NAN;
        ip.scal[4] = logl_f(ip.pr, eo.yPy, ldH, eo.ld);
        ip.scal[5] = (float)tr[0];                          // sum h   (un-projected trace of H^-1: the ML functions, pyx:1567-1603)
        ip.scal[6] = ip.full ? (float)tr[1] : NAN;          // sum h^2
    }
}

__global__ __launch_bounds__(64) void newton_kernel(InspectParams ip)
{
    __shared__ double G[3][IM][IM];
    __shared__ double tr[2];
    __shared__ EvalOut eo;
    const int lane = threadIdx.x;
    const float root = newton_dev(ip.pr, ip.lam, ip.lam_min, ip.lam_max, [&](float lf, EvalOut &e) {
        for (int idx = lane; idx < 3 * IM * IM; idx += 64) (&G[0][0][0])[idx] = 0.0;
        wave_lds_sync();
        inspect_gram0(ip, lf, true, lane, G, tr);
        if (lane == 0) inspect_sweeps(ip, true, G, tr, false, eo);
        wave_lds_sync();
        e = eo;
        wave_lds_sync();
    });
    if (lane == 0) ip.out[0] = root;
}

// the three *_overload scalars on caller-supplied quadratic forms (pyx:1813, :1656, :1675); args: lam, yPy, yPPy, yPPPy,
// trP, trPP, logdet_H, logdet_Wt_H_inv_W
__global__ void reml_scalars_kernel(AssocParams pr, const float *a, float *out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    out[0] = logl_f(pr, a[1], a[6], a[7]);
    out[1] = d1_f(pr, a[0], a[1], a[2], a[4]);
    out[2] = d2_f(pr, a[0], a[1], a[2], a[3], a[4], a[5]);
}

}  // namespace pg

using namespace pg;

extern "C" int pg_fdist_sf_dev(pg_ctx *ctx, int64_t count, const double *F, double dfd, double *pval)
{
    PG_REQUIRE(ctx && F && pval && count >= 0, "pg_fdist_sf_dev: bad arguments");
    if (count == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    fdist_sf_kernel<<<(unsigned)((count + 255) / 256), 256, 0, ctx->stream>>>(count, F, dfd, pval);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

extern "C" int pg_transpose_dev(pg_ctx *ctx, int64_t n, int64_t p, const float *X, int64_t ldX, float *Xr, int64_t ldx)
{
    PG_REQUIRE(ctx && X && Xr && n > 0 && p > 0 && ldx >= n && ldX >= p, "pg_transpose_dev: bad arguments");
    PG_HIP(hipSetDevice(ctx->device));
    dim3 grid((unsigned)((p + 31) / 32), (unsigned)((ldx + 31) / 32));
    transpose_kernel<<<grid, 256, 0, ctx->stream>>>(n, p, X, ldX, Xr, ldx);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

// the SNP-independent scalars of the kernel parameters (shapes, decade lambdas, likelihood constants, the float32-sum plan)
static void fill_params(pg_ctx *ctx, int64_t n, int c, int grid, AssocParams &pr)
{
    pr.n = (int)n; pr.npad = (int)((n + 63) / 64 * 64); pr.c = c; pr.niter = pr.npad / 64;
    pr.nu = (int)(n - c - 1); pr.grid = grid ? 1 : 0; pr.rowf = ((c + 2 + 3) / 4) * 4;
    for (int k = -5; k <= 5; k++) pr.lam11[k + 5] = (float)pow(10.0, (double)(float)k);  // pyx:122,157-158
    {
        const int ctot = c + 1;
        float r = (float)((0.5 * (double)(n - ctot)) * std::log(0.5 * (double)(n - ctot) / M_PI));  // pyx:1821
        r = (float)((double)r - (0.5 * (double)(n - ctot)));                                          // pyx:1822
        pr.logl_c = r;
    }
    pr.nhalf = (int)(n / 2);                                                                          // (n/2): C integer division
    {
        float r = (float)((double)(n / 2) * std::log((double)n / (2.0 * M_PI)));                      // pyx:1552
        pr.ml_c = r - (float)(n / 2);                                                                 // pyx:1554
    }
    pr.leaf = ctx->plan.d_leaf; pr.node = ctx->plan.d_node; pr.level = ctx->plan.d_level; pr.chunk = ctx->plan.d_chunk;
    pr.n_leaf = ctx->plan.n_leaf; pr.n_level = ctx->plan.n_level; pr.n_chunk = ctx->plan.n_chunk;
    pr.n_vals = ctx->plan.n_leaf + ctx->plan.n_node;
}

// ctx->tabs of pg_assoc_dev / pg_assoc_lrt_dev: htab | fixg | t1tab | ldHtab | dtab | srow, each part 256-byte aligned or better
struct AssocTabs { size_t off_fixg, off_t1, off_ldh, off_dtab, off_srow, bytes; };
static AssocTabs assoc_tabs(int npad, int c)
{
    const int M = c + 2, NP = M * (M + 1) / 2;
    AssocTabs T{};
    T.off_fixg = up256((size_t)NLAM * npad * 4);
    T.off_t1 = T.off_fixg + (size_t)NLAM * 2 * NP * 8;
    T.off_ldh = T.off_t1 + NLAM * 8;
    T.off_dtab = up256(T.off_ldh + NLAM * 4);
    T.off_srow = up256(T.off_dtab + NLAM * assoc_dtab_doubles(c) * 8);
    T.bytes = T.off_srow + (assoc_scan_packed(c) ? (size_t)npad * assoc_srow_layout(c).rowf * 4 : 0) + 256;
    return T;
}

// fixed rows + tables + the kernel for one (covariates, SNP block); Wr is n x c with row stride ldw >= c (the LRT's null model
// passes the first c columns of a wider matrix)
static int assoc_run(pg_ctx *ctx, int64_t n, int c, int64_t p, const float *d, const float *Wr, int64_t ldw, const float *yr,
                     const float *Xr, int64_t ldx, int grid, float *beta, float *se, float *tau, float *lambda, double *F,
                     unsigned long long *stats_dev, bool lrt, float *lalt, float *lamalt)
{
    PG_HIP(hipSetDevice(ctx->device));
    int rc = build_npsum_plan(ctx, n);
    if (rc) return rc;

    AssocParams pr{};
    fill_params(ctx, n, c, grid, pr);
    pr.p = p; pr.ldx = ldx; pr.xr = Xr;
    rc = ensure(ctx, &ctx->fixed, &ctx->fixed_bytes, (size_t)pr.npad * pr.rowf * 4);
    if (rc) return rc;
    const AssocTabs T = assoc_tabs(pr.npad, c);
    rc = ensure(ctx, &ctx->tabs, &ctx->tabs_bytes, T.bytes);
    if (rc) return rc;
    if (!ctx->stats) PG_HIP(hipMalloc(&ctx->stats, 16));
    pr.fixed = (const float *)ctx->fixed;
    pr.htab = (float *)ctx->tabs;
    pr.fixg = (double *)((char *)ctx->tabs + T.off_fixg);
    pr.t1tab = (double *)((char *)ctx->tabs + T.off_t1);
    pr.ldHtab = (float *)((char *)ctx->tabs + T.off_ldh);
    pr.dtab = (double *)((char *)ctx->tabs + T.off_dtab);
    pr.srow = (float *)((char *)ctx->tabs + T.off_srow);
    pr.lrt = lrt ? 1 : 0;
    pr.lalt = lalt; pr.lamalt = lamalt;
    pr.beta = beta; pr.se = se; pr.tau = tau; pr.lam = lambda; pr.F = F;
    pr.stats = stats_dev;
    pr.trace = lrt ? nullptr : ctx->eval_trace;
    pr.passes = lrt ? nullptr : ctx->pass_stats;

    build_fixed_kernel<<<(pr.npad + 255) / 256, 256, 0, ctx->stream>>>(pr.n, pr.npad, c, (int)ldw, pr.rowf, d, Wr, yr, (float *)ctx->fixed);
    PG_HIP(hipGetLastError());
    return launch_assoc_any(ctx, pr);
}

extern "C" int pg_assoc_dev(pg_ctx *ctx, int64_t n, int c, int64_t p, const float *d, const float *Wr, const float *yr,
                            const float *Xr, int64_t ldx, int grid, float *beta, float *se, float *tau, float *lambda,
                            double *F, double *pval, unsigned long long *stats_dev)
{
    PG_REQUIRE(ctx && d && Wr && yr && Xr && beta && se && tau && lambda && F, "pg_assoc_dev: NULL argument");
    PG_REQUIRE(n >= 2 && n < (1LL << 30) && p >= 0 && ldx >= n, "pg_assoc_dev: bad shape n=%lld p=%lld ldx=%lld", (long long)n, (long long)p, (long long)ldx);
    if (c < 1 || c > PG_MAX_COVARIATES) {
        set_error("pg_assoc_dev: c=%d covariates not supported by this build (1..%d)", c, PG_MAX_COVARIATES);
        return PG_ENOTSUP;
    }
    PG_REQUIRE(n - c - 1 > 0, "pg_assoc_dev: n - c - 1 must be positive");
    if (p == 0) return PG_OK;
    int rc = assoc_run(ctx, n, c, p, d, Wr, c, yr, Xr, ldx, grid, beta, se, tau, lambda, F, stats_dev, false, nullptr, nullptr);
    if (rc) return rc;
    if (pval) return pg_fdist_sf_dev(ctx, p, F, (double)(n - c - 1), pval);
    return PG_OK;
}

// Everything of the first pg_assoc_dev / pg_assoc_lrt_dev call of a context that blocks the host — the float32-sum plan (built on the
// host, uploaded with synchronous copies after a stream drain) and the scratch allocations — done ahead of time, so that a streaming
// caller's first batch does not stall between its rotation and its association kernel (r4: 6 ms per worker at n = 10 000).
extern "C" int pg_assoc_warm(pg_ctx *ctx, int64_t n, int c)
{
    PG_REQUIRE(ctx && n >= 2 && n < (1LL << 30), "pg_assoc_warm: bad arguments");
    if (c < 1 || c > PG_MAX_COVARIATES) {
        set_error("pg_assoc_warm: c=%d covariates not supported by this build (1..%d)", c, PG_MAX_COVARIATES);
        return PG_ENOTSUP;
    }
    PG_HIP(hipSetDevice(ctx->device));
    int rc = build_npsum_plan(ctx, n);
    if (rc) return rc;
    const int npad = (int)((n + 63) / 64 * 64), rowf = ((c + 2 + 3) / 4) * 4;
    rc = ensure(ctx, &ctx->fixed, &ctx->fixed_bytes, (size_t)npad * rowf * 4);
    if (rc) return rc;
    rc = ensure(ctx, &ctx->tabs, &ctx->tabs_bytes, assoc_tabs(npad, c).bytes);
    if (rc) return rc;
    if (!ctx->stats) PG_HIP(hipMalloc(&ctx->stats, 16));
    return PG_OK;
}

// Work-per-SNP trace for tail analysis (the Brent/Newton path is data-dependent, pyx:1349-1416: up to 101 Newton iterations):
// the next pg_assoc_dev calls of this context write, per SNP, fast evaluations | full evaluations << 16 into trace_dev
// (>= p entries); NULL switches it off.
extern "C" int pg_assoc_set_eval_trace(pg_ctx *ctx, unsigned *trace_dev)
{
    PG_REQUIRE(ctx, "pg_assoc_set_eval_trace: NULL ctx");
    ctx->eval_trace = trace_dev;
    return PG_OK;
}

// Which Gram passes ran: the next pg_assoc_dev calls of this context add, over their SNPs, the passes over n that produced P, Q
// and R (a fused pass counts once for each power it produces; the decade scan is not counted) and the Newton starts that reused
// Brent's P and Q to dev4[0..3]; NULL switches it off.
extern "C" int pg_assoc_set_pass_stats(pg_ctx *ctx, unsigned long long *dev4)
{
    PG_REQUIRE(ctx, "pg_assoc_set_pass_stats: NULL ctx");
    ctx->pass_stats = dev4;
    return PG_OK;
}

#ifdef PG_ASSOC_STAMPS
extern "C" int pgx_assoc_stamps(long long *out4096)    // [1024 SNPs][entry, decade sweeps begin, end, exit] of the last pg_assoc_dev launch
{
    return hipMemcpyFromSymbol(out4096, HIP_SYMBOL(pg::g_assoc_stamps), sizeof(long long) * 4096) == hipSuccess ? 0 : -1;
}
#endif

// ---- several phenotypes over one SNP block: pg_assoc_dev's results for each, with the decade scan's y-free entries shared ----------
// Scratch of one call, in ctx->pheno: the fixed rows and fixg tables of a chunk of PHENO_CHUNK phenotypes, the phenotype-free tables
// (h at the decade lambdas, t1, log|H|), and the scan buffer of a tile of SNPs (bounded: at most 256 MiB unless one SNP is more).
struct PhenoLayout {
    int npad, rowf, NP, tpad_max;
    long long ptile;
    size_t off_htab, off_fixg, off_t1, off_ldh, off_xbuf, bytes;
};
static PhenoLayout pheno_layout(int64_t n, int c, int t, int64_t p)
{
    PhenoLayout L{};
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    L.npad = (int)((n + 63) / 64 * 64); L.rowf = ((c + 2 + 3) / 4) * 4; L.NP = (c + 2) * (c + 3) / 2;
    const int tc = t < PHENO_CHUNK ? t : PHENO_CHUNK;
    L.tpad_max = 1;
    while (L.tpad_max < tc) L.tpad_max <<= 1;
    const size_t per_snp = (size_t)NLAM * 2 * (c + 1 + L.tpad_max) * 8;
    const long long cap = (long long)((256u << 20) / per_snp);
    L.ptile = p < cap ? p : (cap < 1024 ? 1024 : cap);
    if (L.ptile > p) L.ptile = p;
    L.off_htab = up((size_t)PHENO_CHUNK * L.npad * L.rowf * 4);
    L.off_fixg = L.off_htab + up((size_t)NLAM * L.npad * 4);
    L.off_t1 = L.off_fixg + up((size_t)PHENO_CHUNK * NLAM * 2 * L.NP * 8);
    L.off_ldh = L.off_t1 + up(NLAM * 8);
    L.off_xbuf = L.off_ldh + up(NLAM * 4);
    L.bytes = L.off_xbuf + up((size_t)L.ptile * per_snp);
    return L;
}

extern "C" int pg_assoc_pheno_dev(pg_ctx *ctx, int64_t n, int c, int64_t p, int t, const float *d, const float *Wr,
                                  const float *Yr, int64_t ldy, const float *Xr, int64_t ldx, int grid,
                                  float *beta, float *se, float *tau, float *lambda, double *F, double *pval,
                                  unsigned long long *stats_dev)
{
    PG_REQUIRE(ctx && d && Wr && Yr && Xr && beta && se && tau && lambda && F, "pg_assoc_pheno_dev: NULL argument");
    PG_REQUIRE(n >= 2 && n < (1LL << 30) && p >= 0 && ldx >= n, "pg_assoc_pheno_dev: bad shape n=%lld p=%lld ldx=%lld",
               (long long)n, (long long)p, (long long)ldx);
    if (c < 1 || c > PG_MAX_COVARIATES) {
        set_error("pg_assoc_pheno_dev: c=%d covariates not supported by this build (1..%d)", c, PG_MAX_COVARIATES);
        return PG_ENOTSUP;
    }
    PG_REQUIRE(n - c - 1 > 0, "pg_assoc_pheno_dev: n - c - 1 must be positive");
    PG_REQUIRE(t >= 1 && ldy >= n, "pg_assoc_pheno_dev: bad phenotypes t=%d ldy=%lld (n=%lld)", t, (long long)ldy, (long long)n);
    if (p == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    int rc = build_npsum_plan(ctx, n);
    if (rc) return rc;
    const PhenoLayout L = pheno_layout(n, c, t, p);
    rc = ensure(ctx, &ctx->pheno, &ctx->pheno_bytes, L.bytes);
    if (rc) return rc;
    char *base = (char *)ctx->pheno;
    float *fixed = (float *)base;
    double *fixg = (double *)(base + L.off_fixg), *xbuf = (double *)(base + L.off_xbuf);

    AssocParams pr{};
    fill_params(ctx, n, c, grid, pr);
    pr.ldx = ldx;
    pr.htab = (float *)(base + L.off_htab);
    pr.t1tab = (double *)(base + L.off_t1);
    pr.ldHtab = (float *)(base + L.off_ldh);
    pr.stats = stats_dev;
    const size_t fixed_stride = (size_t)L.npad * L.rowf, fixg_stride = (size_t)NLAM * 2 * L.NP;
    for (int k0 = 0; k0 < t; k0 += PHENO_CHUNK) {
        const int tcn = (t - k0) < PHENO_CHUNK ? (t - k0) : PHENO_CHUNK;
        int tpad = 1;
        while (tpad < tcn) tpad <<= 1;
        // per phenotype: its fixed rows [d, W, y_k] and its W,y Gram entries at the decade lambdas (the h, t1 and log|H| tables the
        // setups write are the same for every phenotype)
        for (int j = 0; j < tcn; j++) {
            pr.fixed = fixed + j * fixed_stride;
            pr.fixg = fixg + j * fixg_stride;
            build_fixed_kernel<<<(L.npad + 255) / 256, 256, 0, ctx->stream>>>(pr.n, L.npad, c, c, L.rowf, d, Wr, Yr + (size_t)(k0 + j) * ldy,
                                                                             (float *)pr.fixed);
            PG_HIP(hipGetLastError());
            rc = launch_assoc_pheno(ctx, pr, PhenoLaunch{PhenoLaunch::SETUP, nullptr, 0, 0, 0, nullptr});
            if (rc) return rc;
        }
        pr.xe = c + 1 + tpad; pr.xbuf = xbuf;
        for (int64_t s0 = 0; s0 < p; s0 += L.ptile) {
            pr.p = (p - s0) < L.ptile ? (p - s0) : L.ptile;
            pr.xr = Xr + (size_t)s0 * ldx;
            rc = launch_assoc_pheno(ctx, pr, PhenoLaunch{PhenoLaunch::SCAN, Yr + (size_t)k0 * ldy, ldy, tcn, tpad, xbuf});
            if (rc) return rc;
            for (int j = 0; j < tcn; j++) {
                const size_t o = (size_t)(k0 + j) * p + s0;
                pr.fixed = fixed + j * fixed_stride; pr.fixg = fixg + j * fixg_stride; pr.xcol = c + 1 + j;
                pr.beta = beta + o; pr.se = se + o; pr.tau = tau + o; pr.lam = lambda + o; pr.F = F + o;
                rc = launch_assoc_pheno(ctx, pr, PhenoLaunch{PhenoLaunch::SEARCH, nullptr, 0, tcn, tpad, xbuf});
                if (rc) return rc;
            }
        }
    }
    if (pval) return pg_fdist_sf_dev(ctx, (int64_t)t * p, F, (double)(n - c - 1), pval);
    return PG_OK;
}

// pg_assoc_warm for pg_assoc_pheno_dev: the float32-sum plan and the scratch of a call with t phenotypes over up to p SNPs
extern "C" int pg_assoc_pheno_warm(pg_ctx *ctx, int64_t n, int c, int t, int64_t p)
{
    PG_REQUIRE(ctx && n >= 2 && n < (1LL << 30) && t >= 1 && p >= 1, "pg_assoc_pheno_warm: bad arguments");
    if (c < 1 || c > PG_MAX_COVARIATES) {
        set_error("pg_assoc_pheno_warm: c=%d covariates not supported by this build (1..%d)", c, PG_MAX_COVARIATES);
        return PG_ENOTSUP;
    }
    PG_HIP(hipSetDevice(ctx->device));
    int rc = build_npsum_plan(ctx, n);
    if (rc) return rc;
    return ensure(ctx, &ctx->pheno, &ctx->pheno_bytes, pheno_layout(n, c, t, p).bytes);
}

// ---- GxE: the Wald test of x o e with x among the covariates (assoc_gxe_kernel).  c shared covariates Wr (n x c: W and e in the
// eigenbasis), per SNP the rotated x (row stride ldx) and x o e (ldxe); p-values from F(1, n - c - 2).
extern "C" int pg_assoc_gxe_dev(pg_ctx *ctx, int64_t n, int c, int64_t p, const float *d, const float *Wr, const float *yr,
                                const float *xr, int64_t ldx, const float *xer, int64_t ldxe, float *beta, float *se, float *tau,
                                float *lambda, double *F, double *pval, unsigned long long *stats_dev)
{
    PG_REQUIRE(ctx && d && Wr && yr && xr && xer && beta && se && tau && lambda && F, "pg_assoc_gxe_dev: NULL argument");
    PG_REQUIRE(n >= 2 && n < (1LL << 30) && p >= 0 && ldx >= n && ldxe >= n, "pg_assoc_gxe_dev: bad shape n=%lld p=%lld ldx=%lld ldxe=%lld",
               (long long)n, (long long)p, (long long)ldx, (long long)ldxe);
    if (c < 1 || c + 1 > PG_MAX_COVARIATES) {
        set_error("pg_assoc_gxe_dev: c=%d shared covariates not supported by this build (1..%d)", c, PG_MAX_COVARIATES - 1);
        return PG_ENOTSUP;
    }
    PG_REQUIRE(n - c - 2 > 0, "pg_assoc_gxe_dev: n - c - 2 must be positive");
    if (p == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    int rc = build_npsum_plan(ctx, n);
    if (rc) return rc;
    AssocParams pr{};
    fill_params(ctx, n, c + 1, 0, pr);                 // the full model: c + 1 covariates (nu = n - c - 2, the likelihood constants)
    pr.c = c; pr.rowf = ((c + 2 + 3) / 4) * 4;         // ... over the fixed rows [d, W', y] of the c shared ones
    pr.p = p; pr.ldx = ldx; pr.xr = xr;
    const int NP = (c + 2) * (c + 3) / 2;
    rc = ensure(ctx, &ctx->fixed, &ctx->fixed_bytes, (size_t)pr.npad * pr.rowf * 4);
    if (rc) return rc;
    const size_t off_fixg = ((size_t)NLAM * pr.npad * 4 + 255) & ~(size_t)255;
    const size_t off_t1 = off_fixg + (size_t)NLAM * 2 * NP * 8;
    const size_t off_ldh = off_t1 + NLAM * 8;
    rc = ensure(ctx, &ctx->tabs, &ctx->tabs_bytes, off_ldh + NLAM * 4 + 256);
    if (rc) return rc;
    pr.fixed = (const float *)ctx->fixed;
    pr.htab = (float *)ctx->tabs;
    pr.fixg = (double *)((char *)ctx->tabs + off_fixg);
    pr.t1tab = (double *)((char *)ctx->tabs + off_t1);
    pr.ldHtab = (float *)((char *)ctx->tabs + off_ldh);
    pr.beta = beta; pr.se = se; pr.tau = tau; pr.lam = lambda; pr.F = F;
    pr.stats = stats_dev;
    build_fixed_kernel<<<(pr.npad + 255) / 256, 256, 0, ctx->stream>>>(pr.n, pr.npad, c, c, pr.rowf, d, Wr, yr, (float *)ctx->fixed);
    PG_HIP(hipGetLastError());
    rc = launch_assoc_gxe(ctx, pr, xer, ldxe);
    if (rc) return rc;
    if (pval) return pg_fdist_sf_dev(ctx, p, F, (double)(n - c - 2), pval);
    return PG_OK;
}

// pg_assoc_warm for pg_assoc_gxe_dev (the fixed rows and tables have the shape of c shared covariates)
extern "C" int pg_assoc_gxe_warm(pg_ctx *ctx, int64_t n, int c)
{
    PG_REQUIRE(ctx && n >= 2 && n < (1LL << 30), "pg_assoc_gxe_warm: bad arguments");
    if (c < 1 || c + 1 > PG_MAX_COVARIATES) {
        set_error("pg_assoc_gxe_warm: c=%d shared covariates not supported by this build (1..%d)", c, PG_MAX_COVARIATES - 1);
        return PG_ENOTSUP;
    }
    return pg_assoc_warm(ctx, n, c);
}

namespace pg {
__global__ void gather_col_kernel(int n, int npad, const float *W, int ldw, int col, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < npad) out[i] = (i < n) ? W[(size_t)i * ldw + col] : 0.0f;
}
// D_lrt = 2 (l_alt - l_null) on float32 scalars (lmm/lmm.py:283), p_lrt = chi2(1).sf(D_lrt) = erfc(sqrt(D/2)) (lmm.py:300 writes
// 1 - cdf: the same number above ~1e-16); all four columns widened to float64 like the frame's lambda column
__global__ void lrt_finish_kernel(long long p, const float *lalt, const float *lnull, double *o_lalt, double *o_lnull, double *o_D, double *o_p)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= p) return;
    const float la = lalt[g], ln = lnull[0];
    const float D = __fmul_rn(2.0f, __fsub_rn(la, ln));
    const double Dd = (double)D;
    o_lalt[g] = (double)la; o_lnull[g] = (double)ln; o_D[g] = Dd;
    o_p[g] = (Dd != Dd) ? Dd : (Dd <= 0.0 ? 1.0 : erfc(sqrt(0.5 * Dd)));
}
}  // namespace pg

// ---- N2: pg_assoc_dev plus the likelihood-ratio columns the reference sketches and leaves commented out
// (lmm/lmm.py:137-141, 277-300) from its own ML functions (calc_lambda lmm.py:22-84; likelihood_lambda and derivatives
// pygemma_model.pyx:1542-1603).  Same kernel, instantiated with the ML lambda search appended: the decade scan is shared with the
// REML search (its quadratic forms serve both), roots are refined by brentq + Newton like the reference's scipy calls.
// l_null comes from the same kernel run on the covariates alone (c - 1 covariates + the last one in the SNP's place).
extern "C" int pg_assoc_lrt_dev(pg_ctx *ctx, int64_t n, int c, int64_t p, const float *d, const float *Wr, const float *yr,
                                const float *Xr, int64_t ldx, int grid, float *beta, float *se, float *tau, float *lambda,
                                double *F, double *pval, double *l_alt, double *l_null, double *D_lrt, double *p_lrt)
{
    PG_REQUIRE(ctx && d && Wr && yr && Xr && beta && se && tau && lambda && F && l_alt && l_null && D_lrt && p_lrt, "pg_assoc_lrt_dev: NULL argument");
    PG_REQUIRE(n >= 2 && n < (1LL << 30) && p >= 0 && ldx >= n, "pg_assoc_lrt_dev: bad shape");
    if (c < 1 || c > PG_MAX_COVARIATES) {
        set_error("pg_assoc_lrt_dev: c=%d covariates not supported by this build (1..%d)", c, PG_MAX_COVARIATES);
        return PG_ENOTSUP;
    }
    PG_REQUIRE(n - c - 1 > 0, "pg_assoc_lrt_dev: n - c - 1 must be positive");
    if (p == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    const int64_t npad = (n + 63) / 64 * 64;
    // scratch: [x_null (npad f32) | null outputs: 4 f32 + 1 f64 | l_null f32 | lam_null f32 | l_alt (p f32) | lam_alt (p f32)]
    const size_t off_out = (size_t)npad * 4, off_la = off_out + 64, need = off_la + (size_t)p * 8 + 64;
    int rc = ensure(ctx, &ctx->scratch, &ctx->scratch_bytes, need);
    if (rc) return rc;
    char *sc = (char *)ctx->scratch;
    float *xnull = (float *)sc, *nb = (float *)(sc + off_out), *lnull = nb + 8, *lamnull = nb + 9;
    double *nF = (double *)(sc + off_out + 16);
    float *lalt = (float *)(sc + off_la), *lamalt = lalt + p;
    gather_col_kernel<<<(unsigned)((npad + 255) / 256), 256, 0, ctx->stream>>>((int)n, (int)npad, Wr, c, c - 1, xnull);
    PG_HIP(hipGetLastError());
    rc = assoc_run(ctx, n, c - 1, 1, d, Wr, c, yr, xnull, npad, grid, nb, nb + 1, nb + 2, nb + 3, nF, nullptr, true, lnull, lamnull);
    if (rc) return rc;
    rc = assoc_run(ctx, n, c, p, d, Wr, c, yr, Xr, ldx, grid, beta, se, tau, lambda, F, nullptr, true, lalt, lamalt);
    if (rc) return rc;
    lrt_finish_kernel<<<(unsigned)((p + 255) / 256), 256, 0, ctx->stream>>>(p, lalt, lnull, l_alt, l_null, D_lrt, p_lrt);
    PG_HIP(hipGetLastError());
    if (pval) return pg_fdist_sf_dev(ctx, p, F, (double)(n - c - 1), pval);
    return PG_OK;
}

// ---- the score test's null model (score.hip): lambda0 = the ML lambda of y ~ W, calc_lambda(eigenVals, Y, W) (lmm/lmm.py:22-84).
// It is pg_assoc_lrt_dev's null search: c - 1 covariates with the last one in the SNP's place, the ML search appended; its
// lambda lands in lambda0_dev (one float32, device).
extern "C" int pg_score_null_dev(pg_ctx *ctx, int64_t n, int c, const float *d, const float *Wr, const float *yr, float *lambda0_dev)
{
    PG_REQUIRE(ctx && d && Wr && yr && lambda0_dev, "pg_score_null_dev: NULL argument");
    PG_REQUIRE(n >= 2 && n < (1LL << 30), "pg_score_null_dev: bad shape n=%lld", (long long)n);
    if (c < 1 || c > PG_MAX_COVARIATES) {
        set_error("pg_score_null_dev: c=%d covariates not supported by this build (1..%d)", c, PG_MAX_COVARIATES);
        return PG_ENOTSUP;
    }
    PG_REQUIRE(n - c - 1 > 0, "pg_score_null_dev: n - c - 1 must be positive");
    PG_HIP(hipSetDevice(ctx->device));
    const int64_t npad = (n + 63) / 64 * 64;
    // scratch: [x_null (npad f32) | outputs of the one-SNP run: 4 f32 + 1 f64 | its log-likelihood f32]
    const size_t off_out = (size_t)npad * 4;
    int rc = ensure(ctx, &ctx->scratch, &ctx->scratch_bytes, off_out + 64);
    if (rc) return rc;
    char *sc = (char *)ctx->scratch;
    float *xnull = (float *)sc, *nb = (float *)(sc + off_out), *lnull = nb + 8;
    double *nF = (double *)(sc + off_out + 16);
    gather_col_kernel<<<(unsigned)((npad + 255) / 256), 256, 0, ctx->stream>>>((int)n, (int)npad, Wr, c, c - 1, xnull);
    PG_HIP(hipGetLastError());
    return assoc_run(ctx, n, c - 1, 1, d, Wr, c, yr, xnull, npad, 0, nb, nb + 1, nb + 2, nb + 3, nF, nullptr, true, lnull, lambda0_dev);
}

// ---- inspection surface ----------------------------------------------------------------------------------------------
static int inspect_params(pg_ctx *ctx, int64_t n, int ctot, InspectParams &ip, const float *d)
{
    PG_REQUIRE(n >= 2 && n < (1LL << 30), "inspect: bad n");
    if (ctot < 1 || ctot > PG_MAX_COVARIATES + 1) {
        set_error("inspect: %d columns not supported by this build (1..%d)", ctot, PG_MAX_COVARIATES + 1);
        return PG_ENOTSUP;
    }
    PG_REQUIRE(n - ctot > 0, "inspect: n - c must be positive");
    PG_HIP(hipSetDevice(ctx->device));
    int rc = build_npsum_plan(ctx, n);
    if (rc) return rc;
    AssocParams &pr = ip.pr;
    pr.n = (int)n; pr.npad = (int)((n + 63) / 64 * 64); pr.c = ctot - 1; pr.niter = pr.npad / 64;
    pr.nu = (int)(n - ctot); pr.rowf = 1; pr.fixed = d;
    {
        float r = (float)((0.5 * (double)(n - ctot)) * std::log(0.5 * (double)(n - ctot) / M_PI));  // pyx:1821
        r = (float)((double)r - (0.5 * (double)(n - ctot)));                                          // pyx:1822
        pr.logl_c = r;
    }
    pr.leaf = ctx->plan.d_leaf; pr.node = ctx->plan.d_node; pr.level = ctx->plan.d_level; pr.chunk = ctx->plan.d_chunk;
    pr.n_leaf = ctx->plan.n_leaf; pr.n_level = ctx->plan.n_level; pr.n_chunk = ctx->plan.n_chunk;
    pr.n_vals = ctx->plan.n_leaf + ctx->plan.n_node;
    ip.ctot = ctot; ip.m = ctot + 1; ip.d = d;
    return PG_OK;
}

extern "C" int pg_precompute_mat_dev(pg_ctx *ctx, int64_t n, int ctot, float lam, const float *d, const float *Wx, const float *y,
                                     int full, float *P3, float *Q3, float *R3, float *vecs, float *scal)
{
    PG_REQUIRE(ctx && d && Wx && y && P3 && Q3 && R3 && vecs && scal, "pg_precompute_mat_dev: NULL argument");
    InspectParams ip{};
    int rc = inspect_params(ctx, n, ctot, ip, d);
    if (rc) return rc;
    ip.full = full ? 1 : 0; ip.lam = lam; ip.Wx = Wx; ip.y = y;
    ip.P3 = P3; ip.Q3 = Q3; ip.R3 = R3; ip.vecs = vecs; ip.scal = scal;
    precompute_kernel<<<1, 64, (size_t)ip.pr.n_vals * 4 + 16, ctx->stream>>>(ip);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

extern "C" int pg_newton_dev(pg_ctx *ctx, int64_t n, int ctot, float lam, float lam_min, float lam_max, const float *d,
                             const float *Wx, const float *y, float *root)
{
    PG_REQUIRE(ctx && d && Wx && y && root, "pg_newton_dev: NULL argument");
    InspectParams ip{};
    int rc = inspect_params(ctx, n, ctot, ip, d);
    if (rc) return rc;
    ip.full = 1; ip.lam = lam; ip.lam_min = lam_min; ip.lam_max = lam_max; ip.Wx = Wx; ip.y = y; ip.out = root;
    newton_kernel<<<1, 64, 0, ctx->stream>>>(ip);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

extern "C" int pg_reml_scalars_dev(pg_ctx *ctx, int64_t n, int ctot, const float *args8, float *out3)
{
    PG_REQUIRE(ctx && args8 && out3 && n - ctot > 0, "pg_reml_scalars_dev: bad arguments");
    PG_HIP(hipSetDevice(ctx->device));
    AssocParams pr{};
    pr.n = (int)n; pr.nu = (int)(n - ctot);
    {
        float r = (float)((0.5 * (double)(n - ctot)) * std::log(0.5 * (double)(n - ctot) / M_PI));
        r = (float)((double)r - (0.5 * (double)(n - ctot)));
        pr.logl_c = r;
    }
    reml_scalars_kernel<<<1, 1, 0, ctx->stream>>>(pr, args8, out3);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

// N2 at the model level: likelihood_lambda (pyx:1542-1562), likelihood_derivative1_lambda (pyx:1567-1581),
// likelihood_derivative2_lambda (pyx:1586-1603) from the quadratic forms of precompute_mat — the statements the LRT kernel runs
__global__ void ml_scalars_kernel(AssocParams pr, const float *a, float *out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    out[0] = ml_logl_f(pr, a[1], a[6]);
    out[1] = ml_d1_f(pr, a[0], a[1], a[2], a[4]);
    out[2] = ml_d2_f(pr, a[0], a[1], a[2], a[3], a[4], a[5]);
}
extern "C" int pg_ml_scalars_dev(pg_ctx *ctx, int64_t n, const float *args7, float *out3)
{
    PG_REQUIRE(ctx && args7 && out3 && n >= 2 && n < (1LL << 30), "pg_ml_scalars_dev: bad arguments");
    PG_HIP(hipSetDevice(ctx->device));
    AssocParams pr{};
    pr.n = (int)n;
    pr.nhalf = (int)(n / 2);                                                     // (n/2): C integer division
    {
        float r = (float)((double)(n / 2) * std::log((double)n / (2.0 * M_PI)));  // pyx:1552
        pr.ml_c = r - (float)(n / 2);                                             // pyx:1554
    }
    ml_scalars_kernel<<<1, 1, 0, ctx->stream>>>(pr, args7, out3);
    PG_HIP(hipGetLastError());
    return PG_OK;
}
#else
}  // namespace pg
#endif  // PG_ASSOC_PART
