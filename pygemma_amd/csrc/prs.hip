// prs.hip — polygenic scores straight from raw genotypes (packed .bed records, 8-bit, float32 or float64 blocks, sample- or SNP-major):
// S = G W with G (n x pb) as stored and W (pb x t) fp64 weights, PLINK's --score.  The reduction runs over SNPs, not over samples, so
// the batches of a stream accumulate into one (t x n) result.
//
// Values are the ones the QC pass sees: an element is first rounded to float32; .bed code 01 and NaN / +-Inf are missing (an 8-bit block
// has no missing code).  A missing call is 0, or with impute the fp64 mean mu_g that pg_snp_stats_*_dev reports for its SNP — those
// kernels run as a pre-pass over the batch and the score kernel reads their moments — and every call of an all-missing SNP is 0.
// called[k][i] counts the SNPs with w_gk != 0 at which sample i is called: the product of the 0/1 call mask with [w != 0], exact in fp64.
//
// Both products run on v_mfma_f64_16x16x4_f64 with the SNPs as K, the weight columns as M and the samples as N:
//   A lane (r, q) = w[SNP][column 16 mt + r],  B lane (c, q) = x[SNP][sample 16 nt + c],  C lane (c, q) reg e = S[column 16 mt + q + 4 e][sample c].
// k is only a summation index, so inside a group of 16 SNPs lane (., q) takes the run 4 q .. 4 q + 3 (four adjacent weights of a column,
// four adjacent elements of a sample-major row) and MFMA step s multiplies SNP 4 q + s of A with SNP 4 q + s of B.
// Tiling: a wavefront owns 64 adjacent samples (four N-tiles: one dword of a .bed record each) and 16 or 32 weight columns (two M-tiles
// of scores, or one of scores and one of counts), a workgroup of four wavefronts 256 adjacent samples (64 bytes of every record);
// further columns are further rows of the grid.  Nothing goes through LDS: the genotypes are read as they are stored, the weights
// (8 t bytes per SNP) come from L2.
// Order of summation: the block's SNPs are cut into chunks of PG_PRS_CHUNK from its first SNP; a chunk's partial is one MFMA chain from
// zero (groups of 16 in order, steps 0..3, the four k-groups inside the instruction), and the partials are added to score in ascending
// chunk order by a second kernel over the partials that one workgroup per (chunk, 256 samples) left in the work area: split-K, no
// atomics.  (A workgroup that walks its chunks itself gives the same bits and was slower at every size measured)
#include "geno_src.hpp"

#include <cmath>
#include <type_traits>

namespace pg {

constexpr int PRS_NT = 4;                               // 16-sample N-tiles per wavefront
constexpr int PRS_WAVES = 4;
constexpr int PRS_ROWS = 16 * PRS_NT * PRS_WAVES;       // samples per workgroup
constexpr long long PRS_MAXPB = 1LL << 25;
constexpr long long PRS_MAXGRID = 1LL << 31;            // workgroups per launch, exclusive

typedef double prs_v4d __attribute__((ext_vector_type(4)));

struct PrsArgs {
    int n, t, count_a1;
    long long pb, ldX, ldw, lds, ldp, ngroups;
    const void *X;
    const double *Wt;
    const double *mom;         // the pre-pass's moments (mean of SNP g at mom[4 g]); NULL: no missing call is imputed
    double *score;
    long long *called;
    double *ps;                // chunk partials [chunk][t][ldp] of the scores ...
    int *pc;                   // ... and of the counts
};

static inline long long prs_chunks(long long pb) { return (pb + PG_PRS_CHUNK - 1) / PG_PRS_CHUNK; }
static inline long long prs_groups(long long n) { return (n + PRS_ROWS - 1) / PRS_ROWS; }

struct PrsWork {
    long long *counts;     // [pb][4] the pre-pass's outputs
    double *moments;       // [pb][4]
    void *ss;              // the pre-pass's own work area
    double *ps;            // [chunks][t][ldp]
    int *pc;               // [chunks][t][ldp]
    size_t bytes;
};

static PrsWork prs_work(void *work, long long n, long long pb, int t)
{
    char *b = static_cast<char *>(work);
    PrsWork w;
    size_t o = 0;
    w.counts = reinterpret_cast<long long *>(b + o); o += up256((size_t)pb * 32);
    w.moments = reinterpret_cast<double *>(b + o); o += up256((size_t)pb * 32);
    w.ss = b + o; o += up256(pg_snp_stats_work_bytes(n, pb));
    const size_t part = (size_t)prs_chunks(pb) * t * ((n + 15) / 16 * 16);
    w.ps = reinterpret_cast<double *>(b + o); o += up256(part * 8);
    w.pc = reinterpret_cast<int *>(b + o); o += up256(part * 4);
    w.bytes = o + 256;
    return w;
}

// the four SNPs g .. g + 3 of sample i as they are stored; it: the first sample of i's N-tile.  SNPs >= pb and samples >= n are not read
template <class T, int LAY> struct PrsRaw { T v[4]; };
template <class T> struct PrsRaw<T, GENO_BED> { unsigned w[4]; };      // the N-tile's 16 two-bit calls of each SNP

template <class T, int LAY>
__device__ __forceinline__ void prs_load(PrsRaw<T, LAY> &r, const PrsArgs &a, long long g, long long i, long long it, bool vec)
{
    const T *X = static_cast<const T *>(a.X);
    if constexpr (LAY == GENO_BED) {
        const long long bpr = ((long long)a.n + 3) / 4, b0 = it >> 2;
#pragma unroll
        for (int s = 0; s < 4; s++) {
            unsigned w = 0;
            if (g + s < a.pb && it < a.n) {
                const unsigned char *rec = X + (g + s) * a.ldX;
                if (vec && b0 + 4 <= bpr) w = *reinterpret_cast<const unsigned *>(rec + b0);
                else {
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        if (b0 + q < bpr) w |= (unsigned)rec[b0 + q] << (8 * q);
                }
            }
            r.w[s] = w;
        }
    } else {
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const bool in = g + s < a.pb && i < a.n;
            if constexpr (LAY == GENO_SNP) r.v[s] = in ? X[(g + s) * a.ldX + i] : T(0);
            else r.v[s] = in ? X[i * a.ldX + g + s] : T(0);
        }
    }
}

// SNP s of the run: its value in fp64 and whether the sample is called there; c: the sample's place in its N-tile; in: SNP and sample
// exist; mu: what a missing call takes
template <class T, int LAY>
__device__ __forceinline__ void prs_val(const PrsRaw<T, LAY> &r, int s, int c, bool in, double mu, int count_a1, double &x, double &m)
{
    if constexpr (LAY == GENO_BED) {
        const unsigned code = (r.w[s] >> (2 * c)) & 3u;
        const bool call = in && code != 1u;
        x = call ? (code == 2u ? 1.0 : (((code == 3u) != (count_a1 != 0)) ? 2.0 : 0.0)) : (in ? mu : 0.0);
        m = call ? 1.0 : 0.0;
    } else if constexpr (std::is_floating_point<T>::value) {
        const float v = (float)r.v[s];
        const bool call = in && isfinite(v);
        x = call ? (double)v : (in ? mu : 0.0);
        m = call ? 1.0 : 0.0;
    } else {
        x = in ? (double)r.v[s] : 0.0;
        m = in ? 1.0 : 0.0;
    }
}

// workgroup: chunk blockIdx.x / ngroups, samples [256 grp, 256 (grp + 1)) with grp = blockIdx.x % ngroups, and the weight columns
// [16 MT blockIdx.y, 16 MT (blockIdx.y + 1))
template <class T, int LAY, int MT, bool CNT>
__global__ __launch_bounds__(64 * PRS_WAVES, 2) void prs_kernel(PrsArgs a, bool vec)
{
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), k0 = 16 * MT * blockIdx.y;
    const long long grp = blockIdx.x % a.ngroups, ch = blockIdx.x / a.ngroups;
    const long long i0 = grp * PRS_ROWS + (long long)wave * (16 * PRS_NT);
    if (i0 >= a.n) return;                                             // whole wavefronts leave; nothing below synchronises
    const long long gb = ch * PG_PRS_CHUNK;
    const int ngrp = (int)((min(a.pb, gb + PG_PRS_CHUNK) - gb + 15) / 16);
    prs_v4d acc[PRS_NT][MT], cnt[PRS_NT][MT];
#pragma unroll
    for (int nt = 0; nt < PRS_NT; nt++)
#pragma unroll
        for (int mt = 0; mt < MT; mt++) { acc[nt][mt] = prs_v4d{0.0, 0.0, 0.0, 0.0}; cnt[nt][mt] = prs_v4d{0.0, 0.0, 0.0, 0.0}; }
    // the lane's run of four SNPs of group gi as stored, their means and weights: fetched one group ahead, in flight under the products
    PrsRaw<T, LAY> rawN[PRS_NT];
    double wN[MT][4], muN[4];
    auto fetch = [&](int gi) {
        const long long g = gb + 16 * gi + 4 * q;
#pragma unroll
        for (int nt = 0; nt < PRS_NT; nt++) prs_load<T, LAY>(rawN[nt], a, g, i0 + 16 * nt + c, i0 + 16 * nt, vec);
#pragma unroll
        for (int s = 0; s < 4; s++) {
            muN[s] = (a.mom && g + s < a.pb) ? a.mom[4 * (g + s)] : 0.0;
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                const int k = k0 + 16 * mt + c;
                wN[mt][s] = (k < a.t && g + s < a.pb) ? a.Wt[(long long)k * a.ldw + g + s] : 0.0;
            }
        }
    };
    fetch(0);
    for (int gi = 0; gi < ngrp; gi++) {
        const long long g = gb + 16 * gi + 4 * q;
        PrsRaw<T, LAY> raw[PRS_NT];
        double w[MT][4], mu[4];
#pragma unroll
        for (int nt = 0; nt < PRS_NT; nt++) raw[nt] = rawN[nt];
#pragma unroll
        for (int s = 0; s < 4; s++) {
            mu[s] = muN[s] == muN[s] ? muN[s] : 0.0;               // an all-missing SNP has no mean: its calls are 0
#pragma unroll
            for (int mt = 0; mt < MT; mt++) w[mt][s] = wN[mt][s];
        }
        if (gi + 1 < ngrp) fetch(gi + 1);
#pragma unroll
        for (int s = 0; s < 4; s++) {
            double x[PRS_NT], m[PRS_NT];
#pragma unroll
            for (int nt = 0; nt < PRS_NT; nt++)
                prs_val<T, LAY>(raw[nt], s, c, g + s < a.pb && i0 + 16 * nt + c < a.n, mu[s], a.count_a1, x[nt], m[nt]);
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                const double wnz = w[mt][s] != 0.0 ? 1.0 : 0.0;
#pragma unroll
                for (int nt = 0; nt < PRS_NT; nt++) {
                    acc[nt][mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(w[mt][s], x[nt], acc[nt][mt], 0, 0, 0);
                    if constexpr (CNT) cnt[nt][mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(wnz, m[nt], cnt[nt][mt], 0, 0, 0);
                }
            }
        }
    }
    // the chunk's partial (C layout: sample = lane & 15, column = (lane >> 4) + 4 e) into the work area
#pragma unroll
    for (int nt = 0; nt < PRS_NT; nt++) {
        const long long i = i0 + 16 * nt + c;
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int k = k0 + 16 * mt + q + 4 * e;
                if (i >= a.n || k >= a.t) continue;
                const size_t o = ((size_t)ch * a.t + k) * a.ldp + i;
                a.ps[o] = acc[nt][mt][e];
                if constexpr (CNT) a.pc[o] = (int)cnt[nt][mt][e];
            }
    }
}

// second stage: one lane per (column, sample) adds the chunks 0..R-1 onto score in order
__global__ __launch_bounds__(256) void prs_reduce_kernel(PrsArgs a, long long nchunk)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (i >= a.n) return;
    const size_t o = (size_t)k * a.lds + i;
    double s = a.score[o];
    long long cn = 0;
    for (long long ch = 0; ch < nchunk; ch++) {
        const size_t po = ((size_t)ch * a.t + k) * a.ldp + i;
        s = s + a.ps[po];
        if (a.called) cn += a.pc[po];
    }
    a.score[o] = s;
    if (a.called) a.called[o] += cn;
}

template <class T, int LAY>
static int launch_prs(pg_ctx *ctx, const PrsArgs &a, bool vec)
{
    const long long nchunk = prs_chunks(a.pb);
    // 64 fp64 accumulators a lane at most — two M-tiles of scores, or one of scores and one of counts — so that at two wavefronts per
    // SIMD they stay in VGPRs (from AGPRs this MFMA issues at half its rate).  Further columns take further rows of
    // workgroups, which re-read the genotypes from L2 under products that hide it
    const bool cnt = a.called != nullptr;
    const int mt = (a.t <= 16 || cnt) ? 1 : 2;
    const dim3 grid((unsigned)(a.ngroups * nchunk), (unsigned)((a.t + 16 * mt - 1) / (16 * mt)));
    if (cnt) prs_kernel<T, LAY, 1, true><<<grid, 64 * PRS_WAVES, 0, ctx->stream>>>(a, vec);
    else if (mt == 1) prs_kernel<T, LAY, 1, false><<<grid, 64 * PRS_WAVES, 0, ctx->stream>>>(a, vec);
    else prs_kernel<T, LAY, 2, false><<<grid, 64 * PRS_WAVES, 0, ctx->stream>>>(a, vec);
    PG_HIP(hipGetLastError());
    prs_reduce_kernel<<<dim3((unsigned)((a.n + 255) / 256), (unsigned)a.t), 256, 0, ctx->stream>>>(a, nchunk);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

// the argument checks the two entry points share (after their NULL checks); what: the entry's name
static int prs_check(const char *what, int64_t n, int64_t pb, int t, int64_t ldw, int64_t lds)
{
    PG_REQUIRE(n >= 1 && n < (1LL << 30) && pb >= 0 && pb <= PRS_MAXPB && t >= 1, "%s: bad shape n=%lld pb=%lld t=%d", what, (long long)n,
               (long long)pb, t);
    if (t > PG_PRS_MAX_T) {
        set_error("%s: t=%d weight columns not supported by this build (<= %d per call)", what, t, PG_PRS_MAX_T);
        return PG_ENOTSUP;
    }
    PG_REQUIRE(prs_groups(n) * prs_chunks(pb) < PRS_MAXGRID, "%s: a block of n=%lld x pb=%lld is more than one launch holds (%lld workgroups)", what,
               (long long)n, (long long)pb, PRS_MAXGRID);
    PG_REQUIRE(ldw >= pb && lds >= n, "%s: strides too small: ldw=%lld < pb=%lld or lds=%lld < n=%lld", what, (long long)ldw, (long long)pb,
               (long long)lds, (long long)n);
    return PG_OK;
}

static PrsArgs prs_args(int64_t n, int64_t pb, const void *X, int64_t ldX, int count_a1, int t, const double *Wt, int64_t ldw, const PrsWork &w,
                        bool prepass, double *score, int64_t *called, int64_t lds)
{
    PrsArgs a{};
    a.n = (int)n; a.t = t; a.count_a1 = count_a1;
    a.pb = pb; a.ldX = ldX; a.ldw = ldw; a.lds = lds; a.ldp = (n + 15) / 16 * 16; a.ngroups = prs_groups(n);
    a.X = X; a.Wt = Wt;
    a.mom = prepass ? w.moments : nullptr;
    a.score = score;
    a.called = reinterpret_cast<long long *>(called);
    a.ps = w.ps;
    a.pc = w.pc;
    return a;
}

// a refusal of the pre-pass (a sample-major block of more workgroups than one launch holds) in the name of the entry that made it
static int prs_prepass_refused(const char *what, int rc)
{
    char msg[400];
    snprintf(msg, sizeof msg, "%s", pg_last_error());
    set_error("%s: the pre-pass over the batch was refused: %s", what, msg);
    return rc;
}

}  // namespace pg

using namespace pg;

extern "C" size_t pg_prs_work_bytes(int64_t n, int64_t pb, int t)
{
    if (n < 1 || n >= (1LL << 30) || pb < 0 || pb > PRS_MAXPB || t < 1 || t > PG_PRS_MAX_T || prs_groups(n) * prs_chunks(pb) >= PRS_MAXGRID) return 0;
    return prs_work(nullptr, n, pb, t).bytes;
}

extern "C" int pg_prs_bed_acc_dev(pg_ctx *ctx, int64_t n, int64_t pb, const unsigned char *bed, int64_t ldb, int count_a1, int t, const double *Wt,
                                  int64_t ldw, int impute, void *work, double *score, int64_t *called, int64_t lds)
{
    PG_REQUIRE(ctx && bed && Wt && work && score, "pg_prs_bed_acc_dev: NULL argument");
    int rc = prs_check("pg_prs_bed_acc_dev", n, pb, t, ldw, lds);
    if (rc) return rc;
    PG_REQUIRE(ldb >= (n + 3) / 4, "pg_prs_bed_acc_dev: ldb=%lld < ceil(n / 4), n=%lld", (long long)ldb, (long long)n);
    if (pb == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    const PrsWork w = prs_work(work, n, pb, t);
    if (impute) {
        rc = pg_snp_stats_bed_dev(ctx, n, pb, bed, ldb, count_a1, w.ss, reinterpret_cast<int64_t *>(w.counts), w.moments);
        if (rc) return prs_prepass_refused("pg_prs_bed_acc_dev", rc);
    }
    const PrsArgs a = prs_args(n, pb, bed, ldb, count_a1 != 0, t, Wt, ldw, w, impute != 0, score, called, lds);
    const bool vec = ((uintptr_t)bed % 4 == 0) && ldb % 4 == 0;
    return launch_prs<unsigned char, GENO_BED>(ctx, a, vec);
}

extern "C" int pg_prs_x_acc_dev(pg_ctx *ctx, int64_t n, int64_t pb, const void *X, int dtype, int64_t ldX, int snp_major, int t, const double *Wt,
                                int64_t ldw, int impute, void *work, double *score, int64_t *called, int64_t lds)
{
    PG_REQUIRE(ctx && X && Wt && work && score, "pg_prs_x_acc_dev: NULL argument");
    int rc = prs_check("pg_prs_x_acc_dev", n, pb, t, ldw, lds);
    if (rc) return rc;
    PG_REQUIRE(ldX >= (snp_major ? n : pb), "pg_prs_x_acc_dev: ldX=%lld too small for n=%lld pb=%lld snp_major=%d", (long long)ldX, (long long)n,
               (long long)pb, snp_major);
    if (!dtype_known(dtype)) {
        set_error("pg_prs_x_acc_dev: unknown dtype %d", dtype);
        return PG_ENOTSUP;
    }
    if (pb == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    const PrsWork w = prs_work(work, n, pb, t);
    const bool prepass = impute && dtype >= PG_DTYPE_FLOAT32;          // an 8-bit block has no missing call to impute
    if (prepass) {
        rc = pg_snp_stats_x_dev(ctx, n, pb, X, dtype, ldX, snp_major, w.ss, reinterpret_cast<int64_t *>(w.counts), w.moments);
        if (rc) return prs_prepass_refused("pg_prs_x_acc_dev", rc);
    }
    const PrsArgs a = prs_args(n, pb, X, ldX, 0, t, Wt, ldw, w, prepass, score, called, lds);
    return geno_dispatch(dtype, snp_major != 0, [&](auto src) {
        using S = decltype(src);
        return launch_prs<typename S::type, S::layout>(ctx, a, false);
    });
}
