// snp_stats.hip — per-SNP quality control straight from raw genotypes (packed .bed records, 8-bit, float32 or float64 blocks, sample- or
// SNP-major): the counts {n_miss, n0, n1, n2}, the moments {mean, var, min, max} of the observed values, and the exact Hardy-Weinberg test
// of Wigginton, Cutler and Abecasis (2005) on the counts.  What GEMMA's -miss / -maf / -hwe filters and its n_miss / af columns are made of.
//
// Values are the ones the scans see: an element is first rounded to float32; NaN and +-Inf are missing (an 8-bit block has no missing code,
// a .bed call is missing at code 01).  A SNP whose observed values are all exactly 0, 1 or 2 (a hard-call SNP; every .bed record) takes its
// moments from the integer counts — S1 = n1 + 2 n2, S2 = n1 + 4 n2, mean = S1 / n_obs, var = (n_obs S2 - S1^2) / n_obs^2, one correctly
// rounded division each — so its row is the same bits whatever the storage.  Any other SNP takes fp64 two-pass moments: the sum of the
// observed values, then the sum of (x - mean)^2 over a second sweep, which only such SNPs pay for.
//
// This is a bandwidth kernel; three shapes:
//   .bed        16 lanes per record, 16 bytes (64 calls) per lane and step; the four classes are popcounts of whole words.
//   SNP-major   one wavefront per SNP, 16 bytes per lane and step; the second sweep re-reads the row in the same wavefront.
//   sample-major  lane = 16 bytes of adjacent SNPs (4 bytes of an 8-bit row), workgroup = 256 samples x (64 lanes' SNPs), its four
//               wavefronts on interleaved rows; per-chunk partials go to the work area and a second stage adds the chunks in order (no
//               atomics).  Chunks depend on n alone, so pb = 16 384 float32 columns are 2 560 workgroups at n = 10 000.
// 16-byte loads need the base and the row pitch on 16 bytes (.bed: 4-byte words at a 4-byte pitch, 16-byte at a 16-byte one); otherwise the
// same elements arrive through scalar loads, in the same lanes.
// Determinism: every floating-point sum is one fixed chain — a lane's elements in order, a fixed tree across lanes, wavefronts 0..3, chunks
// 0..R-1 — that depends on n and the layout only: a row depends on its SNP alone, not on pb, the batch boundaries, the pitch or the run.
#include "geno_src.hpp"

#include <cmath>
#include <type_traits>

namespace pg {

constexpr int SS_ROWS = 256;      // samples per chunk of a sample-major block
constexpr long long SS_MAXPB = 1LL << 25;      // SNPs per call, and
constexpr long long SS_MAXGRID = 1LL << 24;    // workgroups of 256 per launch, exclusive: under 2^32 threads, which every launch takes

struct SsAcc {
    int nm, n0, n1, n2;
    float mn, mx;
    double sum;
};

__device__ __forceinline__ void ss_zero(SsAcc &a)
{
    a.nm = a.n0 = a.n1 = a.n2 = 0;
    a.mn = INFINITY; a.mx = -INFINITY;
    a.sum = 0.0;
}

template <class T> __device__ __forceinline__ void ss_add(SsAcc &a, T x)
{
    const float v = (float)x;
    a.n0 += (v == 0.0f); a.n1 += (v == 1.0f); a.n2 += (v == 2.0f);
    if constexpr (std::is_floating_point<T>::value) {
        const bool fin = isfinite(v);
        a.nm += !fin;
        a.mn = fminf(a.mn, fin ? v : INFINITY);
        a.mx = fmaxf(a.mx, fin ? v : -INFINITY);
        a.sum += fin ? (double)v : 0.0;
    } else {
        a.mn = fminf(a.mn, v);
        a.mx = fmaxf(a.mx, v);
        a.sum += (double)v;
    }
}

// the second sweep's term: (x - mean)^2 of an observed element
template <class T> __device__ __forceinline__ void ss_add2(double &ss, T x, double mean)
{
    const float v = (float)x;
    const double d = (double)v - mean;
    if (!std::is_floating_point<T>::value || isfinite(v)) ss = fma(d, d, ss);
}

__device__ __forceinline__ void ss_zero(double &a) { a = 0.0; }
__device__ __forceinline__ void ss_merge(double &a, double b) { a += b; }

__device__ __forceinline__ void ss_merge(SsAcc &a, const SsAcc &b)
{
    a.nm += b.nm; a.n0 += b.n0; a.n1 += b.n1; a.n2 += b.n2;
    a.mn = fminf(a.mn, b.mn); a.mx = fmaxf(a.mx, b.mx);
    a.sum += b.sum;
}

// E elements at p, as one load of E sizeof(T) = 16 (or 4) bytes (vec) or one by one
template <class T, int E> __device__ __forceinline__ void ss_load(T (&r)[E], const T *p, bool vec)
{
    if (vec) __builtin_memcpy(r, __builtin_assume_aligned(p, E * sizeof(T)), E * sizeof(T));
    else {
#pragma unroll
        for (int s = 0; s < E; s++) r[s] = p[s];
    }
}

// counts and moments of one SNP from its totals; returns true when var is still to come from the second sweep (then m[1] is not written)
__device__ __forceinline__ bool ss_finish(long long n, long long nm, long long n0, long long n1, long long n2, double sum, float mn, float mx,
                                          long long *cnt, double *m, double &mean)
{
    cnt[0] = nm; cnt[1] = n0; cnt[2] = n1; cnt[3] = n2;
    const long long nobs = n - nm;
    const double nan = __builtin_nan("");
    mean = nan;
    if (nobs <= 0) {
        m[0] = nan; m[1] = nan; m[2] = nan; m[3] = nan;
        return false;
    }
    if (n0 + n1 + n2 == nobs) {                                        // hard calls: exact integers, one division each
        const long long S1 = n1 + 2 * n2, S2 = n1 + 4 * n2;
        m[0] = (double)S1 / (double)nobs;
        m[1] = (double)(nobs * S2 - S1 * S1) / (double)(nobs * nobs);
        m[2] = n0 ? 0.0 : (n1 ? 1.0 : 2.0);
        m[3] = n2 ? 2.0 : (n1 ? 1.0 : 0.0);
        return false;
    }
    mean = sum / (double)nobs;
    m[0] = mean; m[2] = (double)mn; m[3] = (double)mx;
    return true;
}

// ---- packed .bed records: 16 lanes per SNP -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ss_bed_kernel(int n, long long pb, const unsigned char *bed, long long ldb, int count_a1, bool vec16, bool vec4,
                                                     long long *counts, double *moments)
{
    const int sub = threadIdx.x & 15;
    const long long g = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (g >= pb) return;                                               // whole 16-lane groups leave
    const unsigned char *rec = bed + g * ldb;
    const int bpr = (n + 3) / 4;
    int nm = 0, n1 = 0, n11 = 0;
    for (int b0 = 16 * sub; b0 < bpr; b0 += 256) {
        unsigned w[4];
        if (vec16 && b0 + 16 <= bpr) {
            const uint4 v = *reinterpret_cast<const uint4 *>(rec + b0);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int bq = b0 + 4 * q;
                w[q] = 0;
                if (vec4 && bq + 4 <= bpr) w[q] = *reinterpret_cast<const unsigned *>(rec + bq);
                else {
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (bq + k < bpr) w[q] |= (unsigned)rec[bq + k] << (8 * k);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int left = n - 4 * (b0 + 4 * q);                     // calls of this word that are samples: the pad bits count nowhere
            const unsigned mask = left >= 16 ? 0x55555555u : (left <= 0 ? 0u : (((1u << (2 * left)) - 1u) & 0x55555555u));
            const unsigned lo = w[q] & mask, hi = (w[q] >> 1) & mask;  // low and high bit of the 16 codes
            nm += __popc(lo & ~hi);                                    // 01 missing
            n1 += __popc(hi & ~lo);                                    // 10 heterozygous
            n11 += __popc(lo & hi);                                    // 11
        }
    }
    for (int m = 1; m < 16; m <<= 1) { nm += __shfl_xor(nm, m, 64); n1 += __shfl_xor(n1, m, 64); n11 += __shfl_xor(n11, m, 64); }
    if (sub == 0) {
        const long long n00 = (long long)n - nm - n1 - n11;
        double mean;
        ss_finish(n, nm, count_a1 ? n11 : n00, n1, count_a1 ? n00 : n11, 0.0, 0.0f, 0.0f, counts + 4 * g, moments + 4 * g, mean);
    }
}

// ---- SNP-major arrays: one wavefront per SNP -----------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void ss_snp_kernel(int n, long long pb, const T *X, long long ldX, bool vec, long long *counts, double *moments)
{
    constexpr int E = 16 / sizeof(T);
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= pb) return;
    const T *row = X + g * ldX;
    const int nfull = n / (64 * E);                                    // steps in which every lane's run lies inside the row
    const int t0 = (nfull * 64 + lane) * E;                            // the lane's run of the last, partial step
    SsAcc a;
    ss_zero(a);
#pragma unroll 4
    for (int it = 0; it < nfull; it++) {
        T r[E];
        ss_load<T, E>(r, row + ((size_t)it * 64 + lane) * E, vec);
#pragma unroll
        for (int s = 0; s < E; s++) ss_add<T>(a, r[s]);
    }
#pragma unroll
    for (int s = 0; s < E; s++)
        if (t0 + s < n) ss_add<T>(a, row[t0 + s]);
    for (int m = 1; m < 64; m <<= 1) {                                 // a + b and b + a: every lane ends with the same bits
        SsAcc b;
        b.nm = __shfl_xor(a.nm, m, 64); b.n0 = __shfl_xor(a.n0, m, 64); b.n1 = __shfl_xor(a.n1, m, 64); b.n2 = __shfl_xor(a.n2, m, 64);
        b.mn = __shfl_xor(a.mn, m, 64); b.mx = __shfl_xor(a.mx, m, 64); b.sum = __shfl_xor(a.sum, m, 64);
        ss_merge(a, b);
    }
    long long cnt[4];
    double mo[4], mean;
    const bool need = ss_finish(n, a.nm, a.n0, a.n1, a.n2, a.sum, a.mn, a.mx, cnt, mo, mean);      // the same in every lane
    if (need) {
        double ss = 0.0;
#pragma unroll 4
        for (int it = 0; it < nfull; it++) {
            T r[E];
            ss_load<T, E>(r, row + ((size_t)it * 64 + lane) * E, vec);
#pragma unroll
            for (int s = 0; s < E; s++) ss_add2<T>(ss, r[s], mean);
        }
#pragma unroll
        for (int s = 0; s < E; s++)
            if (t0 + s < n) ss_add2<T>(ss, row[t0 + s], mean);
        for (int m = 1; m < 64; m <<= 1) ss += __shfl_xor(ss, m, 64);
        mo[1] = ss / (double)(n - a.nm);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) { counts[4 * g + k] = cnt[k]; moments[4 * g + k] = mo[k]; }
    }
}

// ---- sample-major arrays: chunk partials in the work area, then a second stage ---------------------------------------------------------
struct SsWork {
    int4 *cnt;         // [R][pb] nm, n0, n1, n2 of a chunk
    double *sum;       // [R][pb]
    double *ss;        // [R][pb] second sweep
    float2 *mm;        // [R][pb] min, max
    double *mean;      // [pb]
    int *need;         // [pb] the SNP takes the second sweep
};

static SsWork ss_work(void *work, long long R, long long pb)
{
    char *b = static_cast<char *>(work);
    const size_t rp = (size_t)R * pb;
    SsWork w;
    w.cnt = reinterpret_cast<int4 *>(b);
    w.sum = reinterpret_cast<double *>(b + rp * 16);
    w.ss = reinterpret_cast<double *>(b + rp * 24);
    w.mm = reinterpret_cast<float2 *>(b + rp * 32);
    w.mean = reinterpret_cast<double *>(b + rp * 40);
    w.need = reinterpret_cast<int *>(b + rp * 40 + (size_t)pb * 8);
    return w;
}

// SNPs per lane of a sample-major block: 16 bytes of float32 or float64, 4 bytes of an 8-bit row (a wavefront reads 256 contiguous bytes
// of it): sixteen SNPs' accumulators per lane would take every register the lane has
template <class T> constexpr int ss_sm_e() { return sizeof(T) == 1 ? 4 : 16 / (int)sizeof(T); }

// workgroup (cb, chunk): lanes' SNPs [64 E cb, 64 E (cb + 1)), samples [256 chunk, 256 (chunk + 1)); wavefront w on rows w, w + 4, ...
template <class T, int PASS>
__global__ __launch_bounds__(256) void ss_sm_kernel(int n, long long pb, const T *X, long long ldX, bool vec, long long ncb, SsWork w)
{
    constexpr int E = ss_sm_e<T>();
    using Part = typename std::conditional<PASS == 1, SsAcc, double>::type;      // the second sweep carries one sum per SNP
    __shared__ Part sh[3][64][E];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long chunk = blockIdx.x / ncb, cb = blockIdx.x % ncb;
    const long long g0 = (cb * 64 + lane) * E;
    const int r0 = (int)chunk * SS_ROWS, r1 = min(n, r0 + SS_ROWS);
    const bool full = g0 + E <= pb;
    Part a[E];
    double mean[E];
    bool need[E];
#pragma unroll
    for (int e = 0; e < E; e++) { ss_zero(a[e]); mean[e] = 0.0; need[e] = false; }
    if constexpr (PASS == 2) {
        int any = 0;
#pragma unroll
        for (int e = 0; e < E; e++)
            if (g0 + e < pb && w.need[g0 + e]) { any = 1; need[e] = true; mean[e] = w.mean[g0 + e]; }
        if (!__syncthreads_or(any)) return;                            // a block of hard calls has no second sweep
    }
#pragma unroll 4
    for (int i = r0 + wave; i < r1; i += 4) {
        const T *p = X + (size_t)i * ldX + g0;
        T r[E];
        if (full) ss_load<T, E>(r, p, vec);
        else {
#pragma unroll
            for (int e = 0; e < E; e++) r[e] = g0 + e < pb ? p[e] : T(0);
        }
#pragma unroll
        for (int e = 0; e < E; e++) {
            if constexpr (PASS == 1) ss_add<T>(a[e], r[e]);
            else if (need[e]) ss_add2<T>(a[e], r[e], mean[e]);
        }
    }
    // wavefronts 1..3 hand their partials to wavefront 0; it adds them in order
    if (wave > 0) {
#pragma unroll
        for (int e = 0; e < E; e++) sh[wave - 1][lane][e] = a[e];
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int v = 0; v < 3; v++)
#pragma unroll
        for (int e = 0; e < E; e++) ss_merge(a[e], sh[v][lane][e]);
#pragma unroll
    for (int e = 0; e < E; e++) {
        if (g0 + e >= pb) continue;
        const size_t o = (size_t)chunk * pb + g0 + e;
        if constexpr (PASS == 1) {
            w.cnt[o] = make_int4(a[e].nm, a[e].n0, a[e].n1, a[e].n2);
            w.sum[o] = a[e].sum;
            w.mm[o] = make_float2(a[e].mn, a[e].mx);
        } else {
            w.ss[o] = a[e];
        }
    }
}

// one lane per SNP adds the chunks 0..R-1 in order
template <int PASS>
__global__ __launch_bounds__(256) void ss_sm_final_kernel(int n, long long pb, long long R, SsWork w, long long *counts, double *moments)
{
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= pb) return;
    if constexpr (PASS == 1) {
        long long nm = 0, n0 = 0, n1 = 0, n2 = 0;
        double sum = 0.0;
        float mn = INFINITY, mx = -INFINITY;
        for (long long r = 0; r < R; r++) {
            const size_t o = (size_t)r * pb + g;
            const int4 c = w.cnt[o];
            const float2 m = w.mm[o];
            nm += c.x; n0 += c.y; n1 += c.z; n2 += c.w;
            sum += w.sum[o];
            mn = fminf(mn, m.x); mx = fmaxf(mx, m.y);
        }
        double mean;
        const bool need = ss_finish(n, nm, n0, n1, n2, sum, mn, mx, counts + 4 * g, moments + 4 * g, mean);
        w.need[g] = need;
        w.mean[g] = mean;
    } else {
        if (!w.need[g]) return;
        double ss = 0.0;
        for (long long r = 0; r < R; r++) ss += w.ss[(size_t)r * pb + g];
        moments[4 * g + 1] = ss / (double)(n - counts[4 * g]);
    }
}

template <class T, int LAY>
static int launch_ss_x(pg_ctx *ctx, int n, long long pb, const void *X, long long ldX, void *work, long long *counts, double *moments)
{
    const T *Xt = static_cast<const T *>(X);
    if (LAY == GENO_SNP) {
        const bool vec = ((uintptr_t)X % 16 == 0) && ((size_t)ldX * sizeof(T)) % 16 == 0;
        static_assert(SS_MAXPB / 4 + 1 < SS_MAXGRID, "one wavefront per SNP");
        ss_snp_kernel<T><<<(unsigned)((pb + 3) / 4), 256, 0, ctx->stream>>>(n, pb, Xt, ldX, vec, counts, moments);
        PG_HIP(hipGetLastError());
        return PG_OK;
    }
    constexpr int E = ss_sm_e<T>();
    const bool vec = ((uintptr_t)X % (E * sizeof(T)) == 0) && ((size_t)ldX * sizeof(T)) % (E * sizeof(T)) == 0;
    const long long R = ((long long)n + SS_ROWS - 1) / SS_ROWS, ncb = (pb + 64 * E - 1) / (64 * E);
    PG_REQUIRE(R * ncb < SS_MAXGRID, "pg_snp_stats_x_dev: a sample-major block of n=%d x pb=%lld is more than one launch holds (%lld workgroups)", n, pb,
               SS_MAXGRID);
    const SsWork w = ss_work(work, R, pb);
    const unsigned grid = (unsigned)(R * ncb), fin = (unsigned)((pb + 255) / 256);
    ss_sm_kernel<T, 1><<<grid, 256, 0, ctx->stream>>>(n, pb, Xt, ldX, vec, ncb, w);
    PG_HIP(hipGetLastError());
    ss_sm_final_kernel<1><<<fin, 256, 0, ctx->stream>>>(n, pb, R, w, counts, moments);
    PG_HIP(hipGetLastError());
    ss_sm_kernel<T, 2><<<grid, 256, 0, ctx->stream>>>(n, pb, Xt, ldX, vec, ncb, w);
    PG_HIP(hipGetLastError());
    ss_sm_final_kernel<2><<<fin, 256, 0, ctx->stream>>>(n, pb, R, w, counts, moments);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

// ---- the exact Hardy-Weinberg test: one lane per SNP ---------------------------------------------------------------------------------
// With N genotypes, nr copies of the rarer allele and nc = 2N - nr of the other, the probabilities of h = nr mod 2, ..., nr heterozygotes
// are built unnormalised from the mode outward:  P(h - 2) = P(h) h (h - 1) / (4 (a + 1)(b + 1)),  P(h + 2) = P(h) 4 a b / ((h + 2)(h + 1)),
// a = (nr - h) / 2 and b = N - h - a the two homozygote counts.  The sweep runs twice: once for sum P and P(n1), once for the sum of the
// terms P(h) <= P(n1) (1 + 2^-30) — the same operations, so the same values.
template <class F> __device__ __forceinline__ void hwe_sweep(long long N, long long nr, long long mid, F visit)
{
    double P = 1.0;
    visit(mid, P);
    long long a = (nr - mid) / 2, b = N - mid - a;
    for (long long h = mid; h >= 2; h -= 2) {
        P = P * ((double)h * (double)(h - 1)) / (4.0 * (double)(a + 1) * (double)(b + 1));
        visit(h - 2, P);
        a++; b++;
    }
    P = 1.0;
    a = (nr - mid) / 2; b = N - mid - a;
    for (long long h = mid; h <= nr - 2; h += 2) {
        P = P * (4.0 * (double)a * (double)b) / ((double)(h + 2) * (double)(h + 1));
        visit(h + 2, P);
        a--; b--;
    }
}

__global__ __launch_bounds__(64) void hwe_kernel(long long n, long long p, const long long *counts, double *pval)
{
    const long long g = (long long)blockIdx.x * 64 + threadIdx.x;
    if (g >= p) return;
    const long long nm = counts[4 * g], n0 = counts[4 * g + 1], n1 = counts[4 * g + 2], n2 = counts[4 * g + 3];
    const long long N = n0 + n1 + n2;
    if (nm < 0 || n0 < 0 || n1 < 0 || n2 < 0 || nm + N != n || N == 0) { pval[g] = __builtin_nan(""); return; }
    const long long nr = 2 * (n0 < n2 ? n0 : n2) + n1, nc = 2 * N - nr;
    if (nr == 0) { pval[g] = 1.0; return; }
    long long mid = nr * nc / (2 * N);
    if ((mid ^ nr) & 1) mid++;
    double sum = 0.0, Pobs = 0.0;
    hwe_sweep(N, nr, mid, [&](long long h, double P) { sum += P; if (h == n1) Pobs = P; });
    const double thr = Pobs * (1.0 + 0x1p-30);
    double tail = 0.0;
    hwe_sweep(N, nr, mid, [&](long long h, double P) { if (P <= thr) tail += P; });
    const double pv = tail / sum;
    pval[g] = pv > 1.0 ? 1.0 : pv;
}

}  // namespace pg

using namespace pg;

extern "C" size_t pg_snp_stats_work_bytes(int64_t n, int64_t pb)
{
    if (n < 1 || n >= (1LL << 30) || pb < 0 || pb > SS_MAXPB) return 0;
    const size_t R = (size_t)((n + SS_ROWS - 1) / SS_ROWS);
    return 256 + R * (size_t)pb * 40 + (size_t)pb * 12;
}

extern "C" int pg_snp_stats_bed_dev(pg_ctx *ctx, int64_t n, int64_t pb, const unsigned char *bed, int64_t ldb, int count_a1, void *work, int64_t *counts,
                                    double *moments)
{
    PG_REQUIRE(ctx && bed && work && counts && moments, "pg_snp_stats_bed_dev: NULL argument");
    PG_REQUIRE(n >= 1 && n < (1LL << 30) && pb >= 0 && pb <= SS_MAXPB && ldb >= (n + 3) / 4, "pg_snp_stats_bed_dev: bad shape n=%lld pb=%lld ldb=%lld",
               (long long)n, (long long)pb, (long long)ldb);
    if (pb == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    const bool vec4 = ((uintptr_t)bed % 4 == 0) && ldb % 4 == 0, vec16 = ((uintptr_t)bed % 16 == 0) && ldb % 16 == 0;
    ss_bed_kernel<<<(unsigned)((pb + 15) / 16), 256, 0, ctx->stream>>>((int)n, pb, bed, ldb, count_a1 != 0, vec16, vec4,
                                                                      reinterpret_cast<long long *>(counts), moments);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

extern "C" int pg_snp_stats_x_dev(pg_ctx *ctx, int64_t n, int64_t pb, const void *X, int dtype, int64_t ldX, int snp_major, void *work, int64_t *counts,
                                  double *moments)
{
    PG_REQUIRE(ctx && X && work && counts && moments, "pg_snp_stats_x_dev: NULL argument");
    PG_REQUIRE(n >= 1 && n < (1LL << 30) && pb >= 0 && pb <= SS_MAXPB && ldX >= (snp_major ? n : pb),
               "pg_snp_stats_x_dev: bad shape n=%lld pb=%lld ldX=%lld snp_major=%d", (long long)n, (long long)pb, (long long)ldX, snp_major);
    if (!dtype_known(dtype)) {
        set_error("pg_snp_stats_x_dev: unknown dtype %d", dtype);
        return PG_ENOTSUP;
    }
    if (pb == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    long long *cnt = reinterpret_cast<long long *>(counts);
    return geno_dispatch(dtype, snp_major != 0, [&](auto src) {
        using S = decltype(src);
        return launch_ss_x<typename S::type, S::layout>(ctx, (int)n, pb, X, ldX, work, cnt, moments);
    });
}

extern "C" int pg_hwe_exact_dev(pg_ctx *ctx, int64_t n, int64_t p, const int64_t *counts, double *pval)
{
    PG_REQUIRE(ctx && counts && pval, "pg_hwe_exact_dev: NULL argument");
    PG_REQUIRE(n >= 1 && n < (1LL << 30) && p >= 0 && p < (1LL << 31), "pg_hwe_exact_dev: bad shape n=%lld p=%lld", (long long)n, (long long)p);
    if (p == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    hwe_kernel<<<(unsigned)((p + 63) / 64), 64, 0, ctx->stream>>>(n, p, reinterpret_cast<const long long *>(counts), pval);
    PG_HIP(hipGetLastError());
    return PG_OK;
}
