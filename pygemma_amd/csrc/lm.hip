// lm.hip — the plain linear model (GEMMA's -lm 1): the K-free baseline every mixed-model scan is read against, straight from raw
// genotypes (packed .bed records, 8-bit, float32 or float64 blocks, sample- or SNP-major) with no eigensolver and no rotation.
//
// For phenotype k, SNP x and covariates W (n x c):  y_k = W alpha + x beta + eps,  df = n - c - 1.
// pg_lm_setup_dev builds, once per (W, Y) and all in fp64, the panel B = [Q | Y~] (n x (c + t), columns padded to a multiple of 16,
// rows to a multiple of 64, pads zero):
//   G = W'W = L L' (Cholesky, score_setup_kernel's failure rule),  Q = W L^-T (forward substitution per sample),
//   D = Q'Y,  Y~ = Y - Q D,  syy_k = y~_k' y~_k.
// Per SNP the scan needs x'B (c + t dot products of length n) and x'x:
//   sxx = x'x - |Q'x|^2,  sxy_k = x'y~_k,  rss_k = syy_k - sxy_k^2 / sxx
//   beta = sxy / sxx,  se = sqrt(rss / (df sxx)),  tau = df / rss,  F = df sxy^2 / (sxx rss)
// x'B is a skinny GEMM on v_mfma_f64_16x16x4_f64 with the genotypes decoded into the A operand as they are read.
//
// Tiling: a workgroup of 4 wavefronts owns 128 SNPs (two 16-SNP row tiles per wavefront) and walks the samples 64 at a time; the
// 64 x NP chunk of the panel is shared through LDS (one fetch from L2 per 128 SNPs).  k is only a summation index, so within a
// chunk lane (row r, k-group q) takes the CONTIGUOUS run of samples 16 q .. 16 q + 15 of its SNP (one 64-byte piece of a float32
// row, 16 bytes of an 8-bit row, 4 bytes of a .bed record) and MFMA step s multiplies sample 16 q + s of A with row 16 q + s of
// the panel chunk.  x'x accumulates on the VALU from the same registers.  The accumulators meet in LDS for the epilogue.
// Determinism: an output element is one fixed chain — chunk after chunk, step after step, the four k-groups inside the
// instruction — whatever the SNP's slot, tile, batch or row pitch; samples >= n enter as exact zeros and pad bytes are never
// read.  No split over samples, no atomics: a row depends only on its SNP and on (W, Y).
#include "geno_src.hpp"

#include <cmath>

namespace pg {


constexpr int LM_KC = 64;                          // samples per chunk: 4 k-groups of 16
constexpr int LM_RT = 2;                           // 16-SNP row tiles per wavefront
constexpr int LM_WAVES = 4;
constexpr int LM_SNPS = 16 * LM_RT * LM_WAVES;     // SNPs per workgroup
constexpr int LM_LDG = PG_MAX_COVARIATES;          // row pitch of G in the work area
constexpr int LM_MAXP = 64;                        // c + t at most: four column tiles
// work area: header | syy (64) | G (30 x 30) | D = Q'Y (c x t <= 1024) | panel (npad x NP)
constexpr size_t LM_OFF_SYY = 256, LM_OFF_G = LM_OFF_SYY + LM_MAXP * 8, LM_OFF_D = LM_OFF_G + (size_t)LM_LDG * LM_LDG * 8,
                 LM_OFF_PANEL = 16384;
static_assert(LM_OFF_D + 1024 * 8 <= LM_OFF_PANEL, "work-area layout");

struct LmHdr {
    int fail;      // the Cholesky of W'W failed (W rank-deficient at 1e-10 relative, or non-finite): every row NaN
    int pad;
};

static inline int lm_np(int c, int t) { return (c + t + 15) / 16 * 16; }
static inline long long lm_npad(long long n) { return (n + LM_KC - 1) / LM_KC * LM_KC; }

typedef double lm_v4d __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double lm_wave_sum(double v)
{
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);   // a + b and b + a: every lane ends with the same bits
    return v;
}

// sum over the 256 threads of a workgroup in a fixed order (every thread gets it)
__device__ __forceinline__ double lm_block_sum(double v, double *red)
{
    v = lm_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return s;
}

// ---- set-up ----------------------------------------------------------------------------------------------------------------------
// G[j][k] = w_j'w_k, j >= k: one workgroup per entry
__global__ __launch_bounds__(256) void lm_gram_kernel(int n, int c, const float *W, double *G)
{
    __shared__ double red[4];
    int j = 0;
    const int e = blockIdx.x;
    while ((j + 1) * (j + 2) / 2 <= e) j++;
    const int k = e - j * (j + 1) / 2;
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc = fma((double)W[(size_t)i * c + j], (double)W[(size_t)i * c + k], acc);
    acc = lm_block_sum(acc, red);
    if (threadIdx.x == 0) G[j * LM_LDG + k] = acc;
}

// the Cholesky of G (every workgroup the same arithmetic on its own copy), then Q = W L^-T for this workgroup's 256 samples into
// columns 0..c-1 of the panel; rows >= n zero
__global__ __launch_bounds__(256) void lm_q_kernel(int n, long long npad, int c, int np, const float *W, const double *G, double *panel, LmHdr *hdr)
{
    __shared__ double Ls[PG_MAX_COVARIATES][PG_MAX_COVARIATES + 1];
    for (int e = threadIdx.x; e < c * c; e += 256) {
        const int j = e / c, k = e % c;
        if (j >= k) Ls[j][k] = G[j * LM_LDG + k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int fail = 0;
        for (int j = 0; j < c; j++) {
            const double gjj = Ls[j][j];
            double s = gjj;
            for (int k = 0; k < j; k++) s = fma(-Ls[j][k], Ls[j][k], s);
            if (!(s > 1e-10 * gjj) || !isfinite(s)) { fail = 1; s = 1.0; }
            const double ljj = sqrt(s);
            Ls[j][j] = ljj;
            for (int i = j + 1; i < c; i++) {
                double t = Ls[i][j];
                for (int k = 0; k < j; k++) t = fma(-Ls[i][k], Ls[j][k], t);
                Ls[i][j] = t / ljj;
            }
        }
        if (blockIdx.x == 0) { hdr->fail = fail; hdr->pad = 0; }
    }
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npad) return;
    double *row = panel + (size_t)i * np;
    if (i >= n) {
        for (int j = 0; j < c; j++) row[j] = 0.0;
        return;
    }
    for (int j = 0; j < c; j++) {                                      // L q = w_i; the thread re-reads its own earlier writes
        double t = (double)W[(size_t)i * c + j];
        for (int k = 0; k < j; k++) t = fma(-Ls[j][k], row[k], t);
        row[j] = t / Ls[j][j];
    }
}

// D[j][k] = q_j'y_k: one workgroup per entry
__global__ __launch_bounds__(256) void lm_qty_kernel(int n, int t, int np, const double *panel, const float *Y, long long ldy, double *D)
{
    __shared__ double red[4];
    const int j = blockIdx.x / t, k = blockIdx.x % t;
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc = fma(panel[(size_t)i * np + j], (double)Y[(size_t)k * ldy + i], acc);
    acc = lm_block_sum(acc, red);
    if (threadIdx.x == 0) D[j * t + k] = acc;
}

// Y~ = Y - Q D into columns c..c+t-1 of the panel; pad columns and rows >= n zero
__global__ __launch_bounds__(256) void lm_resid_kernel(int n, long long npad, int c, int t, int np, const float *Y, long long ldy, const double *D, double *panel)
{
    __shared__ double Ds[1024];
    for (int e = threadIdx.x; e < c * t; e += 256) Ds[e] = D[e];
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npad) return;
    double *row = panel + (size_t)i * np;
    for (int k = c + t; k < np; k++) row[k] = 0.0;
    for (int k = 0; k < t; k++) {
        double r = 0.0;
        if (i < n) {
            r = (double)Y[(size_t)k * ldy + i];
            for (int j = 0; j < c; j++) r = fma(-row[j], Ds[j * t + k], r);
        }
        row[c + k] = r;
    }
}

__global__ __launch_bounds__(256) void lm_syy_kernel(int n, int c, int np, const double *panel, double *syy)
{
    __shared__ double red[4];
    const int k = blockIdx.x;
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) { const double v = panel[(size_t)i * np + c + k]; acc = fma(v, v, acc); }
    acc = lm_block_sum(acc, red);
    if (threadIdx.x == 0) syy[k] = acc;
}

// ---- the scan --------------------------------------------------------------------------------------------------------------------
struct LmArgs {
    int n, c, t, count_a1;
    long long pb, ldX, ldo;
    double df;
    const void *X;
    const double *panel, *syy;
    const LmHdr *hdr;
    float *beta, *se, *tau;
    double *F;
};

// a lane's run of 16 samples of one SNP as it is stored
template <class T, int LAY> struct LmRaw { T v[16]; };
template <class T> struct LmRaw<T, GENO_BED> { unsigned w; };   // 16 two-bit calls

// samples [i, i + 16) of SNP g (i a multiple of 16); samples >= n become the value 0 and their bytes are not read.  vec (uniform): the
// block's base and row pitch allow 16-byte (.bed: 4-byte) loads
template <class T, int LAY>
__device__ __forceinline__ void lm_load(LmRaw<T, LAY> &r, const LmArgs &a, long long g, long long i, bool vec)
{
    const T *X = static_cast<const T *>(a.X);
    if constexpr (LAY == GENO_BED) {
        const long long bpr = ((long long)a.n + 3) / 4, b0 = i >> 2;
        const unsigned char *rec = X + g * a.ldX;
        unsigned w = 0;
        if (vec && b0 + 4 <= bpr) w = *reinterpret_cast<const unsigned *>(rec + b0);
        else {
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (b0 + q < bpr) w |= (unsigned)rec[b0 + q] << (8 * q);
        }
        if (i + 16 > a.n) {                       // calls past the last sample: the code whose value is 0 (never 'missing')
            const unsigned fill = a.count_a1 ? 3u : 0u;
#pragma unroll
            for (int s = 0; s < 16; s++)
                if (i + s >= a.n) w = (w & ~(3u << (2 * s))) | (fill << (2 * s));
        }
        r.w = w;
    } else if constexpr (LAY == GENO_SNP) {
        const T *row = X + g * a.ldX + i;
        if (vec && i + 16 <= a.n) __builtin_memcpy(r.v, __builtin_assume_aligned(row, 16), 16 * sizeof(T));
        else {
#pragma unroll
            for (int s = 0; s < 16; s++) r.v[s] = (i + s < a.n) ? row[s] : T(0);
        }
    } else {
#pragma unroll
        for (int s = 0; s < 16; s++) r.v[s] = (i + s < a.n) ? X[(i + s) * a.ldX + g] : T(0);
    }
}

// element s of the run as the reference's X.astype(np.float32) value, widened to fp64; mu: the float32 imputation value of the SNP
template <class T, int LAY>
__device__ __forceinline__ double lm_val(const LmRaw<T, LAY> &r, int s, double mu, int count_a1)
{
    if constexpr (LAY == GENO_BED) {
        const unsigned code = (r.w >> (2 * s)) & 3u;
        return code == 1u ? mu : (code == 2u ? 1.0 : (((code == 3u) != (count_a1 != 0)) ? 2.0 : 0.0));
    } else {
        return (double)(float)r.v[s];
    }
}

template <class T, int LAY, int NT>
__global__ __launch_bounds__(64 * LM_WAVES) void lm_kernel(LmArgs a, bool vec)
{
    constexpr int NP = 16 * NT, LDB = NP + 1, NB = LM_KC * NP / (64 * LM_WAVES);
    // the panel chunk; row pitch NP + 1: the four k-groups of a fragment read (16 rows apart) fall on two bank halves, the floor
    // for 8-byte reads.  After the last chunk the same bytes stage the accumulators: 16 x LDB per wavefront.
    __shared__ double Bs[LM_KC * LDB];
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long g0 = ((long long)blockIdx.x * LM_WAVES + wave) * (16 * LM_RT);
    long long g[LM_RT];
#pragma unroll
    for (int rt = 0; rt < LM_RT; rt++) {
        const long long gi = g0 + 16 * rt + r;
        g[rt] = gi < a.pb ? gi : a.pb - 1;                              // spare slots re-read the last SNP
    }
    const int nchunk = (a.n + LM_KC - 1) / LM_KC;
    double mu[LM_RT];
    bool called[LM_RT];
#pragma unroll
    for (int rt = 0; rt < LM_RT; rt++) { mu[rt] = 0.0; called[rt] = true; }
    if constexpr (LAY == GENO_BED) {
        // pre-pass over the record: exact counts of het / hom-2 / missing calls (kin_bed_stats_kernel's convention); a missing call
        // takes the fp64 mean of the called genotypes rounded to float32
#pragma unroll
        for (int rt = 0; rt < LM_RT; rt++) {
            int n1 = 0, n2 = 0, nm = 0;
            for (int ch = 0; ch < nchunk; ch++) {
                LmRaw<T, LAY> w;
                lm_load<T, LAY>(w, a, g[rt], (long long)ch * LM_KC + 16 * q, vec);
                const unsigned lo = w.w & 0x55555555u, hi = (w.w >> 1) & 0x55555555u;     // low and high bit of the 16 codes
                nm += __popc(lo & ~hi);                                                  // 01
                n1 += __popc(hi & ~lo);                                                  // 10
                n2 += a.count_a1 ? 16 - __popc(lo | hi) : __popc(lo & hi);               // 00 or 11 (calls past n hold the other one)
            }
            for (int m = 16; m < 64; m <<= 1) { n1 += __shfl_xor(n1, m, 64); n2 += __shfl_xor(n2, m, 64); nm += __shfl_xor(nm, m, 64); }
            const int nc = a.n - nm;
            called[rt] = nc > 0;
            mu[rt] = nc > 0 ? (double)(float)((double)(n1 + 2 * n2) / (double)nc) : 0.0;
        }
    }

    lm_v4d acc[LM_RT][NT];
    double xx[LM_RT];
#pragma unroll
    for (int rt = 0; rt < LM_RT; rt++) {
        xx[rt] = 0.0;
#pragma unroll
        for (int ct = 0; ct < NT; ct++) acc[rt][ct] = lm_v4d{0.0, 0.0, 0.0, 0.0};
    }
    LmRaw<T, LAY> raw[LM_RT];
    double rb[NB];
    auto fetch = [&](int ch) {
#pragma unroll
        for (int rt = 0; rt < LM_RT; rt++) lm_load<T, LAY>(raw[rt], a, g[rt], (long long)ch * LM_KC + 16 * q, vec);
        const double *src = a.panel + (size_t)ch * LM_KC * NP;          // the chunk's rows are contiguous: pitch NP
#pragma unroll
        for (int m = 0; m < NB; m++) rb[m] = src[tid + 256 * m];
    };
    fetch(0);
    for (int ch = 0; ch < nchunk; ch++) {
        __syncthreads();                                                // the previous chunk's fragments have been read
#pragma unroll
        for (int m = 0; m < NB; m++) {
            const int e = tid + 256 * m;
            Bs[(e / NP) * LDB + (e % NP)] = rb[m];
        }
        double av[LM_RT][16];
#pragma unroll
        for (int rt = 0; rt < LM_RT; rt++)
#pragma unroll
            for (int s = 0; s < 16; s++) {
                av[rt][s] = lm_val<T, LAY>(raw[rt], s, mu[rt], a.count_a1);
                xx[rt] = fma(av[rt][s], av[rt][s], xx[rt]);
            }
        __syncthreads();
        if (ch + 1 < nchunk) fetch(ch + 1);                             // in flight under this chunk's products
#pragma unroll
        for (int s = 0; s < 16; s++) {
            double bf[NT];
#pragma unroll
            for (int ct = 0; ct < NT; ct++) bf[ct] = Bs[(16 * q + s) * LDB + 16 * ct + r];
#pragma unroll
            for (int rt = 0; rt < LM_RT; rt++)
#pragma unroll
                for (int ct = 0; ct < NT; ct++) acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[rt][s], bf[ct], acc[rt][ct], 0, 0, 0);
        }
    }
    __syncthreads();

    // ---- epilogue: a row tile's accumulators (C layout: column = lane & 15, row = (lane >> 4) + 4 e) into the wavefront's staging
    // rows; then lane (SNP r, phenotypes q, q + 4, ...) forms the statistics
    const bool fail = a.hdr->fail != 0;
    const double nan = __builtin_nan("");
    double *S = Bs + wave * (16 * LDB);
#pragma unroll
    for (int rt = 0; rt < LM_RT; rt++) {
#pragma unroll
        for (int ct = 0; ct < NT; ct++)
#pragma unroll
            for (int e = 0; e < 4; e++) S[(q + 4 * e) * LDB + 16 * ct + r] = acc[rt][ct][e];
        __syncthreads();
        double x2 = xx[rt];
        x2 += __shfl_xor(x2, 16, 64);
        x2 += __shfl_xor(x2, 32, 64);
        double zz = 0.0;
        for (int j = 0; j < a.c; j++) { const double z = S[r * LDB + j]; zz = fma(z, z, zz); }
        const double sxx = x2 - zz;
        const bool ok = !fail && called[rt] && isfinite(x2) && isfinite(zz) && sxx > 1e-10 * x2;
        const long long gi = g0 + 16 * rt + r;
        if (gi < a.pb) {
            for (int k = q; k < a.t; k += 4) {
                const double sxy = S[r * LDB + a.c + k], syy = a.syy[k];
                double beta = nan, se = nan, tau = nan, Fs = nan;
                if (ok && isfinite(sxy) && isfinite(syy)) {
                    const double rss = syy - (sxy * sxy) / sxx;
                    beta = sxy / sxx;
                    se = sqrt(rss / (a.df * sxx));
                    tau = a.df / rss;
                    Fs = (a.df * (sxy * sxy)) / (sxx * rss);
                }
                const size_t o = (size_t)k * a.ldo + gi;
                a.beta[o] = (float)beta; a.se[o] = (float)se; a.tau[o] = (float)tau; a.F[o] = Fs;
            }
        }
        __syncthreads();
    }
}

template <class T, int LAY>
static int launch_lm(pg_ctx *ctx, int nt, const LmArgs &a, bool vec)
{
    const unsigned grid = (unsigned)((a.pb + LM_SNPS - 1) / LM_SNPS);
    switch (nt) {
        case 1: lm_kernel<T, LAY, 1><<<grid, 64 * LM_WAVES, 0, ctx->stream>>>(a, vec); break;
        case 2: lm_kernel<T, LAY, 2><<<grid, 64 * LM_WAVES, 0, ctx->stream>>>(a, vec); break;
        case 3: lm_kernel<T, LAY, 3><<<grid, 64 * LM_WAVES, 0, ctx->stream>>>(a, vec); break;
        default: lm_kernel<T, LAY, 4><<<grid, 64 * LM_WAVES, 0, ctx->stream>>>(a, vec); break;
    }
    PG_HIP(hipGetLastError());
    return PG_OK;
}

template <class T, int LAY>
static int launch_lm_x(pg_ctx *ctx, int nt, const LmArgs &a)
{
    // 16-byte loads of a SNP-major row need the base and the row pitch on 16 bytes; the values read are the same either way
    const bool vec = LAY == GENO_SNP && ((uintptr_t)a.X % 16 == 0) && ((size_t)a.ldX * sizeof(T)) % 16 == 0;
    return launch_lm<T, LAY>(ctx, nt, a, vec);
}

// the argument checks the three entry points share (after their NULL checks); what: the entry's name
static int lm_check(const char *what, int64_t n, int c, int t)
{
    if (c < 1 || c > PG_MAX_COVARIATES) {
        set_error("%s: c=%d covariates not supported by this build (1..%d)", what, c, PG_MAX_COVARIATES);
        return PG_ENOTSUP;
    }
    PG_REQUIRE(t >= 1, "%s: t=%d phenotypes", what, t);
    if (c + t > LM_MAXP) {
        set_error("%s: c + t = %d panel columns not supported by this build (<= %d)", what, c + t, LM_MAXP);
        return PG_ENOTSUP;
    }
    PG_REQUIRE(n >= 2 && n < (1LL << 30), "%s: bad shape n=%lld", what, (long long)n);
    PG_REQUIRE(n - c - 1 > 0, "%s: n - c - 1 must be positive", what);
    return PG_OK;
}

static LmArgs lm_args(int64_t n, int c, int t, int64_t pb, const void *X, int64_t ldX, int count_a1, const void *work, float *beta, float *se,
                      float *tau, double *F, int64_t ldo)
{
    const char *base = static_cast<const char *>(work);
    LmArgs a{};
    a.n = (int)n; a.c = c; a.t = t; a.count_a1 = count_a1;
    a.pb = pb; a.ldX = ldX; a.ldo = ldo;
    a.df = (double)(n - c - 1);
    a.X = X;
    a.panel = reinterpret_cast<const double *>(base + LM_OFF_PANEL);
    a.syy = reinterpret_cast<const double *>(base + LM_OFF_SYY);
    a.hdr = reinterpret_cast<const LmHdr *>(base);
    a.beta = beta; a.se = se; a.tau = tau; a.F = F;
    return a;
}

static int lm_pvalues(pg_ctx *ctx, int64_t n, int c, int t, int64_t pb, const double *F, double *pval, int64_t ldo)
{
    const double df = (double)(n - c - 1);
    if (ldo == pb) return pg_fdist_sf_dev(ctx, (int64_t)t * pb, F, df, pval);
    for (int k = 0; k < t; k++) {
        const int rc = pg_fdist_sf_dev(ctx, pb, F + (size_t)k * ldo, df, pval + (size_t)k * ldo);
        if (rc) return rc;
    }
    return PG_OK;
}

}  // namespace pg

using namespace pg;

extern "C" size_t pg_lm_work_bytes(int64_t n, int c, int t)
{
    if (n < 1 || c < 1 || t < 1 || c + t > LM_MAXP) return 0;
    return LM_OFF_PANEL + (size_t)lm_npad(n) * lm_np(c, t) * 8;
}

extern "C" int pg_lm_setup_dev(pg_ctx *ctx, int64_t n, int c, int t, const float *W, const float *Y, int64_t ldy, void *work)
{
    PG_REQUIRE(ctx && W && Y && work, "pg_lm_setup_dev: NULL argument");
    int rc = lm_check("pg_lm_setup_dev", n, c, t);
    if (rc) return rc;
    PG_REQUIRE(ldy >= n, "pg_lm_setup_dev: ldy=%lld < n=%lld", (long long)ldy, (long long)n);
    PG_HIP(hipSetDevice(ctx->device));
    char *base = static_cast<char *>(work);
    LmHdr *hdr = reinterpret_cast<LmHdr *>(base);
    double *syy = reinterpret_cast<double *>(base + LM_OFF_SYY), *G = reinterpret_cast<double *>(base + LM_OFF_G);
    double *D = reinterpret_cast<double *>(base + LM_OFF_D), *panel = reinterpret_cast<double *>(base + LM_OFF_PANEL);
    const int np = lm_np(c, t);
    const long long npad = lm_npad(n);
    const unsigned rows = (unsigned)((npad + 255) / 256);
    lm_gram_kernel<<<c * (c + 1) / 2, 256, 0, ctx->stream>>>((int)n, c, W, G);
    PG_HIP(hipGetLastError());
    lm_q_kernel<<<rows, 256, 0, ctx->stream>>>((int)n, npad, c, np, W, G, panel, hdr);
    PG_HIP(hipGetLastError());
    lm_qty_kernel<<<c * t, 256, 0, ctx->stream>>>((int)n, t, np, panel, Y, ldy, D);
    PG_HIP(hipGetLastError());
    lm_resid_kernel<<<rows, 256, 0, ctx->stream>>>((int)n, npad, c, t, np, Y, ldy, D, panel);
    PG_HIP(hipGetLastError());
    lm_syy_kernel<<<t, 256, 0, ctx->stream>>>((int)n, c, np, panel, syy);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

extern "C" int pg_lm_x_dev(pg_ctx *ctx, int64_t n, int c, int t, int64_t pb, const void *X, int dtype, int64_t ldX, int snp_major, const void *work,
                           float *beta, float *se, float *tau, double *F, double *pval, int64_t ldo)
{
    PG_REQUIRE(ctx && X && work && beta && se && tau && F, "pg_lm_x_dev: NULL argument");
    int rc = lm_check("pg_lm_x_dev", n, c, t);
    if (rc) return rc;
    PG_REQUIRE(pb >= 0 && pb < (1LL << 31) && ldX >= (snp_major ? n : pb) && ldo >= pb, "pg_lm_x_dev: bad shape pb=%lld ldX=%lld ldo=%lld snp_major=%d",
               (long long)pb, (long long)ldX, (long long)ldo, snp_major);
    PG_REQUIRE(dtype_known(dtype), "pg_lm_x_dev: unknown dtype %d", dtype);
    if (pb == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    const LmArgs a = lm_args(n, c, t, pb, X, ldX, 0, work, beta, se, tau, F, ldo);
    const int nt = lm_np(c, t) / 16;
    rc = geno_dispatch(dtype, snp_major != 0, [&](auto src) {
        using S = decltype(src);
        return launch_lm_x<typename S::type, S::layout>(ctx, nt, a);
    });
    if (rc) return rc;
    return pval ? lm_pvalues(ctx, n, c, t, pb, F, pval, ldo) : PG_OK;
}

extern "C" int pg_lm_bed_dev(pg_ctx *ctx, int64_t n, int c, int t, int64_t pb, const unsigned char *bed, int64_t ldb, int count_a1, const void *work,
                             float *beta, float *se, float *tau, double *F, double *pval, int64_t ldo)
{
    PG_REQUIRE(ctx && bed && work && beta && se && tau && F, "pg_lm_bed_dev: NULL argument");
    int rc = lm_check("pg_lm_bed_dev", n, c, t);
    if (rc) return rc;
    PG_REQUIRE(pb >= 0 && pb < (1LL << 31) && ldb >= (n + 3) / 4 && ldo >= pb, "pg_lm_bed_dev: bad shape pb=%lld ldb=%lld ldo=%lld", (long long)pb,
               (long long)ldb, (long long)ldo);
    if (pb == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    const LmArgs a = lm_args(n, c, t, pb, bed, ldb, count_a1 != 0, work, beta, se, tau, F, ldo);
    const bool vec = ((uintptr_t)bed % 4 == 0) && ldb % 4 == 0;
    rc = launch_lm<unsigned char, GENO_BED>(ctx, lm_np(c, t) / 16, a, vec);
    if (rc) return rc;
    return pval ? lm_pvalues(ctx, n, c, t, pb, F, pval, ldo) : PG_OK;
}
