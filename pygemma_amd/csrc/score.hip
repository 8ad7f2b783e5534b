// score.hip — the score test at the null model's ML lambda (GEMMA -lmm 3), one pass over the rotated genotypes.
//
// In the eigenbasis, with lambda0 the ML lambda of y ~ W (pg_score_null_dev, assoc.hip) and h_i = 1/(lambda0 d_i + 1):
//   G  = W' H W = L L'  (fp64 Cholesky),   P0 = H - H W G^-1 W' H
//   P_xx = x'Hx - |L^-1 W'Hx|^2,   P_xy = x' P0 y,   P_yy = y'Hy - |L^-1 W'Hy|^2
// Everything that does not involve x is fixed for the call: the setup kernel writes, column-major with row pitch ldf,
//   F[0]      = h
//   F[1 + j]  = column j of B = H W L^-T           (so that B'x = L^-1 W'Hx)
//   F[1 + c]  = P0 y = h o (y - W G^-1 W'Hy)
// and P_yy.  Per SNP the scan needs c + 2 dot products of length n: s = sum h x^2, z = B'x, u = x'P0y — 4 bytes of x for
// (c + 2) fp64 fmas, so the scan is bound by HBM, not by the fp64 VALU.
//
// Tiling: one wavefront takes T SNPs (T = 8 for c <= 5, then min(8, 56 / (c + 2)): 4 at c = 10, 2 at c = 26, 1 from 27) and walks
// the samples 64 at a time, lane l owning samples l, l + 64, ...  Every fixed-vector element a wave fetches (from L2/L1)
// serves its T SNPs from registers.
// Determinism: a SNP's sums are lane-local fma chains in sample order followed by a fixed xor butterfly, the same for every slot
// of the tile, every tile and every ldx (the last, partial step masks samples >= n to exact zeros), so a row depends only on its SNP.
#include "common.hpp"

#include <cmath>

namespace pg {

constexpr int SC_LDF = 64;     // row pitch of the fixed vectors: a multiple of the wave step
constexpr int SC_WAVES = 4;    // wavefronts (= SNP tiles) per workgroup

struct ScoreHdr {
    double pyy;                // y' P0 y
    int fail;                  // the Cholesky of G failed (W rank-deficient at 1e-10 relative): every row NaN except lambda
    int pad;
};

// SNPs per wavefront: T (c + 2) <= 56 fp64 accumulators keep the scan within 256 VGPRs without scratch (c = 6 at T = 8 spilled)
__host__ __device__ constexpr int score_tile(int C) { return 56 / (C + 2) < 8 ? 56 / (C + 2) : 8; }

__device__ __forceinline__ double wave_sum(double v)
{
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);   // a + b and b + a: every lane ends with the same bits
    return v;
}

// One workgroup.  Gram entries (j >= k over the c + 1 columns [W | y]) one per wavefront at a time: lane-local fma chains over
// i = lane, lane + 64, ... then the butterfly; the Cholesky, the two triangular solves and P_yy on one thread; then B and P0 y
// element by element (each thread re-reads its own earlier writes of F: no per-thread arrays, no scratch).
__global__ __launch_bounds__(256) void score_setup_kernel(int n, int c, int ldf, const float *d, const float *Wr, const float *yr,
                                                          float lam0, double *F, ScoreHdr *hdr)
{
    __shared__ double G[PG_MAX_COVARIATES + 1][PG_MAX_COVARIATES + 1];   // lower triangle of [W | y]' H [W | y]; L after the factorisation
    __shared__ double a[PG_MAX_COVARIATES];                                // G^-1 W'Hy
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double lam = (double)lam0;
    for (int i = tid; i < ldf; i += 256) F[i] = (i < n) ? 1.0 / (lam * (double)d[i] + 1.0) : 0.0;
    __syncthreads();
    const int ne = (c + 1) * (c + 2) / 2;
    for (int e = wave; e < ne; e += SC_WAVES) {
        int j = 0;
        while ((j + 1) * (j + 2) / 2 <= e) j++;
        const int k = e - j * (j + 1) / 2;
        double acc = 0.0;
        for (int i = lane; i < n; i += 64) {
            const double cj = (double)(j < c ? Wr[(size_t)i * c + j] : yr[i]);
            const double ck = (double)(k < c ? Wr[(size_t)i * c + k] : yr[i]);
            acc = fma(F[i] * cj, ck, acc);
        }
        acc = wave_sum(acc);
        if (lane == 0) G[j][k] = acc;
    }
    __syncthreads();
    if (tid == 0) {
        int fail = 0;
        for (int j = 0; j < c; j++) {
            const double gjj = G[j][j];
            double s = gjj;
            for (int k = 0; k < j; k++) s = fma(-G[j][k], G[j][k], s);
            if (!(s > 1e-10 * gjj) || !isfinite(s)) { fail = 1; s = 1.0; }
            const double ljj = sqrt(s);
            G[j][j] = ljj;
            for (int i = j + 1; i <= c; i++) {     // row c (y) too: G[c][j] becomes (L^-1 W'Hy)_j
                double t = G[i][j];
                for (int k = 0; k < j; k++) t = fma(-G[i][k], G[j][k], t);
                G[i][j] = t / ljj;
            }
        }
        double pyy = G[c][c];
        for (int k = 0; k < c; k++) pyy = fma(-G[c][k], G[c][k], pyy);
        for (int j = c - 1; j >= 0; j--) {         // L' a = L^-1 W'Hy
            double t = G[c][j];
            for (int k = j + 1; k < c; k++) t = fma(-G[k][j], a[k], t);
            a[j] = t / G[j][j];
        }
        hdr->pyy = pyy;
        hdr->fail = fail;
        hdr->pad = 0;
    }
    __syncthreads();
    for (int i = tid; i < ldf; i += 256) {
        if (i >= n) {
            for (int j = 1; j <= c + 1; j++) F[(size_t)j * ldf + i] = 0.0;
            continue;
        }
        const double h = F[i];
        double r = (double)yr[i];
        for (int j = 0; j < c; j++) {              // L b = w_i, b kept in F until it is scaled by h
            const double wij = (double)Wr[(size_t)i * c + j];
            double t = wij;
            for (int k = 0; k < j; k++) t = fma(-G[j][k], F[(size_t)(1 + k) * ldf + i], t);
            F[(size_t)(1 + j) * ldf + i] = t / G[j][j];
            r = fma(-wij, a[j], r);
        }
        for (int j = 0; j < c; j++) F[(size_t)(1 + j) * ldf + i] *= h;
        F[(size_t)(1 + c) * ldf + i] = h * r;
    }
}

struct ScoreArgs {
    int n, ldf;
    long long p, ldx;
    double df;
    float lam0;
    const float *xr;
    const double *F;
    const ScoreHdr *hdr;
    float *beta, *se, *tau, *lam;
    double *Fs;
};

// one step of the scan: sample i of the T SNPs against the M fixed vectors (MASK: the last, partial step; samples >= n count as
// exact zeros).  One fetch of F per lane and column serves the T SNPs.
template <int C, int T, bool MASK>
__device__ __forceinline__ void score_step(const ScoreArgs &a, const float *const (&row)[T], int i, double (&acc)[T][C + 2])
{
    double xd[T];
#pragma unroll
    for (int t = 0; t < T; t++) xd[t] = (!MASK || i < a.n) ? (double)row[t][i] : 0.0;
#pragma unroll
    for (int j = 0; j < C + 2; j++) {
        const double f = a.F[(size_t)j * a.ldf + i];
#pragma unroll
        for (int t = 0; t < T; t++) acc[t][j] = (j == 0) ? fma(f * xd[t], xd[t], acc[t][j]) : fma(f, xd[t], acc[t][j]);   // s = sum h x x
    }
}

template <int C>
__global__ __launch_bounds__(64 * SC_WAVES, 2) void score_kernel(ScoreArgs a)
{
    constexpr int T = score_tile(C), M = C + 2;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long g0 = ((long long)blockIdx.x * SC_WAVES + wave) * T;
    if (g0 >= a.p) return;
    const double pyy = a.hdr->pyy;
    const bool fail = a.hdr->fail != 0;
    const float *row[T];
#pragma unroll
    for (int t = 0; t < T; t++) row[t] = a.xr + (size_t)(g0 + t < a.p ? g0 + t : a.p - 1) * a.ldx;   // spare slots re-read the last SNP
    double acc[T][M];
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int j = 0; j < M; j++) acc[t][j] = 0.0;
    if (!fail) {
        int i0 = 0;
#pragma unroll 2
        for (; i0 + 64 <= a.n; i0 += 64) score_step<C, T, false>(a, row, i0 + lane, acc);
        if (i0 < a.n) score_step<C, T, true>(a, row, i0 + lane, acc);
    }
    // one butterfly at a time: interleaved, the T M butterflies' shuffle temporaries would double the register file
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int j = 0; j < M; j++) {
            acc[t][j] = wave_sum(acc[t][j]);
            __builtin_amdgcn_sched_barrier(0);
        }
    const double nan = __builtin_nan("");
#pragma unroll
    for (int t = 0; t < T; t++) {
        const long long g = g0 + t;
        if (g >= a.p || lane != t) continue;
        const double s = acc[t][0], pxy = acc[t][C + 1];
        double zz = 0.0;
#pragma unroll
        for (int j = 1; j <= C; j++) zz = fma(acc[t][j], acc[t][j], zz);
        const double pxx = s - zz;
        double beta = nan, se = nan, tau = nan, Fs = nan;
        if (!fail && isfinite(s) && isfinite(zz) && isfinite(pxy) && pxx > 1e-10 * s) {
            const double pxyy = pyy - (pxy * pxy) / pxx;
            beta = pxy / pxx;
            se = sqrt(pxyy / (a.df * pxx));
            tau = a.df / pxyy;
            Fs = ((double)a.n * (pxy * pxy)) / (pyy * pxx);
        }
        a.beta[g] = (float)beta; a.se[g] = (float)se; a.tau[g] = (float)tau; a.lam[g] = a.lam0; a.Fs[g] = Fs;
    }
}

template <int C>
static int launch_score(pg_ctx *ctx, const ScoreArgs &a)
{
    constexpr int T = score_tile(C);
    const long long per = (long long)T * SC_WAVES;
    score_kernel<C><<<(unsigned)((a.p + per - 1) / per), 64 * SC_WAVES, 0, ctx->stream>>>(a);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

static int launch_score_any(pg_ctx *ctx, int c, const ScoreArgs &a)
{
#define PG_SCASE(C) case C: return launch_score<C>(ctx, a);
    switch (c) {
        PG_SCASE(1) PG_SCASE(2) PG_SCASE(3) PG_SCASE(4) PG_SCASE(5) PG_SCASE(6) PG_SCASE(7) PG_SCASE(8) PG_SCASE(9) PG_SCASE(10)
        PG_SCASE(11) PG_SCASE(12) PG_SCASE(13) PG_SCASE(14) PG_SCASE(15) PG_SCASE(16) PG_SCASE(17) PG_SCASE(18) PG_SCASE(19) PG_SCASE(20)
        PG_SCASE(21) PG_SCASE(22) PG_SCASE(23) PG_SCASE(24) PG_SCASE(25) PG_SCASE(26) PG_SCASE(27) PG_SCASE(28) PG_SCASE(29) PG_SCASE(30)
        default: return PG_ENOTSUP;
    }
#undef PG_SCASE
}

}  // namespace pg

using namespace pg;

extern "C" int pg_score_dev(pg_ctx *ctx, int64_t n, int c, int64_t p, const float *d, const float *Wr, const float *yr, float lambda0,
                            const float *Xr, int64_t ldx, float *beta, float *se, float *tau, float *lambda, double *F, double *pval)
{
    PG_REQUIRE(ctx && d && Wr && yr && Xr && beta && se && tau && lambda && F, "pg_score_dev: NULL argument");
    PG_REQUIRE(n >= 2 && n < (1LL << 30) && p >= 0 && ldx >= n, "pg_score_dev: bad shape n=%lld p=%lld ldx=%lld", (long long)n, (long long)p,
               (long long)ldx);
    if (c < 1 || c > PG_MAX_COVARIATES) {
        set_error("pg_score_dev: c=%d covariates not supported by this build (1..%d)", c, PG_MAX_COVARIATES);
        return PG_ENOTSUP;
    }
    PG_REQUIRE(n - c - 1 > 0, "pg_score_dev: n - c - 1 must be positive");
    if (p == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    const int ldf = (int)((n + SC_LDF - 1) / SC_LDF * SC_LDF);
    const size_t off_hdr = (size_t)(c + 2) * ldf * 8;
    int rc = ensure(ctx, &ctx->score, &ctx->score_bytes, off_hdr + 256);
    if (rc) return rc;
    double *Fx = (double *)ctx->score;
    ScoreHdr *hdr = (ScoreHdr *)((char *)ctx->score + off_hdr);
    score_setup_kernel<<<1, 256, 0, ctx->stream>>>((int)n, c, ldf, d, Wr, yr, lambda0, Fx, hdr);
    PG_HIP(hipGetLastError());
    ScoreArgs a{};
    a.n = (int)n; a.ldf = ldf; a.p = p; a.ldx = ldx; a.df = (double)(n - c - 1); a.lam0 = lambda0;
    a.xr = Xr; a.F = Fx; a.hdr = hdr;
    a.beta = beta; a.se = se; a.tau = tau; a.lam = lambda; a.Fs = F;
    rc = launch_score_any(ctx, c, a);
    if (rc) return rc;
    if (pval) return pg_fdist_sf_dev(ctx, p, F, (double)(n - c - 1), pval);
    return PG_OK;
}
