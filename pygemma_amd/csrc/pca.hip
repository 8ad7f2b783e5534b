// pca.hip — the two skinny products of a randomised PCA against the standardised genotypes Z, straight from raw genotypes (packed .bed
// records, 8-bit, float32 or float64 blocks, sample- or SNP-major):  T = Z'Q (pg_pca_proj_*) and Y += Z T (pg_pca_back_*), chained
// through component-major panels (component k of sample i at Q[k ldq + i], of SNP g at T[k ldt + g]), so that the output of one is
// the input of the other.  lmm.pca iterates them; lmm.pca_project is one stream of the second.
//
// Values: an element is first rounded to float32; .bed code 01 and NaN / +-Inf are missing (an 8-bit block has no missing code).  With
// stat[2 g] = mu_g and stat[2 g + 1] = isd_g,  z_gi = fl(fl(x_gi - mu_g) isd_g)  in fp64, two roundings, and 0 for a missing call, a
// sample >= n and a SNP >= pb.  pg_pca_stat_* fills stat from the QC pre-pass (pg_snp_stats_*_dev): mu_g its mean, bit for bit (0
// without a called sample), v = var_g (n_obs / n) — the population variance over all n samples after mean imputation, what
// lmm.kinship(standardize=True) divides by — and isd_g = v > 0 ? 1 / sqrt(v) : 0.  stat is an input of both products: new samples
// are projected with the training panel's moments.
//
// proj, T[k][g] = sum_i z_gi Q[k][i], on v_mfma_f64_16x16x4_f64 with the samples as K, the components as M and the SNPs as N
// (lm.hip's tiling with the operands swapped, so that a store runs along g):
//   A lane (r, q) = Q[16 ct + r][sample],  B lane (c, q) = z[SNP 16 rt + c][sample],  C lane (c, q) reg e = T[16 ct + q + 4 e][SNP c].
// A workgroup of four wavefronts owns 128 SNPs (two 16-SNP tiles per wavefront) and walks the samples 64 at a time; the 64 x l chunk
// of Q is shared through LDS.  Inside a chunk lane (., q) takes the contiguous run of samples 16 q .. 16 q + 15 of its SNP (4 bytes
// of a .bed record, 64 of a float32 row) and MFMA step s multiplies sample 16 q + s.  A hard-call record tabulates its three z values.
// An output is one fixed chain — chunk after chunk, step after step, the four k-groups inside the instruction — that depends only
// on the SNP, its stat and Q: not on the SNP's slot, tile, batch, pitch, alignment or storage.  No split over samples, no atomics.
//
// back, Y[k][i] += sum_g z_gi T[k][g], with the SNPs as K, the components as M and the samples as N — prs.hip's schedule with z in
// the place of x and T in the place of the weights:
//   A lane (r, q) = T[16 mt + r][SNP],  B lane (c, q) = z[SNP][sample 16 nt + c],  C lane (c, q) reg e = Y[16 mt + q + 4 e][sample c].
// A wavefront owns 64 adjacent samples and 16 or 32 components, a workgroup 256 samples and one chunk of PG_PCA_CHUNK SNPs counted
// from the block's first; the chunk's partial is one MFMA chain from zero (groups of 16 SNPs in order, lane (., q) the run 4 q .. 4 q + 3,
// steps 0..3) and a second kernel adds the partials to Y in ascending chunk order: split-K, no atomics.  Y does not depend on the batch
// sizes when every batch but the last holds a multiple of PG_PCA_CHUNK SNPs.
#include "geno_src.hpp"

#include <cmath>
#include <type_traits>

namespace pg {

constexpr int PCA_KC = 64;                              // proj: samples per chunk, 4 k-groups of 16
constexpr int PCA_RT = 2;                               // proj: 16-SNP tiles per wavefront
constexpr int PCA_WAVES = 4;
constexpr int PCA_SNPS = 16 * PCA_RT * PCA_WAVES;       // proj: SNPs per workgroup
constexpr int PCA_NT = 4;                               // back: 16-sample tiles per wavefront
constexpr int PCA_ROWS = 16 * PCA_NT * PCA_WAVES;       // back: samples per workgroup
constexpr long long PCA_MAXPB = 1LL << 25;
constexpr long long PCA_MAXGRID = 1LL << 31;            // workgroups per launch, exclusive

typedef double pca_v4d __attribute__((ext_vector_type(4)));

struct PcaArgs {
    int n, l, count_a1;
    long long pb, ldX, ldq, ldt, ldy, ldp, ngroups;
    const void *X;
    const double *stat;        // [pb][2] mu, isd
    const double *Q;           // proj: l rows of ldq
    const double *Tin;         // back: l rows of ldt
    double *Tout;              // proj
    double *Y;                 // back
    double *ps;                // back: chunk partials [chunk][l][ldp]
};

static inline long long pca_chunks(long long pb) { return (pb + PG_PCA_CHUNK - 1) / PG_PCA_CHUNK; }
static inline long long pca_groups(long long n) { return (n + PCA_ROWS - 1) / PCA_ROWS; }

struct PcaWork {
    long long *counts;     // [pb][4] the pre-pass's outputs
    double *moments;       // [pb][4]
    void *ss;              // the pre-pass's own work area
    double *ps;            // [chunks][l][ldp]
    size_t bytes;
};

// the pre-pass's part comes first and does not depend on l: pg_pca_stat_* takes the work area of any l
static PcaWork pca_work(void *work, long long n, long long pb, int l)
{
    char *b = static_cast<char *>(work);
    PcaWork w;
    size_t o = 0;
    w.counts = reinterpret_cast<long long *>(b + o); o += up256((size_t)pb * 32);
    w.moments = reinterpret_cast<double *>(b + o); o += up256((size_t)pb * 32);
    w.ss = b + o; o += up256(pg_snp_stats_work_bytes(n, pb));
    w.ps = reinterpret_cast<double *>(b + o); o += up256((size_t)pca_chunks(pb) * l * ((n + 15) / 16 * 16) * 8);
    w.bytes = o + 256;
    return w;
}

// z of a stored element: v the element, in: its SNP and sample exist
template <class T>
__device__ __forceinline__ double pca_z(T v, bool in, double mu, double isd)
{
    if constexpr (std::is_floating_point<T>::value) {
        const float f = (float)v;
        return (in && isfinite(f)) ? ((double)f - mu) * isd : 0.0;
    } else {
        return in ? ((double)v - mu) * isd : 0.0;
    }
}

// the dosage of a called .bed code (0, 2 or 3)
__device__ __forceinline__ double pca_bed_x(unsigned code, int count_a1)
{
    return code == 2u ? 1.0 : (((code == 3u) != (count_a1 != 0)) ? 2.0 : 0.0);
}

__global__ __launch_bounds__(256) void pca_stat_kernel(long long pb, long long n, const long long *counts, const double *moments, double *stat)
{
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= pb) return;
    const long long n_obs = n - counts[4 * g];
    const double v = moments[4 * g + 1] * ((double)n_obs / (double)n);
    stat[2 * g] = n_obs > 0 ? moments[4 * g] : 0.0;
    stat[2 * g + 1] = v > 0.0 ? 1.0 / sqrt(v) : 0.0;                    // an all-missing SNP: var is NaN, v > 0 is false
}

// ---- proj ---------------------------------------------------------------------------------------------------------------------------

// a lane's run of 16 samples of one SNP as it is stored
template <class T, int LAY> struct PcaRun { T v[16]; };
template <class T> struct PcaRun<T, GENO_BED> { unsigned w; };   // 16 two-bit calls

// samples [i, i + 16) of SNP g (i a multiple of 16); the bytes of samples >= n are not read.  vec (uniform): the block's base and row
// pitch allow 16-byte (.bed: 4-byte) loads
template <class T, int LAY>
__device__ __forceinline__ void pca_run_load(PcaRun<T, LAY> &r, const PcaArgs &a, long long g, long long i, bool vec)
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
        if (i + 16 > a.n) {                       // calls past the last sample: 'missing', whose z is 0
#pragma unroll
            for (int s = 0; s < 16; s++)
                if (i + s >= a.n) w = (w & ~(3u << (2 * s))) | (1u << (2 * s));
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

// workgroup: SNPs [128 blockIdx.x, 128 (blockIdx.x + 1)), all l = up to 16 CT components.  Two wavefronts per SIMD keep the accumulators
// in VGPRs (from AGPRs this MFMA issues at half its rate); a float64 block's runs of 16, and the sixteen row addresses
// of a sample-major run beside three or four column tiles, need the whole register file: one wavefront per SIMD, nothing spilled
template <class T, int LAY, int CT>
__global__ __launch_bounds__(64 * PCA_WAVES, (sizeof(T) == 8 || (LAY == GENO_SAMPLE && CT >= 3)) ? 1 : 2) void pca_proj_kernel(PcaArgs a, bool vec)
{
    constexpr int NP = 16 * CT, LDB = NP + 1, NB = PCA_KC * NP / (64 * PCA_WAVES);
    // the chunk of Q, [sample][component] at row pitch NP + 1: the four k-groups of a fragment read (16 rows apart) fall on two bank
    // halves, the floor for 8-byte reads, and the transposing writes (a lane per sample) on distinct banks
    __shared__ double Qs[PCA_KC * LDB];
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long g0 = ((long long)blockIdx.x * PCA_WAVES + wave) * (16 * PCA_RT);
    long long g[PCA_RT];
    double mu[PCA_RT], isd[PCA_RT], zt[PCA_RT][4];
#pragma unroll
    for (int rt = 0; rt < PCA_RT; rt++) {
        const long long gi = g0 + 16 * rt + r;
        g[rt] = gi < a.pb ? gi : a.pb - 1;                              // spare slots re-read the last SNP
        mu[rt] = a.stat[2 * g[rt]];
        isd[rt] = a.stat[2 * g[rt] + 1];
        if constexpr (LAY == GENO_BED) {                                // the z of the four codes: the same two roundings
#pragma unroll
            for (unsigned code = 0; code < 4; code++) zt[rt][code] = code == 1u ? 0.0 : (pca_bed_x(code, a.count_a1) - mu[rt]) * isd[rt];
        }
    }
    const int nchunk = (a.n + PCA_KC - 1) / PCA_KC;
    pca_v4d acc[PCA_RT][CT];
#pragma unroll
    for (int rt = 0; rt < PCA_RT; rt++)
#pragma unroll
        for (int ct = 0; ct < CT; ct++) acc[rt][ct] = pca_v4d{0.0, 0.0, 0.0, 0.0};
    PcaRun<T, LAY> raw[PCA_RT];
    double rb[NB];
    auto fetch = [&](int ch) {
#pragma unroll
        for (int rt = 0; rt < PCA_RT; rt++) pca_run_load<T, LAY>(raw[rt], a, g[rt], (long long)ch * PCA_KC + 16 * q, vec);
#pragma unroll
        for (int m = 0; m < NB; m++) {                                  // element (component 4 m + wave, sample lane) of the chunk
            const int k = 4 * m + wave;
            const long long i = (long long)ch * PCA_KC + lane;
            rb[m] = (k < a.l && i < a.n) ? a.Q[(long long)k * a.ldq + i] : 0.0;
        }
    };
    fetch(0);
    for (int ch = 0; ch < nchunk; ch++) {
        __syncthreads();                                                // the previous chunk's fragments have been read
#pragma unroll
        for (int m = 0; m < NB; m++) Qs[lane * LDB + 4 * m + wave] = rb[m];
        const long long i0 = (long long)ch * PCA_KC + 16 * q;
        double zv[PCA_RT][16];
#pragma unroll
        for (int rt = 0; rt < PCA_RT; rt++)
#pragma unroll
            for (int s = 0; s < 16; s++) {
                if constexpr (LAY == GENO_BED) {
                    const unsigned code = (raw[rt].w >> (2 * s)) & 3u;
                    zv[rt][s] = code == 0u ? zt[rt][0] : (code == 2u ? zt[rt][2] : (code == 3u ? zt[rt][3] : 0.0));
                } else {
                    zv[rt][s] = pca_z<T>(raw[rt].v[s], i0 + s < a.n, mu[rt], isd[rt]);
                }
            }
        __syncthreads();
        if (ch + 1 < nchunk) fetch(ch + 1);                             // in flight under this chunk's products
#pragma unroll
        for (int s = 0; s < 16; s++) {
            double qf[CT];
#pragma unroll
            for (int ct = 0; ct < CT; ct++) qf[ct] = Qs[(16 * q + s) * LDB + 16 * ct + r];
#pragma unroll
            for (int rt = 0; rt < PCA_RT; rt++)
#pragma unroll
                for (int ct = 0; ct < CT; ct++) acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(qf[ct], zv[rt][s], acc[rt][ct], 0, 0, 0);
        }
    }
    // C layout: SNP = lane & 15, component = (lane >> 4) + 4 e: sixteen lanes store 128 adjacent bytes of a row of T
#pragma unroll
    for (int rt = 0; rt < PCA_RT; rt++) {
        const long long gi = g0 + 16 * rt + r;
#pragma unroll
        for (int ct = 0; ct < CT; ct++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int k = 16 * ct + q + 4 * e;
                if (gi < a.pb && k < a.l) a.Tout[(long long)k * a.ldt + gi] = acc[rt][ct][e];
            }
    }
}

template <class T, int LAY>
static int launch_proj(pg_ctx *ctx, const PcaArgs &a, bool vec)
{
    const unsigned grid = (unsigned)((a.pb + PCA_SNPS - 1) / PCA_SNPS);
    switch ((a.l + 15) / 16) {
        case 1: pca_proj_kernel<T, LAY, 1><<<grid, 64 * PCA_WAVES, 0, ctx->stream>>>(a, vec); break;
        case 2: pca_proj_kernel<T, LAY, 2><<<grid, 64 * PCA_WAVES, 0, ctx->stream>>>(a, vec); break;
        case 3: pca_proj_kernel<T, LAY, 3><<<grid, 64 * PCA_WAVES, 0, ctx->stream>>>(a, vec); break;
        default: pca_proj_kernel<T, LAY, 4><<<grid, 64 * PCA_WAVES, 0, ctx->stream>>>(a, vec); break;
    }
    PG_HIP(hipGetLastError());
    return PG_OK;
}

// ---- back ---------------------------------------------------------------------------------------------------------------------------

// the four SNPs g .. g + 3 of sample i as they are stored; it: the first sample of i's N-tile.  SNPs >= pb and samples >= n are not read
template <class T, int LAY> struct PcaQuad { T v[4]; };
template <class T> struct PcaQuad<T, GENO_BED> { unsigned w[4]; };      // the N-tile's 16 two-bit calls of each SNP

template <class T, int LAY>
__device__ __forceinline__ void pca_quad_load(PcaQuad<T, LAY> &r, const PcaArgs &a, long long g, long long i, long long it, bool vec)
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

// workgroup: chunk blockIdx.x / ngroups, samples [256 grp, 256 (grp + 1)) with grp = blockIdx.x % ngroups, and the components
// [16 MT blockIdx.y, 16 MT (blockIdx.y + 1))
template <class T, int LAY, int MT>
__global__ __launch_bounds__(64 * PCA_WAVES, 2) void pca_back_kernel(PcaArgs a, bool vec)
{
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), k0 = 16 * MT * blockIdx.y;
    const long long grp = blockIdx.x % a.ngroups, ch = blockIdx.x / a.ngroups;
    const long long i0 = grp * PCA_ROWS + (long long)wave * (16 * PCA_NT);
    if (i0 >= a.n) return;                                             // whole wavefronts leave; nothing below synchronises
    const long long gb = ch * PG_PCA_CHUNK;
    const int ngrp = (int)((min(a.pb, gb + PG_PCA_CHUNK) - gb + 15) / 16);
    pca_v4d acc[PCA_NT][MT];
#pragma unroll
    for (int nt = 0; nt < PCA_NT; nt++)
#pragma unroll
        for (int mt = 0; mt < MT; mt++) acc[nt][mt] = pca_v4d{0.0, 0.0, 0.0, 0.0};
    // the lane's run of four SNPs of group gi as stored, their moments and T: fetched one group ahead, in flight under the products
    PcaQuad<T, LAY> rawN[PCA_NT];
    double tN[MT][4], muN[4], isdN[4];
    auto fetch = [&](int gi) {
        const long long g = gb + 16 * gi + 4 * q;
#pragma unroll
        for (int nt = 0; nt < PCA_NT; nt++) pca_quad_load<T, LAY>(rawN[nt], a, g, i0 + 16 * nt + c, i0 + 16 * nt, vec);
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const bool in = g + s < a.pb;
            muN[s] = in ? a.stat[2 * (g + s)] : 0.0;
            isdN[s] = in ? a.stat[2 * (g + s) + 1] : 0.0;
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                const int k = k0 + 16 * mt + c;
                tN[mt][s] = (k < a.l && in) ? a.Tin[(long long)k * a.ldt + g + s] : 0.0;
            }
        }
    };
    fetch(0);
    for (int gi = 0; gi < ngrp; gi++) {
        const long long g = gb + 16 * gi + 4 * q;
        PcaQuad<T, LAY> raw[PCA_NT];
        double t[MT][4], mu[4], isd[4];
#pragma unroll
        for (int nt = 0; nt < PCA_NT; nt++) raw[nt] = rawN[nt];
#pragma unroll
        for (int s = 0; s < 4; s++) {
            mu[s] = muN[s];
            isd[s] = isdN[s];
#pragma unroll
            for (int mt = 0; mt < MT; mt++) t[mt][s] = tN[mt][s];
        }
        if (gi + 1 < ngrp) fetch(gi + 1);
#pragma unroll
        for (int s = 0; s < 4; s++) {
            double z[PCA_NT];
#pragma unroll
            for (int nt = 0; nt < PCA_NT; nt++) {
                const bool in = g + s < a.pb && i0 + 16 * nt + c < a.n;
                if constexpr (LAY == GENO_BED) {
                    const unsigned code = (raw[nt].w[s] >> (2 * c)) & 3u;
                    z[nt] = (in && code != 1u) ? (pca_bed_x(code, a.count_a1) - mu[s]) * isd[s] : 0.0;
                } else {
                    z[nt] = pca_z<T>(raw[nt].v[s], in, mu[s], isd[s]);
                }
            }
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int nt = 0; nt < PCA_NT; nt++) acc[nt][mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(t[mt][s], z[nt], acc[nt][mt], 0, 0, 0);
        }
    }
    // the chunk's partial (C layout: sample = lane & 15, component = (lane >> 4) + 4 e) into the work area
#pragma unroll
    for (int nt = 0; nt < PCA_NT; nt++) {
        const long long i = i0 + 16 * nt + c;
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int k = k0 + 16 * mt + q + 4 * e;
                if (i >= a.n || k >= a.l) continue;
                a.ps[((size_t)ch * a.l + k) * a.ldp + i] = acc[nt][mt][e];
            }
    }
}

// second stage: one lane per (component, sample) adds the chunks 0..R-1 onto Y in order
__global__ __launch_bounds__(256) void pca_reduce_kernel(PcaArgs a, long long nchunk)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (i >= a.n) return;
    const size_t o = (size_t)k * a.ldy + i;
    double s = a.Y[o];
    for (long long ch = 0; ch < nchunk; ch++) s = s + a.ps[((size_t)ch * a.l + k) * a.ldp + i];
    a.Y[o] = s;
}

template <class T, int LAY>
static int launch_back(pg_ctx *ctx, const PcaArgs &a, bool vec)
{
    const long long nchunk = pca_chunks(a.pb);
    // 32 fp64 accumulators a lane at most (two M-tiles of four N-tiles), in VGPRs at two wavefronts per SIMD; further components take
    // further rows of workgroups, which re-read the genotypes from L2
    const int mt = a.l <= 16 ? 1 : 2;
    const dim3 grid((unsigned)(a.ngroups * nchunk), (unsigned)((a.l + 16 * mt - 1) / (16 * mt)));
    if (mt == 1) pca_back_kernel<T, LAY, 1><<<grid, 64 * PCA_WAVES, 0, ctx->stream>>>(a, vec);
    else pca_back_kernel<T, LAY, 2><<<grid, 64 * PCA_WAVES, 0, ctx->stream>>>(a, vec);
    PG_HIP(hipGetLastError());
    pca_reduce_kernel<<<dim3((unsigned)((a.n + 255) / 256), (unsigned)a.l), 256, 0, ctx->stream>>>(a, nchunk);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

// ---- entry points: one body per product, whatever the storage -----------------------------------------------------------------------------

// a block as an entry point received it
struct PcaBlock {
    const void *X;
    int64_t ld;
    bool bed;
    int count_a1, dtype, snp_major;
};

static inline bool pca_shape_ok(int64_t n, int64_t pb) { return n >= 1 && n < (1LL << 30) && pb >= 0 && pb <= PCA_MAXPB; }

// the checks every entry point shares (after its NULL checks); what: the entry's name
static int pca_check_block(const char *what, int64_t n, int64_t pb, const PcaBlock &b)
{
    PG_REQUIRE(pca_shape_ok(n, pb), "%s: bad shape n=%lld pb=%lld", what, (long long)n, (long long)pb);
    PG_REQUIRE(pca_groups(n) * pca_chunks(pb) < PCA_MAXGRID, "%s: a block of n=%lld x pb=%lld is more than one launch holds (%lld workgroups)", what,
               (long long)n, (long long)pb, PCA_MAXGRID);
    if (b.bed) PG_REQUIRE(b.ld >= (n + 3) / 4, "%s: ldb=%lld < ceil(n / 4), n=%lld", what, (long long)b.ld, (long long)n);
    else PG_REQUIRE(b.ld >= (b.snp_major ? n : pb), "%s: ldX=%lld too small for n=%lld pb=%lld snp_major=%d", what, (long long)b.ld, (long long)n,
                    (long long)pb, b.snp_major);
    if (!b.bed && !dtype_known(b.dtype)) {
        set_error("%s: unknown dtype %d", what, b.dtype);
        return PG_ENOTSUP;
    }
    return PG_OK;
}

static int pca_check_l(const char *what, int l)
{
    PG_REQUIRE(l >= 1, "%s: bad l=%d", what, l);
    if (l > PG_PCA_MAX_L) {
        set_error("%s: l=%d columns not supported by this build (<= %d per call)", what, l, PG_PCA_MAX_L);
        return PG_ENOTSUP;
    }
    return PG_OK;
}

// f(GenoSrc<T, LAYOUT>(), vec) for the block; wide: the kernel reads runs of 16 elements of a SNP-major row
template <class F> static int pca_dispatch(const PcaBlock &b, bool wide, F &&f)
{
    if (b.bed) return f(GenoSrc<unsigned char, GENO_BED>(), ((uintptr_t)b.X % 4 == 0) && b.ld % 4 == 0);
    return geno_dispatch(b.dtype, b.snp_major != 0, [&](auto src) {
        using S = decltype(src);
        const size_t esz = sizeof(typename S::type);
        return f(src, wide && S::layout == GENO_SNP && (uintptr_t)b.X % 16 == 0 && ((size_t)b.ld * esz) % 16 == 0);
    });
}

static PcaArgs pca_args(int64_t n, int64_t pb, const PcaBlock &b, const double *stat, int l)
{
    PcaArgs a{};
    a.n = (int)n; a.l = l; a.count_a1 = b.count_a1 != 0;
    a.pb = pb; a.ldX = b.ld; a.ldp = (n + 15) / 16 * 16; a.ngroups = pca_groups(n);
    a.X = b.X; a.stat = stat;
    return a;
}

static int pca_stat(const char *what, pg_ctx *ctx, int64_t n, int64_t pb, const PcaBlock &b, void *work, double *stat)
{
    PG_REQUIRE(ctx && b.X && work && stat, "%s: NULL argument", what);
    int rc = pca_check_block(what, n, pb, b);
    if (rc) return rc;
    if (pb == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    const PcaWork w = pca_work(work, n, pb, 1);
    rc = b.bed ? pg_snp_stats_bed_dev(ctx, n, pb, static_cast<const unsigned char *>(b.X), b.ld, b.count_a1, w.ss, reinterpret_cast<int64_t *>(w.counts),
                                      w.moments)
               : pg_snp_stats_x_dev(ctx, n, pb, b.X, b.dtype, b.ld, b.snp_major, w.ss, reinterpret_cast<int64_t *>(w.counts), w.moments);
    if (rc) {                                                          // in the name of the entry that made the call
        char msg[400];
        snprintf(msg, sizeof msg, "%s", pg_last_error());
        set_error("%s: the pre-pass over the block was refused: %s", what, msg);
        return rc;
    }
    pca_stat_kernel<<<(unsigned)((pb + 255) / 256), 256, 0, ctx->stream>>>(pb, n, w.counts, w.moments, stat);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

static int pca_proj(const char *what, pg_ctx *ctx, int64_t n, int64_t pb, const PcaBlock &b, const double *stat, int l, const double *Q, int64_t ldq,
                    double *T, int64_t ldt)
{
    PG_REQUIRE(ctx && b.X && stat && Q && T, "%s: NULL argument", what);
    int rc = pca_check_block(what, n, pb, b);
    if (!rc) rc = pca_check_l(what, l);
    if (rc) return rc;
    PG_REQUIRE(ldq >= n && ldt >= pb, "%s: strides too small: ldq=%lld < n=%lld or ldt=%lld < pb=%lld", what, (long long)ldq, (long long)n,
               (long long)ldt, (long long)pb);
    if (pb == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    PcaArgs a = pca_args(n, pb, b, stat, l);
    a.Q = Q; a.ldq = ldq; a.Tout = T; a.ldt = ldt;
    return pca_dispatch(b, true, [&](auto src, bool vec) {
        using S = decltype(src);
        return launch_proj<typename S::type, S::layout>(ctx, a, vec);
    });
}

static int pca_back(const char *what, pg_ctx *ctx, int64_t n, int64_t pb, const PcaBlock &b, const double *stat, int l, const double *T, int64_t ldt,
                    void *work, double *Y, int64_t ldy)
{
    PG_REQUIRE(ctx && b.X && stat && T && work && Y, "%s: NULL argument", what);
    int rc = pca_check_block(what, n, pb, b);
    if (!rc) rc = pca_check_l(what, l);
    if (rc) return rc;
    PG_REQUIRE(ldt >= pb && ldy >= n, "%s: strides too small: ldt=%lld < pb=%lld or ldy=%lld < n=%lld", what, (long long)ldt, (long long)pb,
               (long long)ldy, (long long)n);
    if (pb == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    PcaArgs a = pca_args(n, pb, b, stat, l);
    a.Tin = T; a.ldt = ldt; a.Y = Y; a.ldy = ldy; a.ps = pca_work(work, n, pb, l).ps;
    return pca_dispatch(b, false, [&](auto src, bool vec) {
        using S = decltype(src);
        return launch_back<typename S::type, S::layout>(ctx, a, vec);
    });
}

}  // namespace pg

using namespace pg;

extern "C" size_t pg_pca_work_bytes(int64_t n, int64_t pb, int l)
{
    if (!pca_shape_ok(n, pb) || l < 1 || l > PG_PCA_MAX_L || pca_groups(n) * pca_chunks(pb) >= PCA_MAXGRID) return 0;
    return pca_work(nullptr, n, pb, l).bytes;
}

extern "C" int pg_pca_stat_bed_dev(pg_ctx *ctx, int64_t n, int64_t pb, const unsigned char *bed, int64_t ldb, int count_a1, void *work, double *stat)
{
    return pca_stat("pg_pca_stat_bed_dev", ctx, n, pb, PcaBlock{bed, ldb, true, count_a1, 0, 1}, work, stat);
}

extern "C" int pg_pca_stat_x_dev(pg_ctx *ctx, int64_t n, int64_t pb, const void *X, int dtype, int64_t ldX, int snp_major, void *work, double *stat)
{
    return pca_stat("pg_pca_stat_x_dev", ctx, n, pb, PcaBlock{X, ldX, false, 0, dtype, snp_major}, work, stat);
}

extern "C" int pg_pca_proj_bed_dev(pg_ctx *ctx, int64_t n, int64_t pb, const unsigned char *bed, int64_t ldb, int count_a1, const double *stat, int l,
                                   const double *Q, int64_t ldq, double *T, int64_t ldt)
{
    return pca_proj("pg_pca_proj_bed_dev", ctx, n, pb, PcaBlock{bed, ldb, true, count_a1, 0, 1}, stat, l, Q, ldq, T, ldt);
}

extern "C" int pg_pca_proj_x_dev(pg_ctx *ctx, int64_t n, int64_t pb, const void *X, int dtype, int64_t ldX, int snp_major, const double *stat, int l,
                                 const double *Q, int64_t ldq, double *T, int64_t ldt)
{
    return pca_proj("pg_pca_proj_x_dev", ctx, n, pb, PcaBlock{X, ldX, false, 0, dtype, snp_major}, stat, l, Q, ldq, T, ldt);
}

extern "C" int pg_pca_back_bed_dev(pg_ctx *ctx, int64_t n, int64_t pb, const unsigned char *bed, int64_t ldb, int count_a1, const double *stat, int l,
                                   const double *T, int64_t ldt, void *work, double *Y, int64_t ldy)
{
    return pca_back("pg_pca_back_bed_dev", ctx, n, pb, PcaBlock{bed, ldb, true, count_a1, 0, 1}, stat, l, T, ldt, work, Y, ldy);
}

extern "C" int pg_pca_back_x_dev(pg_ctx *ctx, int64_t n, int64_t pb, const void *X, int dtype, int64_t ldX, int snp_major, const double *stat, int l,
                                 const double *T, int64_t ldt, void *work, double *Y, int64_t ldy)
{
    return pca_back("pg_pca_back_x_dev", ctx, n, pb, PcaBlock{X, ldX, false, 0, dtype, snp_major}, stat, l, T, ldt, work, Y, ldy);
}
