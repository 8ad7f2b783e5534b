// kinship.hip — the relatedness matrix K = Z Z' / p accumulated on the device over SNP batches, from packed PLINK
// .bed records, 8-bit or float genotype blocks, sample- or SNP-major.
//
// Per SNP j (fp64 statistics over all n samples after mean imputation): mu_j, population variance var_j, shift s_j = mu_j
// (standardize) or 0, weight w_j = 1/var_j (standardize, var_j > 0) or 1.  With x_ij the imputed value, z_ij = x_ij - s_j and
// R_kj = w_j z_kj:
//     p K_ik = sum_j z_ij R_kj = sum_j c_ij R_kj + sum_j m_ij ((mu_j - r_j) R_kj) - sum_j (s_j - r_j) R_kj
// r_j = rint(mu_j), c = the value itself minus r_j (0/1/2 codes of a .bed record, an int8/uint8 value: an integer in [-255, 255],
// exact in fp16; 0 for a missing call), m = the 0/1 missing-call indicator.  Centring c on r_j keeps the uncentred part of the
// fp32 sum at |mu_j - r_j| <= 1/2 of R: with c itself, a hom-2 sample against a singleton het among hom-2 calls (R ~ -n) put -2n
// into the sum for the rank-1 term to cancel.  The first two sums are ONE fp16 GEMM over 2 kts K-tiles ([c | m] against
// [R | (mu - r) R]; the indicator half only for a batch with a missing call), R and (mu - r) R each split by round-to-nearest into
// two fp16 planes of S*R (S one power of two per batch: S * w_j max|x - s_j| max(1, |mu_j - r_j|) over all its SNPs in
// [2^14, 2^15) — the (mu - r) R planes are written for every SNP once any has a missing call — so no plane reaches fp16's 65 504
// whatever n; R reaches about n for a singleton het), fp32
// accumulation — the rotation's kernel and error class (rotate_geno.hip: geno_gemm_body).  The last sum is a rank-1 term, computed
// per batch in fp64.  Each batch's tile goes into an fp64 n x n accumulator (lower triangle), so the error of the whole sum is that
// of one batch's fp32 sum; pg_kinship_finish_dev divides by p, rounds to float32 and mirrors.
// Float blocks (not exact in fp16) and every block under PG_KINSHIP_FP32=1 take the fp32 path instead: Zt = (x - s) / sd, SNP-major
// float32, and the fp32-MFMA syrk of rotate.hip with an accumulating epilogue into the same accumulator.
#include "geno_src.hpp"

#include <cmath>

namespace pg {

int kin_geno_gemm(pg_ctx *ctx, long long n, int kts, const unsigned short *A, long long ldA, const unsigned short *B, long long ldB,
                  const float *scale, const double *vk, const int *kflag, double *acc);            // rotate_geno.hip
int syrk_acc_fp32(pg_ctx *ctx, long long kdim, long long n, const float *Zt, long long ldz, double *acc);   // rotate.hip

struct KinPar {
    double *mu, *sh, *w, *isd, *r;   // per SNP of the batch: imputation value, shift, weight of R, 1/sd of the fp32 path, integer centre
    int *flag;                   // [0] the batch has a missing call, [1] max |R|, |mu R| as float bits; float [2], [3] = S, 1/S
};

// work area after the accumulator (pg_kinship_acc_bytes): operands of one batch, the rank-1 partials, per-SNP parameters, flags
struct KinLayout {
    long long kts, ldA, ldB, ldz;
    size_t a, b, vpart, v, par, flag, total;
};
static KinLayout kin_layout(long long n, long long pb)
{
    KinLayout L{};
    L.kts = (pb + 63) / 64;
    L.ldA = 2 * L.kts * 64;             // codes, then indicator, fp16
    L.ldB = 4 * L.kts * 64;             // two planes of S R per K-tile, then of S mu R
    L.ldz = (n + 63) / 64 * 64;         // fp32 path: Zt (pb x ldz) over the same bytes
    size_t off = up256((size_t)n * n * 8);
    L.a = off;
    L.b = L.a + up256((size_t)n * L.ldA * 2);
    off = L.b + up256((size_t)n * L.ldB * 2);
    const size_t zt_end = L.a + up256((size_t)pb * L.ldz * 4);
    off = off > zt_end ? off : zt_end;
    L.vpart = off; off += up256((size_t)L.kts * n * 8);
    L.v = off; off += up256((size_t)n * 8);
    L.par = off; off += up256((size_t)5 * pb * 8);
    L.flag = off; off += 256;
    L.total = off;
    return L;
}

__device__ __forceinline__ unsigned short h16(double v)
{
    const _Float16 h = (_Float16)(float)v;
    unsigned short b;
    __builtin_memcpy(&b, &h, 2);
    return b;
}
__device__ __forceinline__ double f16d(unsigned short b)
{
    _Float16 h;
    __builtin_memcpy(&h, &b, 2);
    return (double)(float)h;
}

// the per-SNP parameters from its fp64 statistics; lo / hi: the smallest / largest called value, miss: the SNP has a missing call
__device__ void kin_params(long long j, double mu, double var, double lo, double hi, bool miss, int standardize, const KinPar &P)
{
    const double s = standardize ? mu : 0.0;
    double w = 1.0, isd = 1.0;
    if (standardize && var > 0.0) { w = 1.0 / var; isd = 1.0 / sqrt(var); }      // sd == 0 -> 1
    const double r = rint(mu);        // the fp16 operand is c - r: exact, and centred to within 1/2 (no cancellation of r R against s R)
    P.mu[j] = mu; P.sh[j] = s; P.w[j] = w; P.isd[j] = isd; P.r[j] = r;
    double dev = fmax(fabs(lo - s), fabs(hi - s));
    if (miss) dev = fmax(dev, fabs(mu - s));
    // the planes of (mu - r) R are written for EVERY SNP of a batch that has a missing call anywhere, so mu - r bounds every SNP's entry
    const double m = w * dev * fmax(1.0, fabs(mu - r));
    if (m > 0.0 && m <= 3.0e38) atomicMax(&P.flag[1], __float_as_int((float)m));   // positive floats order as their bits
    if (miss) atomicOr(&P.flag[0], 1);
}

// .bed record j: exact counts of het / hom (dosage 2) / missing calls, the code convention of decode_bed_kernel.  One block per SNP.
__global__ __launch_bounds__(256) void kin_bed_stats_kernel(long long n, long long pb, const unsigned char *bed, long long ldb, int count_a1,
                                                            int standardize, KinPar P)
{
    __shared__ unsigned cnt[3];
    const long long j = blockIdx.x;
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
    __syncthreads();
    const unsigned char *row = bed + j * ldb;
    unsigned n1 = 0, n2 = 0, nm = 0;
    for (long long b = threadIdx.x; b < (n + 3) / 4; b += blockDim.x) {
        const unsigned byte = row[b];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (4 * b + q >= n) break;
            const unsigned c = (byte >> (2 * q)) & 3u;
            if (c == 1u) nm++;
            else if (c == 2u) n1++;
            else if ((c == 3u) != (count_a1 != 0)) n2++;
        }
    }
    atomicAdd(&cnt[0], n1); atomicAdd(&cnt[1], n2); atomicAdd(&cnt[2], nm);   // integer sums: order-independent
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long c1 = cnt[0], c2 = cnt[1], called = n - (long long)cnt[2];
        const long long sum = c1 + 2 * c2, sq = c1 + 4 * c2;
        double mu = 0.0, var = 0.0, lo = 0.0, hi = 0.0;
        if (called > 0) {
            mu = (double)sum / (double)called;
            var = (double)(called * sq - sum * sum) / ((double)called * (double)n);   // exact integer numerator: sum over called of (c - mu)^2 / n
            lo = (called - c1 - c2 > 0) ? 0.0 : (c1 > 0 ? 1.0 : 2.0);
            hi = c2 > 0 ? 2.0 : (c1 > 0 ? 1.0 : 0.0);
        }
        kin_params(j, mu, var, lo, hi, cnt[2] > 0, standardize, P);
    }
}

// an array block: fp64 two-pass mean and population variance (colstats_kernel's arithmetic), smallest and largest value.
// SNP-major: one block per SNP; sample-major: 64 SNPs per block, 4 row lanes each.  Partials reduced in a fixed order.
template <class T, bool SNPMAJ>
__global__ __launch_bounds__(256) void kin_x_stats_kernel(long long n, long long pb, const T *X, long long ldX, int standardize, KinPar P)
{
    constexpr int NS = SNPMAJ ? 1 : 64, NR = 256 / NS;
    __shared__ double red[NR][NS], rlo[NR][NS], rhi[NR][NS], mean[NS];
    const int c = threadIdx.x % NS, r = threadIdx.x / NS;
    const long long j = (long long)blockIdx.x * NS + c;
    auto at = [&](long long i) { return SNPMAJ ? (double)X[j * ldX + i] : (double)X[i * ldX + j]; };
    double s = 0.0, lo = INFINITY, hi = -INFINITY;
    if (j < pb)
        for (long long i = r; i < n; i += NR) { const double x = at(i); s += x; lo = fmin(lo, x); hi = fmax(hi, x); }
    red[r][c] = s; rlo[r][c] = lo; rhi[r][c] = hi;
    __syncthreads();
    if (r == 0) {
        double t = 0.0;
        for (int k = 0; k < NR; k++) t += red[k][c];
        mean[c] = t / (double)n;
    }
    __syncthreads();
    const double m = mean[c];
    double v = 0.0;
    if (j < pb)
        for (long long i = r; i < n; i += NR) { const double d = at(i) - m; v = fma(d, d, v); }
    __syncthreads();
    red[r][c] = v;
    __syncthreads();
    if (r == 0 && j < pb) {
        double t = 0.0;
        for (int k = 0; k < NR; k++) { t += red[k][c]; lo = fmin(lo, rlo[k][c]); hi = fmax(hi, rhi[k][c]); }
        kin_params(j, m, t / (double)n, lo, hi, false, standardize, P);
    }
}

// a 64-SNP x 64-sample tile of the raw block into LDS as fp64, tv[snp][sample]; a missing .bed call is NaN; outside the block 0
template <class T, int LAY>
__device__ __forceinline__ void kin_load_tile(double (*tv)[65], long long n, long long pb, const T *X, long long ldX, int count_a1,
                                              long long j0, long long i0)
{
    if constexpr (LAY == GENO_BED) {
        for (int e = threadIdx.x; e < 64 * 16; e += blockDim.x) {
            const int sl = e >> 4, b = e & 15;
            const long long j = j0 + sl, byte = i0 / 4 + b;
            const unsigned v = (j < pb && byte < (n + 3) / 4) ? (unsigned)X[j * ldX + byte] : 0u;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const unsigned cc = (v >> (2 * q)) & 3u;
                tv[sl][4 * b + q] = cc == 1u ? (double)NAN : (cc == 2u ? 1.0 : (((cc == 3u) != (count_a1 != 0)) ? 2.0 : 0.0));
            }
        }
    } else {
        for (int e = threadIdx.x; e < 64 * 64; e += blockDim.x) {
            const int sl = (LAY == GENO_SAMPLE) ? (e & 63) : (e >> 6), rl = (LAY == GENO_SAMPLE) ? (e >> 6) : (e & 63);   // contiguous side fastest
            const long long j = j0 + sl, i = i0 + rl;
            tv[sl][rl] = (j < pb && i < n) ? (double)((LAY == GENO_SAMPLE) ? X[i * ldX + j] : X[j * ldX + i]) : 0.0;
        }
    }
}

__device__ __forceinline__ void put16(unsigned short *dst, const unsigned short *h)
{
    uint4 a, b;
    a.x = h[0] | ((unsigned)h[1] << 16); a.y = h[2] | ((unsigned)h[3] << 16); a.z = h[4] | ((unsigned)h[5] << 16); a.w = h[6] | ((unsigned)h[7] << 16);
    b.x = h[8] | ((unsigned)h[9] << 16); b.y = h[10] | ((unsigned)h[11] << 16); b.z = h[12] | ((unsigned)h[13] << 16); b.w = h[14] | ((unsigned)h[15] << 16);
    reinterpret_cast<uint4 *>(dst)[0] = a;
    reinterpret_cast<uint4 *>(dst)[1] = b;
}

// the fp16 operands of one batch.  Block (K-tile t, 64 samples); thread: one sample, 16 SNPs.  Writes A[i][t] (values), A[i][kts + t]
// (indicator), B[i][2t], B[i][2t + 1] (planes of S R), B[i][2(kts + t)], .. + 1 (planes of S mu R) — the indicator halves only when the
// batch has a missing call — and the fp64 partial sum_{j in tile} s_j R_ij of the rank-1 term.  Block (0, 0) publishes S and 1/S.
template <class T, int LAY>
__global__ __launch_bounds__(256) void kin_encode_kernel(long long n, long long pb, const T *X, long long ldX, int count_a1, KinPar P,
                                                         unsigned short *A, long long ldA, unsigned short *B, long long ldB, long long kts,
                                                         double *vpart)
{
    __shared__ double tv[64][65];
    __shared__ double pm[64], ps[64], pw[64], pr[64], vq[64][4];
    const long long t = blockIdx.x, j0 = t * 64, i0 = (long long)blockIdx.y * 64;
    kin_load_tile<T, LAY>(tv, n, pb, X, ldX, count_a1, j0, i0);
    if (threadIdx.x < 64) {
        const long long j = j0 + threadIdx.x;
        pm[threadIdx.x] = j < pb ? P.mu[j] : 0.0;
        ps[threadIdx.x] = j < pb ? P.sh[j] : 0.0;
        pw[threadIdx.x] = j < pb ? P.w[j] : 0.0;       // padding SNPs: R = 0
        pr[threadIdx.x] = j < pb ? P.r[j] : 0.0;
    }
    __syncthreads();
    // S = the power of two that puts max |R|, |mu R| of the batch in [2^14, 2^15) (scale_kernel's rule)
    const int e = (P.flag[1] >> 23) & 0xFF;
    int se = 127 + 14 - (e - 127);
    se = se < 1 ? 1 : (se > 254 ? 254 : se);
    const float S = __int_as_float(se << 23);
    const bool miss = P.flag[0] != 0;
    if (t == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        reinterpret_cast<float *>(P.flag)[2] = S;
        reinterpret_cast<float *>(P.flag)[3] = __int_as_float((254 - se) << 23);
    }
    const int r = threadIdx.x >> 2, qq = threadIdx.x & 3;
    const long long i = i0 + r;
    unsigned short hc[16], hi[16], r1[16], r2[16], m1[16], m2[16];
    double vs = 0.0;
#pragma unroll
    for (int u = 0; u < 16; u++) {
        const int sl = 16 * qq + u;
        const double x = tv[sl][r];
        const bool mis = x != x;
        const double R = pw[sl] * ((mis ? pm[sl] : x) - ps[sl]);
        const double RS = R * (double)S;                        // exact: power of two
        hc[u] = h16(mis ? 0.0 : x - pr[sl]);                   // exact: integers in [-255, 255]
        hi[u] = mis ? 0x3C00 : 0;
        r1[u] = h16(RS); r2[u] = h16(RS - f16d(r1[u]));         // the residual is exact in fp64
        const double MS = (pm[sl] - pr[sl]) * RS;
        m1[u] = h16(MS); m2[u] = h16(MS - f16d(m1[u]));
        vs += (ps[sl] - pr[sl]) * R;
    }
    vq[r][qq] = vs;
    if (i < n) {
        put16(A + i * ldA + t * 64 + 16 * qq, hc);
        put16(B + i * ldB + 2 * t * 64 + 16 * qq, r1);
        put16(B + i * ldB + (2 * t + 1) * 64 + 16 * qq, r2);
        if (miss) {
            put16(A + i * ldA + (kts + t) * 64 + 16 * qq, hi);
            put16(B + i * ldB + 2 * (kts + t) * 64 + 16 * qq, m1);
            put16(B + i * ldB + (2 * (kts + t) + 1) * 64 + 16 * qq, m2);
        }
    }
    __syncthreads();
    if (qq == 0 && i < n) vpart[t * n + i] = ((vq[r][0] + vq[r][1]) + vq[r][2]) + vq[r][3];
}

__global__ void kin_vsum_kernel(long long n, long long kts, const double *vpart, double *v)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    double s = 0.0;
    for (long long t = 0; t < kts; t++) s += vpart[t * n + k];
    v[k] = s;
}

// fp32 path: Zt[j][i] = (float)((x_ij - s_j) / sd_j), the imputed value for a missing call; samples [n, ldz) zero.  Block: 64 x 64.
template <class T, int LAY>
__global__ __launch_bounds__(256) void kin_zt_kernel(long long n, long long pb, const T *X, long long ldX, int count_a1, KinPar P, float *Zt,
                                                     long long ldz)
{
    __shared__ double tv[64][65];
    __shared__ double pm[64], ps[64], pi[64];
    const long long j0 = (long long)blockIdx.x * 64, i0 = (long long)blockIdx.y * 64;
    kin_load_tile<T, LAY>(tv, n, pb, X, ldX, count_a1, j0, i0);
    if (threadIdx.x < 64) {
        const long long j = j0 + threadIdx.x;
        pm[threadIdx.x] = j < pb ? P.mu[j] : 0.0;
        ps[threadIdx.x] = j < pb ? P.sh[j] : 0.0;
        pi[threadIdx.x] = j < pb ? P.isd[j] : 0.0;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 64 * 64; e += blockDim.x) {
        const int sl = e >> 6, rl = e & 63;
        const long long j = j0 + sl, i = i0 + rl;
        if (j < pb && i < ldz) {
            const double x = tv[sl][rl];
            Zt[j * ldz + i] = i < n ? (float)(((x != x ? pm[sl] : x) - ps[sl]) * pi[sl]) : 0.0f;
        }
    }
}

// K = acc / p rounded to float32 (lower triangle of acc), both triangles from the same value: bit-symmetric.  Block: 32 x 32 tile.
__global__ __launch_bounds__(256) void kin_finish_kernel(long long n, long long p, const double *acc, float *K)
{
    __shared__ float tile[32][33];
    const long long c0 = (long long)blockIdx.x * 32, r0 = (long long)blockIdx.y * 32;
    if (c0 > r0) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int rr = ty; rr < 32; rr += 8) {
        const long long row = r0 + rr, col = c0 + tx;
        float v = 0.0f;
        if (row < n && col < n) {
            v = (float)((row >= col ? acc[row * n + col] : acc[col * n + row]) / (double)p);
            K[row * n + col] = v;
        }
        tile[rr][tx] = v;
    }
    __syncthreads();
    if (r0 == c0) return;
    for (int rr = ty; rr < 32; rr += 8) {
        const long long row = c0 + rr, col = r0 + tx;
        if (row < n && col < n) K[row * n + col] = tile[tx][rr];
    }
}

// PG_KINSHIP_FP32=1 sends every block to the fp32 path (A/B, tests)
static bool kin_fp32_forced() { return env_flag("PG_KINSHIP_FP32"); }

static KinPar kin_par(char *base, const KinLayout &L, long long pb)
{
    KinPar P;
    P.mu = (double *)(base + L.par); P.sh = P.mu + pb; P.w = P.sh + pb; P.isd = P.w + pb; P.r = P.isd + pb;
    P.flag = (int *)(base + L.flag);
    return P;
}

// the operands of one batch whose statistics are in P, then its syrk into acc
template <class T, int LAY>
static int kin_batch(pg_ctx *ctx, long long n, long long pb, const T *X, long long ldX, int count_a1, bool fp16, const KinLayout &L, char *base,
                     const KinPar &P)
{
    double *acc = (double *)base;
    if constexpr (sizeof(T) == 1) if (fp16) {     // .bed codes and 8-bit values: exact in fp16
        unsigned short *A = (unsigned short *)(base + L.a), *B = (unsigned short *)(base + L.b);
        double *vpart = (double *)(base + L.vpart), *v = (double *)(base + L.v);
        kin_encode_kernel<T, LAY><<<dim3((unsigned)L.kts, (unsigned)((n + 63) / 64)), 256, 0, ctx->stream>>>(n, pb, X, ldX, count_a1, P, A, L.ldA,
                                                                                                               B, L.ldB, L.kts, vpart);
        PG_HIP(hipGetLastError());
        kin_vsum_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, ctx->stream>>>(n, L.kts, vpart, v);
        PG_HIP(hipGetLastError());
        return kin_geno_gemm(ctx, n, (int)L.kts, A, L.ldA, B, L.ldB, reinterpret_cast<const float *>(P.flag) + 2, v, P.flag, acc);
    }
    float *Zt = (float *)(base + L.a);
    kin_zt_kernel<T, LAY><<<dim3((unsigned)L.kts, (unsigned)(L.ldz / 64)), 256, 0, ctx->stream>>>(n, pb, X, ldX, count_a1, P, Zt, L.ldz);
    PG_HIP(hipGetLastError());
    return syrk_acc_fp32(ctx, pb, n, Zt, L.ldz, acc);
}

template <class T, int LAY>
static int kin_x(pg_ctx *ctx, long long n, long long pb, const T *X, long long ldX, int standardize, bool fp16, const KinLayout &L, char *base)
{
    constexpr bool snp_major = LAY == GENO_SNP;
    const KinPar P = kin_par(base, L, pb);
    PG_HIP(hipMemsetAsync(P.flag, 0, 16, ctx->stream));
    kin_x_stats_kernel<T, snp_major><<<dim3((unsigned)(snp_major ? pb : (pb + 63) / 64)), 256, 0, ctx->stream>>>(n, pb, X, ldX, standardize, P);
    PG_HIP(hipGetLastError());
    return kin_batch<T, LAY>(ctx, n, pb, X, ldX, 0, fp16, L, base, P);
}

}  // namespace pg

using namespace pg;

extern "C" size_t pg_kinship_acc_bytes(int64_t n, int64_t pb)
{
    if (n < 1 || pb < 1) return 0;
    return kin_layout(n, pb).total;
}

extern "C" int pg_kinship_bed_acc_dev(pg_ctx *ctx, int64_t n, int64_t pb, const unsigned char *bed, int64_t ldb, int count_a1, int standardize,
                                      double *acc)
{
    PG_REQUIRE(ctx && bed && acc, "pg_kinship_bed_acc_dev: NULL argument");
    PG_REQUIRE(n > 0 && pb > 0 && ldb >= (n + 3) / 4 && pb < (1LL << 31) && n < (1LL << 31),
               "pg_kinship_bed_acc_dev: bad shape n=%lld pb=%lld ldb=%lld", (long long)n, (long long)pb, (long long)ldb);
    PG_HIP(hipSetDevice(ctx->device));
    const KinLayout L = kin_layout(n, pb);
    char *base = (char *)acc;
    const KinPar P = kin_par(base, L, pb);
    PG_HIP(hipMemsetAsync(P.flag, 0, 16, ctx->stream));
    kin_bed_stats_kernel<<<dim3((unsigned)pb), 256, 0, ctx->stream>>>(n, pb, bed, ldb, count_a1, standardize, P);
    PG_HIP(hipGetLastError());
    return kin_batch<unsigned char, GENO_BED>(ctx, n, pb, bed, ldb, count_a1, !kin_fp32_forced(), L, base, P);
}

extern "C" int pg_kinship_x_acc_dev(pg_ctx *ctx, int64_t n, int64_t pb, const void *X, int dtype, int64_t ldX, int snp_major, int standardize,
                                    double *acc)
{
    PG_REQUIRE(ctx && X && acc, "pg_kinship_x_acc_dev: NULL argument");
    PG_REQUIRE(n > 0 && pb > 0 && ldX >= (snp_major ? n : pb) && pb < (1LL << 31) && n < (1LL << 31),
               "pg_kinship_x_acc_dev: bad shape n=%lld pb=%lld ldX=%lld snp_major=%d", (long long)n, (long long)pb, (long long)ldX, snp_major);
    PG_REQUIRE(dtype_known(dtype), "pg_kinship_x_acc_dev: unknown dtype %d", dtype);
    PG_HIP(hipSetDevice(ctx->device));
    const KinLayout L = kin_layout(n, pb);
    const bool fp16 = !kin_fp32_forced();      // kin_batch takes the fp16 pipe for 8-bit values only
    return geno_dispatch(dtype, snp_major != 0, [&](auto src) {
        using S = decltype(src);
        return kin_x<typename S::type, S::layout>(ctx, n, pb, (const typename S::type *)X, ldX, standardize, fp16, L, (char *)acc);
    });
}

extern "C" int pg_kinship_finish_dev(pg_ctx *ctx, int64_t n, int64_t p, const double *acc, float *K)
{
    PG_REQUIRE(ctx && acc && K, "pg_kinship_finish_dev: NULL argument");
    PG_REQUIRE(n > 0 && p > 0 && n < (1LL << 31), "pg_kinship_finish_dev: bad shape n=%lld p=%lld", (long long)n, (long long)p);
    PG_HIP(hipSetDevice(ctx->device));
    const unsigned nt = (unsigned)((n + 31) / 32);
    kin_finish_kernel<<<dim3(nt, nt), 256, 0, ctx->stream>>>(n, p, acc, K);
    PG_HIP(hipGetLastError());
    return PG_OK;
}
