// king.hip — KING-robust relatedness, IBS similarity and per-sample QC counts on the int8 matrix pipe, accumulated on the
// device over the SNP batches of a stream, from packed .bed records or 8-bit / float32 / float64 blocks, sample- or SNP-major.
//
// Definition.  Elements and hard calls as in ld.hip: missing is .bed code 01, NaN or +-Inf; a SNP is hard-call when every
// non-missing value (in its own precision) is exactly 0, 1 or 2; any other SNP counts as all missing for every sample.  Sample i at a SNP
// has the indicators m (called), h (called and 1), a (called and 0), b (called and 2); a pair (i, j) has the int32 sums over all SNPs
//     N = sum m_i m_j    HH = sum h_i h_j    IBS0 = sum (a_i b_j + b_i a_j)    Hij = sum h_i m_j  (not symmetric; Hji is the transposed entry)
// and exactly IBS1 = Hij + Hji - 2 HH, IBS2 = N - IBS0 - IBS1;
//     phi = float32((double)(HH - 2 IBS0) / (double)(Hij + Hji)), NaN when Hij + Hji == 0;
//     ibs = float32(1 - (double)(IBS1 + 2 IBS0) / (double)(2 N)), NaN when N == 0.
// Everything but the last division is integer arithmetic: the sums are testable for equality, a sample against itself or a copy gives 0.5.
//
// One batch of pb SNPs becomes three sample-major int8 planes c = b - a, h, m of n rows each, rows of ldk = pb rounded up to the K-tile of
// 128 SNPs, zero past SNP pb.  c c' = concordant - opposite homozygotes and (m - h)(m - h)' = N - Hij - Hji + HH = both homozygous, so
// IBS0 = ((N - Hij - Hji + HH) - c c') / 2.  The accumulators (int32, n x n, row pitch n) hold c c', HH, N and Hij.
//
// The encode transposes through LDS: a workgroup takes 256 samples x 128 SNPs, reads the records (64 consecutive bytes of each) or the
// array rows along their contiguous side, leaves one class byte per call in LDS (bit 0 h, bit 1 b, bit 2 a, 0 missing), and every thread
// then turns 16 class bytes of one sample into the three 16-byte plane stores with word-wide bit operations; 8 adjacent lanes write the 128
// contiguous bytes of a sample's K-tile.  The per-sample counts come from the same words (popcounts) and go out as integer atomics.  Arrays
// are screened for SNPs that are not hard-call in a pass of their own BEFORE the encode (their calls are then classed missing), so no plane
// is ever written and taken back.
//
// The pair kernel runs the 256 x 256 int8 GEMM tile of i8_pair.hpp with samples as output rows and the batch's SNPs as K.  The grid is
// (lower-triangle pairs of sample tiles) x (products); a workgroup adds its product into its accumulator.
//   no missing call in the batch (device flag): m = 1 on every hard-call SNP, so N grows by the batch's hard-call SNP count and Hij by i's
//     het total of the batch (king_fold_kernel adds them to a scalar and a vector that the finish adds back): products c c' and h h' only;
//   general: c c', h h', m m', h m' (rows I, columns J) and h m' with the tiles swapped (rows J, columns I: the other triangle of Hij,
//     written along its rows; skipped on the diagonal, where the fourth product is the whole tile).
// PG_KING_PLANES=1 sends every batch down the general path (tests, A/B timing); both paths produce the same integers.
// A SNP of an array that is not hard-call does NOT raise the missing-call flag although every call of it is classed missing: its planes are
// all zero, so it adds nothing to any product, and the two-product path stays exact because king_fold_kernel counts N over the hard-call
// SNPs only (pb minus the screen's flags) and the het totals never see such a SNP.
// PG_KING_TIMING=1 puts events around the encode and the pair kernel of every batch and waits for them (pg_king_last_batch_ms reads the
// two times; tools/bench_king.py).  The results are the same; the call no longer returns before the batch is done.
#include "geno_src.hpp"
#include "i8_pair.hpp"

#include <type_traits>

namespace pg {

constexpr int KG_BK = I8P_BK;       // SNPs per K-tile
constexpr int KG_T = 256;           // samples per output tile side
constexpr int KG_ES = 256;          // samples per encode workgroup
constexpr int KG_EK = 4;            // K-tiles per encode workgroup: fewer atomics per sample
constexpr int KG_EROW = 144;        // LDS bytes per sample row of the encode tile: 128 class bytes and one 16-byte pad
constexpr long long KG_MAXN = 1LL << 20;       // exclusive: every grid dimension fits (the finish: n / 32 tiles a side)
constexpr long long KG_MAXPB = 1LL << 31;      // exclusive: every count fits int32

// The accumulator block.  [0, zero) lives across batches and starts as zeros: the four n x n int32 matrices, the no-missing-path totals
// (per-sample het calls as int64, hard-call SNPs as one int64) and the n x 5 int64 per-sample counts.  [zero, total) is rewritten by
// every batch: the missing-call flag, the batch's per-sample het totals, the not-hard-call flags of its SNPs, its three planes.
struct KingLayout {
    long long ldk;
    size_t mat, hfast, samp, nfast, zero, flag, hb, bad, planes, plane, total;
};
static KingLayout king_layout(long long n, long long pb)
{
    KingLayout L;
    L.ldk = (pb + KG_BK - 1) / KG_BK * KG_BK;
    L.mat = up256((size_t)n * n * 4);
    L.hfast = 4 * L.mat;
    L.samp = L.hfast + up256((size_t)n * 8);
    L.nfast = L.samp + up256((size_t)n * 40);
    L.zero = L.nfast + 256;
    L.flag = L.zero;
    L.hb = L.flag + 256;
    L.bad = L.hb + up256((size_t)n * 4);
    L.planes = L.bad + up256((size_t)pb * 4);
    L.plane = (size_t)n * L.ldk;
    L.total = L.planes + 3 * L.plane;
    return L;
}

// ---- encode -----------------------------------------------------------------------------------------------------------------------------
// a value other than a hard call or a missing one, in the element's own precision (ld_classify's rule)
template <class T> __device__ __forceinline__ int king_bad(T x)
{
    if constexpr (std::is_floating_point<T>::value) return (isfinite(x) && x != T(0) && x != T(1) && x != T(2)) ? 1 : 0;
    else return ((int)x < 0 || (int)x > 2) ? 1 : 0;
}
// the class byte of an element of a hard-call SNP: 1 het, 2 hom 2, 4 hom 0, 0 missing
template <class T> __device__ __forceinline__ int king_class(T x)
{
    return x == T(1) ? 1 : (x == T(2) ? 2 : (x == T(0) ? 4 : 0));
}

// SNP-major array: one workgroup per SNP
template <class T> __global__ __launch_bounds__(256) void king_screen_snp_kernel(int n, long long ld, const T *X, int *bad)
{
    const long long g = blockIdx.x;
    int bd = 0;
    for (int i = threadIdx.x; i < n; i += 256) bd |= king_bad<T>(X[g * ld + i]);
    if (__syncthreads_or(bd) && threadIdx.x == 0) bad[g] = 1;
}
// sample-major array: lane = SNP (the loads of a wavefront are adjacent), workgroup = 64 SNPs x 1024 samples
template <class T> __global__ __launch_bounds__(256) void king_screen_sample_kernel(int n, long long pb, long long ld, const T *X, int *bad)
{
    const long long g = (long long)blockIdx.x * 64 + (threadIdx.x & 63);
    if (g >= pb) return;
    const long long r0 = (long long)blockIdx.y * 1024, r1 = min((long long)n, r0 + 1024);
    int bd = 0;
    for (long long i = r0 + (threadIdx.x >> 6); i < r1; i += 4) bd |= king_bad<T>(X[i * ld + g]);
    if (bd) atomicOr(&bad[g], 1);
}

struct KingEnc {
    int n, count_a1;
    long long pb, ld, ldk;
    signed char *img;                 // the c plane; h and m `plane` bytes further each (IMG only)
    size_t plane;
    const int *bad;                   // arrays: SNPs that are not hard-call
    int *flag, *hb;                   // the batch holds a missing call; per-sample het totals of the batch (or NULL)
    unsigned long long *samp;         // n x 5: n_obs, n_miss, n0, n1, n2
};

// Workgroup (x: KG_EK K-tiles, y: 256 samples).
template <class T, int LAYOUT, bool IMG> __global__ __launch_bounds__(256) void king_encode_kernel(KingEnc q, const T *X)
{
    __shared__ __attribute__((aligned(16))) unsigned char cls[KG_ES * KG_EROW];
    const int tid = threadIdx.x, qq = tid & 7;
    const long long i0 = (long long)blockIdx.y * KG_ES;
    const long long kt0 = (long long)blockIdx.x * KG_EK, kt1 = min(kt0 + KG_EK, q.ldk / KG_BK);
    int ch[8], ca[8], cb[8];
#pragma unroll
    for (int it = 0; it < 8; it++) ch[it] = ca[it] = cb[it] = 0;
    int miss = 0;
    for (long long kt = kt0; kt < kt1; kt++) {
        const long long g0 = kt * KG_BK;
        if constexpr (LAYOUT == GENO_BED) {
            const long long nbytes = ((long long)q.n + 3) / 4;
            for (int e = tid; e < KG_BK * (KG_ES / 4); e += 256) {
                const int sl = e >> 6, b = e & 63;
                const long long g = g0 + sl, byte = i0 / 4 + b;
                const unsigned v = (g < q.pb && byte < nbytes) ? (unsigned)X[g * q.ld + byte] : 0x55u;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const unsigned c = (v >> (2 * k)) & 3u;          // 00 -> 0, 10 -> 1, 11 -> 2, 01 missing
                    int cl = c == 0u ? 4 : (c == 2u ? 1 : (c == 3u ? 2 : 0));
                    if (q.count_a1 && (cl & 6)) cl ^= 6;
                    if (g >= q.pb || i0 + 4 * b + k >= q.n) cl = 0;
                    else miss |= cl == 0;
                    cls[(4 * b + k) * KG_EROW + sl] = (unsigned char)cl;
                }
            }
        } else if constexpr (LAYOUT == GENO_SNP) {
            const long long i = i0 + tid;
            for (int sl = 0; sl < KG_BK; sl++) {
                const long long g = g0 + sl;
                int cl = 0;
                if (g < q.pb && i < q.n && !q.bad[g]) { cl = king_class<T>(X[g * q.ld + i]); miss |= cl == 0; }
                cls[tid * KG_EROW + sl] = (unsigned char)cl;
            }
        } else {
            const int sl = tid & (KG_BK - 1);
            const long long g = g0 + sl;
            const bool live = g < q.pb && !q.bad[g];
            for (int il = tid >> 7; il < KG_ES; il += 2) {
                int cl = 0;
                if (live && i0 + il < q.n) { cl = king_class<T>(X[(i0 + il) * q.ld + g]); miss |= cl == 0; }
                cls[il * KG_EROW + sl] = (unsigned char)cl;
            }
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 8; it++) {
            const int s = it * 32 + (tid >> 3);
            const uint4 w4 = *reinterpret_cast<const uint4 *>(cls + s * KG_EROW + 16 * qq);
            const unsigned w[4] = {w4.x, w4.y, w4.z, w4.w};
            unsigned cw[4], hw[4], mw[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const unsigned h = w[k] & 0x01010101u, b = (w[k] >> 1) & 0x01010101u, a = (w[k] >> 2) & 0x01010101u;
                hw[k] = h; mw[k] = h | b | a; cw[k] = b | (a * 0xFFu);      // a byte of a is 0 or 1: no carry between bytes; 0xFF = -1
                ch[it] += __popc(h); ca[it] += __popc(a); cb[it] += __popc(b);
            }
            if constexpr (IMG) {
                if (i0 + s < q.n) {
                    signed char *row = q.img + (size_t)(i0 + s) * q.ldk + g0 + 16 * qq;
                    *reinterpret_cast<uint4 *>(row) = make_uint4(cw[0], cw[1], cw[2], cw[3]);
                    *reinterpret_cast<uint4 *>(row + q.plane) = make_uint4(hw[0], hw[1], hw[2], hw[3]);
                    *reinterpret_cast<uint4 *>(row + 2 * q.plane) = make_uint4(mw[0], mw[1], mw[2], mw[3]);
                }
            }
        }
        __syncthreads();
    }
    // `miss` is about calls of hard-call SNPs only: a flagged SNP is all zeros in every plane and is left out of the totals' N (see the top)
    if (__syncthreads_or(miss) && tid == 0) atomicOr(q.flag, 1);
    // the counts of this workgroup's SNPs: the 8 lanes of a sample meet, one of them adds.  Integer atomics: the same bits in any order.
    const long long nsnp = min(q.pb, kt1 * KG_BK) - kt0 * KG_BK;
#pragma unroll
    for (int it = 0; it < 8; it++) {
        int h = ch[it], a = ca[it], b = cb[it];
        for (int k = 1; k < 8; k <<= 1) { h += __shfl_xor(h, k, 64); a += __shfl_xor(a, k, 64); b += __shfl_xor(b, k, 64); }
        const long long i = i0 + it * 32 + (tid >> 3);
        if (qq != 0 || i >= q.n) continue;
        unsigned long long *t = q.samp + 5 * i;
        const int obs = h + a + b;
        if (obs) atomicAdd(t, (unsigned long long)obs);
        if (nsnp - obs) atomicAdd(t + 1, (unsigned long long)(nsnp - obs));
        if (a) atomicAdd(t + 2, (unsigned long long)a);
        if (h) atomicAdd(t + 3, (unsigned long long)h);
        if (b) atomicAdd(t + 4, (unsigned long long)b);
        if (q.hb && h) atomicAdd(q.hb + i, h);
    }
}

template <class T, int LAYOUT, bool IMG> static int launch_king_encode(pg_ctx *ctx, KingEnc q, const void *X, int *bad)
{
    const T *Xt = static_cast<const T *>(X);
    const unsigned sy = (unsigned)((q.n + KG_ES - 1) / KG_ES);
    if constexpr (LAYOUT == GENO_SNP) {
        king_screen_snp_kernel<T><<<(unsigned)q.pb, 256, 0, ctx->stream>>>(q.n, q.ld, Xt, bad);
        PG_HIP(hipGetLastError());
    } else if constexpr (LAYOUT == GENO_SAMPLE) {
        king_screen_sample_kernel<T><<<dim3((unsigned)((q.pb + 63) / 64), (unsigned)((q.n + 1023) / 1024)), 256, 0, ctx->stream>>>(q.n, q.pb, q.ld, Xt, bad);
        PG_HIP(hipGetLastError());
    }
    q.bad = bad;
    const long long kts = q.ldk / KG_BK;
    king_encode_kernel<T, LAYOUT, IMG><<<dim3((unsigned)((kts + KG_EK - 1) / KG_EK), sy), 256, 0, ctx->stream>>>(q, Xt);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

template <bool IMG> static int king_encode_any(pg_ctx *ctx, const KingEnc &q, const void *X, int dtype, int snp_major, int *bad)
{
    if (dtype < 0) return launch_king_encode<unsigned char, GENO_BED, IMG>(ctx, q, X, bad);
    return geno_dispatch(dtype, snp_major != 0, [&](auto src) {
        using S = decltype(src);
        return launch_king_encode<typename S::type, S::layout, IMG>(ctx, q, X, bad);
    });
}

// a batch without a missing call: its N and Hij are totals, kept apart from the matrices
__global__ __launch_bounds__(256) void king_fold_kernel(int n, long long pb, int planes, const int *flag, const int *bad, const int *hb,
                                                        long long *hfast, long long *nfast)
{
    __shared__ int nbad;
    if (planes || *flag) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) hfast[i] += hb[i];
    if (blockIdx.x != 0) return;
    if (threadIdx.x == 0) nbad = 0;
    __syncthreads();
    int nb = 0;
    if (bad)
        for (long long g = threadIdx.x; g < pb; g += 256) nb += bad[g] != 0;
    if (nb) atomicAdd(&nbad, nb);
    __syncthreads();
    if (threadIdx.x == 0) *nfast += pb - nbad;
}

// ---- the pair kernel --------------------------------------------------------------------------------------------------------------------
struct KingPair {
    int n, KT, planes;
    long long ldk;
    const signed char *img;
    size_t plane;
    const int *flag;
    int *acc[4];                      // c c', HH, N, Hij
};

__global__ __launch_bounds__(512, 1) void king_pair_kernel(KingPair q)
{
    const int prod = blockIdx.y;      // 0: c c', 1: h h', 2: m m', 3: h_I m_J', 4: h_J m_I'
    if (prod >= 2 && !(q.planes || *q.flag)) return;
    long long I = (long long)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);
    while (I * (I + 1) / 2 > (long long)blockIdx.x) I--;
    while ((I + 1) * (I + 2) / 2 <= (long long)blockIdx.x) I++;
    const long long J = (long long)blockIdx.x - I * (I + 1) / 2;      // J <= I
    if (prod == 4 && I == J) return;
    const int pa = prod == 0 ? 0 : (prod == 2 ? 2 : 1), pb = prod == 0 ? 0 : (prod == 1 ? 1 : 2);
    const long long abase = (prod == 4 ? J : I) * KG_T, bbase = (prod == 4 ? I : J) * KG_T;
    int *const dst = q.acc[prod < 3 ? prod : 3];

    const int tid = threadIdx.x;
    const I8pLane ln = i8p_lane();
    const int *const stg = i8p_staged();
    intx4 acc[4][8];
    i8p_zero(acc);
    // DMA sources.  Rows past sample n repeat the last sample: their products are never read.
    const signed char *srcA[4], *srcB[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int row = i8p_src_row(ln, t);
        const long long ga = min(abase + row, (long long)q.n - 1), gb = min(bbase + row, (long long)q.n - 1);
        srcA[t] = q.img + pa * q.plane + (size_t)ga * q.ldk + i8p_src_byte(ln, row);
        srcB[t] = q.img + pb * q.plane + (size_t)gb * q.ldk + i8p_src_byte(ln, row);
    }
    i8p_products(ln, srcA, srcB, q.KT, acc);
    // ---- epilogue: the accumulators meet through LDS, one 128-row half of A at a time, and are added to the matrix
#pragma unroll 1
    for (int half = 0; half < 2; half++) {
        i8p_stage(ln, half, acc);
        for (int idx = tid; idx < 128 * KG_T; idx += 512) {
            const int sa = idx >> 8, sb = idx & (KG_T - 1);
            const long long i = abase + half * 128 + sa, j = bbase + sb;
            if (i < q.n && j < q.n) dst[i * q.n + j] += stg[sa * I8P_LDW + sb];
        }
        __syncthreads();
    }
}

// ---- finish -------------------------------------------------------------------------------------------------------------------------------
struct KingAcc {
    long long n;
    const int *cc, *hh, *nn, *hm;
    const long long *hfast, *nfast;
};

// the counts of the pair (i, j), i >= j, from the lower triangle of the symmetric accumulators and both triangles of Hij
__device__ __forceinline__ void king_pair_counts(const KingAcc &A, long long i, long long j, long long &N, long long &HH, long long &IBS0,
                                                 long long &Hij, long long &Hji)
{
    const long long o = i * A.n + j;
    N = A.nn[o] + *A.nfast;
    HH = A.hh[o];
    Hij = A.hm[o] + A.hfast[i];
    Hji = A.hm[j * A.n + i] + A.hfast[j];
    IBS0 = ((N - Hij - Hji + HH) - A.cc[o]) / 2;
}

__device__ __forceinline__ float king_value(int what, long long N, long long HH, long long IBS0, long long Hij, long long Hji)
{
    if (what == 0) return Hij + Hji == 0 ? __builtin_nanf("") : (float)((double)(HH - 2 * IBS0) / (double)(Hij + Hji));
    const long long IBS1 = Hij + Hji - 2 * HH;
    return N == 0 ? __builtin_nanf("") : (float)(1.0 - (double)(IBS1 + 2 * IBS0) / (double)(2 * N));
}

// phi or ibs as float32, both triangles from the same value: bit-symmetric.  Block: 32 x 32 tile on or below the diagonal.
__global__ __launch_bounds__(256) void king_finish_kernel(KingAcc A, int what, float *out)
{
    __shared__ float tile[32][33];
    const long long c0 = (long long)blockIdx.x * 32, r0 = (long long)blockIdx.y * 32, n = A.n;
    if (c0 > r0) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int rr = ty; rr < 32; rr += 8) {
        const long long row = r0 + rr, col = c0 + tx;
        float v = 0.0f;
        if (row < n && col < n) {
            long long N, HH, IBS0, Hij, Hji;
            king_pair_counts(A, max(row, col), min(row, col), N, HH, IBS0, Hij, Hji);
            v = king_value(what, N, HH, IBS0, Hij, Hji);
            out[row * n + col] = v;
        }
        tile[rr][tx] = v;
    }
    __syncthreads();
    if (r0 == c0) return;
    for (int rr = ty; rr < 32; rr += 8) {
        const long long row = c0 + rr, col = r0 + tx;
        if (row < n && col < n) out[row * n + col] = tile[tx][rr];
    }
}

// the five count matrices N, HH, IBS0, Hij, IBS1, n x n each, every entry of both triangles
__global__ __launch_bounds__(256) void king_counts_kernel(KingAcc A, int *counts)
{
    const long long n = A.n, row = blockIdx.x, col = (long long)blockIdx.y * 256 + threadIdx.x;
    if (col >= n) return;
    long long N, HH, IBS0, Hij, Hji;
    king_pair_counts(A, max(row, col), min(row, col), N, HH, IBS0, Hij, Hji);
    const size_t o = (size_t)(row * n + col), nn = (size_t)n * n;
    counts[o] = (int)N;
    counts[nn + o] = (int)HH;
    counts[2 * nn + o] = (int)IBS0;
    counts[3 * nn + o] = (int)(row >= col ? Hij : Hji);
    counts[4 * nn + o] = (int)(Hij + Hji - 2 * HH);
}

static bool king_shape_ok(int64_t n, int64_t pb) { return n >= 1 && n < KG_MAXN && pb >= 1 && pb < KG_MAXPB; }

static KingAcc king_acc(int64_t n, const void *acc)
{
    const KingLayout L = king_layout(n, 1);
    const char *base = static_cast<const char *>(acc);
    KingAcc A;
    A.n = n;
    A.cc = reinterpret_cast<const int *>(base); A.hh = reinterpret_cast<const int *>(base + L.mat);
    A.nn = reinterpret_cast<const int *>(base + 2 * L.mat); A.hm = reinterpret_cast<const int *>(base + 3 * L.mat);
    A.hfast = reinterpret_cast<const long long *>(base + L.hfast); A.nfast = reinterpret_cast<const long long *>(base + L.nfast);
    return A;
}

static thread_local float king_last_ms[2] = {0.0f, 0.0f};      // PG_KING_TIMING: encode (memset, screen, encode, fold) and pair kernel of the last batch

// one batch: screen and encode, fold the totals of a batch without a missing call, then the products.  dtype < 0: .bed records.
static int king_batch(pg_ctx *ctx, int64_t n, int64_t pb, const void *X, int dtype, int64_t ld, int snp_major, int count_a1, void *acc)
{
    const KingLayout L = king_layout(n, pb);
    char *base = static_cast<char *>(acc);
    const long long nt = (n + KG_T - 1) / KG_T;
    PG_HIP(hipSetDevice(ctx->device));
    const bool timing = env_flag("PG_KING_TIMING");
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    if (timing) {
        for (int k = 0; k < 3; k++) PG_HIP(hipEventCreate(&ev[k]));
        PG_HIP(hipEventRecord(ev[0], ctx->stream));
    }
    PG_HIP(hipMemsetAsync(base + L.flag, 0, L.planes - L.flag, ctx->stream));
    int *flag = reinterpret_cast<int *>(base + L.flag), *hb = reinterpret_cast<int *>(base + L.hb), *bad = reinterpret_cast<int *>(base + L.bad);
    KingEnc e;
    e.n = (int)n; e.count_a1 = count_a1 != 0; e.pb = pb; e.ld = ld; e.ldk = L.ldk;
    e.img = reinterpret_cast<signed char *>(base + L.planes); e.plane = L.plane; e.bad = nullptr;
    e.flag = flag; e.hb = hb; e.samp = reinterpret_cast<unsigned long long *>(base + L.samp);
    const int rc = king_encode_any<true>(ctx, e, X, dtype, snp_major, bad);
    if (rc != PG_OK) return rc;
    const int planes = env_flag("PG_KING_PLANES");
    king_fold_kernel<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>((int)n, pb, planes, flag, dtype < 0 ? nullptr : bad, hb,
                                                                              reinterpret_cast<long long *>(base + L.hfast),
                                                                              reinterpret_cast<long long *>(base + L.nfast));
    PG_HIP(hipGetLastError());
    if (timing) PG_HIP(hipEventRecord(ev[1], ctx->stream));
    KingPair q;
    q.n = (int)n; q.KT = (int)(L.ldk / KG_BK); q.planes = planes; q.ldk = L.ldk; q.img = e.img; q.plane = L.plane; q.flag = flag;
    for (int k = 0; k < 4; k++) q.acc[k] = reinterpret_cast<int *>(base + k * L.mat);
    PG_HIP(i8p_lds_limit<king_pair_kernel>(ctx->device));
    king_pair_kernel<<<dim3((unsigned)(nt * (nt + 1) / 2), 5), 512, I8P_LDS, ctx->stream>>>(q);
    PG_HIP(hipGetLastError());
    if (timing) {
        PG_HIP(hipEventRecord(ev[2], ctx->stream));
        PG_HIP(hipEventSynchronize(ev[2]));
        PG_HIP(hipEventElapsedTime(&king_last_ms[0], ev[0], ev[1]));
        PG_HIP(hipEventElapsedTime(&king_last_ms[1], ev[1], ev[2]));
        for (int k = 0; k < 3; k++) PG_HIP(hipEventDestroy(ev[k]));
    }
    return PG_OK;
}

// the count kernel alone, into the caller's n x 5 array; the flags live in the context's scratch
static int king_stats(pg_ctx *ctx, int64_t n, int64_t pb, const void *X, int dtype, int64_t ld, int snp_major, int count_a1, int64_t *sample5)
{
    PG_HIP(hipSetDevice(ctx->device));
    const size_t need = 256 + up256((size_t)pb * 4);
    const int rc = ensure(ctx, &ctx->scratch, &ctx->scratch_bytes, need);
    if (rc != PG_OK) return rc;
    char *base = static_cast<char *>(ctx->scratch);
    PG_HIP(hipMemsetAsync(base, 0, need, ctx->stream));
    KingEnc e;
    e.n = (int)n; e.count_a1 = count_a1 != 0; e.pb = pb; e.ld = ld; e.ldk = (pb + KG_BK - 1) / KG_BK * KG_BK;
    e.img = nullptr; e.plane = 0; e.bad = nullptr; e.flag = reinterpret_cast<int *>(base); e.hb = nullptr;
    e.samp = reinterpret_cast<unsigned long long *>(sample5);
    return king_encode_any<false>(ctx, e, X, dtype, snp_major, reinterpret_cast<int *>(base + 256));
}

}  // namespace pg

using namespace pg;

extern "C" size_t pg_king_acc_bytes(int64_t n, int64_t pb)
{
    if (!king_shape_ok(n, pb)) return 0;
    return king_layout(n, pb).total;
}

extern "C" int pg_king_last_batch_ms(float *encode_ms, float *pair_ms)
{
    PG_REQUIRE(encode_ms && pair_ms, "pg_king_last_batch_ms: NULL argument");
    *encode_ms = king_last_ms[0]; *pair_ms = king_last_ms[1];
    return PG_OK;
}

extern "C" size_t pg_king_zero_bytes(int64_t n)
{
    if (!king_shape_ok(n, 1)) return 0;
    return king_layout(n, 1).zero;
}

#define KING_CHECK_BED(who, dst)                                                                                                            \
    PG_REQUIRE(ctx && bed && dst, who ": NULL argument");                                                                                   \
    PG_REQUIRE(king_shape_ok(n, pb) && ldb >= (n + 3) / 4, who ": bad shape n=%lld pb=%lld ldb=%lld", (long long)n, (long long)pb, (long long)ldb)
#define KING_CHECK_X(who, dst)                                                                                                              \
    PG_REQUIRE(ctx && X && dst, who ": NULL argument");                                                                                     \
    PG_REQUIRE(king_shape_ok(n, pb) && ldX >= (snp_major ? n : pb), who ": bad shape n=%lld pb=%lld ldX=%lld snp_major=%d", (long long)n,  \
               (long long)pb, (long long)ldX, snp_major);                                                                                   \
    if (!dtype_known(dtype)) {                                                                                                              \
        set_error(who ": unknown dtype %d", dtype);                                                                                         \
        return PG_ENOTSUP;                                                                                                                  \
    }

extern "C" int pg_king_bed_acc_dev(pg_ctx *ctx, int64_t n, int64_t pb, const unsigned char *bed, int64_t ldb, int count_a1, void *acc)
{
    KING_CHECK_BED("pg_king_bed_acc_dev", acc);
    PG_REQUIRE((uintptr_t)acc % 16 == 0, "pg_king_bed_acc_dev: the accumulator must lie on 16 bytes");
    return king_batch(ctx, n, pb, bed, -1, ldb, 1, count_a1, acc);
}

extern "C" int pg_king_x_acc_dev(pg_ctx *ctx, int64_t n, int64_t pb, const void *X, int dtype, int64_t ldX, int snp_major, void *acc)
{
    KING_CHECK_X("pg_king_x_acc_dev", acc);
    PG_REQUIRE((uintptr_t)acc % 16 == 0, "pg_king_x_acc_dev: the accumulator must lie on 16 bytes");
    return king_batch(ctx, n, pb, X, dtype, ldX, snp_major != 0, 0, acc);
}

extern "C" int pg_sample_stats_bed_acc_dev(pg_ctx *ctx, int64_t n, int64_t pb, const unsigned char *bed, int64_t ldb, int count_a1, int64_t *sample5)
{
    KING_CHECK_BED("pg_sample_stats_bed_acc_dev", sample5);
    return king_stats(ctx, n, pb, bed, -1, ldb, 1, count_a1, sample5);
}

extern "C" int pg_sample_stats_x_acc_dev(pg_ctx *ctx, int64_t n, int64_t pb, const void *X, int dtype, int64_t ldX, int snp_major, int64_t *sample5)
{
    KING_CHECK_X("pg_sample_stats_x_acc_dev", sample5);
    return king_stats(ctx, n, pb, X, dtype, ldX, snp_major != 0, 0, sample5);
}

extern "C" int pg_king_finish_dev(pg_ctx *ctx, int64_t n, const void *acc, int what, float *out)
{
    PG_REQUIRE(ctx && acc && out, "pg_king_finish_dev: NULL argument");
    PG_REQUIRE(king_shape_ok(n, 1) && (what == 0 || what == 1), "pg_king_finish_dev: bad argument n=%lld what=%d", (long long)n, what);
    PG_HIP(hipSetDevice(ctx->device));
    const unsigned nt = (unsigned)((n + 31) / 32);
    king_finish_kernel<<<dim3(nt, nt), 256, 0, ctx->stream>>>(king_acc(n, acc), what, out);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

extern "C" int pg_king_counts_dev(pg_ctx *ctx, int64_t n, const void *acc, int32_t *counts5, int64_t *sample5)
{
    PG_REQUIRE(ctx && acc && counts5 && sample5, "pg_king_counts_dev: NULL argument");
    PG_REQUIRE(king_shape_ok(n, 1), "pg_king_counts_dev: bad shape n=%lld", (long long)n);
    PG_HIP(hipSetDevice(ctx->device));
    king_counts_kernel<<<dim3((unsigned)n, (unsigned)((n + 255) / 256)), 256, 0, ctx->stream>>>(king_acc(n, acc), counts5);
    PG_HIP(hipGetLastError());
    PG_HIP(hipMemcpyAsync(sample5, static_cast<const char *>(acc) + king_layout(n, 1).samp, (size_t)n * 40, hipMemcpyDeviceToDevice, ctx->stream));
    return PG_OK;
}
