// ld.hip — linkage disequilibrium on the int8 matrix pipe: the pairwise-complete Pearson r between hard-call SNPs (PLINK's --r), from
// packed .bed records or 8-bit / float32 / float64 blocks, sample- or SNP-major.  What LD pruning, clumping and a region's LD matrix read.
//
// Definition.  A SNP is hard-call when every non-missing value (in its own precision, no rounding) is exactly 0, 1 or 2; missing is
// .bed code 01, NaN or +-Inf; any other SNP counts as all missing.  With m_a[i] in {0, 1} "sample i is called" and x_a[i] its code (0 where
// missing), a pair (a, b) has the six int32 sums
//     N = sum m_a m_b   Sa = sum x_a m_b   Sb = sum m_a x_b   Sab = sum x_a x_b   Saa = sum x_a^2 m_b   Sbb = sum m_a x_b^2
// and, exactly in int64, ca = N Saa - Sa^2, cb = N Sbb - Sb^2, cab = N Sab - Sa Sb;  r = clamp(cab / sqrt((double)ca (double)cb), -1, 1),
// rounded once to float32, NaN when ca <= 0 or cb <= 0.  Everything up to the last line is integer arithmetic: the sums are testable for
// equality, and a copy of a SNP gives exactly 1, its flip 2 - x exactly -1.
//
// The LD image (opaque to the caller; pg_ld_image_bytes): three SNP-major int8 planes x, m, x^2 of pe rows each, rows of ldk = n rounded up to
// the K-tile of 128 samples, ZERO in every plane past sample n (a pad sample with m = 1 would count in N), then one int4 per SNP:
// {sum x, sum x^2, missing calls, not hard-call}.  A SNP that is not hard-call has all-zero planes and n missing calls.
//
// The pair kernel runs the 256 x 256 int8 GEMM tile of i8_pair.hpp.  A workgroup owns a pair of SNP tiles of LD_T1 = 252 SNPs.  When no SNP of either tile holds a missing call — imputed data, 8-bit arrays —
// it takes ONE product: rows = the x planes of 252 SNPs a side, N = n, and Sa, Sb, Saa, Sbb are the per-SNP totals.  Otherwise it walks the
// 3 x 3 pairs of sub-tiles of LD_T3 = 84 SNPs with "planes as output rows": each 128-row half of an operand tile holds 42 SNPs as rows
// [0, 42) x, [42, 84) m, [84, 126) x^2 (two rows spare), so that a staged half carries whole SNPs, and the epilogue picks the six sums out of
// the 3 x 3 plane products (three of them are waste).  Nine GEMM tiles instead of one for the same pairs; both paths produce the same integers.
// PG_LD_PLANES=1 sends every tile pair down the three-plane path (tests, A/B timing).
// Two output mappings: a dense block r[ia][ib], and a band, band[j][k] = r(j, j + 1 + k), for which only the tile pairs (and, inside the
// three-plane path, the sub-tile pairs) that meet the band are launched or run.  A third epilogue keeps nothing per pair: the band's pairs,
// each within a reach of its row, as r^2 in fixed point summed per SNP (LD scores, pg_ld_score_dev).
#include "geno_src.hpp"
#include "i8_pair.hpp"
#include "ld_layout.hpp"

#include <cmath>
#include <type_traits>

namespace pg {

constexpr int LD_T1 = 252;        // SNPs per tile side, one-product path
constexpr int LD_T3 = 84;         // SNPs per sub-tile side, three-plane path: 2 halves x 42 SNPs x 3 planes
constexpr int LD_H3 = 42;
constexpr long long LD_MAXN = 1LL << 28;      // exclusive: every sum fits int32 (4 n < 2^31), every product int64
constexpr long long LD_MAXPE = 1LL << 31;
constexpr long long LD_SCORE_MAXW = 1LL << 28;      // exclusive: a SNP's 2 w pairs of at most 2^32 each stay inside int64


// ---- encode -----------------------------------------------------------------------------------------------------------------------------
// one element -> code, called, not-a-hard-call
template <class T> __device__ __forceinline__ void ld_classify(T x, int &code, int &m, int &bad)
{
    if constexpr (std::is_floating_point<T>::value) {      // in the element's own precision: a double 1 + 1e-12 is not the hard call 1
        m = isfinite(x) ? 1 : 0;
        code = (m && x == T(1)) ? 1 : ((m && x == T(2)) ? 2 : 0);
        bad = (m && x != T(0) && x != T(1) && x != T(2)) ? 1 : 0;
    } else {
        const int v = (int)x;
        m = 1;
        bad = (v < 0 || v > 2) ? 1 : 0;
        code = bad ? 0 : v;
    }
}

struct LdEnc {
    int n, count_a1;
    long long pb, ld, pe, ldk, at, ngb;
    signed char *img;
    int4 *tot;
};

// A lane encodes 16 consecutive samples of one SNP:
// three 16-byte stores.  SNP-major sources: one workgroup per SNP, lanes along the samples.  Sample-major: lane = SNP (the loads of a wavefront
// are adjacent), workgroup = 64 SNPs x 1024 samples.  The totals are integer atomics: the same bits in any order.
template <class T, int LAYOUT> __global__ __launch_bounds__(256) void ld_encode_kernel(LdEnc q, const T *X)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ngrp = (int)(q.ldk / 16);
    long long g;
    int grp0, grp1, step;
    if constexpr (LAYOUT == GENO_SAMPLE) {
        const long long chunk = blockIdx.x / q.ngb, gb = blockIdx.x % q.ngb;
        g = gb * 64 + lane;
        grp0 = (int)chunk * 64 + wave; grp1 = min(ngrp, (int)chunk * 64 + 64); step = 4;
    } else {
        g = blockIdx.x;
        grp0 = threadIdx.x; grp1 = ngrp; step = 256;
    }
    int s1 = 0, s2 = 0, nm = 0, bad = 0;
    if (g < q.pb) {
        signed char *row = q.img + (size_t)(q.at + g) * q.ldk;
        const size_t plane = (size_t)q.pe * q.ldk;
        for (int grp = grp0; grp < grp1; grp += step) {
            unsigned xw[4] = {0, 0, 0, 0}, mw[4] = {0, 0, 0, 0}, qw[4] = {0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < 16; s++) {
                const int i = grp * 16 + s;
                int code = 0, m = 0, bd = 0;
                if (i < q.n) {
                    if constexpr (LAYOUT == GENO_BED) {
                        const int c = (X[(size_t)g * q.ld + (i >> 2)] >> (2 * (i & 3))) & 3;      // 00 -> 0, 10 -> 1, 11 -> 2, 01 missing
                        m = c != 1;
                        code = c == 0 ? 0 : (c == 2 ? 1 : (c == 3 ? 2 : 0));
                        if (q.count_a1 && m) code = 2 - code;
                    } else if constexpr (LAYOUT == GENO_SNP) ld_classify<T>(X[(size_t)g * q.ld + i], code, m, bd);
                    else ld_classify<T>(X[(size_t)i * q.ld + g], code, m, bd);
                    nm += 1 - m;
                }
                const int sh = 8 * (s & 3);
                xw[s >> 2] |= (unsigned)code << sh; mw[s >> 2] |= (unsigned)m << sh; qw[s >> 2] |= (unsigned)(code * code) << sh;
                s1 += code; s2 += code * code; bad |= bd;
            }
            *reinterpret_cast<uint4 *>(row + (size_t)grp * 16) = make_uint4(xw[0], xw[1], xw[2], xw[3]);
            *reinterpret_cast<uint4 *>(row + plane + (size_t)grp * 16) = make_uint4(mw[0], mw[1], mw[2], mw[3]);
            *reinterpret_cast<uint4 *>(row + 2 * plane + (size_t)grp * 16) = make_uint4(qw[0], qw[1], qw[2], qw[3]);
        }
    }
    if constexpr (LAYOUT != GENO_SAMPLE) {      // the wavefront is one SNP's
        for (int k = 1; k < 64; k <<= 1) {
            s1 += __shfl_xor(s1, k, 64); s2 += __shfl_xor(s2, k, 64); nm += __shfl_xor(nm, k, 64); bad += __shfl_xor(bad, k, 64);
        }
        if (lane != 0) return;
    }
    if (g >= q.pb) return;
    int *t = reinterpret_cast<int *>(q.tot + q.at + g);
    if (s1) atomicAdd(t, s1);
    if (s2) atomicAdd(t + 1, s2);
    if (nm) atomicAdd(t + 2, nm);
    if (bad) atomicAdd(t + 3, bad);
}

// a SNP that turned out not to be hard-call: all missing
__global__ __launch_bounds__(256) void ld_fixup_kernel(LdEnc q)
{
    const long long g = blockIdx.x;
    int4 *t = q.tot + q.at + g;
    const int bad = t->w;
    __syncthreads();
    if (!bad) return;
    const size_t plane = (size_t)q.pe * q.ldk;
    signed char *row = q.img + (size_t)(q.at + g) * q.ldk;
    for (long long o = 16LL * threadIdx.x; o < q.ldk; o += 16 * 256)
#pragma unroll
        for (int pl = 0; pl < 3; pl++) *reinterpret_cast<uint4 *>(row + pl * plane + o) = make_uint4(0, 0, 0, 0);
    if (threadIdx.x == 0) *t = make_int4(0, 0, q.n, 1);
}

template <class T, int LAYOUT> static int launch_ld_encode(pg_ctx *ctx, LdEnc q, const void *X, const char *who)
{
    long long grid = q.pb;
    if (LAYOUT == GENO_SAMPLE) {
        q.ngb = (q.pb + 63) / 64;
        grid = q.ngb * ((q.ldk / 16 + 63) / 64);
    }
    PG_REQUIRE(grid < (1LL << 31), "%s: a block of n=%d x pb=%lld is more than one launch holds", who, q.n, q.pb);
    PG_HIP(hipMemsetAsync(q.tot + q.at, 0, (size_t)q.pb * 16, ctx->stream));
    ld_encode_kernel<T, LAYOUT><<<(unsigned)grid, 256, 0, ctx->stream>>>(q, static_cast<const T *>(X));
    PG_HIP(hipGetLastError());
    if (LAYOUT != GENO_BED) {
        ld_fixup_kernel<<<(unsigned)q.pb, 256, 0, ctx->stream>>>(q);
        PG_HIP(hipGetLastError());
    }
    return PG_OK;
}

// ---- the pair kernel --------------------------------------------------------------------------------------------------------------------
struct LdPair {
    int n, KT, band, planes, tiles_b;
    long long ldk;
    const signed char *A, *B;         // x planes; m and x^2 planes pea (peb) * ldk bytes further each
    long long pea, peb;
    const int4 *ta, *tb;
    long long a0, na, b0, nb;         // SNPs [a0, a0 + na) of A against [b0, b0 + nb) of B; band: B = A, b0 = a0, nb = have - a0
    long long w;
    float *r;
    long long ldr;
    int *sums;
    // the score epilogue (band pairs only): every pair within min(w, reach[row]) credits both of its SNPs
    const int *reach;
    int adjust;
    long long *sum;
    int *npairs, *nobs;
};

// r and the six sums of one pair, to their place (o: element index of the pair in the output)
__device__ __forceinline__ void ld_store(const LdPair &q, long long o, bool valid, long long N, long long Sa, long long Sb, long long Saa, long long Sbb,
                                         long long Sab)
{
    float rv = __builtin_nanf("");
    if (valid) {
        const long long ca = N * Saa - Sa * Sa, cb = N * Sbb - Sb * Sb, cab = N * Sab - Sa * Sb;
        if (ca > 0 && cb > 0) {
            double v = (double)cab / __dsqrt_rn((double)ca * (double)cb);
            v = v > 1.0 ? 1.0 : (v < -1.0 ? -1.0 : v);
            rv = (float)v;
        }
    } else N = Sa = Sb = Saa = Sbb = Sab = 0;
    q.r[o] = rv;
    if (q.sums) {
        int *s = q.sums + o * 6;
        s[0] = (int)N; s[1] = (int)Sa; s[2] = (int)Sb; s[3] = (int)Saa; s[4] = (int)Sbb; s[5] = (int)Sab;
    }
}

// ---- the score epilogue: a pair's r^2 in fixed point at 2^-32, summed per SNP in integers ---------------------------------
// the accumulators of a (sub-)tile pair, behind the pair tile's LDS: 256 int64 sums and 256 int32 counts of the columns (the B
// SNPs), then the same of the rows (the A SNPs)
constexpr int LD_SCORE_LDS = I8P_LDS + 2 * 256 * 12;
__device__ __forceinline__ unsigned long long *ld_acc_sum(int side) { return reinterpret_cast<unsigned long long *>(i8p_lds + I8P_LDS + side * 256 * 12); }
__device__ __forceinline__ int *ld_acc_cnt(int side) { return reinterpret_cast<int *>(i8p_lds + I8P_LDS + side * 256 * 12 + 256 * 8); }

// q = rint(2^32 r^2) of a pair, r^2 = min(cab^2 / (ca cb), 1) less the ldsc bias (1 - r^2) / (N - 2) when `adjust`: three (five)
// correctly rounded fp64 operations on exact integers, so a host model gets the same bits.  false: the pair is undefined.
__device__ __forceinline__ bool ld_r2_fixed(int adjust, long long N, long long Sa, long long Sb, long long Saa, long long Sbb, long long Sab,
                                            long long &qv)
{
    const long long ca = N * Saa - Sa * Sa, cb = N * Sbb - Sb * Sb, cab = N * Sab - Sa * Sb;
    if (ca <= 0 || cb <= 0 || (adjust && N <= 2)) return false;
    double r2 = ((double)cab * (double)cab) / ((double)ca * (double)cb);
    r2 = r2 > 1.0 ? 1.0 : r2;
    if (adjust) r2 = r2 - (1.0 - r2) / (double)(N - 2);
    qv = __double2ll_rn(r2 * 4294967296.0);
    return true;
}

// One staged half.  LW lanes walk a row, lane + LW c its columns: 64 for the 252-SNP tile, 32 (two rows to a wavefront) for the 84-SNP
// sub-tile, whose rows would leave 44 of 128 column slots idle.  A row belongs to one wavefront in one half: its sum meets in a
// reduction over the LW lanes and is stored to the row accumulator; the column sums meet in the column accumulators, where the lanes
// of a row add to LW different words.
template <int LW> __device__ __forceinline__ void ld_score_half(const LdPair &q, const I8pLane ln, int half, int T, long long as0, long long as1,
                                                                long long bs0, long long bs1, long long bend)
{
    constexpr bool three = LW == 32;
    constexpr int RW = 64 / LW, ha = three ? LD_H3 : 128;
    const int *const stg = i8p_staged();
    const int lr = ln.lane / LW, lc = ln.lane % LW;
#pragma unroll 1
    for (int sa0 = ln.wave * RW; sa0 < ha; sa0 += 8 * RW) {
        const int sa = sa0 + lr;
        const long long ja = as0 + half * ha + sa;
        bool row = sa < ha && ja < as1;
        long long lim = 0;                                          // partners ja + 1 .. ja + lim
        if (row) lim = q.reach ? min(q.w, (long long)q.reach[ja]) : q.w;
        row = row && lim > 0 && bs0 <= ja + lim && bs0 + T > ja + 1;
        if (!__any(row)) continue;
        int4 a = make_int4(0, 0, 0, 0);
        if (!three && row) a = q.ta[ja];
        long long rs = 0;
        int rc = 0;
#pragma unroll 1
        for (int sb = lc; sb < T; sb += LW) {
            const long long jb = bs0 + sb, k = jb - ja - 1;
            if (!row || jb >= bs1 || jb >= bend || k < 0 || k >= lim) continue;      // bend: q.w is clamped to `have` for the first row only
            long long N, Sa, Sb, Saa, Sbb, Sab, qv;
            if (three) {
                const int *s = stg + sa * I8P_LDW + (sb / LD_H3) * 128 + sb % LD_H3;      // [plane of a][plane of b] at (pa 42) rows, (pb 42) columns
                Sab = s[0];                        Sb = s[LD_H3 * I8P_LDW];                 Sa = s[LD_H3];
                N = s[LD_H3 * I8P_LDW + LD_H3];     Saa = s[2 * LD_H3 * I8P_LDW + LD_H3];    Sbb = s[LD_H3 * I8P_LDW + 2 * LD_H3];
            } else {
                const int4 b = q.tb[jb];
                N = q.n; Sa = a.x; Saa = a.y; Sb = b.x; Sbb = b.y;
                Sab = stg[sa * I8P_LDW + sb];
            }
            if (ld_r2_fixed(q.adjust, N, Sa, Sb, Saa, Sbb, Sab, qv)) {
                rs += qv; rc += 1;
                atomicAdd(ld_acc_sum(0) + sb, (unsigned long long)qv);
                atomicAdd(ld_acc_cnt(0) + sb, 1);
            }
        }
        for (int k = 1; k < LW; k <<= 1) {
            rs += __shfl_xor(rs, k, 64); rc += __shfl_xor(rc, k, 64);
        }
        if (lc == 0 && rc) {
            ld_acc_sum(1)[half * ha + sa] = (unsigned long long)rs;
            ld_acc_cnt(1)[half * ha + sa] = rc;
        }
    }
}

// The accumulators of a finished (sub-)tile pair (the last half's barrier is behind us) go out: threads [0, 256) the columns from bs0,
// threads [256, 512) the rows from as0, one 64-bit and one 32-bit atomic per SNP with a defined pair, 64 neighbouring SNPs to a
// wavefront; and zeros for the next pair, whose first add lies behind the barriers of its products.
__device__ __forceinline__ void ld_score_out(const LdPair &q, long long as0, long long bs0)
{
    const int side = threadIdx.x >> 8, t = threadIdx.x & 255;
    const unsigned long long s = ld_acc_sum(side)[t];
    const int c = ld_acc_cnt(side)[t];
    if (c) {      // a defined pair: the SNP is one with data
        const long long g = (side ? as0 : bs0) + t;
        atomicAdd(reinterpret_cast<unsigned long long *>(q.sum + g), s);
        atomicAdd(q.npairs + g, c);
        ld_acc_sum(side)[t] = 0;
        ld_acc_cnt(side)[t] = 0;
    }
}

// SCORE = false: r (and the six sums) of every pair to a block or a band.  SCORE = true: the band's pairs, each within its row's reach,
// reduced to the fixed-point sum of r^2 and the pair count of both of its SNPs; the rows' called-sample counts to nobs.
template <bool SCORE> __global__ __launch_bounds__(512, 1) void ld_pair_kernel(LdPair q)
{
    const int tid = threadIdx.x;
    const I8pLane ln = i8p_lane();
    const long long tile_a = blockIdx.x / q.tiles_b, tile_b = blockIdx.x % q.tiles_b + (q.band ? tile_a : 0);
    const long long abase = q.a0 + tile_a * LD_T1, bbase = q.b0 + tile_b * LD_T1;
    const long long aend = q.a0 + q.na, bend = q.b0 + q.nb;      // one past the last SNP with data on either side
    // does either tile hold a missing call?
    int miss = q.planes;
    for (int k = tid; k < 2 * LD_T1; k += 512) {
        const bool sideb = k >= LD_T1;
        const long long g = (sideb ? bbase : abase) + (sideb ? k - LD_T1 : k);
        if (g < (sideb ? bend : aend)) miss |= (sideb ? q.tb : q.ta)[g].z != 0;
    }
    const bool three = __syncthreads_or(miss) != 0;
    const int T = three ? LD_T3 : LD_T1, nsub = three ? 3 : 1;
    const int *const stg = i8p_staged();
    if constexpr (SCORE) {
        ld_acc_sum(tid >> 8)[tid & 255] = 0;      // ordered before the first add by the barriers of the first products
        ld_acc_cnt(tid >> 8)[tid & 255] = 0;
        // the rows' own called samples, once per A tile: n - missing calls where the SNP's own variance term is positive
        if (tile_b == tile_a)
            for (int k = tid; k < LD_T1; k += 512) {
                const long long g = abase + k;
                if (g >= aend) continue;
                const int4 t = q.ta[g];
                const long long nm = (long long)q.n - t.z;
                q.nobs[g] = nm * t.y - (long long)t.x * t.x > 0 ? (int)nm : 0;
            }
    }

#pragma unroll 1
    for (int sub = 0; sub < nsub * nsub; sub++) {
        const long long as0 = abase + (sub / nsub) * T, bs0 = bbase + (sub % nsub) * T;      // first SNPs of the (sub-)tiles
        const long long as1 = min(as0 + T, aend);                                            // one past the last A SNP with an output
        if (as0 >= aend) continue;
        // the B SNPs that pair with an output: dense [b0, bend), band (as0, as1 - 1 + w]
        const long long bs1 = q.band ? min(bs0 + T, as1 + q.w) : min(bs0 + T, bend);
        if (bs0 >= bs1 || (q.band && bs0 + T <= as0 + 1)) continue;
        const bool data = bs0 < bend;                                                        // band: partners at or past `have` are NaN
        if constexpr (SCORE)
            if (!data) continue;                                                             // ... and credit nobody
        intx4 acc[4][8];
        i8p_zero(acc);
        if (data) {
            // DMA sources.  Rows without a SNP (the spare rows, SNPs past the window) repeat the window's last SNP: their products are never read.
            const signed char *srcA[4], *srcB[4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int row = i8p_src_row(ln, t);
                int pl = 0, s = row;
                if (three) {
                    const int h = row >> 7, rr = row & 127;
                    pl = min(rr / LD_H3, 2); s = h * LD_H3 + rr % LD_H3;
                }
                const long long ga = min(as0 + s, aend - 1), gb = min(bs0 + s, bend - 1);
                srcA[t] = q.A + ((size_t)pl * q.pea + ga) * q.ldk + i8p_src_byte(ln, row);
                srcB[t] = q.B + ((size_t)pl * q.peb + gb) * q.ldk + i8p_src_byte(ln, row);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the stores of the previous epilogue are not counted against the loads below
            i8p_products(ln, srcA, srcB, q.KT, acc);
        }
        // ---- epilogue: the accumulators meet through LDS, one 128-row half of A at a time
        if constexpr (SCORE) {
#pragma unroll 1
            for (int half = 0; half < 2; half++) {
                i8p_stage(ln, half, acc);
                if (three) ld_score_half<32>(q, ln, half, T, as0, as1, bs0, bs1, bend);
                else ld_score_half<64>(q, ln, half, T, as0, as1, bs0, bs1, bend);
                __syncthreads();
            }
            ld_score_out(q, as0, bs0);
        } else {
#pragma unroll 1
            for (int half = 0; half < 2; half++) {
                i8p_stage(ln, half, acc);
                const int ha = three ? LD_H3 : 128;                   // A SNPs in this half
                for (int idx = tid; idx < ha * T; idx += 512) {
                    const int sa = idx / T, sb = idx - sa * T;
                    const long long ja = as0 + half * ha + sa, jb = bs0 + sb;
                    if (ja >= as1 || jb >= bs1 || half * ha + sa >= T) continue;
                    long long o;
                    if (q.band) {
                        const long long k = jb - ja - 1;
                        if (k < 0 || k >= q.w) continue;
                        o = (ja - q.a0) * q.ldr + k;
                    } else o = (ja - q.a0) * q.ldr + (jb - q.b0);
                    const bool valid = jb < bend;
                    long long N = 0, Sa = 0, Sb = 0, Saa = 0, Sbb = 0, Sab = 0;
                    if (valid && three) {
                        const int *s = stg + sa * I8P_LDW + (sb / LD_H3) * 128 + sb % LD_H3;      // [plane of a][plane of b] at (pa 42) rows, (pb 42) columns
                        Sab = s[0];                        Sb = s[LD_H3 * I8P_LDW];                 Sa = s[LD_H3];
                        N = s[LD_H3 * I8P_LDW + LD_H3];     Saa = s[2 * LD_H3 * I8P_LDW + LD_H3];    Sbb = s[LD_H3 * I8P_LDW + 2 * LD_H3];
                    } else if (valid) {
                        const int4 a = q.ta[ja], b = q.tb[jb];
                        N = q.n; Sa = a.x; Saa = a.y; Sb = b.x; Sbb = b.y;
                        Sab = stg[sa * I8P_LDW + sb];
                    }
                    ld_store(q, o, valid, N, Sa, Sb, Saa, Sbb, Sab);
                }
                __syncthreads();
            }
        }
    }
}

template <bool SCORE> static int launch_ld_pair(pg_ctx *ctx, LdPair q, long long tiles_a, long long tiles_b, const char *who)
{
    PG_REQUIRE(tiles_a * tiles_b < (1LL << 31), "%s: too many tiles (%lld x %lld)", who, tiles_a, tiles_b);
    q.tiles_b = (int)tiles_b;
    q.planes = env_flag("PG_LD_PLANES");
    constexpr int lds = SCORE ? LD_SCORE_LDS : I8P_LDS;
    PG_HIP((i8p_lds_limit<ld_pair_kernel<SCORE>, lds>(ctx->device)));
    ld_pair_kernel<SCORE><<<(unsigned)(tiles_a * tiles_b), 512, lds, ctx->stream>>>(q);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

static bool ld_shape_ok(int64_t n, int64_t pe) { return n >= 1 && n < LD_MAXN && pe >= 1 && pe < LD_MAXPE; }
static bool ld_aligned(const void *image) { return (uintptr_t)image % 16 == 0; }      // 16-byte stores and LDS-DMA loads of whole rows

}  // namespace pg

using namespace pg;

extern "C" size_t pg_ld_image_bytes(int64_t n, int64_t pe)
{
    if (!ld_shape_ok(n, pe)) return 0;
    return ld_layout(n, pe).total;
}

static LdEnc ld_enc(int64_t n, int64_t pb, int64_t ld, int count_a1, void *image, int64_t pe, int64_t at)
{
    const LdLayout L = ld_layout(n, pe);
    LdEnc q;
    q.n = (int)n; q.count_a1 = count_a1 != 0; q.pb = pb; q.ld = ld; q.pe = pe; q.ldk = L.ldk; q.at = at; q.ngb = 1;
    q.img = static_cast<signed char *>(image);
    q.tot = reinterpret_cast<int4 *>(static_cast<char *>(image) + L.totals);
    return q;
}

extern "C" int pg_ld_encode_bed_dev(pg_ctx *ctx, int64_t n, int64_t pb, const unsigned char *bed, int64_t ldb, int count_a1, void *image, int64_t pe,
                                    int64_t at)
{
    PG_REQUIRE(ctx && bed && image, "pg_ld_encode_bed_dev: NULL argument");
    PG_REQUIRE(ld_aligned(image), "pg_ld_encode_bed_dev: the image must lie on 16 bytes");
    PG_REQUIRE(ld_shape_ok(n, pe) && pb >= 0 && at >= 0 && at + pb <= pe && ldb >= (n + 3) / 4,
               "pg_ld_encode_bed_dev: bad shape n=%lld pb=%lld ldb=%lld pe=%lld at=%lld", (long long)n, (long long)pb, (long long)ldb, (long long)pe,
               (long long)at);
    if (pb == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    return launch_ld_encode<unsigned char, GENO_BED>(ctx, ld_enc(n, pb, ldb, count_a1, image, pe, at), bed, "pg_ld_encode_bed_dev");
}

extern "C" int pg_ld_encode_x_dev(pg_ctx *ctx, int64_t n, int64_t pb, const void *X, int dtype, int64_t ldX, int snp_major, void *image, int64_t pe,
                                  int64_t at)
{
    PG_REQUIRE(ctx && X && image, "pg_ld_encode_x_dev: NULL argument");
    PG_REQUIRE(ld_aligned(image), "pg_ld_encode_x_dev: the image must lie on 16 bytes");
    PG_REQUIRE(ld_shape_ok(n, pe) && pb >= 0 && at >= 0 && at + pb <= pe && ldX >= (snp_major ? n : pb),
               "pg_ld_encode_x_dev: bad shape n=%lld pb=%lld ldX=%lld snp_major=%d pe=%lld at=%lld", (long long)n, (long long)pb, (long long)ldX, snp_major,
               (long long)pe, (long long)at);
    if (!dtype_known(dtype)) {
        set_error("pg_ld_encode_x_dev: unknown dtype %d", dtype);
        return PG_ENOTSUP;
    }
    if (pb == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    const LdEnc q = ld_enc(n, pb, ldX, 0, image, pe, at);
    return geno_dispatch(dtype, snp_major != 0, [&](auto src) {
        using S = decltype(src);
        return launch_ld_encode<typename S::type, S::layout>(ctx, q, X, "pg_ld_encode_x_dev");
    });
}

// Rows move towards the front in runs of `from` SNPs, in stream order: source and destination of one copy never overlap.  That is
// 4 ceil(count / from) device-to-device copies: a carry much longer than the batch behind it (window >> snp_batch) pays for it in launches.
extern "C" int pg_ld_shift_dev(pg_ctx *ctx, int64_t n, void *image, int64_t pe, int64_t from, int64_t count)
{
    PG_REQUIRE(ctx && image, "pg_ld_shift_dev: NULL argument");
    PG_REQUIRE(ld_shape_ok(n, pe) && from >= 0 && count >= 0 && from + count <= pe, "pg_ld_shift_dev: bad shape n=%lld pe=%lld from=%lld count=%lld",
               (long long)n, (long long)pe, (long long)from, (long long)count);
    if (from == 0 || count == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    const LdLayout L = ld_layout(n, pe);
    char *base = static_cast<char *>(image);
    for (int64_t c = 0; c < count; c += from) {
        const size_t m = (size_t)(count - c < from ? count - c : from);
        for (int pl = 0; pl < 3; pl++)
            PG_HIP(hipMemcpyAsync(base + pl * L.plane + (size_t)c * L.ldk, base + pl * L.plane + (size_t)(from + c) * L.ldk, m * L.ldk,
                                  hipMemcpyDeviceToDevice, ctx->stream));
        PG_HIP(hipMemcpyAsync(base + L.totals + (size_t)c * 16, base + L.totals + (size_t)(from + c) * 16, m * 16, hipMemcpyDeviceToDevice, ctx->stream));
    }
    return PG_OK;
}

extern "C" int pg_ld_block_dev(pg_ctx *ctx, int64_t n, const void *A, int64_t pea, int64_t a0, int64_t na, const void *B, int64_t peb, int64_t b0,
                               int64_t nb, float *r, int64_t ldr, int *sums)
{
    PG_REQUIRE(ctx && A && B && r, "pg_ld_block_dev: NULL argument");
    PG_REQUIRE(ld_aligned(A) && ld_aligned(B), "pg_ld_block_dev: the images must lie on 16 bytes");
    PG_REQUIRE(ld_shape_ok(n, pea) && ld_shape_ok(n, peb) && a0 >= 0 && na >= 0 && a0 + na <= pea && b0 >= 0 && nb >= 0 && b0 + nb <= peb && ldr >= nb,
               "pg_ld_block_dev: bad shape n=%lld A [%lld, +%lld) of %lld, B [%lld, +%lld) of %lld, ldr=%lld", (long long)n, (long long)a0, (long long)na,
               (long long)pea, (long long)b0, (long long)nb, (long long)peb, (long long)ldr);
    if (na == 0 || nb == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    const LdLayout La = ld_layout(n, pea), Lb = ld_layout(n, peb);
    LdPair q;
    q.n = (int)n; q.ldk = La.ldk; q.KT = (int)(La.ldk / LD_BK); q.band = 0; q.w = 0;
    q.A = static_cast<const signed char *>(A); q.pea = pea; q.ta = reinterpret_cast<const int4 *>(static_cast<const char *>(A) + La.totals);
    q.B = static_cast<const signed char *>(B); q.peb = peb; q.tb = reinterpret_cast<const int4 *>(static_cast<const char *>(B) + Lb.totals);
    q.a0 = a0; q.na = na; q.b0 = b0; q.nb = nb; q.r = r; q.ldr = ldr; q.sums = sums;
    q.reach = nullptr; q.adjust = 0; q.sum = nullptr; q.npairs = q.nobs = nullptr;
    return launch_ld_pair<false>(ctx, q, (na + LD_T1 - 1) / LD_T1, (nb + LD_T1 - 1) / LD_T1, "pg_ld_block_dev");
}

extern "C" int pg_ld_band_dev(pg_ctx *ctx, int64_t n, const void *image, int64_t pe, int64_t j0, int64_t rows, int64_t have, int64_t w, float *band,
                              int64_t ldo, int *sums)
{
    PG_REQUIRE(ctx && image && band, "pg_ld_band_dev: NULL argument");
    PG_REQUIRE(ld_aligned(image), "pg_ld_band_dev: the image must lie on 16 bytes");
    PG_REQUIRE(ld_shape_ok(n, pe) && j0 >= 0 && rows >= 0 && j0 + rows <= have && have <= pe && w >= 1 && w < LD_MAXPE && ldo >= w,
               "pg_ld_band_dev: bad shape n=%lld rows [%lld, +%lld), have=%lld of %lld, w=%lld, ldo=%lld", (long long)n, (long long)j0, (long long)rows,
               (long long)have, (long long)pe, (long long)w, (long long)ldo);
    if (rows == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    const LdLayout L = ld_layout(n, pe);
    LdPair q;
    q.n = (int)n; q.ldk = L.ldk; q.KT = (int)(L.ldk / LD_BK); q.band = 1; q.w = w;
    q.A = q.B = static_cast<const signed char *>(image); q.pea = q.peb = pe;
    q.ta = q.tb = reinterpret_cast<const int4 *>(static_cast<const char *>(image) + L.totals);
    q.a0 = q.b0 = j0; q.na = rows; q.nb = have - j0; q.r = band; q.ldr = ldo; q.sums = sums;
    q.reach = nullptr; q.adjust = 0; q.sum = nullptr; q.npairs = q.nobs = nullptr;
    // the partners of A tile t, SNPs (252 t, 252 t + 251 + w], lie in the B tiles t .. t + (251 + w) / 252
    return launch_ld_pair<false>(ctx, q, (rows + LD_T1 - 1) / LD_T1, 1 + (LD_T1 - 1 + w) / LD_T1, "pg_ld_band_dev");
}

extern "C" int pg_ld_score_dev(pg_ctx *ctx, int64_t n, const void *image, int64_t pe, int64_t j0, int64_t rows, int64_t have, int64_t w,
                               const int32_t *reach, int adjust, int64_t *sum, int32_t *npairs, int32_t *nobs)
{
    PG_REQUIRE(ctx && image && sum && npairs && nobs, "pg_ld_score_dev: NULL argument");
    PG_REQUIRE(ld_aligned(image), "pg_ld_score_dev: the image must lie on 16 bytes");
    PG_REQUIRE((uintptr_t)sum % 8 == 0, "pg_ld_score_dev: sum must lie on 8 bytes");
    PG_REQUIRE(ld_shape_ok(n, pe) && j0 >= 0 && rows >= 0 && j0 + rows <= have && have <= pe && w >= 1 && w < LD_SCORE_MAXW,
               "pg_ld_score_dev: bad shape n=%lld rows [%lld, +%lld), have=%lld of %lld, w=%lld", (long long)n, (long long)j0, (long long)rows,
               (long long)have, (long long)pe, (long long)w);
    if (rows == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    const LdLayout L = ld_layout(n, pe);
    LdPair q;
    q.n = (int)n; q.ldk = L.ldk; q.KT = (int)(L.ldk / LD_BK); q.band = 1;
    q.w = w < have - 1 - j0 ? w : have - 1 - j0;      // no partner at or past `have`: the B tiles beyond it are not launched
    q.A = q.B = static_cast<const signed char *>(image); q.pea = q.peb = pe;
    q.ta = q.tb = reinterpret_cast<const int4 *>(static_cast<const char *>(image) + L.totals);
    q.a0 = q.b0 = j0; q.na = rows; q.nb = have - j0; q.r = nullptr; q.ldr = 0; q.sums = nullptr;
    q.reach = reach; q.adjust = adjust != 0; q.sum = reinterpret_cast<long long *>(sum); q.npairs = npairs; q.nobs = nobs;
    return launch_ld_pair<true>(ctx, q, (rows + LD_T1 - 1) / LD_T1, 1 + (LD_T1 - 1 + q.w) / LD_T1, "pg_ld_score_dev");
}
