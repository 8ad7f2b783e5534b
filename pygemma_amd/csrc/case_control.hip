// case_control.hip — per-SNP tests of a 0/1 trait on contingency tables (PLINK's --assoc, --model, --fisher and --mh), straight from
// packed .bed records: every statistic is a function of exact integer counts.
//
// Samples fall into 2 S groups, (stratum k, case) = group 2 k and (stratum k, control) = group 2 k + 1, S = 1..16; a sample without a
// status or a stratum is in no group and is counted nowhere.  pg_cc_setup_dev turns (status, stratum) into one mask word per group and
// 16-sample .bed word: bit 2 t is set when sample 16 j + t is a member, so a mask is a subset of 0x55555555 and the bits of the samples
// >= n are clear; it also counts the members of every group.  pg_cc_pack_x_dev turns an array block (8-bit, float32, float64; sample- or
// SNP-major) into records in .bed coding (0 -> 00, missing -> 01, 1 -> 10, 2 -> 11; the pad calls of the last byte 00) and flags the
// SNPs that hold another observed value, so the counting kernel has one shape: pg_cc_count_dev, for a record word with the low bits lo
// and the high bits hi of its 16 calls and a group's mask M, adds popc(lo & ~hi & M) missing, popc(hi & ~lo & M) heterozygous and
// popc(lo & hi & M) calls of code 11; code 00 is the group's size less the three.
//
// This is a bandwidth kernel; its shapes:
//   count       16 lanes per record, 16 bytes (64 calls) per lane and step, as the QC kernel reads records (snp_stats.hip): 16-byte,
//               4-byte or byte-wise loads by the alignment of base and pitch; a lane never reads past ceil(n/4) bytes of its record, and
//               the pad bits of the last byte are cleared by the masks (by n, never by what the bytes hold).  The 6 S counters live in
//               registers: the kernel is compiled for 1, 2, 4, 8 and 16 strata with the loop over the groups unrolled, so no counter is
//               indexed at run time (no scratch).  A butterfly (__shfl_xor over 1, 2, 4, 8) leaves the totals in all 16 lanes; lane k
//               then forms stratum k's allelic table and its four Cochran-Mantel-Haenszel terms, and lane 0 adds them in stratum order.
//   pack, SNP-major     one wavefront per SNP, 16 bytes per lane and step; a lane's 16, 4 or 2 codes are 4 bytes, 1 byte or half a byte
//                       (joined with the neighbour lane's) of the record.
//   pack, sample-major  lane = 16 bytes of adjacent SNPs (4 bytes of an 8-bit row), wavefront = 64 samples (16 bytes of every record) with
//                       sixteen rows of loads in flight, workgroup = 256 samples: the four wavefronts write adjacent 16-byte pieces of the
//                       same records.  The coding of an element is selects only; nothing between a load and its store branches per lane.
//   stats       one lane per SNP.
// No atomics, no split over samples: a row depends on its SNP, the status and the strata alone — not on pb, the pitch, the batch or the run.
//
// Operation order (fp64, -ffp-contract=off; (double)(...) is the one conversion of an exact int64, * and / round once each):
//   2 x 2 table a b / c d with margins r1 = a + b, r2 = c + d, c1 = a + c, c2 = b + d, T = r1 + r2:
//       chi2 = ((double)T * (D * D)) / ((double)(r1 r2) * (double)(c1 c2)),  D = (double)(a d - b c);  NaN when a margin is 0
//     allelic: a = A_case, b = 2 R - A_case, c = A_ctrl, d = 2 S' - A_ctrl;  dominant: r1 + r2, r0 / s1 + s2, s0;  recessive: r2, r0 + r1 / s2, s0 + s1
//   or      = (double)(a d) / (double)(b c) of the allelic table;  +inf when b c = 0 < a d, NaN when both are 0
//   af      = (double)A / (double)(2 R)                                     (cases; controls alike)
//   trend   = ((double)N * (U * U)) / ((double)(R S') * V),  U = (double)(N A_case - R A_tot),  V = (double)(N (n1 + 4 n2) - A_tot^2);  NaN when V = 0
//   geno    = t0 + t1 + t2 (left to right),  t_i = (d_i * d_i) / ((double)(R S') * (double)n_i),  d_i = (double)(r_i N - R n_i);  NaN when an n_i = 0
//             (the six cells (O - E)^2 / E of the 2 x 3 table, the two of a column joined exactly: 1 / R + 1 / S' = N / (R S'))
//   CMH, stratum k with allelic table a b / c d (contributing when it holds a called case and a called control), in the order k = 0 .. S - 1:
//       u   += (double)(a T - r1 c1) / (double)T
//       v   += ((double)(r1 r2) * (double)(c1 c2)) / ((double)(T T) * (double)(T - 1))
//       sad += (double)(a d) / (double)T,   sbc += (double)(b c) / (double)T
//     chi2_cmh = (u * u) / v, NaN when v = 0;  or_mh = sad / sbc, NaN when sbc = 0
//   Fisher, on the allelic table: x = a runs over lo = max(0, r1 + c1 - T) .. hi = min(r1, c1); the hypergeometric probabilities are built
//     unnormalised from the mode (r1 + 1)(c1 + 1) / (T + 2) (clamped to lo .. hi) outward,
//       P(x - 1) = P(x) * (double)(x (T - r1 - c1 + x)) / (double)((r1 - x + 1)(c1 - x + 1)),
//       P(x + 1) = P(x) * (double)((r1 - x)(c1 - x)) / (double)((x + 1)(T - r1 - c1 + x + 1)),
//     in two sweeps of the same operations (so the same values): sum P and P(a), then the sum of the terms <= P(a) (1 + 2^-30), downward
//     terms first; p = min(1, tail / sum).
//   Every statistic of a row is NaN when the row has no called case or no called control.
// Integer ranges: n < 2^30, so a count is < 2^30, an allele count and a margin of an allelic table < 2^31 (T <= 2^31 - 2), and every
// product of two of them < 2^62: each cross-difference above is exact in int64 (the arithmetic stands next to each).
#include "geno_src.hpp"
#include "../../include/pygemma_cc.h"

#include <cmath>
#include <type_traits>

namespace pg {

constexpr int CC_MAXS = PG_CC_MAX_STRATA;
constexpr long long CC_MAXPB = 1LL << 25;       // SNPs per call
constexpr long long CC_MAXGRID = 1LL << 24;     // workgroups of 256 per launch, exclusive: under 2^32 threads
constexpr int CC_ROWS = 256;                    // samples per workgroup of a sample-major pack
constexpr size_t CC_HEAD = 256;                 // bytes of the work area in front of the masks: the 2 S group sizes (int32)

// mask words per group: one per 16 samples, up to a multiple of four (a lane takes the masks of its four record words in one 16-byte load)
static inline long long cc_words(long long n) { return ((n + 15) / 16 + 3) & ~3LL; }

// ---- set-up: the group masks and sizes ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cc_mask_kernel(int n, int S, long long W, const signed char *status, const int *stratum, unsigned *masks)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= 2 * S * W) return;
    const int g = (int)(t / W);
    const long long j = t % W;
    unsigned m = 0;
    for (int k = 0; k < 16; k++) {
        const long long i = 16 * j + k;
        if (i >= n) break;
        const int st = status[i], sk = stratum ? stratum[i] : 0;
        if (sk == (g >> 1) && st == ((g & 1) ? 0 : 1)) m |= 1u << (2 * k);
    }
    masks[t] = m;
}

// one wavefront per group counts its members
__global__ __launch_bounds__(64) void cc_size_kernel(long long W, const unsigned *masks, int *sizes)
{
    const unsigned *row = masks + (size_t)blockIdx.x * W;
    int c = 0;
    for (long long j = threadIdx.x; j < W; j += 64) c += __popc(row[j]);
    for (int m = 1; m < 64; m <<= 1) c += __shfl_xor(c, m, 64);
    if (threadIdx.x == 0) sizes[blockIdx.x] = c;
}

// ---- pack: array blocks -> records ---------------------------------------------------------------------------------------------------
// the 2-bit code of one element, and whether it is an observed value other than 0, 1, 2: in the element's own precision, as the LD
// encoder judges a hard call (a float64 1 + 1e-12 is no hard call, a finite 1e300 is a value)
// Selects, no branches: sixteen or sixty-four of these stand between a load and its store.
template <class T> __device__ __forceinline__ unsigned cc_code(T x, unsigned &soft)
{
    if constexpr (std::is_floating_point<T>::value) {
        const bool z = x == T(0), o = x == T(1), t = x == T(2);
        unsigned code = z ? 0u : 1u;
        code = o ? 2u : code;
        code = t ? 3u : code;
        soft |= (unsigned)(!(z | o | t) & isfinite(x));
        return code;
    } else {
        const unsigned u = (unsigned char)x;                           // an int8 -1 is 255: a value, and no call
        const bool ok = u <= 2u;
        soft |= (unsigned)!ok;
        return ok ? u + (u != 0u) : 1u;
    }
}

// E elements at p, as one load of E sizeof(T) = 16 (or 4) bytes (vec) or one by one
template <class T, int E> __device__ __forceinline__ void cc_load(T (&r)[E], const T *p, bool vec)
{
    if (vec) __builtin_memcpy(r, __builtin_assume_aligned(p, E * sizeof(T)), E * sizeof(T));
    else {
#pragma unroll
        for (int s = 0; s < E; s++) r[s] = p[s];
    }
}

// the bytes [b, b + 4) of a record from one word, those below bpr: one 4-byte store where the address allows, else byte by byte
__device__ __forceinline__ void cc_store4(unsigned char *row, int b, int bpr, unsigned w, bool vec4)
{
    if (vec4 && b + 4 <= bpr) *reinterpret_cast<unsigned *>(row + b) = w;
    else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (b + k < bpr) row[b + k] = (unsigned char)(w >> (8 * k));
    }
}

// X, rec and hard do not overlap: the loads of the next steps need not wait for the stores of this one
template <class T>
__global__ __launch_bounds__(256) void cc_pack_snp_kernel(int n, long long pb, const T *__restrict__ X, long long ldX, bool vec, unsigned char *__restrict__ rec,
                                                          long long ldb, bool vec4, unsigned char *__restrict__ hard)
{
    constexpr int E = 16 / sizeof(T);                                  // 16, 4 or 2 calls per lane and step: 4 bytes, 1 byte, half a byte
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= pb) return;
    const T *row = X + g * ldX;
    unsigned char *out = rec + g * ldb;
    const int bpr = (n + 3) / 4;
    const int nfull = n / (64 * E);                                    // steps in which every lane's run lies inside the row
    unsigned soft = 0;
    auto emit = [&](int t0, const T (&r)[E]) {
        unsigned w = 0;
#pragma unroll
        for (int s = 0; s < E; s++) w |= cc_code<T>(r[s], soft) << (2 * s);
        if constexpr (E == 16) cc_store4(out, t0 / 4, bpr, w, vec4);
        else if constexpr (E == 4) {
            if (t0 / 4 < bpr) out[t0 / 4] = (unsigned char)w;
        } else {
            const unsigned up = __shfl_xor(w, 1, 64);                  // every lane of the wavefront is here
            if (!(lane & 1) && t0 / 4 < bpr) out[t0 / 4] = (unsigned char)(w | (up << 4));
        }
    };
    auto step = [&](int it) {
        const int t0 = (it * 64 + lane) * E;
        T r[E];
        cc_load<T, E>(r, row + t0, vec);
        emit(t0, r);
    };
    if constexpr (E == 2) {                                            // the cross-lane join keeps this loop as it is
        for (int it = 0; it < nfull; it++) step(it);
    } else {
#pragma unroll 4
        for (int it = 0; it < nfull; it++) step(it);
    }
    if (nfull * 64 * E < n) {                                          // the partial step: guarded element loads, calls past n are 00
        const int t0 = (nfull * 64 + lane) * E;
        T r[E];
#pragma unroll
        for (int s = 0; s < E; s++) r[s] = t0 + s < n ? row[t0 + s] : T(0);
        emit(t0, r);
    }
    if (soft) hard[g] = 0;
}

// SNPs per lane of a sample-major block, as the QC kernel takes them
template <class T> constexpr int cc_sm_e() { return sizeof(T) == 1 ? 4 : 16 / (int)sizeof(T); }

// workgroup (cb, chunk): lanes' SNPs [64 E cb, 64 E (cb + 1)), samples [256 chunk, 256 (chunk + 1)), wavefront w its samples [64 w, 64 w + 64)
template <class T>
__global__ __launch_bounds__(256) void cc_pack_sm_kernel(int n, long long pb, const T *__restrict__ X, long long ldX, bool vec, long long ncb,
                                                         unsigned char *__restrict__ rec, long long ldb, bool vec16, bool vec4, unsigned char *__restrict__ hard)
{
    constexpr int E = cc_sm_e<T>();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // the same in every lane, and known to be
    const long long chunk = blockIdx.x / ncb, cb = blockIdx.x % ncb;
    const long long g0 = (cb * 64 + lane) * E;
    const long long r0 = chunk * CC_ROWS + 64 * wave;                  // the wavefront's first sample: a multiple of 64
    if (r0 >= n || g0 >= pb) return;
    const bool fast = vec && (cb + 1) * 64 * E <= pb;                  // the same in every lane of the workgroup: one 16-byte (4-byte) load per row
    const int bpr = (n + 3) / 4, b0 = (int)(r0 / 4);
    unsigned w[E][4];
    unsigned soft[E];
#pragma unroll
    for (int e = 0; e < E; e++) soft[e] = 0;
#pragma unroll
    for (int e = 0; e < E; e++) w[e][0] = w[e][1] = w[e][2] = w[e][3] = 0;
#pragma unroll 1
    for (int q = 0; q < 4; q++) {                                      // not unrolled: sixteen rows of loads in flight, not sixty-four
        // a row past the last is read as the last one (no branch between the loads) and its calls are 00
        T r[16][E];
#pragma unroll
        for (int t = 0; t < 16; t++) {
            const long long i = r0 + 16 * q + t;
            const T *p = X + (size_t)(i < n ? i : n - 1) * ldX + g0;
            if (fast) cc_load<T, E>(r[t], p, true);
            else {
#pragma unroll
                for (int e = 0; e < E; e++) r[t][e] = p[g0 + e < pb ? e : 0];      // a column past the last is read as the lane's first
            }
        }
        unsigned acc[E];
#pragma unroll
        for (int e = 0; e < E; e++) acc[e] = 0;
#pragma unroll
        for (int t = 0; t < 16; t++) {
            const unsigned in = r0 + 16 * q + t < n ? 3u : 0u;       // no branch: the flag of a repeated last row changes nothing
#pragma unroll
            for (int e = 0; e < E; e++) acc[e] |= (cc_code<T>(r[t][e], soft[e]) & in) << (2 * t);
        }
#pragma unroll
        for (int e = 0; e < E; e++) {                                  // q is the same in every lane: no register is indexed at run time
#pragma unroll
            for (int k = 0; k < 4; k++) w[e][k] = q == k ? acc[e] : w[e][k];
        }
    }
#pragma unroll
    for (int e = 0; e < E; e++) {
        if (g0 + e >= pb) continue;
        if (soft[e]) hard[g0 + e] = 0;
        unsigned char *out = rec + (g0 + e) * ldb;
        if (vec16 && b0 + 16 <= bpr) *reinterpret_cast<uint4 *>(out + b0) = make_uint4(w[e][0], w[e][1], w[e][2], w[e][3]);
        else {
#pragma unroll
            for (int q = 0; q < 4; q++) cc_store4(out, b0 + 4 * q, bpr, w[e][q], vec4);
        }
    }
}

template <class T, int LAY>
static int launch_cc_pack(pg_ctx *ctx, int n, long long pb, const void *X, long long ldX, unsigned char *rec, long long ldb, unsigned char *hard)
{
    const T *Xt = static_cast<const T *>(X);
    const bool vec4 = ((uintptr_t)rec % 4 == 0) && ldb % 4 == 0, vec16 = ((uintptr_t)rec % 16 == 0) && ldb % 16 == 0;
    if (LAY == GENO_SNP) {
        const bool vec = ((uintptr_t)X % 16 == 0) && ((size_t)ldX * sizeof(T)) % 16 == 0;
        static_assert(CC_MAXPB / 4 + 1 < CC_MAXGRID, "one wavefront per SNP");
        cc_pack_snp_kernel<T><<<(unsigned)((pb + 3) / 4), 256, 0, ctx->stream>>>(n, pb, Xt, ldX, vec, rec, ldb, vec4, hard);
        PG_HIP(hipGetLastError());
        return PG_OK;
    }
    constexpr int E = cc_sm_e<T>();
    const bool vec = ((uintptr_t)X % (E * sizeof(T)) == 0) && ((size_t)ldX * sizeof(T)) % (E * sizeof(T)) == 0;
    const long long R = ((long long)n + CC_ROWS - 1) / CC_ROWS, ncb = (pb + 64 * E - 1) / (64 * E);
    cc_pack_sm_kernel<T><<<(unsigned)(R * ncb), 256, 0, ctx->stream>>>(n, pb, Xt, ldX, vec, ncb, rec, ldb, vec16, vec4, hard);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

// ---- count: 16 lanes per record ------------------------------------------------------------------------------------------------------
// SB: the strata the registers hold (S <= SB); the loops over the groups are unrolled, the guard g < 2 S is the same in every lane
template <int SB>
__global__ __launch_bounds__(256) void cc_count_kernel(int n, long long pb, const unsigned char *bed, long long ldb, int count_a1, int S, bool vec16, bool vec4,
                                                       const int *sizes, const unsigned *masks, long long W, const unsigned char *hard, long long *counts,
                                                       double *cmh)
{
    const int sub = threadIdx.x & 15;
    const long long g = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (g >= pb) return;                                               // whole 16-lane groups leave
    const unsigned char *rec = bed + g * ldb;
    const bool dead = hard && !hard[g];                                // not a hard-call SNP: no call is counted
    const int bpr = dead ? 0 : (n + 3) / 4;
    int c[2 * SB][3];
#pragma unroll
    for (int q = 0; q < 2 * SB; q++) c[q][0] = c[q][1] = c[q][2] = 0;
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
        unsigned ms[4], ht[4], hh[4];                                  // 01 missing, 10 heterozygous, 11: on the low bit of every call
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const unsigned lo = w[q], hi = w[q] >> 1;                  // the masks keep the low bit of a call, and of a sample < n only
            ms[q] = lo & ~hi; ht[q] = hi & ~lo; hh[q] = lo & hi;
        }
        const unsigned *mrow = masks + (b0 >> 2);                      // b0 / 4 is a multiple of 4 and b0 / 4 + 4 <= W: 16 bytes inside the row
#pragma unroll
        for (int q = 0; q < 2 * SB; q++) {
            if (q < 2 * S) {
                const uint4 M = *reinterpret_cast<const uint4 *>(mrow + (size_t)q * W);
                c[q][0] += __popc(ms[0] & M.x) + __popc(ms[1] & M.y) + __popc(ms[2] & M.z) + __popc(ms[3] & M.w);
                c[q][1] += __popc(ht[0] & M.x) + __popc(ht[1] & M.y) + __popc(ht[2] & M.z) + __popc(ht[3] & M.w);
                c[q][2] += __popc(hh[0] & M.x) + __popc(hh[1] & M.y) + __popc(hh[2] & M.z) + __popc(hh[3] & M.w);
            }
        }
    }
    // totals in all 16 lanes, then lane k takes stratum k: miss, het and code 11 of its cases and controls
    int cs[3] = {0, 0, 0}, ct[3] = {0, 0, 0};
#pragma unroll
    for (int q = 0; q < 2 * SB; q++) {
        if (q < 2 * S) {
#pragma unroll
            for (int j = 0; j < 3; j++) {
                int v = c[q][j];
                for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m, 64);
                if (sub == (q >> 1)) {
                    if (q & 1) ct[j] = v; else cs[j] = v;
                }
            }
        }
    }
    const bool mine = sub < S && !dead;
    const long long size_r = mine ? sizes[2 * sub] : 0, size_s = mine ? sizes[2 * sub + 1] : 0;
    // genotype counts of the stratum: code 00 by subtraction; codes 00 and 11 are 0 and 2 copies of the counted allele, swapped by count_a1
    const long long rm = cs[0], r1 = cs[1], r11 = cs[2], r00 = size_r - rm - r1 - r11;
    const long long sm = ct[0], s1 = ct[1], s11 = ct[2], s00 = size_s - sm - s1 - s11;
    const long long r0 = count_a1 ? r11 : r00, r2 = count_a1 ? r00 : r11, s0 = count_a1 ? s11 : s00, s2 = count_a1 ? s00 : s11;
    // the stratum's allelic table a b / c d; every entry and margin < 2^31
    const long long Rk = r0 + r1 + r2, Sk = s0 + s1 + s2;
    const long long a = r1 + 2 * r2, b = 2 * Rk - a, cc = s1 + 2 * s2, d = 2 * Sk - cc;
    const long long m1 = a + b, m2 = cc + d, k1 = a + cc, k2 = b + d, T = m1 + m2;
    double tu = 0.0, tv = 0.0, tad = 0.0, tbc = 0.0;
    if (Rk > 0 && Sk > 0) {                                            // then T >= 4
        tu = (double)(a * T - m1 * k1) / (double)T;                    // a T, m1 k1 < 2^62
        tv = ((double)(m1 * m2) * (double)(k1 * k2)) / ((double)(T * T) * (double)(T - 1));      // m1 m2, k1 k2 <= (T / 2)^2 < 2^60, T T < 2^62
        tad = (double)(a * d) / (double)T;
        tbc = (double)(b * cc) / (double)T;
    }
    long long tab[8] = {r0, r1, r2, rm, s0, s1, s2, sm};               // pooled over the strata: lanes >= S hold zeros
#pragma unroll
    for (int j = 0; j < 8; j++)
        for (int m = 1; m < 16; m <<= 1) tab[j] += __shfl_xor(tab[j], m, 64);
    double u = 0.0, v = 0.0, sad = 0.0, sbc = 0.0;
    const int base = threadIdx.x & 48;                                 // lane 0 of this record within the wavefront
    for (int k = 0; k < S; k++) {                                      // stratum order; a stratum that contributes nothing adds +0.0
        u += __shfl(tu, base + k, 64); v += __shfl(tv, base + k, 64);
        sad += __shfl(tad, base + k, 64); sbc += __shfl(tbc, base + k, 64);
    }
    if (sub == 0) {
#pragma unroll
        for (int j = 0; j < 8; j++) counts[8 * g + j] = tab[j];
        if (tab[0] + tab[1] + tab[2] == 0 || tab[4] + tab[5] + tab[6] == 0) u = v = sad = sbc = __builtin_nan("");
        cmh[4 * g] = u; cmh[4 * g + 1] = v; cmh[4 * g + 2] = sad; cmh[4 * g + 3] = sbc;
    }
}

// ---- statistics: one lane per SNP ---------------------------------------------------------------------------------------------------
// entries < 2^31 (allelic) or < 2^30: a d, b c, r1 r2, c1 c2 < 2^62
__device__ __forceinline__ double cc_chi2_2x2(long long a, long long b, long long c, long long d)
{
    const long long r1 = a + b, r2 = c + d, c1 = a + c, c2 = b + d, T = r1 + r2;
    if (r1 == 0 || r2 == 0 || c1 == 0 || c2 == 0) return __builtin_nan("");
    const double D = (double)(a * d - b * c);
    return ((double)T * (D * D)) / ((double)(r1 * r2) * (double)(c1 * c2));
}

// the two directions of the hypergeometric recurrence from the mode; the products of two factors < 2^31 are exact in int64
template <class F> __device__ __forceinline__ void fisher_sweep(long long r1, long long c1, long long T, long long lo, long long hi, long long mode, F visit)
{
    const long long off = T - r1 - c1;                                 // d - a
    double P = 1.0;
    visit(mode, P);
    for (long long x = mode; x > lo; x--) {
        P = P * (double)(x * (off + x)) / (double)((r1 - x + 1) * (c1 - x + 1));
        visit(x - 1, P);
    }
    P = 1.0;
    for (long long x = mode; x < hi; x++) {
        P = P * (double)((r1 - x) * (c1 - x)) / (double)((x + 1) * (off + x + 1));
        visit(x + 1, P);
    }
}

__device__ __forceinline__ double cc_fisher(long long a, long long b, long long c, long long d)
{
    const long long r1 = a + b, c1 = a + c, T = a + b + c + d;
    const long long lo = r1 + c1 - T > 0 ? r1 + c1 - T : 0, hi = r1 < c1 ? r1 : c1;
    long long mode = (r1 + 1) * (c1 + 1) / (T + 2);                    // (r1 + 1)(c1 + 1) < 2^62
    mode = mode < lo ? lo : (mode > hi ? hi : mode);
    double sum = 0.0, Pobs = 0.0;
    fisher_sweep(r1, c1, T, lo, hi, mode, [&](long long x, double P) { sum += P; if (x == a) Pobs = P; });
    const double thr = Pobs * (1.0 + 0x1p-30);
    double tail = 0.0;
    fisher_sweep(r1, c1, T, lo, hi, mode, [&](long long x, double P) { if (P <= thr) tail += P; });
    const double pv = tail / sum;
    return pv > 1.0 ? 1.0 : pv;
}

__global__ __launch_bounds__(64) void cc_stats_kernel(long long p, const long long *counts, const double *cmh, int fisher, double *stat)
{
    const long long g = (long long)blockIdx.x * 64 + threadIdx.x;
    if (g >= p) return;
    const long long *t = counts + 8 * g;
    const long long r0 = t[0], r1 = t[1], r2 = t[2], s0 = t[4], s1 = t[5], s2 = t[6];
    const long long R = r0 + r1 + r2, Sp = s0 + s1 + s2, N = R + Sp;
    const double nan = __builtin_nan("");
    double *o = stat + PG_CC_NSTAT * g;
    bool ok = R > 0 && Sp > 0;
    for (int j = 0; j < 8; j++) ok = ok && t[j] >= 0 && t[j] < (1LL << 30);
    ok = ok && N < (1LL << 30);
    if (!ok) {
        for (int j = 0; j < PG_CC_NSTAT; j++) o[j] = nan;
        return;
    }
    const long long n0 = r0 + s0, n1 = r1 + s1, n2 = r2 + s2;
    const long long a = r1 + 2 * r2, b = 2 * R - a, c = s1 + 2 * s2, d = 2 * Sp - c, At = a + c;
    o[0] = (double)a / (double)(2 * R);
    o[1] = (double)c / (double)(2 * Sp);
    o[2] = (double)(a * d) / (double)(b * c);                          // x / 0 = +inf, 0 / 0 = NaN
    o[3] = cc_chi2_2x2(a, b, c, d);
    // trend: N A_case, R A_tot < 2^30 2^31; N (n1 + 4 n2) <= 4 N^2 < 2^62 and A_tot^2 < 2^62, their difference N sum w^2 n - (sum w n)^2 >= 0
    const long long Ui = N * a - R * At, Vi = N * (n1 + 4 * n2) - At * At;
    if (Vi == 0) o[4] = nan;
    else {
        const double U = (double)Ui;
        o[4] = ((double)N * (U * U)) / ((double)(R * Sp) * (double)Vi);                          // R S' < 2^60
    }
    // genotypic: r_i N, R n_i < 2^60
    if (n0 == 0 || n1 == 0 || n2 == 0) o[5] = nan;
    else {
        const double RS = (double)(R * Sp);
        const double d0 = (double)(r0 * N - R * n0), d1 = (double)(r1 * N - R * n1), d2 = (double)(r2 * N - R * n2);
        const double t0 = (d0 * d0) / (RS * (double)n0), t1 = (d1 * d1) / (RS * (double)n1), t2 = (d2 * d2) / (RS * (double)n2);
        o[5] = t0 + t1 + t2;
    }
    o[6] = cc_chi2_2x2(r1 + r2, r0, s1 + s2, s0);
    o[7] = cc_chi2_2x2(r2, r0 + r1, s2, s0 + s1);
    o[8] = fisher ? cc_fisher(a, b, c, d) : nan;
    if (cmh) {
        const double u = cmh[4 * g], v = cmh[4 * g + 1], sad = cmh[4 * g + 2], sbc = cmh[4 * g + 3];
        o[9] = v == 0.0 ? nan : (u * u) / v;
        o[10] = sbc == 0.0 ? nan : sad / sbc;
    } else {
        o[9] = nan; o[10] = nan;
    }
}

}  // namespace pg

using namespace pg;

extern "C" size_t pg_cc_work_bytes(int64_t n, int S)
{
    if (n < 1 || n >= (1LL << 30) || S < 1 || S > CC_MAXS) return 0;
    return CC_HEAD + (size_t)2 * S * (size_t)cc_words(n) * 4;
}

extern "C" int pg_cc_setup_dev(pg_ctx *ctx, int64_t n, int S, const signed char *status, const int *stratum, void *work)
{
    PG_REQUIRE(ctx && status && work, "pg_cc_setup_dev: NULL argument");
    PG_REQUIRE(n >= 1 && n < (1LL << 30) && (uintptr_t)work % 16 == 0, "pg_cc_setup_dev: bad shape n=%lld, or work off 16 bytes", (long long)n);
    if (S < 1 || S > CC_MAXS) {
        set_error("pg_cc_setup_dev: S=%d strata outside 1..%d", S, CC_MAXS);
        return PG_ENOTSUP;
    }
    PG_HIP(hipSetDevice(ctx->device));
    const long long W = cc_words(n), total = 2 * S * W;                // < 2^5 2^26
    int *sizes = static_cast<int *>(work);
    unsigned *masks = reinterpret_cast<unsigned *>(static_cast<char *>(work) + CC_HEAD);
    cc_mask_kernel<<<(unsigned)((total + 255) / 256), 256, 0, ctx->stream>>>((int)n, S, W, status, stratum, masks);
    PG_HIP(hipGetLastError());
    cc_size_kernel<<<2 * S, 64, 0, ctx->stream>>>(W, masks, sizes);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

extern "C" int pg_cc_pack_x_dev(pg_ctx *ctx, int64_t n, int64_t pb, const void *X, int dtype, int64_t ldX, int snp_major, unsigned char *rec, int64_t ldb,
                                unsigned char *hard)
{
    PG_REQUIRE(ctx && X && rec && hard, "pg_cc_pack_x_dev: NULL argument");
    PG_REQUIRE(n >= 1 && n < (1LL << 30) && pb >= 0 && pb <= CC_MAXPB && ldX >= (snp_major ? n : pb) && ldb >= (n + 3) / 4,
               "pg_cc_pack_x_dev: bad shape n=%lld pb=%lld ldX=%lld snp_major=%d ldb=%lld", (long long)n, (long long)pb, (long long)ldX, snp_major,
               (long long)ldb);
    if (!dtype_known(dtype)) {
        set_error("pg_cc_pack_x_dev: unknown dtype %d", dtype);
        return PG_ENOTSUP;
    }
    if (!snp_major) {
        const long long E = dtype == PG_DTYPE_FLOAT64 ? 2 : 4;                  // cc_sm_e
        const long long R = (n + CC_ROWS - 1) / CC_ROWS, ncb = (pb + 64 * E - 1) / (64 * E);
        PG_REQUIRE(R * ncb < CC_MAXGRID, "pg_cc_pack_x_dev: a sample-major block of n=%lld x pb=%lld is more than one launch holds (%lld workgroups)",
                   (long long)n, (long long)pb, CC_MAXGRID);
    }
    if (pb == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    PG_HIP(hipMemsetAsync(hard, 1, (size_t)pb, ctx->stream));           // the kernels only ever store 0
    return geno_dispatch(dtype, snp_major != 0, [&](auto src) {
        using Sr = decltype(src);
        return launch_cc_pack<typename Sr::type, Sr::layout>(ctx, (int)n, pb, X, ldX, rec, ldb, hard);
    });
}

extern "C" int pg_cc_count_dev(pg_ctx *ctx, int64_t n, int64_t pb, const unsigned char *rec, int64_t ldb, int count_a1, int S, const void *work,
                               const unsigned char *hard, int64_t *counts, double *cmh)
{
    PG_REQUIRE(ctx && rec && work && counts && cmh, "pg_cc_count_dev: NULL argument");
    PG_REQUIRE(n >= 1 && n < (1LL << 30) && pb >= 0 && pb <= CC_MAXPB && ldb >= (n + 3) / 4 && (uintptr_t)work % 16 == 0,
               "pg_cc_count_dev: bad shape n=%lld pb=%lld ldb=%lld, or work off 16 bytes", (long long)n, (long long)pb, (long long)ldb);
    if (S < 1 || S > CC_MAXS) {
        set_error("pg_cc_count_dev: S=%d strata outside 1..%d", S, CC_MAXS);
        return PG_ENOTSUP;
    }
    if (pb == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    const bool vec4 = ((uintptr_t)rec % 4 == 0) && ldb % 4 == 0, vec16 = ((uintptr_t)rec % 16 == 0) && ldb % 16 == 0;
    const int *sizes = static_cast<const int *>(work);
    const unsigned *masks = reinterpret_cast<const unsigned *>(static_cast<const char *>(work) + CC_HEAD);
    const long long W = cc_words(n);
    long long *cnt = reinterpret_cast<long long *>(counts);
    const unsigned grid = (unsigned)((pb + 15) / 16);
    static_assert(CC_MAXPB / 16 + 1 < CC_MAXGRID, "16 records per workgroup");
#define CC_LAUNCH(SB) cc_count_kernel<SB><<<grid, 256, 0, ctx->stream>>>((int)n, pb, rec, ldb, count_a1 != 0, S, vec16, vec4, sizes, masks, W, hard, cnt, cmh)
    if (S <= 1) CC_LAUNCH(1);
    else if (S <= 2) CC_LAUNCH(2);
    else if (S <= 4) CC_LAUNCH(4);
    else if (S <= 8) CC_LAUNCH(8);
    else CC_LAUNCH(16);
#undef CC_LAUNCH
    PG_HIP(hipGetLastError());
    return PG_OK;
}

extern "C" int pg_cc_stats_dev(pg_ctx *ctx, int64_t p, const int64_t *counts, const double *cmh, int fisher, double *stat)
{
    PG_REQUIRE(ctx && counts && stat, "pg_cc_stats_dev: NULL argument");
    PG_REQUIRE(p >= 0 && p < (1LL << 31), "pg_cc_stats_dev: bad shape p=%lld", (long long)p);
    if (p == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    cc_stats_kernel<<<(unsigned)((p + 63) / 64), 64, 0, ctx->stream>>>(p, reinterpret_cast<const long long *>(counts), cmh, fisher, stat);
    PG_HIP(hipGetLastError());
    return PG_OK;
}
