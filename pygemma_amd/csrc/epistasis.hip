// epistasis.hip — pairwise SNP x SNP interaction on the int8 matrix pipe: the allele-table odds-ratio test of PLINK's --fast-epistasis
// (case/control, or case-only) over every pair of two windows of SNPs, reduced on the device to the pairs above a chi2 cut and a
// per-SNP summary.
//
// Definition.  Samples carry a group g: 1 case, 0 control, anything else in neither.  With x, m of a SNP as ld.hip defines
// them, a pair (a, b) has per group G the four int32 sums over the samples of G
//     N = sum m_a m_b   Sa = sum x_a m_b   Sb = sum m_a x_b   Sab = sum x_a x_b
// and, exactly in int64, the allele table A = 4 N - 2 Sa - 2 Sb + Sab, B = 2 Sb - Sab, C = 2 Sa - Sab, D = Sab.  A group is defined when
// A + B, C + D, A + C and B + D are positive.  The doubled cells are t = 2 cell + z, z = 1 when one of the four cells is 0 (that is 1/2
// added to every cell), and in fp64, one rounding per operation,
//     L = log((tA tD) / (tB tC))      v = (2 / tA + 2 / tD) + (2 / tB + 2 / tC)
// case/control: z = (L1 - L0) / sqrt(v1 + v0), defined when both groups are; case-only: z = L1 / sqrt(v1).  chi2 = z z.  The pairing of
// the terms makes z(a, b) and z(b, a) the same bits.
//
// The epistasis image (opaque; pg_epi_image_bytes): six SNP-major int8 planes with the LD image's row pitch, zero past sample n,
//     0: x [g = 1]   1: x [g = 0]   2: m [g = 1]   3: m [g = 0]   4: x [g >= 0]   5: m [g >= 0]      ([g >= 0]: case or control)
// then one int4 per SNP {sum x in cases, sum x in controls, called cases, called controls}, one int per SNP "a missing call among the
// cases and controls", and the two group sizes.  pg_epi_split_dev derives it from an LD image, so every encoder of ld.hip serves it.
//
// The pair kernel runs the tile of i8_pair.hpp with "planes as output rows".  A workgroup owns 128 SNPs of A against 256 SNPs of B.
// When no SNP of either side holds a missing call among the cases and controls it takes ONE product: each 128-row half of A is 64 SNPs x
// {plane 0, plane 1}, the 256 rows of B are plane 4 of 256 SNPs; the product is Sab of both groups, N is the group's size and Sa, Sb are
// the per-SNP totals.  Otherwise it walks the 2 x 2 pairs of sub-tiles of 64 x 128 SNPs: each half of A is 32 SNPs x {planes 0..3},
// B is 128 SNPs x {plane 4, plane 5}, and the eight products of a pair are its eight sums: no output row is wasted.  Both paths give the
// same integers.  PG_EPI_PLANES=1 sends every tile pair down the second path (tests, A/B timing).
#include "geno_src.hpp"
#include "i8_pair.hpp"
#include "ld_layout.hpp"

#include <cmath>

namespace pg {

constexpr int EPI_TA = 128, EPI_TB = 256;         // SNPs of A and of B per workgroup
constexpr long long EPI_MAXN = 1LL << 28;         // exclusive, as LD: every sum fits int32
constexpr long long EPI_MAXPE = 1LL << 31;

struct EpiLayout {
    long long ldk;
    size_t plane, totals, flags, header, total;
};
static EpiLayout epi_layout(long long n, long long pe)
{
    EpiLayout L;
    L.ldk = (n + LD_BK - 1) / LD_BK * LD_BK;
    L.plane = (size_t)pe * L.ldk;
    L.totals = up256(6 * L.plane);
    L.flags = L.totals + up256((size_t)pe * 16);
    L.header = L.flags + up256((size_t)pe * 4);
    L.total = L.header + 256;
    return L;
}

// ---- split: an LD image's x and m planes and the group vector -> the six planes and the per-SNP totals -------------------------------------
struct EpiSplit {
    int n;
    long long ldk, from;
    size_t ld_plane, plane;
    const signed char *ld;
    const signed char *group;
    signed char *img;
    int4 *tot;
    int *flag, *header;
};

__device__ __forceinline__ int epi_bytes(unsigned v) { return (int)((v & 0xff) + ((v >> 8) & 0xff) + ((v >> 16) & 0xff) + (v >> 24)); }

// One workgroup per SNP, a lane per 16 samples: two 16-byte loads, six 16-byte stores.  Bandwidth-bound: 2 n bytes in, 6 n out.
__global__ __launch_bounds__(256) void epi_split_kernel(EpiSplit q)
{
    __shared__ int red[4][6];
    const long long g = q.from + blockIdx.x;
    const signed char *xr = q.ld + (size_t)g * q.ldk, *mr = xr + q.ld_plane;
    signed char *out = q.img + (size_t)g * q.ldk;
    int s[6] = {0, 0, 0, 0, 0, 0};      // sum x cases, sum x controls, called cases, called controls, cases, controls
    for (long long o = 16LL * threadIdx.x; o < q.ldk; o += 16 * 256) {
        const uint4 xv = *reinterpret_cast<const uint4 *>(xr + o), mv = *reinterpret_cast<const uint4 *>(mr + o);
        const unsigned xw[4] = {xv.x, xv.y, xv.z, xv.w}, mw[4] = {mv.x, mv.y, mv.z, mv.w};
        unsigned o0[4], o1[4], o2[4], o3[4], o4[4], o5[4];
#pragma unroll
        for (int w = 0; w < 4; w++) {
            unsigned k1 = 0, k0 = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const long long i = o + 4 * w + b;
                const int gi = i < q.n ? (int)q.group[i] : -1;
                k1 |= (gi == 1 ? 0xffu : 0u) << (8 * b);
                k0 |= (gi == 0 ? 0xffu : 0u) << (8 * b);
            }
            o0[w] = xw[w] & k1; o1[w] = xw[w] & k0; o2[w] = mw[w] & k1; o3[w] = mw[w] & k0;
            o4[w] = xw[w] & (k1 | k0); o5[w] = mw[w] & (k1 | k0);
            s[0] += epi_bytes(o0[w]); s[1] += epi_bytes(o1[w]); s[2] += epi_bytes(o2[w]); s[3] += epi_bytes(o3[w]);
            s[4] += __popc(k1) >> 3; s[5] += __popc(k0) >> 3;
        }
        *reinterpret_cast<uint4 *>(out + o) = make_uint4(o0[0], o0[1], o0[2], o0[3]);
        *reinterpret_cast<uint4 *>(out + q.plane + o) = make_uint4(o1[0], o1[1], o1[2], o1[3]);
        *reinterpret_cast<uint4 *>(out + 2 * q.plane + o) = make_uint4(o2[0], o2[1], o2[2], o2[3]);
        *reinterpret_cast<uint4 *>(out + 3 * q.plane + o) = make_uint4(o3[0], o3[1], o3[2], o3[3]);
        *reinterpret_cast<uint4 *>(out + 4 * q.plane + o) = make_uint4(o4[0], o4[1], o4[2], o4[3]);
        *reinterpret_cast<uint4 *>(out + 5 * q.plane + o) = make_uint4(o5[0], o5[1], o5[2], o5[3]);
    }
#pragma unroll
    for (int t = 0; t < 6; t++)
        for (int k = 1; k < 64; k <<= 1) s[t] += __shfl_xor(s[t], k, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int t = 0; t < 6; t++) red[threadIdx.x >> 6][t] = s[t];
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int t = 0; t < 6; t++) s[t] = red[0][t] + red[1][t] + red[2][t] + red[3][t];
        q.tot[g] = make_int4(s[0], s[1], s[2], s[3]);
        q.flag[g] = (s[2] != s[4] || s[3] != s[5]) ? 1 : 0;
        q.header[0] = s[4]; q.header[1] = s[5];      // every SNP of an image is split with the same group vector: the same two numbers
    }
}

// ---- the pair kernel --------------------------------------------------------------------------------------------------------------------
struct EpiPair {
    int n, KT, planes, tiles_b, upper, mode;
    long long ldk;
    const signed char *A, *B;         // plane 0; plane k lies k * pea (peb) * ldk bytes further
    long long pea, peb;
    const int4 *ta, *tb;
    const int *fa, *fb, *header;
    long long a0, na, b0, nb;         // SNPs [a0, a0 + na) of A against [b0, b0 + nb) of B
    long long ga0, gb0;               // the global index of SNP a0 of A, b0 of B: what the records and the per-SNP arrays are indexed by
    double chi2_min;
    unsigned long long *count;
    int4 *hits;
    long long cap;
    int *ntot, *nsig;
    unsigned long long *best;
    int *sums;
};

// the accumulators of a workgroup's tile pair, behind the pair tile's LDS: per side (0: the 256 columns, the B SNPs; 1: the 128 rows,
// the A SNPs) 256 64-bit maxima, 256 pair counts, 256 hit counts
constexpr int EPI_LDS = I8P_LDS + 2 * 256 * 16;
__device__ __forceinline__ unsigned long long *epi_acc_best(int side) { return reinterpret_cast<unsigned long long *>(i8p_lds + I8P_LDS + side * 256 * 16); }
__device__ __forceinline__ int *epi_acc_tot(int side) { return reinterpret_cast<int *>(i8p_lds + I8P_LDS + side * 256 * 16 + 256 * 8); }
__device__ __forceinline__ int *epi_acc_sig(int side) { return reinterpret_cast<int *>(i8p_lds + I8P_LDS + side * 256 * 16 + 256 * 12); }

// L and v of one group from its four sums; false: the group is not defined for the pair
__device__ __forceinline__ bool epi_terms(long long N, long long Sa, long long Sb, long long Sab, double &L, double &v)
{
    const long long A = 4 * N - 2 * Sa - 2 * Sb + Sab, B = 2 * Sb - Sab, C = 2 * Sa - Sab, D = Sab;
    if (A + B <= 0 || C + D <= 0 || A + C <= 0 || B + D <= 0) return false;
    const long long z = (A == 0 || B == 0 || C == 0 || D == 0) ? 1 : 0;
    const double tA = (double)(2 * A + z), tB = (double)(2 * B + z), tC = (double)(2 * C + z), tD = (double)(2 * D + z);
    L = log((tA * tD) / (tB * tC));
    v = (2.0 / tA + 2.0 / tD) + (2.0 / tB + 2.0 / tC);
    return true;
}

// One staged half: HA SNPs of A (rows) x TB SNPs of B (columns).  A wavefront walks rows wave, wave + 8, ...; its lanes the columns
// lane, lane + 64, ...  The sums of a row meet in a reduction over the lanes and go to the row accumulators; the columns' go there as LDS
// atomics.  as0, bs0: the first SNPs of the (sub-)tiles; abase, bbase: of the workgroup's tiles.
template <bool PLANES> __device__ __forceinline__ void epi_half(const EpiPair &q, const I8pLane ln, int half, long long as0, long long bs0,
                                                                long long abase, long long bbase, long long aend, long long bend, int n1, int n0)
{
    constexpr int HA = PLANES ? 32 : 64, TB = PLANES ? 128 : 256;
    const int *const stg = i8p_staged();
#pragma unroll 1
    for (int sa = ln.wave; sa < HA; sa += 8) {
        const long long ja = as0 + half * HA + sa;
        if (ja >= aend) break;
        const long long ga = q.ga0 + (ja - q.a0);
        int4 a = make_int4(0, 0, 0, 0);
        if (!PLANES) a = q.ta[ja];
        int rtot = 0, rsig = 0;
        unsigned long long rbest = 0;
#pragma unroll 1
        for (int sb = ln.lane; sb < TB; sb += 64) {
            const long long jb = bs0 + sb, gb = q.gb0 + (jb - q.b0);
            const bool visit = jb < bend && (!q.upper || ga < gb);
            bool hit = false;
            double z = 0.0;
            if (visit) {
                long long N1, Sa1, Sb1, Sab1, N0, Sa0, Sb0, Sab0;
                if (PLANES) {      // rows [32 k, 32 k + 32): plane k of A; columns [0, 128): plane 4 of B (x), [128, 256): plane 5 (m)
                    const int *s = stg + sa * I8P_LDW + sb;
                    Sab1 = s[0];                  Sa1 = s[128];
                    Sab0 = s[32 * I8P_LDW];       Sa0 = s[32 * I8P_LDW + 128];
                    Sb1 = s[64 * I8P_LDW];        N1 = s[64 * I8P_LDW + 128];
                    Sb0 = s[96 * I8P_LDW];        N0 = s[96 * I8P_LDW + 128];
                } else {           // rows [0, 64): plane 0 of A, [64, 128): plane 1
                    const int4 b = q.tb[jb];
                    N1 = n1; Sa1 = a.x; Sb1 = b.x; Sab1 = stg[sa * I8P_LDW + sb];
                    N0 = n0; Sa0 = a.y; Sb0 = b.y; Sab0 = stg[(64 + sa) * I8P_LDW + sb];
                }
                if (q.sums) {
                    int *o = q.sums + ((size_t)(ja - q.a0) * q.nb + (jb - q.b0)) * 8;
                    o[0] = (int)N1; o[1] = (int)Sa1; o[2] = (int)Sb1; o[3] = (int)Sab1;
                    o[4] = (int)N0; o[5] = (int)Sa0; o[6] = (int)Sb0; o[7] = (int)Sab0;
                }
                double L1 = 0.0, v1 = 0.0, L0 = 0.0, v0 = 0.0;
                bool def = epi_terms(N1, Sa1, Sb1, Sab1, L1, v1);
                if (def && q.mode == 0) def = epi_terms(N0, Sa0, Sb0, Sab0, L0, v0);
                if (def) {
                    z = q.mode == 0 ? (L1 - L0) / __dsqrt_rn(v1 + v0) : L1 / __dsqrt_rn(v1);
                    const double chi2 = z * z;
                    hit = chi2 >= q.chi2_min;
                    const unsigned long long key = (unsigned long long)__float_as_uint((float)chi2) << 32;
                    const unsigned long long ka = key | (unsigned)~(unsigned)gb, kb = key | (unsigned)~(unsigned)ga;
                    rtot += 1; rsig += hit ? 1 : 0; rbest = ka > rbest ? ka : rbest;
                    const int col = (int)(jb - bbase);
                    atomicAdd(epi_acc_tot(0) + col, 1);
                    if (hit) atomicAdd(epi_acc_sig(0) + col, 1);
                    atomicMax(epi_acc_best(0) + col, kb);
                }
            }
            // the hits of a wavefront take their slots with one atomic
            const unsigned long long mask = __ballot(hit);
            if (mask) {
                unsigned long long base = 0;
                const int leader = __ffsll((long long)mask) - 1;
                if (ln.lane == leader) base = atomicAdd(q.count, (unsigned long long)__popcll(mask));
                base = __shfl(base, leader, 64);
                if (hit) {
                    const unsigned long long slot = base + __popcll(mask & ((1ULL << ln.lane) - 1));
                    if (slot < (unsigned long long)q.cap) {
                        const long long zb = __double_as_longlong(z);
                        q.hits[slot] = make_int4((int)ga, (int)gb, (int)(zb & 0xffffffffLL), (int)(zb >> 32));
                    }
                }
            }
        }
        for (int k = 1; k < 64; k <<= 1) {
            rtot += __shfl_xor(rtot, k, 64); rsig += __shfl_xor(rsig, k, 64);
            const unsigned long long o = __shfl_xor(rbest, k, 64);
            rbest = o > rbest ? o : rbest;
        }
        if (ln.lane == 0 && rtot) {
            const int row = (int)(ja - abase);
            atomicAdd(epi_acc_tot(1) + row, rtot);
            atomicAdd(epi_acc_sig(1) + row, rsig);
            atomicMax(epi_acc_best(1) + row, rbest);
        }
    }
}

__global__ __launch_bounds__(512, 1) void epi_pair_kernel(EpiPair q)
{
    const int tid = threadIdx.x;
    const I8pLane ln = i8p_lane();
    // Workgroups go to the eight XCDs round-robin by their index.  With tile_b = index % tiles_b an XCD would own fixed columns of the
    // tile grid, and under `upper` the ones left of the diagonal return at once: the XCDs with the right-hand columns had half as much
    // again to do (8192 x 8192, upper: 3.03 ms against 3.91 ms dense for 54 % of its tiles).  Rotating each row by its number spreads
    // every column over all of them.
    const long long tile_a = blockIdx.x / q.tiles_b, tile_b = (blockIdx.x % q.tiles_b + tile_a) % q.tiles_b;
    const long long abase = q.a0 + tile_a * EPI_TA, bbase = q.b0 + tile_b * EPI_TB;
    const long long aend = q.a0 + q.na, bend = q.b0 + q.nb;      // one past the last SNP of either window
    // upper triangle: a tile pair whose smallest a is not below its largest b holds no pair to visit
    if (q.upper && q.ga0 + (abase - q.a0) >= q.gb0 + (min(bbase + EPI_TB, bend) - 1 - q.b0)) return;
    int miss = q.planes;
    for (int k = tid; k < EPI_TA + EPI_TB; k += 512) {
        const bool sideb = k >= EPI_TA;
        const long long g = sideb ? bbase + (k - EPI_TA) : abase + k;
        if (g < (sideb ? bend : aend)) miss |= (sideb ? q.fb : q.fa)[g];
    }
    const bool planes = __syncthreads_or(miss) != 0;
    const int n1 = q.header[0], n0 = q.header[1];
    epi_acc_best(tid >> 8)[tid & 255] = 0;      // ordered before the first add by the barriers of the first products
    epi_acc_tot(tid >> 8)[tid & 255] = 0;
    epi_acc_sig(tid >> 8)[tid & 255] = 0;
    const int nsub = planes ? 2 : 1, TA = planes ? 64 : EPI_TA, TB = planes ? 128 : EPI_TB;

#pragma unroll 1
    for (int sub = 0; sub < nsub * nsub; sub++) {
        const long long as0 = abase + (sub / nsub) * TA, bs0 = bbase + (sub % nsub) * TB;
        if (as0 >= aend || bs0 >= bend) continue;
        if (q.upper && q.ga0 + (as0 - q.a0) >= q.gb0 + (min(bs0 + TB, bend) - 1 - q.b0)) continue;
        intx4 acc[4][8];
        i8p_zero(acc);
        // DMA sources.  Rows of SNPs past a window repeat the window's last SNP: their products are never read.
        const signed char *srcA[4], *srcB[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int row = i8p_src_row(ln, t), h = row >> 7, rr = row & 127;
            const int pla = planes ? rr >> 5 : rr >> 6, sna = planes ? h * 32 + (rr & 31) : h * 64 + (rr & 63);
            const int plb = planes ? 4 + h : 4, snb = planes ? rr : row;
            const long long ga = min(as0 + sna, aend - 1), gb = min(bs0 + snb, bend - 1);
            srcA[t] = q.A + ((size_t)pla * q.pea + ga) * q.ldk + i8p_src_byte(ln, row);
            srcB[t] = q.B + ((size_t)plb * q.peb + gb) * q.ldk + i8p_src_byte(ln, row);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the stores of the previous epilogue are not counted against the loads below
        i8p_products(ln, srcA, srcB, q.KT, acc);
#pragma unroll 1
        for (int half = 0; half < 2; half++) {
            i8p_stage(ln, half, acc);
            if (planes) epi_half<true>(q, ln, half, as0, bs0, abase, bbase, aend, bend, n1, n0);
            else epi_half<false>(q, ln, half, as0, bs0, abase, bbase, aend, bend, n1, n0);
            __syncthreads();
        }
    }
    __syncthreads();
    // the accumulators go out: threads [0, 256) the columns from bbase, threads [256, 512) the rows from abase, one atomic per array
    // and SNP with a defined pair
    const int side = tid >> 8, t = tid & 255;
    const int c = epi_acc_tot(side)[t];
    if (c) {
        const long long g = side ? q.ga0 + (abase - q.a0) + t : q.gb0 + (bbase - q.b0) + t;
        const int sg = epi_acc_sig(side)[t];
        if (q.ntot) atomicAdd(q.ntot + g, c);
        if (q.nsig && sg) atomicAdd(q.nsig + g, sg);
        if (q.best) atomicMax(q.best + g, epi_acc_best(side)[t]);
    }
}

static bool epi_shape_ok(int64_t n, int64_t pe) { return n >= 1 && n < EPI_MAXN && pe >= 1 && pe < EPI_MAXPE; }
static bool epi_aligned(const void *p, int to) { return (uintptr_t)p % to == 0; }

}  // namespace pg

using namespace pg;

extern "C" size_t pg_epi_image_bytes(int64_t n, int64_t pe)
{
    if (!epi_shape_ok(n, pe)) return 0;
    return epi_layout(n, pe).total;
}

extern "C" int pg_epi_split_dev(pg_ctx *ctx, int64_t n, const void *ld_image, int64_t pe, int64_t from, int64_t count, const signed char *group,
                                void *epi_image)
{
    PG_REQUIRE(ctx && ld_image && group && epi_image, "pg_epi_split_dev: NULL argument");
    PG_REQUIRE(epi_aligned(ld_image, 16) && epi_aligned(epi_image, 16), "pg_epi_split_dev: the images must lie on 16 bytes");
    PG_REQUIRE(epi_shape_ok(n, pe) && from >= 0 && count >= 0 && from + count <= pe, "pg_epi_split_dev: bad shape n=%lld pe=%lld from=%lld count=%lld",
               (long long)n, (long long)pe, (long long)from, (long long)count);
    if (count == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    const LdLayout Ld = ld_layout(n, pe);
    const EpiLayout L = epi_layout(n, pe);
    EpiSplit q;
    q.n = (int)n; q.ldk = L.ldk; q.from = from; q.ld_plane = Ld.plane; q.plane = L.plane;
    q.ld = static_cast<const signed char *>(ld_image); q.group = group;
    q.img = static_cast<signed char *>(epi_image);
    q.tot = reinterpret_cast<int4 *>(q.img + L.totals);
    q.flag = reinterpret_cast<int *>(q.img + L.flags);
    q.header = reinterpret_cast<int *>(q.img + L.header);
    epi_split_kernel<<<(unsigned)count, 256, 0, ctx->stream>>>(q);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

extern "C" int pg_epi_block_dev(pg_ctx *ctx, int64_t n, const void *A, int64_t pea, int64_t a0, int64_t na, int64_t ga0, const void *B, int64_t peb,
                                int64_t b0, int64_t nb, int64_t gb0, int mode, int upper, double chi2_min, uint64_t *count, void *hits, int64_t cap,
                                int32_t *n_tot, int32_t *n_sig, uint64_t *best, int32_t *sums)
{
    PG_REQUIRE(ctx && A && B && count && (hits || cap == 0), "pg_epi_block_dev: NULL argument");
    PG_REQUIRE(cap >= 0, "pg_epi_block_dev: cap=%lld is negative", (long long)cap);
    PG_REQUIRE(std::isfinite(chi2_min) && chi2_min >= 0.0, "pg_epi_block_dev: chi2_min=%g is not a finite number >= 0", chi2_min);
    if (mode != PG_EPI_CASE_CONTROL && mode != PG_EPI_CASE_ONLY) {
        set_error("pg_epi_block_dev: unknown mode %d", mode);
        return PG_ENOTSUP;
    }
    PG_REQUIRE(epi_aligned(A, 16) && epi_aligned(B, 16) && epi_aligned(hits, 16) && epi_aligned(count, 8) && epi_aligned(best, 8),
               "pg_epi_block_dev: the images and hits must lie on 16 bytes, count and best on 8");
    PG_REQUIRE(epi_shape_ok(n, pea) && epi_shape_ok(n, peb) && a0 >= 0 && na >= 0 && a0 + na <= pea && b0 >= 0 && nb >= 0 && b0 + nb <= peb && ga0 >= 0 &&
                   gb0 >= 0 && ga0 + na < EPI_MAXPE && gb0 + nb < EPI_MAXPE,
               "pg_epi_block_dev: bad shape n=%lld A [%lld, +%lld) of %lld at %lld, B [%lld, +%lld) of %lld at %lld", (long long)n, (long long)a0,
               (long long)na, (long long)pea, (long long)ga0, (long long)b0, (long long)nb, (long long)peb, (long long)gb0);
    if (na == 0 || nb == 0) return PG_OK;
    const long long tiles_a = (na + EPI_TA - 1) / EPI_TA, tiles_b = (nb + EPI_TB - 1) / EPI_TB;
    PG_REQUIRE(tiles_a * tiles_b < (1LL << 31), "pg_epi_block_dev: too many tiles (%lld x %lld)", tiles_a, tiles_b);
    PG_HIP(hipSetDevice(ctx->device));
    const EpiLayout La = epi_layout(n, pea), Lb = epi_layout(n, peb);
    const char *a = static_cast<const char *>(A), *b = static_cast<const char *>(B);
    EpiPair q;
    q.n = (int)n; q.ldk = La.ldk; q.KT = (int)(La.ldk / LD_BK); q.planes = env_flag("PG_EPI_PLANES"); q.tiles_b = (int)tiles_b;
    q.upper = upper != 0; q.mode = mode;
    q.A = reinterpret_cast<const signed char *>(a); q.pea = pea; q.ta = reinterpret_cast<const int4 *>(a + La.totals);
    q.fa = reinterpret_cast<const int *>(a + La.flags); q.header = reinterpret_cast<const int *>(a + La.header);
    q.B = reinterpret_cast<const signed char *>(b); q.peb = peb; q.tb = reinterpret_cast<const int4 *>(b + Lb.totals);
    q.fb = reinterpret_cast<const int *>(b + Lb.flags);
    q.a0 = a0; q.na = na; q.b0 = b0; q.nb = nb; q.ga0 = ga0; q.gb0 = gb0;
    q.chi2_min = chi2_min; q.count = reinterpret_cast<unsigned long long *>(count); q.hits = static_cast<int4 *>(hits); q.cap = cap;
    q.ntot = n_tot; q.nsig = n_sig; q.best = reinterpret_cast<unsigned long long *>(best); q.sums = sums;
    PG_HIP((i8p_lds_limit<epi_pair_kernel, EPI_LDS>(ctx->device)));
    epi_pair_kernel<<<(unsigned)(tiles_a * tiles_b), 512, EPI_LDS, ctx->stream>>>(q);
    PG_HIP(hipGetLastError());
    return PG_OK;
}
