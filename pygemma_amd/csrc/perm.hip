// perm.hip — max(T) permutation tests of a case/control trait on the int8 matrix pipe (PLINK's --assoc --mperm B and --model trend
// --mperm B): the statistic of every SNP under B labellings at once, reduced on the device to 8 bytes per SNP and 8 per labelling.
//
// Definition.  Samples carry a study flag s in {0, 1}; a sample with no status or no stratum has s = 0.  A labelling l_b is
// a 0/1 vector with l_b <= s: the samples it calls cases.  For a hard-call SNP, with x, m as ld.hip defines them, the per-SNP totals
// over the study samples are
//     At = sum x s      Nc = sum m s      Q = sum x^2 s  (= n1 + 4 n2)
// with a flag "a study sample is uncalled", and per labelling
//     a = sum x l_b     R = sum m l_b
// The sums are int32; everything derived from them is exact in int64.
//
// Operation order (fp64, -ffp-contract=off; (double)(...) is the one conversion of an exact int64, * and / round once each), that of
// case_control.hip:
//   allelic: the 2 x 2 table a, b = 2 R - a / c = At - a, d = 2 (Nc - R) - c with margins r1 = a + b, r2 = c + d, c1 = a + c,
//            c2 = b + d, T = r1 + r2:
//       chi2 = ((double)T * (D * D)) / ((double)(r1 r2) * (double)(c1 c2)),  D = (double)(a d - b c);  NaN when a margin is 0
//   trend:   N = Nc, S' = Nc - R, U = (double)(N a - R At), V = (double)(N Q - At^2):
//       chi2 = ((double)N * (U * U)) / ((double)(R S') * V);  NaN when V = 0
//   Both are NaN when R = 0 or R = Nc.
// With l_b the observed status the result is pg_cc_stats_dev's chi2_allelic / chi2_trend, bit for bit: a permuted statistic equals the
// observed one exactly when the tables are equal, so `>=` counts ties as PLINK defines them.
// Integer ranges: n < 2^28, so Nc, R < 2^28, a, At < 2^29, Q < 2^30, the margins of the allelic table < 2^30 and every product of two of
// these < 2^60: each cross-difference above is exact in int64.
//
// Label rows: int8 0/1 at pitch ldk = n rounded up to the K-tile of 128 samples, zero past sample n and where s = 0; the study flags are
// one such row.
//
// The block kernel runs the tile of i8_pair.hpp with "planes as output rows", SNPs as A rows and labellings as B rows.  A workgroup owns
// 256 SNPs against 256 labellings.  When no SNP of the tile has a flag it takes ONE product: the 256 rows of A are plane x of 256 SNPs,
// the product is a, and R is the labelling's case count (every study sample is called).  Otherwise it walks two sub-tiles of 128 SNPs:
// each 128-row half of A is 64 SNPs x {x, m}, and the two products of a SNP are a and R.  Both paths give the same integers.
// PG_PERM_PLANES=1 sends every tile down the second path (tests, A/B timing).
// The epilogue works on the halves i8p_stage releases: a wavefront walks rows (SNPs) wave, wave + 8, ..., its lanes the columns
// (labellings) lane, lane + 64, lane + 128, lane + 192 — the same four for every row, so a lane keeps their maxima in registers.  The
// count of a row meets in a reduction over the lanes (a row belongs to one wavefront, once), the maxima of a column in an LDS integer
// atomic max per lane at the end; then one global integer atomic per SNP and per labelling.
#include "i8_pair.hpp"
#include "ld_layout.hpp"
#include "../../include/pygemma_perm.h"

namespace pg {

constexpr int PERM_T = 256;                       // SNPs and labellings per workgroup
constexpr long long PERM_MAXN = 1LL << 28;        // exclusive, as LD: every sum fits int32
constexpr long long PERM_MAXPE = 1LL << 31;

// ---- the case count of every labelling: one wavefront per row ---------------------------------------------------------------------------
__device__ __forceinline__ int perm_bytes(unsigned v) { return (int)((v & 0xff) + ((v >> 8) & 0xff) + ((v >> 16) & 0xff) + (v >> 24)); }

__global__ __launch_bounds__(64) void perm_label_count_kernel(long long ldk, const signed char *labels, int *counts)
{
    const signed char *row = labels + (size_t)blockIdx.x * ldk;
    int c = 0;
    for (long long o = 16LL * threadIdx.x; o < ldk; o += 16 * 64) {
        const uint4 v = *reinterpret_cast<const uint4 *>(row + o);
        c += perm_bytes(v.x) + perm_bytes(v.y) + perm_bytes(v.z) + perm_bytes(v.w);
    }
    for (int k = 1; k < 64; k <<= 1) c += __shfl_xor(c, k, 64);
    if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// ---- totals: an LD image's x and m planes and the study row -> {At, Nc, Q, flag} ------------------------------------------------------------
// One workgroup per SNP, a lane per 16 samples: three 16-byte loads.  Bandwidth-bound: 3 n bytes in, 16 out.
__global__ __launch_bounds__(256) void perm_totals_kernel(long long ldk, long long from, size_t ld_plane, const signed char *ld, const int4 *ld_tot,
                                                          const signed char *study, int4 *out)
{
    __shared__ int red[4][4];
    const long long g = from + blockIdx.x;
    const signed char *xr = ld + (size_t)g * ldk, *mr = xr + ld_plane;
    int s[4] = {0, 0, 0, 0};      // heterozygous, homozygous for the counted allele, called, study samples
    for (long long o = 16LL * threadIdx.x; o < ldk; o += 16 * 256) {
        const uint4 xv = *reinterpret_cast<const uint4 *>(xr + o), mv = *reinterpret_cast<const uint4 *>(mr + o);
        const uint4 sv = *reinterpret_cast<const uint4 *>(study + o);
        const unsigned xw[4] = {xv.x, xv.y, xv.z, xv.w}, mw[4] = {mv.x, mv.y, mv.z, mv.w}, sw[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const unsigned k = (sw[w] & 0x01010101u) * 0xffu;      // a byte of ones per study sample
            const unsigned x = xw[w] & k;                          // codes 0, 1, 2: bit 0 heterozygous, bit 1 homozygous
            s[0] += __popc(x & 0x01010101u); s[1] += __popc(x & 0x02020202u);
            s[2] += __popc(mw[w] & k & 0x01010101u); s[3] += __popc(k & 0x01010101u);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; t++)
        for (int k = 1; k < 64; k <<= 1) s[t] += __shfl_xor(s[t], k, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int t = 0; t < 4; t++) red[threadIdx.x >> 6][t] = s[t];
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int t = 0; t < 4; t++) s[t] = red[0][t] + red[1][t] + red[2][t] + red[3][t];
        const int flag = (s[2] != s[3] ? 1 : 0) | (ld_tot[g].w ? 2 : 0);
        out[blockIdx.x] = make_int4(s[0] + 2 * s[1], s[2], s[0] + 4 * s[1], flag);
    }
}

// ---- the block kernel ---------------------------------------------------------------------------------------------------------------------
struct PermBlock {
    int KT, planes, tiles_b, test;
    long long ldk;
    const signed char *A;             // plane x; plane m lies `plane` bytes further
    size_t plane;
    const signed char *labels;
    const int4 *tot;                  // of SNP a0 + ia at [ia]
    const int *labc;                  // of labelling jb at [jb]
    long long a0, na, b0, nb;
    double *dense;
    long long ldo;
    const double *obs;
    unsigned *n_ge;
    unsigned long long *max_null;
};

// the accumulators of a workgroup's tile, behind the pair tile's LDS: 256 64-bit maxima of the columns (labellings), 256 counts of the
// rows (SNPs)
constexpr int PERM_LDS = I8P_LDS + 256 * 8 + 256 * 4;
__device__ __forceinline__ unsigned long long *perm_acc_max() { return reinterpret_cast<unsigned long long *>(i8p_lds + I8P_LDS); }
__device__ __forceinline__ unsigned *perm_acc_ge() { return reinterpret_cast<unsigned *>(i8p_lds + I8P_LDS + 256 * 8); }

// STAT = false (the bench's build only, -DPG_PERM_BENCH_NOSTAT): the statistic is stubbed out by one conversion, the rest of the epilogue stays
template <bool STAT> __device__ __forceinline__ double perm_stat(int test, long long At, long long Nc, long long Q, long long a, long long R)
{
    if (!STAT) return (double)(a + R);
    const double nan = __builtin_nan("");
    if (R <= 0 || R >= Nc) return nan;
    if (test == PG_PERM_ALLELIC) {
        const long long b = 2 * R - a, c = At - a, d = 2 * (Nc - R) - c;
        const long long r1 = a + b, r2 = c + d, c1 = a + c, c2 = b + d, T = r1 + r2;
        if (r1 == 0 || r2 == 0 || c1 == 0 || c2 == 0) return nan;
        const double D = (double)(a * d - b * c);
        return ((double)T * (D * D)) / ((double)(r1 * r2) * (double)(c1 * c2));
    }
    const long long Sp = Nc - R, Ui = Nc * a - R * At, Vi = Nc * Q - At * At;
    if (Vi == 0) return nan;
    const double U = (double)Ui;
    return ((double)Nc * (U * U)) / ((double)(R * Sp) * (double)Vi);
}

// One staged half: HA SNPs (rows) x 256 labellings (columns); as0: the first SNP of the (sub-)tile, abase, bbase: of the workgroup's tile.
// cmax: the lane's four column maxima.
template <bool PLANES, bool STAT>
__device__ __forceinline__ void perm_half(const PermBlock &q, const I8pLane ln, int half, long long as0, long long abase, long long bbase, long long aend,
                                          long long bend, const int (&labc)[4], unsigned long long (&cmax)[4])
{
    constexpr int HA = PLANES ? 64 : 128;
    const int *const stg = i8p_staged();
#pragma unroll 1
    for (int sa = ln.wave; sa < HA; sa += 8) {
        const long long ja = as0 + half * HA + sa;
        if (ja >= aend) break;
        const int4 t = q.tot[ja - q.a0];
        const double ob = q.n_ge ? q.obs[ja - q.a0] : 0.0;
        unsigned rge = 0;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int sb = ln.lane + 64 * c;
            const long long jb = bbase + sb;
            if (jb < bend) {
                const long long a = stg[sa * I8P_LDW + sb];
                const long long R = PLANES ? stg[(64 + sa) * I8P_LDW + sb] : labc[c];
                const double v = perm_stat<STAT>(q.test, t.x, t.y, t.z, a, R);
                if (q.dense) q.dense[(ja - q.a0) * q.ldo + (jb - q.b0)] = v;
                rge += v >= ob ? 1u : 0u;                              // a NaN on either side: false
                const unsigned long long bits = v == v ? (unsigned long long)__double_as_longlong(v) : 0ULL;      // v >= +0.0: ordered as integers
                cmax[c] = bits > cmax[c] ? bits : cmax[c];
            }
        }
        if (q.n_ge) {
            for (int k = 1; k < 64; k <<= 1) rge += __shfl_xor(rge, k, 64);
            if (ln.lane == 0) perm_acc_ge()[ja - abase] = rge;      // the row is this wavefront's alone, once per workgroup
        }
    }
}

template <bool STAT> __global__ __launch_bounds__(512, 1) void perm_block_kernel(PermBlock q)
{
    const int tid = threadIdx.x;
    const I8pLane ln = i8p_lane();
    const long long tile_a = blockIdx.x / q.tiles_b, tile_b = blockIdx.x % q.tiles_b;
    const long long abase = q.a0 + tile_a * PERM_T, bbase = q.b0 + tile_b * PERM_T;
    const long long aend = q.a0 + q.na, bend = q.b0 + q.nb;      // one past the last SNP, the last labelling
    // does a SNP of the tile carry a flag?
    int miss = q.planes;
    if (tid < PERM_T && abase + tid < aend) miss |= q.tot[abase + tid - q.a0].w;
    const bool planes = __syncthreads_or(miss) != 0;
    if (tid < 256) perm_acc_max()[tid] = 0;      // ordered before the first add by the barriers of the first products
    else perm_acc_ge()[tid - 256] = 0;
    int labc[4];
    unsigned long long cmax[4] = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const long long jb = bbase + ln.lane + 64 * c;
        labc[c] = jb < bend ? q.labc[jb] : 0;
    }
    const int nsub = planes ? 2 : 1, TA = planes ? 128 : PERM_T;

#pragma unroll 1
    for (int sub = 0; sub < nsub; sub++) {
        const long long as0 = abase + sub * TA;
        if (as0 >= aend) continue;
        intx4 acc[4][8];
        i8p_zero(acc);
        // DMA sources.  Rows past a window repeat the window's last SNP, its last labelling: their products are never read.
        const signed char *srcA[4], *srcB[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int row = i8p_src_row(ln, t), h = row >> 7, rr = row & 127;
            const int pla = planes ? rr >> 6 : 0, sna = planes ? h * 64 + (rr & 63) : row;
            const long long ga = min(as0 + sna, aend - 1), gb = min(bbase + row, bend - 1);
            srcA[t] = q.A + (size_t)pla * q.plane + (size_t)ga * q.ldk + i8p_src_byte(ln, row);
            srcB[t] = q.labels + (size_t)gb * q.ldk + i8p_src_byte(ln, row);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the stores of the previous epilogue are not counted against the loads below
        i8p_products(ln, srcA, srcB, q.KT, acc);
#pragma unroll 1
        for (int half = 0; half < 2; half++) {
            i8p_stage(ln, half, acc);
            if (planes) perm_half<true, STAT>(q, ln, half, as0, abase, bbase, aend, bend, labc, cmax);
            else perm_half<false, STAT>(q, ln, half, as0, abase, bbase, aend, bend, labc, cmax);
            __syncthreads();
        }
    }
    if (q.max_null) {
#pragma unroll
        for (int c = 0; c < 4; c++)
            if (cmax[c]) atomicMax(perm_acc_max() + ln.lane + 64 * c, cmax[c]);
    }
    __syncthreads();
    // the accumulators go out: threads [0, 256) the labellings from bbase, threads [256, 512) the SNPs from abase
    if (tid < 256) {
        const unsigned long long m = perm_acc_max()[tid];
        if (q.max_null && m && bbase + tid < bend) atomicMax(q.max_null + (bbase - q.b0) + tid, m);
    } else {
        const int t = tid - 256;
        const unsigned c = perm_acc_ge()[t];
        if (q.n_ge && c && abase + t < aend) atomicAdd(q.n_ge + (abase - q.a0) + t, c);
    }
}

static bool perm_shape_ok(int64_t n, int64_t pe) { return n >= 1 && n < PERM_MAXN && pe >= 1 && pe < PERM_MAXPE; }
static bool perm_aligned(const void *p, int to) { return (uintptr_t)p % to == 0; }
static long long perm_ldk(int64_t n) { return (n + LD_BK - 1) / LD_BK * LD_BK; }

}  // namespace pg

using namespace pg;

extern "C" size_t pg_perm_label_bytes(int64_t n, int64_t nb)
{
    if (!perm_shape_ok(n, nb)) return 0;
    return up256((size_t)nb * perm_ldk(n));
}

extern "C" int pg_perm_label_counts_dev(pg_ctx *ctx, int64_t n, const signed char *labels, int64_t nb, int32_t *counts)
{
    PG_REQUIRE(ctx && labels && counts, "pg_perm_label_counts_dev: NULL argument");
    PG_REQUIRE(perm_aligned(labels, 16), "pg_perm_label_counts_dev: the labels must lie on 16 bytes");
    PG_REQUIRE(n >= 1 && n < PERM_MAXN && nb >= 0 && nb < PERM_MAXPE, "pg_perm_label_counts_dev: bad shape n=%lld nb=%lld", (long long)n, (long long)nb);
    if (nb == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    perm_label_count_kernel<<<(unsigned)nb, 64, 0, ctx->stream>>>(perm_ldk(n), labels, counts);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

extern "C" int pg_perm_totals_dev(pg_ctx *ctx, int64_t n, const void *image, int64_t pe, int64_t from, int64_t count, const signed char *study,
                                  int32_t *totals)
{
    PG_REQUIRE(ctx && image && study && totals, "pg_perm_totals_dev: NULL argument");
    PG_REQUIRE(perm_aligned(image, 16) && perm_aligned(study, 16) && perm_aligned(totals, 16),
               "pg_perm_totals_dev: the image, the study row and the totals must lie on 16 bytes");
    PG_REQUIRE(perm_shape_ok(n, pe) && from >= 0 && count >= 0 && from + count <= pe, "pg_perm_totals_dev: bad shape n=%lld pe=%lld from=%lld count=%lld",
               (long long)n, (long long)pe, (long long)from, (long long)count);
    if (count == 0) return PG_OK;
    PG_HIP(hipSetDevice(ctx->device));
    const LdLayout L = ld_layout(n, pe);
    const signed char *img = static_cast<const signed char *>(image);
    perm_totals_kernel<<<(unsigned)count, 256, 0, ctx->stream>>>(L.ldk, from, L.plane, img, reinterpret_cast<const int4 *>(img + L.totals), study,
                                                                   reinterpret_cast<int4 *>(totals));
    PG_HIP(hipGetLastError());
    return PG_OK;
}

extern "C" int pg_perm_block_dev(pg_ctx *ctx, int64_t n, const void *image, int64_t pe, int64_t a0, int64_t na, const int32_t *totals,
                                 const signed char *labels, const int32_t *lab_counts, int64_t b0, int64_t nb, int test, double *dense, int64_t ldo,
                                 const double *obs, uint32_t *n_ge, uint64_t *max_null)
{
    PG_REQUIRE(ctx && image && totals && labels && lab_counts && (obs || !n_ge), "pg_perm_block_dev: NULL argument");
    if (test != PG_PERM_ALLELIC && test != PG_PERM_TREND) {
        set_error("pg_perm_block_dev: unknown test %d", test);
        return PG_ENOTSUP;
    }
    PG_REQUIRE(perm_aligned(image, 16) && perm_aligned(labels, 16) && perm_aligned(totals, 16) && perm_aligned(dense, 8) && perm_aligned(obs, 8) &&
                   perm_aligned(max_null, 8) && perm_aligned(n_ge, 4) && perm_aligned(lab_counts, 4),
               "pg_perm_block_dev: the image, the labels and the totals must lie on 16 bytes, dense, obs and max_null on 8");
    PG_REQUIRE(perm_shape_ok(n, pe) && a0 >= 0 && na >= 0 && a0 + na <= pe && b0 >= 0 && nb >= 0 && b0 + nb < PERM_MAXPE && (!dense || ldo >= nb),
               "pg_perm_block_dev: bad shape n=%lld SNPs [%lld, +%lld) of %lld, labellings [%lld, +%lld), ldo=%lld", (long long)n, (long long)a0,
               (long long)na, (long long)pe, (long long)b0, (long long)nb, (long long)ldo);
    if (na == 0 || nb == 0) return PG_OK;
    const long long tiles_a = (na + PERM_T - 1) / PERM_T, tiles_b = (nb + PERM_T - 1) / PERM_T;
    PG_REQUIRE(tiles_a * tiles_b < (1LL << 31), "pg_perm_block_dev: too many tiles (%lld x %lld)", tiles_a, tiles_b);
    PG_HIP(hipSetDevice(ctx->device));
    const LdLayout L = ld_layout(n, pe);
    PermBlock q;
    q.KT = (int)(L.ldk / LD_BK); q.planes = env_flag("PG_PERM_PLANES"); q.tiles_b = (int)tiles_b; q.test = test;
    q.ldk = L.ldk; q.A = static_cast<const signed char *>(image); q.plane = L.plane; q.labels = labels;
    q.tot = reinterpret_cast<const int4 *>(totals); q.labc = lab_counts;
    q.a0 = a0; q.na = na; q.b0 = b0; q.nb = nb;
    q.dense = dense; q.ldo = ldo; q.obs = obs; q.n_ge = n_ge; q.max_null = reinterpret_cast<unsigned long long *>(max_null);
#ifdef PG_PERM_BENCH_NOSTAT
    constexpr bool stat = false;
#else
    constexpr bool stat = true;
#endif
    PG_HIP((i8p_lds_limit<perm_block_kernel<stat>, PERM_LDS>(ctx->device)));
    perm_block_kernel<stat><<<(unsigned)(tiles_a * tiles_b), 512, PERM_LDS, ctx->stream>>>(q);
    PG_HIP(hipGetLastError());
    return PG_OK;
}
