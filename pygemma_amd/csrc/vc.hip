// vc.hip (libpygemma_vc.so, a library of its own that needs libpygemma_hip.so for contexts, errors and scratch) — dense fp64 linear algebra of the multi-component REML (lmm.reml): V = sum_i s_i K_i + s_k I for several kinship matrices that
// share no eigenvectors, its Cholesky factor, log determinant and explicit inverse, tr(V^-1 K_i), symmetric matrix x panel products, and
// one evaluation of the REML objective (log likelihood, score, average information) that chains them on the context's stream.
//
// Matrices are row-major; of a symmetric or triangular matrix only the LOWER triangle (with the diagonal) is read or written.  The
// entry points that take a caller's matrix (pg_vc_combine_dev, pg_potrf_dev, pg_potri_dev) leave its strict upper triangle and the pad
// of a pitched row as they were.  The fp64-MFMA GEMM (dgemm.hpp) writes whole 128 x 128 diagonal tiles of a lower-only product, so the
// blocked algorithms run in work matrices of pitch ldw = n rounded up to 16 whose upper triangle is free for that, and a caller's
// matrix goes in and out through a copy of its lower triangle.  pg_vc_eval_dev works in its own three work matrices and copies nothing.
//
// potrf, right-looking in blocks of 64 columns:  the 64 x 64 diagonal block is factored and its factor inverted by one workgroup in
// LDS (vc_diag_kernel); the panel below it is multiplied by that inverse, 64 rows per workgroup, and leaves twice — in place, and
// transposed (k-major) into PT (vc_panel_kernel); two panels make one rank-128 update  A22 -= PT' PT  of the trailing matrix through
// the lower-only GEMM, the shape of the band reduction's update (the first panel updates the second one's 64 columns on its own).  A pivot that is not a positive finite number sets *info to 1 + its index (the first
// one only), is replaced by 1, and every later diagonal block is left alone: the call runs to its end on finite or non-finite junk
// inside the matrix and nowhere else.
// potri:  X = L^-1 level by level — the 64 x 64 diagonal inverses by one workgroup each (vc_trtri_kernel), then for b = 64, 128, ...
// every pair of adjacent b-blocks takes  X21 = -X22 (L21 X11)  as two batched GEMMs — and A^-1 = X'X through the lower-only GEMM.
// Both the level products and X'X run over the zero upper half of X: 4/3 n^3 flops where 2/3 n^3 would do.
// trdot: a workgroup per row (cyclic), fp64 accumulation, a fixed LDS tree per workgroup, partials summed by one workgroup in a
// fixed tree: no atomics, the same bits on every run.
// symv: a workgroup per 64 output rows walks the 64-column tiles of its row block in order; tiles right of the diagonal are read from
// the transposed position (rows below), the diagonal tile is mirrored from its lower half: every stored element of the lower triangle
// is read twice, none of the upper once.  An output is one fixed chain over the columns in ascending order.
#include "dgemm.hpp"
#include "../../include/pygemma_vc.h"

#include <cmath>
#include <vector>

namespace pg {

constexpr int VB = 64, VP = 65;                         // block size, LDS pitch of a block
constexpr int VC_MAXK = 64;                             // matrices per call
constexpr int VC_RHS = 32;                              // right-hand sides per symv, panel columns per Gram
constexpr int VC_DIAG_LDS = 2 * VB * VP * 8;            // two blocks (the block and its inverse; panel rows and the inverse): 66 560 bytes, dynamic (above the static limit)
constexpr int VC_PART = 1024;                           // workgroups of a trdot
constexpr int VC_GRAM_WG = 256;                         // workgroups of a Gram
constexpr size_t VC_SMALL = (size_t)(VC_PART + VC_GRAM_WG * 1024) * 8;      // the partials at the head of ctx->scratch

static inline long long vc_ldw(long long n) { return (n + 15) / 16 * 16; }

__device__ __forceinline__ double vc_block_sum(double v, double *sh)
{
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) sh[tid] = sh[tid] + sh[tid + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// ---- combine ------------------------------------------------------------------------------------------------------------------------

struct VcCombineArgs {
    const void *K[VC_MAXK];
    long long ldk[VC_MAXK];
    double s[VC_MAXK + 1];
    unsigned char f64[VC_MAXK];
    int k, zero_upper;
    long long n, ldv;
    double *V;
};

// row blockIdx.x; zero_upper: the work-matrix form, which also clears the columns right of the diagonal
__global__ __launch_bounds__(256) void vc_combine_kernel(VcCombineArgs a)
{
    const long long i = blockIdx.x, jend = a.zero_upper ? a.n : i + 1;
    for (long long j = threadIdx.x; j < jend; j += 256) {
        double v = 0.0;
        if (j <= i) {
            for (int t = 0; t < a.k; t++) {
                const double x = a.f64[t] ? static_cast<const double *>(a.K[t])[i * a.ldk[t] + j] : (double)static_cast<const float *>(a.K[t])[i * a.ldk[t] + j];
                v = v + a.s[t] * x;
            }
            if (j == i) v = v + a.s[a.k];
        }
        a.V[i * a.ldv + j] = v;
    }
}

__global__ __launch_bounds__(256) void vc_copy_lower_kernel(long long n, const double *src, long long lds_, double *dst, long long ldd, int zero_upper)
{
    const long long i = blockIdx.x, jend = zero_upper ? n : i + 1;
    for (long long j = threadIdx.x; j < jend; j += 256) dst[i * ldd + j] = (j <= i) ? src[i * lds_ + j] : 0.0;
}

// ---- the 64 x 64 block in LDS --------------------------------------------------------------------------------------------------------

// A (pitch VP): the lower triangle of a symmetric block -> its Cholesky factor.  *bad (LDS, -1 on entry): the first pivot refused
__device__ __forceinline__ void vc_chol64(double *A, int *bad)
{
    const int tid = threadIdx.x;
    for (int k = 0; k < VB; k++) {
        __syncthreads();
        double p = A[k * VP + k];
        const bool isbad = !(p > 0.0) || !(p < 1.0e300);
        if (isbad) p = 1.0;
        const double d = sqrt(p);
        __syncthreads();                                   // every thread has the pivot before it is replaced
        if (isbad && tid == 0 && *bad < 0) *bad = k;
        if (tid < VB) {
            if (tid == k) A[k * VP + k] = d;
            else if (tid > k) A[tid * VP + k] = A[tid * VP + k] / d;
        }
        __syncthreads();
        const int i = tid >> 2;
        if (i > k) {
            const double lik = A[i * VP + k];
            for (int j = k + 1 + (tid & 3); j <= i; j += 4) A[i * VP + j] = fma(-lik, A[j * VP + k], A[i * VP + j]);
        }
    }
    __syncthreads();
}

// X = L^-1 for the lower-triangular L in A: lane c of the first wavefront owns column c (X[i][c] = 0 above the diagonal)
__device__ __forceinline__ void vc_trtri64(const double *A, double *X)
{
    const int c = threadIdx.x;
    if (c < VB) {
        for (int i = 0; i < VB; i++) {
            double s = (i == c) ? 1.0 : 0.0;
            for (int k = 0; k < i; k++) s = fma(-A[i * VP + k], X[k * VP + c], s);
            X[i * VP + c] = (i >= c) ? s / A[i * VP + i] : 0.0;
        }
    }
    __syncthreads();
}

// the jb x jb block at G (lower triangle) into A, bordered by the identity up to 64 x 64
__device__ __forceinline__ void vc_block_load(double *A, const double *G, long long ld, int jb)
{
    for (int idx = threadIdx.x; idx < VB * VB; idx += 256) {
        const int i = idx >> 6, j = idx & 63;
        A[i * VP + j] = (i < jb && j <= i) ? G[i * ld + j] : ((i == j) ? 1.0 : 0.0);
    }
    __syncthreads();
}

// potrf's diagonal step: block (j0, j0) of size jb -> its factor in place, the factor's inverse (64 x 64, pitch 64, zeros above the
// diagonal) to Linv.  Nothing happens once *info is set.
__global__ __launch_bounds__(256) void vc_diag_kernel(double *G, long long ld, int jb, long long j0, double *Linv, int *info)
{
    extern __shared__ double vlds[];
    double *A = vlds, *X = vlds + VB * VP;
    __shared__ int bad;
    if (*info != 0) return;                                // uniform: before any barrier
    if (threadIdx.x == 0) bad = -1;
    vc_block_load(A, G, ld, jb);
    vc_chol64(A, &bad);
    vc_trtri64(A, X);
    for (int idx = threadIdx.x; idx < VB * VB; idx += 256) {
        const int i = idx >> 6, j = idx & 63;
        if (i < jb && j <= i) G[i * ld + j] = A[i * VP + j];
        Linv[idx] = X[i * VP + j];
    }
    if (threadIdx.x == 0 && bad >= 0) *info = (int)(j0 + bad) + 1;
}

// potri's diagonal step, every block at once: block blockIdx.x of L -> its inverse into the same block of X (lower triangle)
__global__ __launch_bounds__(256) void vc_trtri_kernel(const double *Lm, long long ldl, long long n, double *Xm, long long ldx)
{
    extern __shared__ double vlds[];
    double *A = vlds, *X = vlds + VB * VP;
    const long long j0 = (long long)blockIdx.x * VB;
    const int jb = (int)((n - j0 < VB) ? n - j0 : VB);
    vc_block_load(A, Lm + j0 * (ldl + 1), ldl, jb);
    vc_trtri64(A, X);
    double *O = Xm + j0 * (ldx + 1);
    for (int idx = threadIdx.x; idx < VB * VB; idx += 256) {
        const int i = idx >> 6, j = idx & 63;
        if (i < jb && j <= i) O[i * ldx + j] = X[i * VP + j];
    }
}

// potrf's panel step: rows [64 blockIdx.x, + 64) of the M x 64 panel A21 <- A21 Linv', in place and transposed into PT (64 x M, pitch ldpt)
__global__ __launch_bounds__(256) void vc_panel_kernel(double *A21, long long lda, long long M, const double *Linv, double *PT, long long ldpt)
{
    extern __shared__ double vlds[];
    double *At = vlds, *Li = vlds + VB * VP;
    const int tid = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * VB;
    for (int idx = tid; idx < VB * VB; idx += 256) {
        const int r = idx >> 6, cc = idx & 63;
        At[r * VP + cc] = (r0 + r < M) ? A21[(r0 + r) * lda + cc] : 0.0;
        Li[r * VP + cc] = Linv[idx];
    }
    __syncthreads();
    const int r = tid & 63, kq = (tid >> 6) * 16;
    double out[16];
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const int k = kq + q;
        double s = 0.0;
        for (int cc = 0; cc <= k; cc++) s = fma(At[r * VP + cc], Li[k * VP + cc], s);
        out[q] = s;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; q++) {
        At[r * VP + kq + q] = out[q];
        if (r0 + r < M) PT[(long long)(kq + q) * ldpt + r0 + r] = out[q];
    }
    __syncthreads();
    for (int idx = tid; idx < VB * VB; idx += 256) {
        const int rr = idx >> 6, cc = idx & 63;
        if (r0 + rr < M) A21[(r0 + rr) * lda + cc] = At[rr * VP + cc];
    }
}

// mode 0: 2 sum_j log A[j][j]; mode 1: sum_j A[j][j].  One workgroup, a fixed tree
__global__ __launch_bounds__(256) void vc_diag_sum_kernel(long long n, const double *A, long long lda, int mode, double *out)
{
    __shared__ double sh[256];
    double s = 0.0;
    for (long long j = threadIdx.x; j < n; j += 256) {
        const double d = A[j * (lda + 1)];
        s = s + (mode ? d : log(d));
    }
    const double t = vc_block_sum(s, sh);
    if (threadIdx.x == 0) *out = mode ? t : 2.0 * t;
}

// ---- trdot ----------------------------------------------------------------------------------------------------------------------------

template <class TB>
__global__ __launch_bounds__(256) void vc_trdot_kernel(long long n, const double *A, long long lda, const TB *B, long long ldb, double *part)
{
    __shared__ double sh[256];
    double sd = 0.0, so = 0.0;
    for (long long i = blockIdx.x; i < n; i += gridDim.x) {
        const double *ar = A + i * lda;
        const TB *br = B + i * ldb;
        for (long long j = threadIdx.x; j < i; j += 256) so = fma(ar[j], (double)br[j], so);
        if (threadIdx.x == 0) sd = fma(ar[i], (double)br[i], sd);
    }
    const double t = vc_block_sum(sd + 2.0 * so, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void vc_part_sum_kernel(int np, const double *part, double *out)
{
    __shared__ double sh[256];
    double s = 0.0;
    for (int j = threadIdx.x; j < np; j += 256) s = s + part[j];
    const double t = vc_block_sum(s, sh);
    if (threadIdx.x == 0) *out = t;
}

// ---- symv -----------------------------------------------------------------------------------------------------------------------------

template <class TA>
__global__ __launch_bounds__(256) void vc_symv_kernel(long long n, const TA *A, long long lda, int m, const double *X, long long ldx, double *Y, long long ldy)
{
    __shared__ double T[VB * VP], xs[VB * VC_RHS];
    const int tid = threadIdx.x, r = tid & 63, g = tid >> 6;      // g: the right-hand sides 8 g .. 8 g + 7 (uniform over a wavefront)
    const long long I = blockIdx.x, i0 = I * VB, nJ = (n + VB - 1) / VB;
    double acc[8];
#pragma unroll
    for (int q = 0; q < 8; q++) acc[q] = 0.0;
    for (int idx = tid; idx < VB * VC_RHS; idx += 256) xs[idx] = 0.0;
    for (long long J = 0; J < nJ; J++) {
        const long long j0 = J * VB;
        __syncthreads();
        for (int idx = tid; idx < VB * VB; idx += 256) {
            const int a = idx >> 6, b = idx & 63;
            if (J < I) {
                const long long gi = i0 + a, gj = j0 + b;
                T[a * VP + b] = (gi < n) ? (double)A[gi * lda + gj] : 0.0;
            } else if (J > I) {                            // stored below the diagonal: rows j0 .., columns i0 ..
                const long long gi = j0 + a, gj = i0 + b;
                T[b * VP + a] = (gi < n && gj < n) ? (double)A[gi * lda + gj] : 0.0;
            } else if (b <= a) {
                const long long gi = i0 + a, gj = i0 + b;
                const double v = (gi < n) ? (double)A[gi * lda + gj] : 0.0;
                T[a * VP + b] = v;
                if (b < a) T[b * VP + a] = v;
            }
        }
        for (int idx = tid; idx < VB * m; idx += 256) {
            const int jj = idx / m, cc = idx % m;
            xs[jj * VC_RHS + cc] = (j0 + jj < n) ? X[(j0 + jj) * ldx + cc] : 0.0;
        }
        __syncthreads();
        if (8 * g < m) {
            for (int jj = 0; jj < VB; jj++) {
                const double t = T[r * VP + jj];
#pragma unroll
                for (int q = 0; q < 8; q++) acc[q] = fma(t, xs[jj * VC_RHS + 8 * g + q], acc[q]);
            }
        }
    }
    if (i0 + r < n) {
#pragma unroll
        for (int q = 0; q < 8; q++)
            if (8 * g + q < m) Y[(i0 + r) * ldy + 8 * g + q] = acc[q];
    }
}

// ---- Gram of two skinny panels: out[a][b] = sum_i P[i][a] Q[i][b], a < ma <= 32, b < mb <= 32 --------------------------------------------

__global__ __launch_bounds__(256) void vc_gram_kernel(long long n, long long rows_per_wg, const double *P, long long ldp, int ma, const double *Q, long long ldq,
                                                      int mb, double *part)
{
    __shared__ double ps[VB * 33], qs[VB * 33];
    const int tid = threadIdx.x, a = tid >> 3, b0 = (tid & 7) * 4;
    const long long beg = (long long)blockIdx.x * rows_per_wg, end = (beg + rows_per_wg < n) ? beg + rows_per_wg : n;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long s0 = beg; s0 < end; s0 += VB) {
        __syncthreads();
        for (int idx = tid; idx < VB * 32; idx += 256) {
            const int rr = idx >> 5, cc = idx & 31;
            const bool in = s0 + rr < end;
            ps[rr * 33 + cc] = (in && cc < ma) ? P[(s0 + rr) * ldp + cc] : 0.0;
            qs[rr * 33 + cc] = (in && cc < mb) ? Q[(s0 + rr) * ldq + cc] : 0.0;
        }
        __syncthreads();
        for (int rr = 0; rr < VB; rr++) {
            const double pa = ps[rr * 33 + a];
#pragma unroll
            for (int q = 0; q < 4; q++) acc[q] = fma(pa, qs[rr * 33 + b0 + q], acc[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) part[(size_t)blockIdx.x * 1024 + a * 32 + b0 + q] = acc[q];
}

__global__ __launch_bounds__(256) void vc_gram_sum_kernel(int nwg, const double *part, int ma, int mb, double *out, int ldo)
{
    const int t = blockIdx.x * 256 + threadIdx.x, a = t >> 5, b = t & 31;
    if (a >= ma || b >= mb) return;
    double s = 0.0;
    for (int g = 0; g < nwg; g++) s = s + part[(size_t)g * 1024 + t];
    out[a * ldo + b] = s;
}

// ---- the fitted-value step of an evaluation -----------------------------------------------------------------------------------------------

struct VcPyArgs {
    long long n;
    int c, kk;
    const double *Z;          // n x 32: V^-1 [W y]
    double *Qp;               // n x 32: [V^-1 W, P y]
    double *U;                // n x kk: column kk - 1 <- P y
    double *Py;               // n, or nullptr
    double beta[PG_MAX_COVARIATES];
};

__global__ __launch_bounds__(256) void vc_py_kernel(VcPyArgs a)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const double *z = a.Z + i * VC_RHS;
    double *q = a.Qp + i * VC_RHS;
    double s = 0.0;
    for (int t = 0; t < a.c; t++) {
        q[t] = z[t];
        s = fma(z[t], a.beta[t], s);
    }
    const double py = z[a.c] - s;
    q[a.c] = py;
    a.U[i * a.kk + a.kk - 1] = py;
    if (a.Py) a.Py[i] = py;
}

__global__ __launch_bounds__(256) void vc_column_kernel(long long n, const double *src, long long lds_, double *dst, long long ldd)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i * ldd] = src[i * lds_];
}

// ---- host drivers ---------------------------------------------------------------------------------------------------------------------------

static int vc_lds_attr(pg_ctx *ctx)
{
    static std::atomic<unsigned> done_mask{0};             // a per-device function attribute, set on a device's first call
    const unsigned bit = 1u << (ctx->device & 31);
    if (!(done_mask.load(std::memory_order_acquire) & bit)) {
        PG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&vc_diag_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, VC_DIAG_LDS));
        PG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&vc_trtri_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, VC_DIAG_LDS));
        PG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&vc_panel_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, VC_DIAG_LDS));
        done_mask.fetch_or(bit, std::memory_order_release);
    }
    return PG_OK;
}

struct VcMats {
    int k;
    const void *const *K;
    const int *f64;
    const int64_t *ldk;
};

static int vc_check_mats(const char *what, int64_t n, int k, const VcMats &m)
{
    PG_REQUIRE(n >= 1 && n < (1LL << 30), "%s: bad n=%lld", what, (long long)n);
    PG_REQUIRE(k >= 0 && k <= VC_MAXK, "%s: k=%d matrices, 0 to %d are supported", what, k, VC_MAXK);
    PG_REQUIRE(k == 0 || (m.K && m.f64 && m.ldk), "%s: NULL argument", what);
    for (int t = 0; t < k; t++) PG_REQUIRE(m.K[t] && m.ldk[t] >= n, "%s: matrix %d is NULL or its ldk=%lld < n=%lld", what, t, (long long)m.ldk[t], (long long)n);
    return PG_OK;
}

static int vc_combine(pg_ctx *ctx, long long n, const VcMats &m, const double *s, double *V, long long ldv, bool zero_upper)
{
    VcCombineArgs a{};
    for (int t = 0; t < m.k; t++) { a.K[t] = m.K[t]; a.ldk[t] = m.ldk[t]; a.f64[t] = m.f64[t] != 0; a.s[t] = s[t]; }
    a.s[m.k] = s[m.k];
    a.k = m.k; a.zero_upper = zero_upper; a.n = n; a.ldv = ldv; a.V = V;
    vc_combine_kernel<<<(unsigned)n, 256, 0, ctx->stream>>>(a);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

// W (pitch ldw, a work matrix: its upper triangle is written freely) -> its factor in the lower triangle.  Dinv: 4096 doubles, PT: 128 ldw.
// Two 64-column panels per step: the first one's rank-64 update goes to the next 64 columns only (a skinny GEMM), the second panel is
// stored 64 columns into PT so that rows 0 .. 127 of PT + 64 are [P1 P2]' of the rows below both, and the trailing matrix takes ONE
// rank-128 update: half the passes over the trailing triangle, which is what the factorisation's time is made of.
static int vc_potrf_ws(pg_ctx *ctx, long long n, double *W, long long ldw, int *info_dev, double *Dinv, double *PT)
{
    int rc = vc_lds_attr(ctx);
    if (rc) return rc;
    auto diag = [&](long long j, int jb) {
        vc_diag_kernel<<<1, 256, VC_DIAG_LDS, ctx->stream>>>(W + j * (ldw + 1), ldw, jb, j, Dinv, info_dev);
        return hipGetLastError();
    };
    auto panel = [&](long long row, long long col, long long M, double *pt) {      // rows row .., columns col .. col + 63
        vc_panel_kernel<<<(unsigned)((M + VB - 1) / VB), 256, VC_DIAG_LDS, ctx->stream>>>(W + row * ldw + col, ldw, M, Dinv, pt, ldw);
        return hipGetLastError();
    };
    for (long long j = 0; j < n; j += 2 * VB) {
        const int jb = (int)std::min<long long>(VB, n - j);
        PG_HIP(diag(j, jb));
        const long long M1 = n - j - jb;
        if (M1 <= 0) break;
        PG_HIP(panel(j + VB, j, M1, PT));
        const int nb2 = (int)std::min<long long>(VB, M1);
        DgemmDesc u;                                           // columns j + 64 .. of the rows below the first panel: -= P1 P1[0 : nb2]'
        u.transA = true; u.M = M1; u.N = nb2; u.K = VB; u.alpha = -1.0; u.beta = 1.0;
        u.A = PT; u.lda = ldw; u.B = PT; u.ldb = ldw; u.C = W + (j + VB) * (ldw + 1); u.ldc = ldw; u.allow_splitk = false;
        rc = dgemm_ex(ctx, u);
        if (rc) return rc;
        PG_HIP(diag(j + VB, nb2));
        const long long M2 = M1 - nb2;
        if (M2 <= 0) break;
        PG_HIP(panel(j + 2 * VB, j + VB, M2, PT + VB * ldw + VB));
        DgemmDesc d;
        d.transA = true; d.M = M2; d.N = M2; d.K = 2 * VB; d.alpha = -1.0; d.beta = 1.0;
        d.A = PT + VB; d.lda = ldw; d.B = PT + VB; d.ldb = ldw; d.C = W + (j + 2 * VB) * (ldw + 1); d.ldc = ldw;
        d.lower_only = true; d.allow_splitk = false;
        rc = dgemm_ex(ctx, d);
        if (rc) return rc;
    }
    return PG_OK;
}

// X (pitch ldx) <- L^-1 and O (pitch ldo) <- (L L')^-1, lower triangles; both are work matrices of n rows.  L is only read
static int vc_potri_ws(pg_ctx *ctx, long long n, const double *Lm, long long ldl, double *X, long long ldx, double *O, long long ldo)
{
    int rc = vc_lds_attr(ctx);
    if (rc) return rc;
    PG_HIP(hipMemsetAsync(X, 0, (size_t)n * ldx * sizeof(double), ctx->stream));
    vc_trtri_kernel<<<(unsigned)((n + VB - 1) / VB), 256, VC_DIAG_LDS, ctx->stream>>>(Lm, ldl, n, X, ldx);
    PG_HIP(hipGetLastError());
    for (long long b = VB; b < n; b *= 2) {
        const long long np = (n - b + 2 * b - 1) / (2 * b);                 // pairs whose second block is not empty
        const long long b2 = std::min<long long>(b, n - (2 * (np - 1) * b + b));      // rows of the last pair's second block
        DgemmDesc d;                                                       // T = L21 X11, in O where X21 will be
        d.M = (np == 1) ? b2 : b; d.N = b; d.K = b;
        d.A = Lm + b * ldl; d.lda = ldl; d.B = X; d.ldb = ldx; d.C = O + b * ldo; d.ldc = ldo;
        d.nbatch = (int)np; d.strideA = 2 * b * (ldl + 1); d.strideB = 2 * b * (ldx + 1); d.strideC = 2 * b * (ldo + 1);
        d.M_last = (np == 1) ? 0 : b2; d.allow_splitk = false;
        rc = dgemm_ex(ctx, d);
        if (rc) return rc;
        DgemmDesc e;                                                       // X21 = -X22 T
        e.M = (np == 1) ? b2 : b; e.N = b; e.K = (np == 1) ? b2 : b; e.alpha = -1.0;
        e.A = X + b * (ldx + 1); e.lda = ldx; e.B = O + b * ldo; e.ldb = ldo; e.C = X + b * ldx; e.ldc = ldx;
        e.nbatch = (int)np; e.strideA = 2 * b * (ldx + 1); e.strideB = 2 * b * (ldo + 1); e.strideC = 2 * b * (ldx + 1);
        e.M_last = (np == 1) ? 0 : b2; e.K_last = (np == 1) ? 0 : b2; e.allow_splitk = false;
        rc = dgemm_ex(ctx, e);
        if (rc) return rc;
    }
    DgemmDesc f;                                                           // A^-1 = X'X
    f.transA = true; f.M = n; f.N = n; f.K = n; f.A = X; f.lda = ldx; f.B = X; f.ldb = ldx; f.C = O; f.ldc = ldo;
    f.lower_only = true; f.allow_splitk = false;
    return dgemm_ex(ctx, f);
}

static int vc_trdot(pg_ctx *ctx, long long n, const double *A, long long lda, const void *B, int b_is_f64, long long ldb, double *part, double *out)
{
    const int np = (int)std::min<long long>(n, VC_PART);
    if (b_is_f64) vc_trdot_kernel<double><<<np, 256, 0, ctx->stream>>>(n, A, lda, static_cast<const double *>(B), ldb, part);
    else vc_trdot_kernel<float><<<np, 256, 0, ctx->stream>>>(n, A, lda, static_cast<const float *>(B), ldb, part);
    PG_HIP(hipGetLastError());
    vc_part_sum_kernel<<<1, 256, 0, ctx->stream>>>(np, part, out);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

static int vc_symv(pg_ctx *ctx, long long n, const void *A, int a_is_f64, long long lda, int m, const double *X, long long ldx, double *Y, long long ldy)
{
    const unsigned grid = (unsigned)((n + VB - 1) / VB);
    if (a_is_f64) vc_symv_kernel<double><<<grid, 256, 0, ctx->stream>>>(n, static_cast<const double *>(A), lda, m, X, ldx, Y, ldy);
    else vc_symv_kernel<float><<<grid, 256, 0, ctx->stream>>>(n, static_cast<const float *>(A), lda, m, X, ldx, Y, ldy);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

// out (ma x mb, pitch ldo) = P'Q for panels of any width, 32 x 32 blocks at a time; part: VC_GRAM_WG x 1024 doubles
static int vc_gram(pg_ctx *ctx, long long n, const double *P, long long ldp, int ma, const double *Q, long long ldq, int mb, double *part, double *out, int ldo)
{
    const long long slabs = (n + VB - 1) / VB, nwg = std::min<long long>(slabs, VC_GRAM_WG), rows = (slabs + nwg - 1) / nwg * VB;
    const int used = (int)((n + rows - 1) / rows);
    for (int a0 = 0; a0 < ma; a0 += 32)
        for (int b0 = 0; b0 < mb; b0 += 32) {
            const int wa = std::min(32, ma - a0), wb = std::min(32, mb - b0);
            vc_gram_kernel<<<used, 256, 0, ctx->stream>>>(n, rows, P + a0, ldp, wa, Q + b0, ldq, wb, part);
            PG_HIP(hipGetLastError());
            vc_gram_sum_kernel<<<4, 256, 0, ctx->stream>>>(used, part, wa, wb, out + (size_t)a0 * ldo + b0, ldo);
            PG_HIP(hipGetLastError());
        }
    return PG_OK;
}

// the context's generic scratch: its head holds the partials, `extra` bytes follow.  The GEMM keeps its split-K slabs there too, so
// every product of this unit is launched with allow_splitk = false
static int vc_scratch(pg_ctx *ctx, size_t extra, char **base)
{
    int rc = ensure(ctx, &ctx->scratch, &ctx->scratch_bytes, VC_SMALL + extra + 256);
    if (rc) return rc;
    *base = static_cast<char *>(ctx->scratch);
    return PG_OK;
}
static inline double *vc_trdot_part(char *base) { return reinterpret_cast<double *>(base); }
static inline double *vc_gram_part(char *base) { return reinterpret_cast<double *>(base) + VC_PART; }

// ---- one evaluation --------------------------------------------------------------------------------------------------------------------------

struct VcWork {
    double *W0, *W1, *W2, *Dinv, *PT, *Z, *Qp, *S, *U, *R, *small;
    int *info;
    size_t bytes;
};
constexpr size_t VC_SM_G0 = 128;                           // small: [0] log|V|, [1 + i] tr(V^-1 K_i); the Grams from here, 1024 doubles each
static inline size_t vc_small_len(int k) { return VC_SM_G0 + (size_t)(k + 2) * 1024 + (size_t)(k + 1) * (k + 1); }

static VcWork vc_work(void *work, long long n, int k)
{
    char *b = static_cast<char *>(work);
    const size_t ldw = (size_t)vc_ldw(n), kk = (size_t)k + 1;
    VcWork w;
    size_t o = 0;
    auto take = [&](size_t doubles) { double *p = reinterpret_cast<double *>(b + o); o += up256(doubles * 8); return p; };
    w.W0 = take((size_t)n * ldw); w.W1 = take((size_t)n * ldw); w.W2 = take((size_t)n * ldw);
    w.Dinv = take(VB * VB); w.PT = take(2 * VB * ldw);
    w.Z = take((size_t)n * VC_RHS); w.Qp = take((size_t)n * VC_RHS); w.S = take((size_t)n * VC_RHS);
    w.U = take((size_t)n * kk); w.R = take((size_t)n * kk);
    w.small = take(vc_small_len(k));
    w.info = reinterpret_cast<int *>(b + o); o += 256;
    w.bytes = o;
    return w;
}

// lower Cholesky of the c x c matrix A (row-major, lower read) on the host -> L; false when a pivot is not positive
static bool vc_host_chol(int c, const double *A, double *Lh)
{
    for (int i = 0; i < c; i++)
        for (int j = 0; j <= i; j++) {
            double s = A[i * c + j];
            for (int t = 0; t < j; t++) s -= Lh[i * c + t] * Lh[j * c + t];
            if (i == j) {
                if (!(s > 0.0) || !std::isfinite(s)) return false;
                Lh[i * c + i] = std::sqrt(s);
            } else Lh[i * c + j] = s / Lh[j * c + j];
        }
    return true;
}

// x <- (L L')^-1 x
static void vc_host_solve(int c, const double *Lh, double *x)
{
    for (int i = 0; i < c; i++) {
        double s = x[i];
        for (int t = 0; t < i; t++) s -= Lh[i * c + t] * x[t];
        x[i] = s / Lh[i * c + i];
    }
    for (int i = c - 1; i >= 0; i--) {
        double s = x[i];
        for (int t = i + 1; t < c; t++) s -= Lh[t * c + i] * x[t];
        x[i] = s / Lh[i * c + i];
    }
}

}  // namespace pg

using namespace pg;

extern "C" int pg_vc_combine_dev(pg_ctx *ctx, int64_t n, int k, const void *const *K, const int *k_is_f64, const int64_t *ldk, const double *s, double *V,
                                 int64_t ldv)
{
    PG_REQUIRE(ctx && s && V, "pg_vc_combine_dev: NULL argument");
    const VcMats m{k, K, k_is_f64, ldk};
    int rc = vc_check_mats("pg_vc_combine_dev", n, k, m);
    if (rc) return rc;
    PG_REQUIRE(ldv >= n, "pg_vc_combine_dev: ldv=%lld < n=%lld", (long long)ldv, (long long)n);
    PG_HIP(hipSetDevice(ctx->device));
    return vc_combine(ctx, n, m, s, V, ldv, false);
}

extern "C" int pg_potrf_dev(pg_ctx *ctx, int64_t n, double *A, int64_t lda, int *info_dev)
{
    PG_REQUIRE(ctx && A && info_dev, "pg_potrf_dev: NULL argument");
    PG_REQUIRE(n >= 1 && n < (1LL << 30) && lda >= n, "pg_potrf_dev: bad shape n=%lld lda=%lld", (long long)n, (long long)lda);
    PG_HIP(hipSetDevice(ctx->device));
    const long long ldw = vc_ldw(n);
    char *base;
    int rc = vc_scratch(ctx, ((size_t)n * ldw + VB * VB + (size_t)2 * VB * ldw) * 8 + 512, &base);
    if (rc) return rc;
    double *W = reinterpret_cast<double *>(base + VC_SMALL), *Dinv = W + (size_t)n * ldw, *PT = Dinv + VB * VB;
    PG_HIP(hipMemsetAsync(info_dev, 0, sizeof(int), ctx->stream));
    vc_copy_lower_kernel<<<(unsigned)n, 256, 0, ctx->stream>>>(n, A, lda, W, ldw, 1);
    PG_HIP(hipGetLastError());
    rc = vc_potrf_ws(ctx, n, W, ldw, info_dev, Dinv, PT);
    if (rc) return rc;
    vc_copy_lower_kernel<<<(unsigned)n, 256, 0, ctx->stream>>>(n, W, ldw, A, lda, 0);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

extern "C" int pg_potrf_logdet_dev(pg_ctx *ctx, int64_t n, const double *A, int64_t lda, double *out)
{
    PG_REQUIRE(ctx && A && out, "pg_potrf_logdet_dev: NULL argument");
    PG_REQUIRE(n >= 1 && n < (1LL << 30) && lda >= n, "pg_potrf_logdet_dev: bad shape n=%lld lda=%lld", (long long)n, (long long)lda);
    PG_HIP(hipSetDevice(ctx->device));
    vc_diag_sum_kernel<<<1, 256, 0, ctx->stream>>>(n, A, lda, 0, out);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

extern "C" size_t pg_potri_work_bytes(int64_t n)
{
    if (n < 1 || n >= (1LL << 30)) return 0;
    return 2 * up256((size_t)n * vc_ldw(n) * 8);
}

extern "C" int pg_potri_dev(pg_ctx *ctx, int64_t n, const double *L, int64_t ldl, double *Ainv, int64_t ldi, double *work)
{
    PG_REQUIRE(ctx && L && Ainv && work, "pg_potri_dev: NULL argument");
    PG_REQUIRE(n >= 1 && n < (1LL << 30) && ldl >= n && ldi >= n, "pg_potri_dev: bad shape n=%lld ldl=%lld ldi=%lld", (long long)n, (long long)ldl, (long long)ldi);
    PG_REQUIRE((uintptr_t)work % 16 == 0, "pg_potri_dev: work must be 16-byte aligned");
    PG_HIP(hipSetDevice(ctx->device));
    const long long ldw = vc_ldw(n);
    double *X = work, *O = reinterpret_cast<double *>(reinterpret_cast<char *>(work) + up256((size_t)n * ldw * 8));
    int rc = vc_potri_ws(ctx, n, L, ldl, X, ldw, O, ldw);
    if (rc) return rc;
    vc_copy_lower_kernel<<<(unsigned)n, 256, 0, ctx->stream>>>(n, O, ldw, Ainv, ldi, 0);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

extern "C" int pg_sym_trdot_dev(pg_ctx *ctx, int64_t n, const double *A, int64_t lda, const void *B, int b_is_f64, int64_t ldb, double *out)
{
    PG_REQUIRE(ctx && A && B && out, "pg_sym_trdot_dev: NULL argument");
    PG_REQUIRE(n >= 1 && n < (1LL << 30) && lda >= n && ldb >= n, "pg_sym_trdot_dev: bad shape n=%lld lda=%lld ldb=%lld", (long long)n, (long long)lda, (long long)ldb);
    PG_HIP(hipSetDevice(ctx->device));
    char *base;
    int rc = vc_scratch(ctx, 0, &base);
    if (rc) return rc;
    return vc_trdot(ctx, n, A, lda, B, b_is_f64, ldb, vc_trdot_part(base), out);
}

extern "C" int pg_symv_dev(pg_ctx *ctx, int64_t n, const void *A, int a_is_f64, int64_t lda, int m, const double *X, int64_t ldx, double *Y, int64_t ldy)
{
    PG_REQUIRE(ctx && A && X && Y, "pg_symv_dev: NULL argument");
    PG_REQUIRE(n >= 1 && n < (1LL << 30) && lda >= n, "pg_symv_dev: bad shape n=%lld lda=%lld", (long long)n, (long long)lda);
    PG_REQUIRE(m >= 1 && m <= VC_RHS && ldx >= m && ldy >= m, "pg_symv_dev: m=%d right-hand sides (1 to %d) at ldx=%lld, ldy=%lld", m, VC_RHS, (long long)ldx,
               (long long)ldy);
    PG_HIP(hipSetDevice(ctx->device));
    return vc_symv(ctx, n, A, a_is_f64, lda, m, X, ldx, Y, ldy);
}

extern "C" size_t pg_vc_work_bytes(int64_t n, int k)
{
    if (n < 1 || n >= (1LL << 30) || k < 1 || k > VC_MAXK) return 0;
    return vc_work(nullptr, n, k).bytes;
}

extern "C" int pg_vc_out_len(int k, int c)
{
    if (k < 1 || k > VC_MAXK || c < 1 || c > PG_MAX_COVARIATES) return 0;
    const int kk = k + 1;
    return 4 + 3 * kk + kk * kk + c + c * c;
}

extern "C" int pg_vc_eval_dev(pg_ctx *ctx, int64_t n, int k, int c, const void *const *K, const int *k_is_f64, const int64_t *ldk, const double *sigma,
                              const double *Wy, void *work, double *out, double *Py, int *info)
{
    PG_REQUIRE(ctx && sigma && Wy && work && out && info, "pg_vc_eval_dev: NULL argument");
    const VcMats m{k, K, k_is_f64, ldk};
    int rc = vc_check_mats("pg_vc_eval_dev", n, k, m);
    if (rc) return rc;
    PG_REQUIRE(k >= 1 && c >= 1 && c <= PG_MAX_COVARIATES && n > c, "pg_vc_eval_dev: k=%d, c=%d, n=%lld: k >= 1, 1 <= c <= %d < n", k, c, (long long)n,
               PG_MAX_COVARIATES);
    PG_REQUIRE((uintptr_t)work % 256 == 0, "pg_vc_eval_dev: work must be 256-byte aligned");
    PG_HIP(hipSetDevice(ctx->device));
    const int kk = k + 1, m1 = c + 1, nout = pg_vc_out_len(k, c);
    const long long ldw = vc_ldw(n);
    const VcWork w = vc_work(work, n, k);
    char *base;
    rc = vc_scratch(ctx, 0, &base);
    if (rc) return rc;
    double *tpart = vc_trdot_part(base), *gpart = vc_gram_part(base);
    hipStream_t st = ctx->stream;
    for (int t = 0; t < nout; t++) out[t] = std::nan("");
    *info = 0;

    // V, its factor, log|V|
    rc = vc_combine(ctx, n, m, sigma, w.W0, ldw, true);
    if (rc) return rc;
    PG_HIP(hipMemsetAsync(w.info, 0, sizeof(int), st));
    rc = vc_potrf_ws(ctx, n, w.W0, ldw, w.info, w.Dinv, w.PT);
    if (rc) return rc;
    PG_HIP(hipMemcpyAsync(info, w.info, sizeof(int), hipMemcpyDeviceToHost, st));
    PG_HIP(hipStreamSynchronize(st));
    if (*info != 0) return PG_OK;                          // V is not positive definite here: the caller shortens its step
    vc_diag_sum_kernel<<<1, 256, 0, st>>>(n, w.W0, ldw, 0, w.small);
    PG_HIP(hipGetLastError());
    // V^-1, tr(V^-1 K_i), V^-1 [W y] and [W y]' V^-1 [W y]
    rc = vc_potri_ws(ctx, n, w.W0, ldw, w.W1, ldw, w.W2, ldw);
    if (rc) return rc;
    for (int t = 0; t < k; t++) {
        rc = vc_trdot(ctx, n, w.W2, ldw, K[t], k_is_f64[t], ldk[t], tpart, w.small + 1 + t);
        if (rc) return rc;
    }
    vc_diag_sum_kernel<<<1, 256, 0, st>>>(n, w.W2, ldw, 1, w.small + 1 + k);
    PG_HIP(hipGetLastError());
    rc = vc_symv(ctx, n, w.W2, 1, ldw, m1, Wy, m1, w.Z, VC_RHS);
    if (rc) return rc;
    double *G0 = w.small + VC_SM_G0;
    rc = vc_gram(ctx, n, Wy, m1, m1, w.Z, VC_RHS, m1, gpart, G0, 32);
    if (rc) return rc;
    std::vector<double> sm(vc_small_len(k));
    PG_HIP(hipMemcpyAsync(sm.data(), w.small, (VC_SM_G0 + 1024) * 8, hipMemcpyDeviceToHost, st));
    PG_HIP(hipStreamSynchronize(st));
    // the c x c pieces on the host
    std::vector<double> xvx((size_t)c * c), lh((size_t)c * c, 0.0), xvxinv((size_t)c * c, 0.0), beta(c);
    for (int a = 0; a < c; a++)
        for (int b = 0; b < c; b++) xvx[a * c + b] = sm[VC_SM_G0 + (a >= b ? a * 32 + b : b * 32 + a)];
    if (!vc_host_chol(c, xvx.data(), lh.data())) {
        set_error("pg_vc_eval_dev: W'V^-1 W is not positive definite (the %d covariates are collinear)", c);
        return PG_EINVAL;
    }
    double ldxvx = 0.0;
    for (int a = 0; a < c; a++) ldxvx += std::log(lh[a * c + a]);
    ldxvx *= 2.0;
    for (int a = 0; a < c; a++) beta[a] = sm[VC_SM_G0 + a * 32 + c];
    double yviy = sm[VC_SM_G0 + c * 32 + c], bty = 0.0;
    std::vector<double> xvy(beta);
    vc_host_solve(c, lh.data(), beta.data());
    for (int a = 0; a < c; a++) bty += xvy[a] * beta[a];
    for (int b = 0; b < c; b++) {
        std::vector<double> e(c, 0.0);
        e[b] = 1.0;
        vc_host_solve(c, lh.data(), e.data());
        for (int a = 0; a < c; a++) xvxinv[a * c + b] = e[a];
    }
    const double ypy = yviy - bty, ldv = sm[0];
    // P y, u_i = K_i P y (u_k = P y), the Grams of [V^-1 W, P y] with K_i [V^-1 W, P y], R = V^-1 U and U'R
    VcPyArgs pa{};
    pa.n = n; pa.c = c; pa.kk = kk; pa.Z = w.Z; pa.Qp = w.Qp; pa.U = w.U; pa.Py = Py;
    for (int a = 0; a < c; a++) pa.beta[a] = beta[a];
    const unsigned nb = (unsigned)((n + 255) / 256);
    vc_py_kernel<<<nb, 256, 0, st>>>(pa);
    PG_HIP(hipGetLastError());
    for (int t = 0; t < k; t++) {
        rc = vc_symv(ctx, n, K[t], k_is_f64[t], ldk[t], m1, w.Qp, VC_RHS, w.S, VC_RHS);
        if (rc) return rc;
        vc_column_kernel<<<nb, 256, 0, st>>>(n, w.S + c, VC_RHS, w.U + t, kk);
        PG_HIP(hipGetLastError());
        rc = vc_gram(ctx, n, w.Qp, VC_RHS, m1, w.S, VC_RHS, m1, gpart, G0 + (size_t)(1 + t) * 1024, 32);
        if (rc) return rc;
    }
    rc = vc_gram(ctx, n, w.Qp, VC_RHS, m1, w.Qp, VC_RHS, m1, gpart, G0 + (size_t)(1 + k) * 1024, 32);
    if (rc) return rc;
    for (int t0 = 0; t0 < kk; t0 += VC_RHS) {
        rc = vc_symv(ctx, n, w.W2, 1, ldw, std::min(VC_RHS, kk - t0), w.U + t0, kk, w.R + t0, kk);
        if (rc) return rc;
    }
    double *UR = G0 + (size_t)(k + 2) * 1024;
    rc = vc_gram(ctx, n, w.U, kk, kk, w.R, kk, kk, gpart, UR, kk);
    if (rc) return rc;
    PG_HIP(hipMemcpyAsync(sm.data(), w.small, sm.size() * 8, hipMemcpyDeviceToHost, st));
    PG_HIP(hipStreamSynchronize(st));
    // assembly
    double *score = out + 4, *AI = score + kk, *obeta = AI + kk * kk, *oinv = obeta + c, *trpk = oinv + c * c, *ypkpy = trpk + kk;
    std::vector<double> zu((size_t)kk * c), hz((size_t)kk * c);             // Zw'u_i and (X'V^-1 X)^-1 Zw'u_i
    for (int t = 0; t < kk; t++) {
        const double *Gt = sm.data() + VC_SM_G0 + (size_t)(1 + t) * 1024;
        double tr = 0.0;
        for (int a = 0; a < c; a++)
            for (int b = 0; b < c; b++) tr += xvxinv[a * c + b] * Gt[b * 32 + a];
        trpk[t] = sm[1 + t] - tr;
        ypkpy[t] = Gt[c * 32 + c];
        score[t] = -0.5 * (trpk[t] - ypkpy[t]);
        for (int a = 0; a < c; a++) zu[t * c + a] = Gt[a * 32 + c];
    }
    for (int t = 0; t < kk; t++)
        for (int a = 0; a < c; a++) {
            double s = 0.0;
            for (int b = 0; b < c; b++) s += xvxinv[a * c + b] * zu[t * c + b];
            hz[t * c + a] = s;
        }
    const double *URh = sm.data() + VC_SM_G0 + (size_t)(k + 2) * 1024;
    for (int i = 0; i < kk; i++)
        for (int j = 0; j <= i; j++) {                     // one value for (i, j) and (j, i): the matrix is symmetric to the bit
            double s = 0.0, t = 0.0;
            for (int a = 0; a < c; a++) { s += zu[i * c + a] * hz[j * c + a]; t += zu[j * c + a] * hz[i * c + a]; }
            AI[i * kk + j] = AI[j * kk + i] = 0.5 * (0.5 * (URh[i * kk + j] + URh[j * kk + i]) - 0.5 * (s + t));
        }
    out[0] = -0.5 * (ldv + ldxvx + ypy);
    out[1] = ldv;
    out[2] = ldxvx;
    out[3] = ypy;
    for (int a = 0; a < c; a++) obeta[a] = beta[a];
    for (int t = 0; t < c * c; t++) oinv[t] = xvxinv[t];
    return PG_OK;
}
