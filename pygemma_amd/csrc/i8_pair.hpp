// i8_pair.hpp — the 256 x 256 int8 pair tile that ld_pair_kernel and king_pair_kernel share: 512 threads as 4 x 2 waves
// of 64 (A rows) x 128 (B rows), v_mfma_i32_16x16x64_i8, K-tiles of 128 bytes in XOR-swizzled 128-byte LDS rows filled by global_load_lds,
// two buffers, and the accumulators released through LDS one 128-row half of A at a time.  A kernel keeps its own prologue (which rows of
// which planes are the operands: srcA, srcB) and its own epilogue (what becomes of the staged sums).
// rotate_geno_i8_kernel is NOT built from these pieces: its loop is scheduled differently (A and B staged apart, fragments held across
// phases, saddr DMA), and only the LDS image — swizzle, row pitch, staging pitch — is the same.
#pragma once
#include "common.hpp"

#include <atomic>

namespace pg {

typedef int intx4 __attribute__((ext_vector_type(4)));

constexpr int I8P_BK = 128;                 // bytes of K per K-tile: one LDS row
constexpr int I8P_TBUF = 256 * I8P_BK;      // one operand's K-tile
// words per staged accumulator row: the 4 row groups of a store (rows 4 apart) x 16 columns fall on 64 different banks
constexpr int I8P_LDW = 260;
constexpr int I8P_LDS = 128 * I8P_LDW * 4 > 4 * I8P_TBUF ? 128 * I8P_LDW * 4 : 4 * I8P_TBUF;      // dynamic LDS of a pair kernel

// The dynamic LDS of a pair kernel: the two buffers of both operands' K-tiles and, over the same bytes, the staged half of the sums.  The
// pieces below name it themselves, and take the lane geometry by value: with the LDS handed in as a pointer and the geometry by
// reference, the compiler's address arithmetic in the loop came out without its inbounds / no-wrap facts, and KING's pair kernel measured
// 0.3 - 0.5 % slower than with the loop written out in the kernel (two alternations; a process differs from the next by about as much).
// In this form the optimised IR is the written-out loop's but for block order, and it measures level (profiles/i8_pair_refactor.json).
extern __shared__ __attribute__((aligned(1024))) unsigned char i8p_lds[];
__device__ __forceinline__ int *i8p_staged() { return reinterpret_cast<int *>(i8p_lds); }

// the 16-byte chunk of LDS row `row` that holds chunk `chunk` of the K-tile
__device__ __forceinline__ int i8p_swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

struct I8pLane {
    int wave, lane;
    int wm, wn;                 // the wave's place among the 4 x 2
    int lrow, lchunk;           // DMA: a wave instruction fills 8 rows of 8 chunks
    int chunk0;                 // MFMA: the lane's chunk of a 64-byte K-step
};
__device__ __forceinline__ I8pLane i8p_lane()
{
    const int tid = threadIdx.x;
    I8pLane g;
    g.wave = __builtin_amdgcn_readfirstlane(tid >> 6); g.lane = tid & 63;
    g.wm = g.wave >> 1; g.wn = g.wave & 1;
    g.lrow = g.lane >> 3; g.lchunk = g.lane & 7; g.chunk0 = g.lane >> 4;
    return g;
}
// DMA sources: a lane stages its row of the four 8-row strips t of the wave's 32 rows, either operand.  src[t] = the first byte of the
// operand's row i8p_src_row(g, t), plus i8p_src_byte(g, row): the lane reads the chunk that belongs at its place of the swizzled LDS row.
__device__ __forceinline__ int i8p_src_row(const I8pLane g, int t) { return g.wave * 32 + 8 * t + g.lrow; }
__device__ __forceinline__ int i8p_src_byte(const I8pLane g, int row) { return i8p_swz(row, g.lchunk) * 16; }

__device__ __forceinline__ void i8p_zero(intx4 (&acc)[4][8])
{
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 8; j++)
#pragma unroll
            for (int e = 0; e < 4; e++) acc[i][j][e] = 0;
}

// acc += A B' over KT K-tiles: all eight waves stage their 32 rows of both operands of K-tile kt + 1, wait for their own loads of K-tile
// kt, meet at a barrier and issue the 64 MFMAs of their 64 x 128 quarter.  Every row of srcA, srcB must be readable over KT * 128 bytes.
__device__ __forceinline__ void i8p_products(const I8pLane g, const signed char *(&srcA)[4], const signed char *(&srcB)[4], int KT,
                                             intx4 (&acc)[4][8])
{
    unsigned char *const lds = i8p_lds;
    const int lane = g.lane;
    auto dma = [&](int stage) {
        unsigned char *dA = lds + (stage & 1) * 2 * I8P_TBUF + (g.wave * 32) * 128, *dB = dA + I8P_TBUF;
        const size_t k = (size_t)stage * I8P_BK;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(srcA[t] + k),
                                             (__attribute__((address_space(3))) void *)(dA + 8 * t * 128), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(srcB[t] + k),
                                             (__attribute__((address_space(3))) void *)(dB + 8 * t * 128), 16, 0, 0);
        }
    };
    dma(0);
    for (int kt = 0; kt < KT; kt++) {
        if (kt + 1 < KT) { dma(kt + 1); asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); }
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                  // K-tile kt of every wave has landed
        const unsigned char *Acur = lds + (kt & 1) * 2 * I8P_TBUF, *Bcur = Acur + I8P_TBUF;
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            intx4 fa[4], fb[8];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int row = g.wm * 64 + i * 16 + (lane & 15);
                fa[i] = *reinterpret_cast<const intx4 *>(Acur + row * 128 + i8p_swz(row, 4 * ks + g.chunk0) * 16);
            }
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int row = g.wn * 128 + j * 16 + (lane & 15);
                fb[j] = *reinterpret_cast<const intx4 *>(Bcur + row * 128 + i8p_swz(row, 4 * ks + g.chunk0) * 16);
            }
#pragma unroll
            for (int j = 0; j < 8; j++)
#pragma unroll
                for (int i = 0; i < 4; i++) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();                                  // every wave has read buffer kt & 1: stage kt + 2 may overwrite it
    }
}

// rows [128 half, 128 half + 128) of the tile to i8p_staged(), 256 sums a row at pitch I8P_LDW, and the barrier after which every thread may
// read them.  The caller puts a barrier behind its reads: the next half, or the next tile's DMA, overwrites the same LDS.
__device__ __forceinline__ void i8p_stage(const I8pLane g, int half, const intx4 (&acc)[4][8])
{
    int *const stg = i8p_staged();
    if ((g.wm >> 1) == half) {
        const int rb = (g.wm & 1) * 64;
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 8; j++)
#pragma unroll
                for (int e = 0; e < 4; e++)
                    stg[(rb + i * 16 + 4 * (g.lane >> 4) + e) * I8P_LDW + g.wn * 128 + j * 16 + (g.lane & 15)] = acc[i][j][e];
    }
    __syncthreads();
}

// raises Kernel's dynamic-LDS limit to I8P_LDS (or to Bytes, for a kernel that keeps something of its own behind the tile), once per device
template <auto Kernel, int Bytes = I8P_LDS> static hipError_t i8p_lds_limit(int device)
{
    static std::atomic<unsigned long long> done{0};
    const unsigned long long bit = 1ULL << (device & 63);
    if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, Bytes);
    if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
    return e;
}

}  // namespace pg
