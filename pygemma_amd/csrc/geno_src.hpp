// geno_src.hpp — the three ways a batch of genotypes reaches a kernel, and the one fork from an array's (dtype, snp_major) to the kernel's
// <T, LAYOUT>.  An entry point checks its own arguments first (dtype_known; what it returns for an unknown dtype is its own contract, see
// pygemma_hip.h) and decides its own alignment rules.
#pragma once
#include "common.hpp"

namespace pg {

// packed .bed records (T = unsigned char) | (n x pb) sample-major array | (pb x n) SNP-major array
enum { GENO_BED = 0, GENO_SAMPLE = 1, GENO_SNP = 2 };

static inline bool dtype_known(int dtype) { return dtype >= PG_DTYPE_INT8 && dtype <= PG_DTYPE_FLOAT64; }

template <class T, int LAYOUT> struct GenoSrc {
    typedef T type;
    static constexpr int layout = LAYOUT;
};

// f(GenoSrc<T, LAYOUT>()) for an array of a known dtype:  [&](auto src) { using S = decltype(src); return launch<typename S::type, S::layout>(...); }
template <class F> static inline int geno_dispatch(int dtype, bool snp_major, F &&f)
{
    switch (dtype) {
        case PG_DTYPE_INT8: return snp_major ? f(GenoSrc<signed char, GENO_SNP>()) : f(GenoSrc<signed char, GENO_SAMPLE>());
        case PG_DTYPE_UINT8: return snp_major ? f(GenoSrc<unsigned char, GENO_SNP>()) : f(GenoSrc<unsigned char, GENO_SAMPLE>());
        case PG_DTYPE_FLOAT32: return snp_major ? f(GenoSrc<float, GENO_SNP>()) : f(GenoSrc<float, GENO_SAMPLE>());
        default: return snp_major ? f(GenoSrc<double, GENO_SNP>()) : f(GenoSrc<double, GENO_SAMPLE>());
    }
}

}  // namespace pg
