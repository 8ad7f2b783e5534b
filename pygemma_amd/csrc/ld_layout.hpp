// ld_layout.hpp — where the planes and the per-SNP totals of an LD image lie (csrc/ld.hip writes it, csrc/epistasis.hip reads it).
#pragma once
#include "i8_pair.hpp"

namespace pg {

constexpr int LD_BK = I8P_BK;     // samples per K-tile

struct LdLayout {
    long long ldk;
    size_t plane, totals, total;
};
static LdLayout ld_layout(long long n, long long pe)
{
    LdLayout L;
    L.ldk = (n + LD_BK - 1) / LD_BK * LD_BK;
    L.plane = (size_t)pe * L.ldk;
    L.totals = (3 * L.plane + 255) & ~(size_t)255;
    L.total = L.totals + (size_t)pe * 16 + 256;
    return L;
}

}  // namespace pg
