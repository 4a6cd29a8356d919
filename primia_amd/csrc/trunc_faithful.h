// The faithful truncation of a shared product ("Truncation that cannot wrap"; defined in
// tests/secure_faithful_nets.py): what csrc/ring.hip's chain and csrc/secure_local.hip's fused forms share, so that both
// compute one arithmetic.
//
// Shares z_0 + z_1 = z (mod 2^64) with |z| < 2^62.  u_0 = z_0 + 2^62, u_1 = z_1 share z + 2^62 in [0, 2^63), so the carry of
// u_0 + u_1 is w = m_0 OR m_1 with m_j = u_j >> 63, and  out_j = u_j / d (unsigned) - w_j q64 - [j = 0] q62  with
// q64 = floor(2^64 / d), q62 = floor(2^62 / d) is floor(z / d) + e, e in {-1, 0, 1, 2}, for EVERY mask.
#pragma once
#include <stdint.h>

namespace primia {

struct FaithDiv {
    unsigned long long d, magic, q64, q62;
};

// d in [1, 2^62); false otherwise.  magic = floor(2^64 / d) (2^64 - 1 for d = 1): see faith_udiv.
static inline bool faith_div_make(int64_t div, FaithDiv* f) {
    if (div <= 0 || div >= ((int64_t)1 << 62)) return false;
    const unsigned long long d = (unsigned long long)div, all = ~0ULL;
    f->d = d;
    f->q64 = d == 1 ? 0 : all / d + (all % d == d - 1 ? 1 : 0);      // floor(2^64 / d) mod 2^64
    f->q62 = (1ULL << 62) / d;
    f->magic = d == 1 ? all : f->q64;
    return true;
}

// floor(u / d) for every u < 2^64 without a 64-bit division: with M = floor(2^64 / d), u M / 2^64 <= u / d and
// u / d - u M / 2^64 = u (2^64 / d - M) / 2^64 < 1, so the high word of u M is floor(u / d) or one less, and one comparison
// of the remainder settles it.  (d = 1: M = 2^64 - 1 gives u - 1 for u > 0, corrected the same way.)
__device__ __forceinline__ unsigned long long faith_udiv(unsigned long long u, const FaithDiv& f) {
    unsigned long long q = __umul64hi(u, f.magic);
    if (u - q * f.d >= f.d) ++q;
    return q;
}

// party j's output share from its u_j and its share w_j of the carry
__device__ __forceinline__ unsigned long long faith_finish(int j, unsigned long long u, unsigned long long w, const FaithDiv& f) {
    return faith_udiv(u, f) - w * f.q64 - (j == 0 ? f.q62 : 0ULL);
}

}  // namespace primia
