// The DEFINITION of DP-SGD's device noise and the one pass that applies it, shared by the entry points that take sigma as
// a host float (dp_noise.hip) and the ones that form it from a clipping norm held on the device (dp_clip.hip).  The
// arithmetic is described at the top of dp_noise.hip; tests/dp_noise_ref.py is its float64 form.
#pragma once
#include "chacha_block.h"

namespace primia {

// Box-Muller on one 64-bit keystream word (a = low half, c = high half)
__device__ __forceinline__ void dp_noise_pair(uint32_t a, uint32_t c, float& z_even, float& z_odd) {
    const float u1 = (float)((a >> 8) + 1u) * 0x1p-24f;      // integers <= 2^24: both conversions are exact
    const float u2 = (float)(c >> 8) * 0x1p-24f;
    const float r = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincospif(2.0f * u2, &sn, &cs);
    z_even = r * cs;
    z_odd = r * sn;
}

// z[0..15] = the 16 standard normal values of ChaCha20 block `ctr`: what every consumer of the stream reads
__device__ __forceinline__ void dp_noise_block(const ChaChaKey& key, uint64_t ctr, float (&z)[16]) {
    uint32_t x[16];
    chacha20_block(key, ctr, x);
#pragma unroll
    for (int p = 0; p < 8; ++p) dp_noise_pair(x[2 * p], x[2 * p + 1], z[2 * p], z[2 * p + 1]);
}

// One thread = one 64-byte block = 16 gradient elements: g = (g + z * sigma) * inv_b.  ACC = true reads a second,
// read-only arena `acc` and the expression gets v = acc + g in front: g = ((acc + g) + z * sigma) * inv_b, the same
// rounding as ACC = false applied to the float32 sum.  The acc loads are issued with the g loads.
template <bool ACC>
__device__ __forceinline__ void dp_noise_add_block(const ChaChaKey& key, uint64_t block0, const uint64_t* __restrict__ counter,
                                                   float* __restrict__ g, const float* __restrict__ acc, int64_t n,
                                                   float sigma, float inv_b) {
    const int64_t blk = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (blk * 16 >= n) return;
    float* o = g + blk * 16;
    const float* a = ACC ? acc + blk * 16 : nullptr;
    const bool full = blk * 16 + 16 <= n;
    f32x4 v[4], w[4];
    if (full) {     // issued before the 20 rounds: their latency hides behind the integer work
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = *(const f32x4*)(o + 4 * i);
        if (ACC) {
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] = *(const f32x4*)(a + 4 * i);
        }
    }
    const uint64_t ctr = block0 + (counter ? *counter : 0) + (uint64_t)blk;
    float z[16];
    dp_noise_block(key, ctr, z);
    if (full) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (ACC) v[i] = w[i] + v[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[i][j] = dp_noise_apply(v[i][j], z[4 * i + j], sigma, inv_b);
            *(f32x4*)(o + 4 * i) = v[i];
        }
    } else {        // the partial last block: its first n % 16 values
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (blk * 16 + i < n) {
                const float vi = ACC ? a[i] + o[i] : o[i];
                o[i] = dp_noise_apply(vi, z[i], sigma, inv_b);
            }
    }
}

}  // namespace primia
