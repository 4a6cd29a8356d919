// The ChaCha20 block function, shared by the keystream kernel (chacha.hip) and the DP-SGD noise kernel (dp_noise.hip).
//
// State layout of the original ChaCha20: constants in words 0-3, the 256-bit key in 4-11, a 64-bit block counter in
// 12-13, a 64-bit nonce in 14-15; with counter < 2^32 the block equals RFC 8439's for the nonce (word13, word14, word15).
#pragma once
#include "common.h"

namespace primia {

__device__ __forceinline__ uint32_t rotl32(uint32_t v, int c) { return (v << c) | (v >> (32 - c)); }

#define PRIMIA_QR(a, b, c, d) \
    a += b; d ^= a; d = rotl32(d, 16); \
    c += d; b ^= c; b = rotl32(b, 12); \
    a += b; d ^= a; d = rotl32(d, 8);  \
    c += d; b ^= c; b = rotl32(b, 7);

struct ChaChaKey {
    uint32_t k[8];
    uint32_t n[2];
};

// key k0..k3 as little-endian 64-bit words, 64-bit nonce: what every entry point of the C ABI takes
static inline ChaChaKey chacha_key(uint64_t k0, uint64_t k1, uint64_t k2, uint64_t k3, uint64_t nonce) {
    ChaChaKey key;
    const uint64_t kk[4] = {k0, k1, k2, k3};
    for (int i = 0; i < 4; ++i) {
        key.k[2 * i] = (uint32_t)kk[i];
        key.k[2 * i + 1] = (uint32_t)(kk[i] >> 32);
    }
    key.n[0] = (uint32_t)nonce;
    key.n[1] = (uint32_t)(nonce >> 32);
    return key;
}

// x[0..15] = the 16 output words of block `ctr` (64 bytes of keystream, little-endian)
__device__ __forceinline__ void chacha20_block(const ChaChaKey& key, uint64_t ctr, uint32_t (&x)[16]) {
    const uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u,
                            key.k[0], key.k[1], key.k[2], key.k[3], key.k[4], key.k[5], key.k[6], key.k[7],
                            (uint32_t)ctr, (uint32_t)(ctr >> 32), key.n[0], key.n[1]};   // 12,13 counter; 14,15 nonce
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = s[i];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        PRIMIA_QR(x[0], x[4], x[8], x[12])
        PRIMIA_QR(x[1], x[5], x[9], x[13])
        PRIMIA_QR(x[2], x[6], x[10], x[14])
        PRIMIA_QR(x[3], x[7], x[11], x[15])
        PRIMIA_QR(x[0], x[5], x[10], x[15])
        PRIMIA_QR(x[1], x[6], x[11], x[12])
        PRIMIA_QR(x[2], x[7], x[8], x[13])
        PRIMIA_QR(x[3], x[4], x[9], x[14])
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] += s[i];
}

}  // namespace primia
