// DP-SGD's Gaussian mechanism drawn from the ChaCha20 keystream and applied to the gradient in one pass:
//     g[i] = (g[i] + sigma * z[i]) * inv_batch,   z ~ N(0, 1), never written to memory.
//
// The pair it replaces (torch.randn + primia_dp_add_noise) draws z from a Philox generator seeded by the command line;
// the privacy guarantee of the Gaussian mechanism rests on z being unpredictable, exactly as additive sharing rests on
// the provider's masks (chacha.hip), so z comes from the same cipher under a key from the operating system's entropy pool.
//
// The noise is DEFINED by this arithmetic (tests/dp_noise_ref.py is its float64 form):
//   element i lives in ChaCha20 block B = (counter ? *counter : 0) + block_offset + i / 16, output words x[0..15];
//   for p = (i % 16) / 2:  a = x[2p], c = x[2p + 1]   (low / high half of 64-bit keystream word 8B + p)
//     u1 = ((a >> 8) + 1) * 2^-24 in (0, 1],   u2 = (c >> 8) * 2^-24 in [0, 1),   r = sqrtf(-2 logf(u1))
//     even i: r * cos(2 pi u2),   odd i: r * sin(2 pi u2)      (precise float32 functions; sincospif(2 u2) is exact
//                                                               in its argument)
// 24-bit uniforms truncate the tail at sqrt(-2 ln 2^-24) = sqrt(48 ln 2) = 5.77 standard deviations — the same class as the
// float generator it replaces; not a statement about floating-point attacks on the Gaussian mechanism.
//
// One thread = one 64-byte block = 16 gradient elements, read and written as four 16-byte accesses; a workgroup covers
// 4096 elements.  (The other mapping measured — four lanes per block, 16 bytes each, every lane computing the block —
// is tools/micro/dp_noise_mapping.hip; profiles/dp_noise.txt has both.)
#include "dp_noise_core.h"

namespace primia {

// ACC = false: primia_dp_noise_add as described above (`acc` is not read).  ACC = true (primia_dp_noise_add_acc: the last
// pass of a step cut into micro-batches, primia_amd/dp_micro.py) adds the clipped sums of the earlier passes in front.
// The body is dp_noise_core.h's, shared with the kernels that read the clipping norm from the device (dp_clip.hip).
template <bool ACC>
__global__ __launch_bounds__(256) void dp_noise_add_kernel(ChaChaKey key, uint64_t block0, const uint64_t* __restrict__ counter,
                                                           float* __restrict__ g, const float* __restrict__ acc, int64_t n,
                                                           float sigma, float inv_b) {
    dp_noise_add_block<ACC>(key, block0, counter, g, acc, n, sigma, inv_b);
}

// The clipped sum of one micro-batch pass into the step's fp32 accumulator: acc = g (the first pass) or acc += g.  One
// HBM-bound pass: a thread moves four 16-byte chunks 4 KiB apart (a wave's access is 1 KiB contiguous), every load issued
// before the first store; the n % 4 elements behind the last whole chunk go through scalar accesses of block 0.
template <bool OVERWRITE>
__global__ __launch_bounds__(256) void dp_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g, int64_t n) {
    const int64_t n4 = n >> 2;
    const int64_t base = (int64_t)blockIdx.x * 1024 + threadIdx.x;      // in 16-byte chunks
    const f32x4* g4 = (const f32x4*)g;
    f32x4* a4 = (f32x4*)acc;
    f32x4 v[4], w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t i = base + u * 256;
        if (i < n4) {
            v[u] = g4[i];
            if (!OVERWRITE) w[u] = a4[i];
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t i = base + u * 256;
        if (i < n4) a4[i] = OVERWRITE ? v[u] : w[u] + v[u];
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t j = n4 * 4 + threadIdx.x;
        acc[j] = OVERWRITE ? g[j] : acc[j] + g[j];
    }
}

}  // namespace primia

using namespace primia;

extern "C" int64_t primia_dp_noise_blocks(int64_t n) { return n <= 0 ? 0 : (n + 15) / 16; }

extern "C" int primia_dp_noise_add(uint64_t k0, uint64_t k1, uint64_t k2, uint64_t k3, uint64_t nonce,
                                   const uint64_t* counter, uint64_t block_offset, float* g, int64_t n, float sigma,
                                   float inv_batch, primia_stream_t st) {
    if (n == 0) return PRIMIA_OK;  // empty input: no-op, pointers may be null
    PRIMIA_REQUIRE(g && n > 0 && ((uintptr_t)g & 15) == 0);
    const ChaChaKey key = chacha_key(k0, k1, k2, k3, nonce);
    const int64_t blocks = primia_dp_noise_blocks(n);
    dp_noise_add_kernel<false><<<ceil_div(blocks, 256), 256, 0, (hipStream_t)st>>>(key, block_offset, counter, g, nullptr, n,
                                                                                   sigma, inv_batch);
    return launch_status();
}

extern "C" int primia_dp_noise_add_acc(uint64_t k0, uint64_t k1, uint64_t k2, uint64_t k3, uint64_t nonce,
                                       const uint64_t* counter, uint64_t block_offset, float* g, const float* acc, int64_t n,
                                       float sigma, float inv_batch, primia_stream_t st) {
    if (n == 0) return PRIMIA_OK;  // empty input: no-op, pointers may be null
    PRIMIA_REQUIRE(g && acc && n > 0 && ((uintptr_t)g & 15) == 0 && ((uintptr_t)acc & 15) == 0);
    const ChaChaKey key = chacha_key(k0, k1, k2, k3, nonce);
    const int64_t blocks = primia_dp_noise_blocks(n);
    dp_noise_add_kernel<true><<<ceil_div(blocks, 256), 256, 0, (hipStream_t)st>>>(key, block_offset, counter, g, acc, n,
                                                                                  sigma, inv_batch);
    return launch_status();
}

extern "C" int primia_dp_accumulate(float* acc, const float* g, int64_t n, int overwrite, primia_stream_t st) {
    if (n == 0) return PRIMIA_OK;  // empty input: no-op, pointers may be null
    PRIMIA_REQUIRE(acc && g && n > 0 && ((uintptr_t)acc & 15) == 0 && ((uintptr_t)g & 15) == 0);
    const int grid = ceil_div(n >> 2, 1024) > 0 ? ceil_div(n >> 2, 1024) : 1;      // (n < 4: the scalar tail alone)
    if (overwrite)
        dp_accumulate_kernel<true><<<grid, 256, 0, (hipStream_t)st>>>(acc, g, n);
    else
        dp_accumulate_kernel<false><<<grid, 256, 0, (hipStream_t)st>>>(acc, g, n);
    return launch_status();
}
