// NumPy's legacy generator on the GPU: the float64 stream of np.random.RandomState(seed).random_sample, bit for bit.
//
// What it replaces: F.elastic_transform of albumentations 0.4.6 draws its two displacement fields with
// `random_state.rand(h, w)` — 2 x 224 x 224 doubles per image from a RandomState seeded with a Python integer, so far drawn
// on the host and copied to the device (800 KB per firing image).  The stream is MT19937 seeded by init_genrand; a double
// takes two tempered 32-bit outputs a, b: ((a >> 5) * 2^26 + (b >> 6)) / 2^53.
//
// MT19937 as a stream: x[0..623] is the seeded state, x[n] = x[n-227] ^ twist(x[n-624], x[n-623]), output n = temper(x[624+n]).
// Words x[n .. n+226] depend only on words before x[n], so a STEP computes 227 words in parallel.  Two steps are 454 words =
// 227 doubles, so a ROUND (step, barrier, step, barrier, temper + convert + store 227 doubles) never splits a double.
//
// One workgroup per seed; the state is a ring of 1024 words in LDS (word x[n] at slot n & 1023), nothing of it goes to global
// memory.  A step overwrites the slots of x[n-1024 .. n-798]: the recurrence reads no further back than x[n-624], and the
// round before has converted every word it produced, so no barrier is needed between a round's stores and the next step.
// Integer arithmetic is 32-bit; the conversion is exact in float64 (a * 2^26 + b < 2^53, and 2^-53 is a scaling).
#include "common.h"

namespace primia {

constexpr int kMtN = 624, kMtStep = 227, kMtRing = 1024;
constexpr int kMtThreads = 256;

__device__ __forceinline__ uint32_t mt_twist(uint32_t u, uint32_t v) {
    const uint32_t y = (u & 0x80000000u) | (v & 0x7fffffffu);
    return (y >> 1) ^ ((v & 1u) ? 0x9908b0dfu : 0u);
}

__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    return y ^ (y >> 18);
}

// words x[base .. base+226] from the words before them (base: x index mod 2^32, which keeps the slot)
template <int T>
__device__ __forceinline__ void mt_step(uint32_t* ring, uint32_t base, int tid) {
    for (int t = tid; t < kMtStep; t += T) {
        const uint32_t n = base + t;
        ring[n & (kMtRing - 1)] = ring[(n - kMtStep) & (kMtRing - 1)] ^
                                  mt_twist(ring[(n - kMtN) & (kMtRing - 1)], ring[(n - kMtN + 1) & (kMtRing - 1)]);
    }
    __syncthreads();
}

// T threads per generator (a multiple of 64): 256 runs a step on four SIMDs at once, 64 runs it as four passes of one wave
template <int T>
__global__ __launch_bounds__(T) void mt19937_fields_kernel(const uint32_t* __restrict__ seeds, int64_t skip, int64_t count,
                                                           double* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint32_t ring[kMtRing];
    const int tid = threadIdx.x;
    if (tid == 0) {                                         // init_genrand: 623 dependent steps
        uint32_t v = seeds[blockIdx.x];
        ring[0] = v;
        for (uint32_t i = 1; i < kMtN; ++i) {
            v = 1812433253u * (v ^ (v >> 30)) + i;
            ring[i] = v;
        }
    }
    __syncthreads();
    double* row = out + (int64_t)blockIdx.x * count;
    const int64_t end = skip + count;                        // doubles [skip, end) of the stream are the row
    uint32_t base = kMtN;
    for (int64_t d0 = 0; d0 < end; d0 += kMtStep, base += 2 * kMtStep) {
        mt_step<T>(ring, base, tid);
        mt_step<T>(ring, base + kMtStep, tid);
        if (d0 + kMtStep <= skip) continue;                  // (uniform: a round wholly inside the skipped prefix)
        for (int t = tid; t < kMtStep; t += T) {
            const int64_t d = d0 + t;
            const u32x2 w = *(const u32x2*)&ring[(base + 2 * t) & (kMtRing - 1)];      // base even: the pair is 8-byte aligned
            const uint32_t a = mt_temper(w[0]) >> 5, b = mt_temper(w[1]) >> 6;
            const double v = ((double)a * 67108864.0 + (double)b) * (1.0 / 9007199254740992.0);
            if (d >= skip && d < end) row[d - skip] = v;
        }
    }
}

}  // namespace primia

using namespace primia;

extern "C" int primia_mt19937_fields_batch(const uint32_t* seeds, int n, int64_t skip, int64_t count, double* out,
                                           primia_stream_t st) {
    if (n == 0) return PRIMIA_OK;
    PRIMIA_REQUIRE(seeds && out && n > 0 && n <= PRIMIA_BATCH_MAX / 2 && skip >= 0 && count > 0 && skip <= INT64_MAX - count &&
                   ((uintptr_t)out & 7) == 0 && ((uintptr_t)seeds & 3) == 0);
    mt19937_fields_kernel<kMtThreads><<<n, kMtThreads, 0, (hipStream_t)st>>>(seeds, skip, count, out);
    return launch_status();
}
