// Thread mappings of the DP-SGD noise kernel (primia_amd/csrc/dp_noise.hip) against each other, at the gradient arena's size.
//
//   block   : one lane = one ChaCha20 block = 64 contiguous bytes of g (four 16-byte accesses, 64 bytes apart between
//             lanes) — the library's kernel, included below, not copied
//   quarter : one lane = one 16-byte quarter of a block: a wave's access is 1 KiB contiguous, but the four lanes of a
//             block each run the 20 rounds (4x the integer work) and keep two of the eight Box-Muller pairs
//
// Build:  hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/micro/dp_noise_mapping.hip -o tools/micro/dp_noise_mapping
// Run:    tools/micro/dp_noise_mapping [n = 11178051] [rounds = 20] [calls per round = 50]
// Prints the median and the range over the rounds of the time per call (device events around `calls` back-to-back
// launches, the two mappings alternating round by round), and whether the two mappings produce the same bits.
#include "../../primia_amd/csrc/dp_noise.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace primia {

__global__ __launch_bounds__(256) void dp_noise_add_quarter_kernel(ChaChaKey key, uint64_t block0,
                                                                   const uint64_t* __restrict__ counter, float* __restrict__ g,
                                                                   int64_t n, float sigma, float inv_b) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;     // 16-byte quarter = 4 elements
    if (q * 4 >= n) return;
    float* o = g + q * 4;
    const bool full = q * 4 + 4 <= n;
    f32x4 v;
    if (full) v = *(const f32x4*)o;
    const uint64_t ctr = block0 + (counter ? *counter : 0) + (uint64_t)(q >> 2);
    uint32_t x[16];
    chacha20_block(key, ctr, x);
    const int part = (int)(q & 3);
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = part == 0 ? x[j] : part == 1 ? x[4 + j] : part == 2 ? x[8 + j] : x[12 + j];
    float z[4];
    dp_noise_pair(w[0], w[1], z[0], z[1]);
    dp_noise_pair(w[2], w[3], z[2], z[3]);
    if (full) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (v[j] + z[j] * sigma) * inv_b;
        *(f32x4*)o = v;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (q * 4 + j < n) o[j] = (o[j] + z[j] * sigma) * inv_b;
    }
}

}  // namespace primia

#define CHECK(e)                                                                        \
    do {                                                                                \
        hipError_t err_ = (e);                                                          \
        if (err_ != hipSuccess) {                                                       \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(err_)); \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

int main(int argc, char** argv) {
    const int64_t n = argc > 1 ? atoll(argv[1]) : 11178051;
    const int rounds = argc > 2 ? atoi(argv[2]) : 20, calls = argc > 3 ? atoi(argv[3]) : 50;
    if (n <= 0 || rounds <= 0 || calls <= 0) return 2;
    const ChaChaKey key = chacha_key(0x0706050403020100ull, 0x0f0e0d0c0b0a0908ull, 0x1716151413121110ull,
                                     0x1f1e1d1c1b1a1918ull, 0x4a00000000ull);
    const size_t bytes = (size_t)((n + 15) / 16 * 16) * sizeof(float);
    float *ga, *gb;
    CHECK(hipMalloc(&ga, bytes));
    CHECK(hipMalloc(&gb, bytes));
    auto launch = [&](int which, float* g, float inv_b) {
        if (which == 0)
            dp_noise_add_kernel<false><<<ceil_div((n + 15) / 16, 256), 256>>>(key, 7, nullptr, g, nullptr, n, 1.3f, inv_b);
        else
            dp_noise_add_quarter_kernel<<<ceil_div((n + 3) / 4, 256), 256>>>(key, 7, nullptr, g, n, 1.3f, inv_b);
    };
    // same bits?
    CHECK(hipMemset(ga, 0, bytes));
    CHECK(hipMemset(gb, 0, bytes));
    launch(0, ga, 0.125f);
    launch(1, gb, 0.125f);
    CHECK(hipDeviceSynchronize());
    std::vector<uint32_t> ha(n), hb(n);
    CHECK(hipMemcpy(ha.data(), ga, (size_t)n * 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(hb.data(), gb, (size_t)n * 4, hipMemcpyDeviceToHost));
    int64_t diff = 0;
    for (int64_t i = 0; i < n; ++i) diff += ha[i] != hb[i];
    printf("n = %lld: %lld elements differ between the two mappings\n", (long long)n, (long long)diff);
    // time per call; inv_b = 0.5 keeps g bounded over thousands of calls
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    std::vector<float> t[2];
    for (int r = -2; r < rounds; ++r)       // two warm-up rounds
        for (int which = 0; which < 2; ++which) {
            CHECK(hipEventRecord(e0));
            for (int c = 0; c < calls; ++c) launch(which, ga, 0.5f);
            CHECK(hipEventRecord(e1));
            CHECK(hipEventSynchronize(e1));
            float ms;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            if (r >= 0) t[which].push_back(ms * 1000.0f / calls);
        }
    CHECK(hipGetLastError());
    const char* names[2] = {"block   (one lane = 64 bytes)", "quarter (one lane = 16 bytes)"};
    for (int which = 0; which < 2; ++which) {
        std::sort(t[which].begin(), t[which].end());
        const float med = t[which][t[which].size() / 2];
        printf("%s: median %.1f us per call (min %.1f, max %.1f; %d rounds x %d calls), %.0f GB/s of g read + written\n",
               names[which], med, t[which].front(), t[which].back(), rounds, calls, 2.0 * n * 4 / med * 1e-3);
    }
    return diff != 0;
}
