// DP-SGD with an adaptive clipping norm C held in a device word (quantile-based adaptive clipping: Andrew, Thakkar,
// McMahan, Ramaswamy, NeurIPS 2021; primia_amd/dp_clip.py).
//
// A C that moves every step cannot be a launch argument: a captured training step (graphed_train) freezes its launch
// arguments, so C is read from memory by the kernels that need it and written by the one that moves it:
//   * dp_clip_factors_dev_kernel: the clip factors of dp_clip_factor_kernel / dp_clip_factor_masked_kernel with
//     max_norm = *clip_norm, and the two counts the update releases — below = #{valid n : sq_n <= C^2}, valid;
//   * dp_noise_add_dev_kernel / dp_add_noise_dev_kernel: sigma = noise_multiplier * *clip_norm as one float32 product in
//     front of the arithmetic of dp_noise_core.h / common.h;
//   * dp_clip_update_kernel: C' = clamp(C * exp(-eta * (b - gamma)), c_min, c_max) with b = (below - valid / 2 +
//     sigma_b * z0) / B + 1 / 2, float64 inside, rounded once; z0 is given, or element 0 of a block of the noise stream.
#include "dp_noise_core.h"

#include <cmath>

namespace primia {

// ONE block walks the batch (a DP-SGD batch is at most a few thousand samples): per-thread counts, a wave reduction, then
// the four waves' counts through LDS, added in a fixed order by thread 0.  No atomics: the counts are a pure function of
// the inputs, and the step stays bitwise reproducible.
__global__ __launch_bounds__(256) void dp_clip_factors_dev_kernel(const double* __restrict__ sq, const int64_t* __restrict__ target,
                                                                  float* __restrict__ clip, int N,
                                                                  const float* __restrict__ clip_norm,
                                                                  int32_t* __restrict__ counts, int overwrite) {
    const float c = *clip_norm;
    const double c2 = (double)c * (double)c;
    int below = 0, valid = 0;
    for (int n = threadIdx.x; n < N; n += 256) {
        const bool ok = target == nullptr || target[n] >= 0;
        const double s = sq[n];
        clip[n] = ok ? dp_clip_factor(s, c) : 0.f;
        valid += ok ? 1 : 0;
        below += (ok && s <= c2) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        below += __shfl_xor(below, o, 64);
        valid += __shfl_xor(valid, o, 64);
    }
    __shared__ int sh_below[4], sh_valid[4];
    if ((threadIdx.x & 63) == 0) {
        sh_below[threadIdx.x >> 6] = below;
        sh_valid[threadIdx.x >> 6] = valid;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int b = sh_below[0] + sh_below[1] + sh_below[2] + sh_below[3];
        const int v = sh_valid[0] + sh_valid[1] + sh_valid[2] + sh_valid[3];
        counts[0] = overwrite ? b : counts[0] + b;
        counts[1] = overwrite ? v : counts[1] + v;
    }
}

template <bool ACC>
__global__ __launch_bounds__(256) void dp_noise_add_dev_kernel(ChaChaKey key, uint64_t block0, const uint64_t* __restrict__ counter,
                                                               float* __restrict__ g, const float* __restrict__ acc, int64_t n,
                                                               const float* __restrict__ clip_norm, float noise_multiplier,
                                                               float inv_b) {
    const float sigma = noise_multiplier * *clip_norm;
    dp_noise_add_block<ACC>(key, block0, counter, g, acc, n, sigma, inv_b);
}

// (grid and loop of gn.hip's dp_noise_kernel / dp_noise_acc_kernel)
template <bool ACC>
__global__ __launch_bounds__(256) void dp_add_noise_dev_kernel(float* __restrict__ g, const float* __restrict__ acc,
                                                               const float* __restrict__ noise, long n,
                                                               const float* __restrict__ clip_norm, float noise_multiplier,
                                                               float inv_b) {
    const float sigma = noise_multiplier * *clip_norm;
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        g[i] = dp_noise_apply(ACC ? acc[i] + g[i] : g[i], noise[i], sigma, inv_b);
}

struct ClipUpdate {
    float sigma_b, inv_batch, eta, gamma, c_min, c_max;
};

// The geometric update on the released fraction.  NaN (a non-finite z0 from a host tensor) and an underflowed product go
// to c_min, an overflowed one to c_max: the stored C is always inside [c_min, c_max], whose ends are float32 values.
__device__ __forceinline__ void dp_clip_update_apply(float* clip_norm, const int32_t* counts, float z0, const ClipUpdate& u,
                                                     float* released) {
    const double s = ((double)counts[0] - 0.5 * (double)counts[1]) + (double)u.sigma_b * (double)z0;
    const double b = s * (double)u.inv_batch + 0.5;
    double c = (double)*clip_norm * exp(-(double)u.eta * (b - (double)u.gamma));
    if (!(c >= (double)u.c_min)) c = (double)u.c_min;
    if (c > (double)u.c_max) c = (double)u.c_max;
    *clip_norm = (float)c;
    if (released) *released = (float)b;
}

__global__ void dp_clip_update_kernel(float* clip_norm, const int32_t* counts, const float* z, ClipUpdate u, float* released) {
    if (threadIdx.x == 0) dp_clip_update_apply(clip_norm, counts, *z, u, released);
}

__global__ void dp_clip_update_chacha_kernel(ChaChaKey key, uint64_t block0, const uint64_t* counter, float* clip_norm,
                                             const int32_t* counts, ClipUpdate u, float* released) {
    if (threadIdx.x != 0) return;
    float z[16];
    dp_noise_block(key, block0 + (counter ? *counter : 0), z);
    dp_clip_update_apply(clip_norm, counts, z[0], u, released);
}

static inline bool clip_update_ok(float sigma_b, float inv_batch, float eta, float gamma, float c_min, float c_max) {
    return std::isfinite(sigma_b) && std::isfinite(inv_batch) && std::isfinite(eta) && std::isfinite(gamma) &&
           std::isfinite(c_min) && std::isfinite(c_max) && sigma_b > 0.f && inv_batch > 0.f && eta >= 0.f && gamma > 0.f &&
           gamma < 1.f && c_min > 0.f && c_min <= c_max;
}

}  // namespace primia

using namespace primia;

extern "C" int primia_dp_clip_factors_dev(const double* sq, const int64_t* target, float* clip, int N, const float* clip_norm,
                                          int32_t* counts, int overwrite, primia_stream_t st) {
    PRIMIA_REQUIRE(sq && clip && clip_norm && counts && N > 0);
    dp_clip_factors_dev_kernel<<<1, 256, 0, (hipStream_t)st>>>(sq, target, clip, N, clip_norm, counts, overwrite);
    return launch_status();
}

extern "C" int primia_dp_noise_add_dev(uint64_t k0, uint64_t k1, uint64_t k2, uint64_t k3, uint64_t nonce,
                                       const uint64_t* counter, uint64_t block_offset, float* g, const float* acc, int64_t n,
                                       const float* clip_norm, float noise_multiplier, float inv_batch, primia_stream_t st) {
    if (n == 0) return PRIMIA_OK;  // empty input: no-op, pointers may be null
    PRIMIA_REQUIRE(g && clip_norm && n > 0 && ((uintptr_t)g & 15) == 0 && ((uintptr_t)acc & 15) == 0);
    const ChaChaKey key = chacha_key(k0, k1, k2, k3, nonce);
    const int grid = ceil_div(primia_dp_noise_blocks(n), 256);
    if (acc)
        dp_noise_add_dev_kernel<true><<<grid, 256, 0, (hipStream_t)st>>>(key, block_offset, counter, g, acc, n, clip_norm,
                                                                        noise_multiplier, inv_batch);
    else
        dp_noise_add_dev_kernel<false><<<grid, 256, 0, (hipStream_t)st>>>(key, block_offset, counter, g, nullptr, n, clip_norm,
                                                                         noise_multiplier, inv_batch);
    return launch_status();
}

extern "C" int primia_dp_add_noise_dev(float* g, const float* acc, const float* noise, int64_t n, const float* clip_norm,
                                       float noise_multiplier, float inv_batch, primia_stream_t st) {
    if (n == 0) return PRIMIA_OK;  // empty input: no-op, pointers may be null
    PRIMIA_REQUIRE(g && noise && clip_norm && n > 0);
    const long b = (n + 255) / 256;
    const int grid = (int)(b > 4096 ? 4096 : b);
    if (acc)
        dp_add_noise_dev_kernel<true><<<grid, 256, 0, (hipStream_t)st>>>(g, acc, noise, n, clip_norm, noise_multiplier,
                                                                        inv_batch);
    else
        dp_add_noise_dev_kernel<false><<<grid, 256, 0, (hipStream_t)st>>>(g, nullptr, noise, n, clip_norm, noise_multiplier,
                                                                         inv_batch);
    return launch_status();
}

extern "C" int primia_dp_clip_update(float* clip_norm, const int32_t* counts, const float* z, float sigma_b, float inv_batch,
                                     float eta, float gamma, float c_min, float c_max, float* released,
                                     primia_stream_t st) {
    PRIMIA_REQUIRE(clip_norm && counts && z && clip_update_ok(sigma_b, inv_batch, eta, gamma, c_min, c_max));
    const ClipUpdate u = {sigma_b, inv_batch, eta, gamma, c_min, c_max};
    dp_clip_update_kernel<<<1, 64, 0, (hipStream_t)st>>>(clip_norm, counts, z, u, released);
    return launch_status();
}

extern "C" int primia_dp_clip_update_chacha(uint64_t k0, uint64_t k1, uint64_t k2, uint64_t k3, uint64_t nonce,
                                            const uint64_t* counter, uint64_t block_offset, float* clip_norm,
                                            const int32_t* counts, float sigma_b, float inv_batch, float eta, float gamma,
                                            float c_min, float c_max, float* released, primia_stream_t st) {
    PRIMIA_REQUIRE(clip_norm && counts && clip_update_ok(sigma_b, inv_batch, eta, gamma, c_min, c_max));
    const ChaChaKey key = chacha_key(k0, k1, k2, k3, nonce);
    const ClipUpdate u = {sigma_b, inv_batch, eta, gamma, c_min, c_max};
    dp_clip_update_chacha_kernel<<<1, 64, 0, (hipStream_t)st>>>(key, block_offset, counter, clip_norm, counts, u, released);
    return launch_status();
}
