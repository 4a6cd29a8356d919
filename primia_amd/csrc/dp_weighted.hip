// DP-SGD with class weights (primia_amd/dp_weights.py): the per-sample weighted loss gradient and
// the one-off noised release of the per-class record counts the weights are formed from.
//
// nn.CrossEntropyLoss(weight = w) divides by the sum of the weights of the batch (`den` in xent_kernel, pool_fc_loss.hip).
// Under DP-SGD that would make every sample's gradient a function of which other samples were drawn, and a record would
// no longer be bounded by its own clipped gradient.  The DP form is per sample, loss_n = w[y_n] * CE_n, with the
// normalisation of w fixed before training (balanced_weights: equal counts give w = 1); what is clipped is
// w[y_n] * scale * (softmax - onehot), scale = 1 / views.
//
// The weights themselves come from counts of private records, so the counts are released ONCE through a Gaussian
// mechanism: counts_out[c] = max(0, rint(count_c + sigma * z_c)), z from the caller or from one block of the client's
// ChaCha20 noise stream through dp_noise_block, the function that defines every z of primia_dp_noise_add.
#include "dp_noise_core.h"

#include <cmath>

namespace primia {

constexpr int kCountClasses = 16;       // one block of the noise stream holds 16 values (kMaxClasses of pool_fc_loss.hip)

// One block as xent_hard_masked_kernel (dp_sample.hip): the softmax in fp64, each dlogits element rounded once, counts and
// sums through a wave64 shuffle and LDS in a fixed order.  No atomics: a pure function of its inputs.
__global__ __launch_bounds__(256) void xent_dp_weighted_kernel(const float* __restrict__ logits,
                                                               const int64_t* __restrict__ target,
                                                               const float* __restrict__ class_weight, float scale,
                                                               float* __restrict__ loss, float* __restrict__ dlogits, int N,
                                                               int C) {
    __shared__ double sh_num[4];
    __shared__ int sh_cnt[4];
    double num = 0.0;
    int cnt = 0;
    for (int n = threadIdx.x; n < N; n += 256) {
        const float* o = logits + (long)n * C;
        float* d = dlogits ? dlogits + (long)n * C : nullptr;
        const int64_t t = target[n];
        if (t < 0) {                            // padding
            if (d)
                for (int c = 0; c < C; ++c) d[c] = 0.f;
            continue;
        }
        ++cnt;
        if (t >= C) {                           // as primia_xent_hard: poison instead of reading out of bounds
            num = __builtin_nan("");
            if (d)
                for (int c = 0; c < C; ++c) d[c] = __builtin_nanf("");
            continue;
        }
        const double w = (double)class_weight[t];
        const double ws = w * (double)scale;
        double mx = o[0];
        for (int c = 1; c < C; ++c) mx = fmax(mx, (double)o[c]);
        double se = 0.0;
        for (int c = 0; c < C; ++c) se += exp((double)o[c] - mx);
        num += w * (mx + log(se) - (double)o[t]);
        if (d)
            for (int c = 0; c < C; ++c) d[c] = (float)(ws * (exp((double)o[c] - mx) / se - (c == (int)t ? 1.0 : 0.0)));
    }
    num = wave_sum(num);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0) {
        sh_num[threadIdx.x >> 6] = num;
        sh_cnt[threadIdx.x >> 6] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int valid = sh_cnt[0] + sh_cnt[1] + sh_cnt[2] + sh_cnt[3];
        const double s = sh_num[0] + sh_num[1] + sh_num[2] + sh_num[3];
        loss[0] = valid ? (float)(s / valid) : 0.f;
    }
}

// One block: the histogram in LDS (integer atomics: the counts do not depend on their order), then thread c < C releases
// class c.  CHACHA: z is block block0 + *counter of the noise stream, drawn by thread 0 while the others count.
template <bool CHACHA>
__global__ __launch_bounds__(256) void dp_class_counts_kernel(ChaChaKey key, uint64_t block0,
                                                              const uint64_t* __restrict__ counter,
                                                              const int64_t* __restrict__ targets, int64_t n, int C,
                                                              const float* __restrict__ z, float sigma,
                                                              int64_t* __restrict__ counts_out) {
    __shared__ unsigned long long hist[kCountClasses];
    __shared__ float sh_z[kCountClasses];
    const int tid = threadIdx.x;
    if (tid < kCountClasses) {
        hist[tid] = 0ull;
        if (!CHACHA) sh_z[tid] = (z && tid < C) ? z[tid] : 0.f;
    }
    if (CHACHA && tid == 0) {
        float zz[16];
        dp_noise_block(key, block0 + (counter ? *counter : 0), zz);
#pragma unroll
        for (int i = 0; i < 16; ++i) sh_z[i] = zz[i];
    }
    __syncthreads();
    for (int64_t i = tid; i < n; i += 256) {
        const int64_t t = targets[i];
        if (t >= 0 && t < C) atomicAdd(&hist[t], 1ull);
    }
    __syncthreads();
    if (tid < C) {
        const double v = rint((double)hist[tid] + (double)sigma * (double)sh_z[tid]);
        counts_out[tid] = v > 0.0 ? (int64_t)v : 0;      // (a NaN z releases 0)
    }
}

}  // namespace primia

using namespace primia;

extern "C" int primia_xent_dp_weighted(const float* logits, const int64_t* target, const float* class_weight, float scale,
                                       float* loss, float* dlogits, int N, int C, primia_stream_t st) {
    PRIMIA_REQUIRE(logits && target && class_weight && loss && N > 0 && C > 0);
    PRIMIA_REQUIRE(std::isfinite(scale) && scale > 0.f);
    xent_dp_weighted_kernel<<<1, 256, 0, (hipStream_t)st>>>(logits, target, class_weight, scale, loss, dlogits, N, C);
    return launch_status();
}

static inline bool class_counts_ok(const int64_t* targets, int64_t n, int C, float sigma, const int64_t* counts_out) {
    return counts_out && (targets || n == 0) && n >= 0 && C > 0 && C <= kCountClasses && std::isfinite(sigma) && sigma >= 0.f;
}

extern "C" int primia_dp_class_counts(const int64_t* targets, int64_t n, int C, const float* z, float sigma,
                                      int64_t* counts_out, primia_stream_t st) {
    PRIMIA_REQUIRE(class_counts_ok(targets, n, C, sigma, counts_out));
    dp_class_counts_kernel<false><<<1, 256, 0, (hipStream_t)st>>>(ChaChaKey{}, 0, nullptr, targets, n, C, z, sigma,
                                                                  counts_out);
    return launch_status();
}

extern "C" int primia_dp_class_counts_chacha(uint64_t k0, uint64_t k1, uint64_t k2, uint64_t k3, uint64_t nonce,
                                             const uint64_t* counter, uint64_t block_offset, const int64_t* targets,
                                             int64_t n, int C, float sigma, int64_t* counts_out, primia_stream_t st) {
    PRIMIA_REQUIRE(class_counts_ok(targets, n, C, sigma, counts_out));
    const ChaChaKey key = chacha_key(k0, k1, k2, k3, nonce);
    dp_class_counts_kernel<true><<<1, 256, 0, (hipStream_t)st>>>(key, block_offset, counter, targets, n, C, nullptr, sigma,
                                                                 counts_out);
    return launch_status();
}
