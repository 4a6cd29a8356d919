// DP-SGD with Poisson-sampled batches: the sampler, the gather into a fixed-capacity batch, and the two kernels of the
// step that know about padded slots.
//
// The sampled-Gaussian RDP bound (primia_amd/dp_accountant.py) holds for batches in which every record takes part
// independently with probability q, by a draw nobody can predict.  The loaders this replaces shuffle with torch.randperm
// seeded from the command line.  Here record i of n reads one 64-bit word of a ChaCha20 keystream keyed from the
// operating system's entropy pool and joins the batch iff word < threshold = floor(q * 2^64).  A Poisson batch changes
// size at every step; the step's buffers and its captured graph do not: the batch has `capacity` slots, the selected
// records fill the first ones in ascending order, and the rest are PADDING — index -1, a zero image, target -1 — which
// the masked loss and clip kernels below turn into a zero dlogits row and a zero clip factor, so that a padded slot
// contributes exactly nothing to the clipped sum.
//
// primia_poisson_select is ONE workgroup of 1024 threads walking n in chunks of 8192 records: thread t of a chunk
// computes one ChaCha20 block = 8 records; positions come from a stable scan of per-lane counts (a lane holds 8 records,
// so its count is the popcount of its 8-bit selection mask where a one-record-per-lane kernel would take a wave ballot;
// lane prefix by shuffles, wave totals through LDS, the running base carried in a register by every thread), so the
// output is a pure function of the arguments — no atomic decides a position.  Selection is latency- not bandwidth-work
// (n is a hospital's record count: thousands), and a single workgroup needs no second launch and no inter-workgroup
// hand-off.
#include "chacha_block.h"

namespace primia {

constexpr int kSelThreads = 1024;
constexpr int kSelWaves = kSelThreads / 64;

__global__ __launch_bounds__(kSelThreads) void poisson_select_kernel(ChaChaKey key, uint64_t block0,
                                                                     const uint64_t* __restrict__ counter,
                                                                     uint64_t threshold, int64_t n, int capacity,
                                                                     int64_t* __restrict__ idx, int32_t* __restrict__ count,
                                                                     uint64_t* __restrict__ overflow_events) {
    __shared__ int wave_tot[2][kSelWaves];      // double-buffered: one barrier per chunk
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t first = block0 + (counter ? *counter : 0);
    const int64_t nblocks = (n + 7) / 8;
    int64_t base = 0;                           // records selected in earlier chunks: the same value in every thread
    int buf = 0;
    for (int64_t c0 = 0; c0 < nblocks; c0 += kSelThreads, buf ^= 1) {
        const int64_t blk = c0 + tid;
        uint32_t mask = 0;
        if (blk < nblocks) {
            uint32_t x[16];
            chacha20_block(key, first + (uint64_t)blk, x);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint64_t w = (uint64_t)x[2 * j] | ((uint64_t)x[2 * j + 1] << 32);
                if (blk * 8 + j < n && w < threshold) mask |= 1u << j;
            }
        }
        const int mine = __popc(mask);
        int incl = mine;                        // inclusive prefix over the wave's lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (lane == 63) wave_tot[buf][wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kSelWaves; ++w) {
            const int t = wave_tot[buf][w];
            if (w < wave) before += t;
            total += t;
        }
        int64_t pos = base + before + (incl - mine);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (mask & (1u << j)) {
                if (pos < capacity) idx[pos] = blk * 8 + j;
                ++pos;
            }
        }
        base += total;
    }
    const int64_t kept = base < capacity ? base : capacity;
    for (int64_t s = kept + tid; s < capacity; s += kSelThreads) idx[s] = -1;
    if (tid == 0) {
        count[0] = (int32_t)base;
        count[1] = (int32_t)kept;
        if (base > capacity) *overflow_events += 1;     // the only writer: one workgroup, one thread
    }
}

// One 16-byte chunk per thread and step; a slot's chunks are split over `parts` blocks.  Output slot o = s * views + v is
// row base + ((first_walk + v) % repetitions) * n_rows + idx[s] of `data`: view v of record idx[s] among `repetitions`
// stored walks of n_rows rows — or, with one walk and one view, row idx[s] of the split that starts at `base`.
__global__ __launch_bounds__(256) void gather_rows_kernel(const u32x4* __restrict__ data, int64_t row_chunks,
                                                          int64_t n_rows, const int64_t* __restrict__ targets,
                                                          const int64_t* __restrict__ idx, int64_t base,
                                                          int64_t first_walk, int repetitions, int views,
                                                          u32x4* __restrict__ out, int64_t* __restrict__ out_targets,
                                                          int parts) {
    const int o = blockIdx.x / parts, part = blockIdx.x % parts;
    const int s = o / views, v = o - s * views;
    const int64_t r = idx[s];
    const bool valid = r >= 0 && r < n_rows;    // everything else is padding: nothing is read
    const int64_t row = base + ((first_walk + v) % repetitions) * n_rows + r;
    u32x4* dst = out + (int64_t)o * row_chunks;
    const int64_t c0 = (int64_t)part * 256 + threadIdx.x, step = (int64_t)parts * 256;
    if (valid) {
        const u32x4* src = data + row * row_chunks;
        for (int64_t c = c0; c < row_chunks; c += step) dst[c] = src[c];
    } else {
        const u32x4 zero = {0u, 0u, 0u, 0u};
        for (int64_t c = c0; c < row_chunks; c += step) dst[c] = zero;
    }
    if (part == 0 && threadIdx.x == 0) out_targets[o] = valid ? targets[row] : -1;
}

// clip_slots[n] = clip[n / views]: a record's clip factor on each of its slots
__global__ void dp_expand_clip_kernel(const float* __restrict__ clip, float* __restrict__ clip_slots, int N, int views) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n < N) clip_slots[n] = clip[n / views];
}

// Cross entropy over the valid rows (target >= 0) of a padded batch, single block as xent_kernel (pool_fc_loss.hip).
// Rows are a handful of classes wide and N is a batch size, so the softmax is formed in fp64 and rounded once: a valid
// dlogits row is the fp32 rounding of softmax - onehot, the per-sample loss gradient DP-SGD clips.
__global__ __launch_bounds__(256) void xent_hard_masked_kernel(const float* __restrict__ logits,
                                                               const int64_t* __restrict__ target, float* __restrict__ loss,
                                                               float* __restrict__ dlogits, int N, int C) {
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
        double mx = o[0];
        for (int c = 1; c < C; ++c) mx = fmax(mx, (double)o[c]);
        double se = 0.0;
        for (int c = 0; c < C; ++c) se += exp((double)o[c] - mx);
        num += mx + log(se) - (double)o[t];
        if (d)
            for (int c = 0; c < C; ++c) d[c] = (float)(exp((double)o[c] - mx) / se - (c == (int)t ? 1.0 : 0.0));
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

__global__ void dp_clip_factor_masked_kernel(const double* __restrict__ sq, const int64_t* __restrict__ target,
                                             float* __restrict__ clip, int N, float max_norm) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    clip[n] = target[n] < 0 ? 0.f : dp_clip_factor(sq[n], max_norm);      // dp_clip_factor_kernel's expression (common.h)
}

}  // namespace primia

using namespace primia;

extern "C" int64_t primia_poisson_blocks(int64_t n) { return n <= 0 ? 0 : (n + 7) / 8; }

extern "C" int primia_poisson_select(uint64_t k0, uint64_t k1, uint64_t k2, uint64_t k3, uint64_t nonce,
                                     const uint64_t* counter, uint64_t block_offset, uint64_t threshold, int64_t n,
                                     int capacity, int64_t* idx, int32_t* count, uint64_t* overflow_events,
                                     primia_stream_t st) {
    PRIMIA_REQUIRE(idx && count && overflow_events && n >= 0 && n <= INT32_MAX && capacity > 0);
    const ChaChaKey key = chacha_key(k0, k1, k2, k3, nonce);
    poisson_select_kernel<<<1, kSelThreads, 0, (hipStream_t)st>>>(key, block_offset, counter, threshold, n, capacity, idx,
                                                                   count, overflow_events);
    return launch_status();
}

static int gather_rows(const void* data, int64_t row_elems, int64_t n_rows, const int64_t* targets, const int64_t* idx,
                       int64_t base, int64_t first_walk, int repetitions, int views, void* out, int64_t* out_targets,
                       int capacity, int dtype, primia_stream_t st) {
    PRIMIA_REQUIRE(data && targets && idx && out && out_targets);
    PRIMIA_REQUIRE(row_elems > 0 && n_rows >= 0 && base >= 0 && first_walk >= 0 && repetitions >= 1 && views >= 1 &&
                   capacity > 0);
    PRIMIA_REQUIRE(dtype == PRIMIA_F32 || dtype == PRIMIA_BF16);
    const int64_t per_chunk = dtype == PRIMIA_F32 ? 4 : 8;
    PRIMIA_REQUIRE(row_elems % per_chunk == 0 && ((uintptr_t)data & 15) == 0 && ((uintptr_t)out & 15) == 0);
    const int64_t row_chunks = row_elems / per_chunk;
    int64_t parts = (row_chunks + 1023) / 1024;      // four chunks per thread where the row is long enough
    if (parts > 64) parts = 64;
    PRIMIA_REQUIRE((int64_t)capacity * views * parts <= INT32_MAX);
    gather_rows_kernel<<<(unsigned)(capacity * views * parts), 256, 0, (hipStream_t)st>>>(
        (const u32x4*)data, row_chunks, n_rows, targets, idx, base, first_walk, repetitions, views, (u32x4*)out,
        out_targets, (int)parts);
    return launch_status();
}

extern "C" int primia_gather_batch(const void* data, int64_t row_elems, int64_t n_rows, const int64_t* targets,
                                   const int64_t* idx, int64_t row_offset, void* out, int64_t* out_targets, int capacity,
                                   int dtype, primia_stream_t st) {
    return gather_rows(data, row_elems, n_rows, targets, idx, row_offset, 0, 1, 1, out, out_targets, capacity, dtype, st);
}

extern "C" int primia_gather_records(const void* data, int64_t row_elems, int64_t n_rows, const int64_t* targets,
                                     const int64_t* idx, int64_t first_walk, int repetitions, int views, void* out,
                                     int64_t* out_targets, int capacity, int dtype, primia_stream_t st) {
    return gather_rows(data, row_elems, n_rows, targets, idx, 0, first_walk, repetitions, views, out, out_targets,
                       capacity, dtype, st);
}

extern "C" int primia_dp_expand_clip(const float* clip, float* clip_slots, int N, int views, primia_stream_t st) {
    PRIMIA_REQUIRE(clip && clip_slots && N > 0 && views >= 1 && N % views == 0);
    dp_expand_clip_kernel<<<(N + 255) / 256, 256, 0, (hipStream_t)st>>>(clip, clip_slots, N, views);
    return launch_status();
}

extern "C" int primia_xent_hard_masked(const float* logits, const int64_t* target, float* loss, float* dlogits, int N,
                                       int C, primia_stream_t st) {
    PRIMIA_REQUIRE(logits && target && loss && N > 0 && C > 0);
    xent_hard_masked_kernel<<<1, 256, 0, (hipStream_t)st>>>(logits, target, loss, dlogits, N, C);
    return launch_status();
}

extern "C" int primia_dp_clip_factors_masked(const double* sq, const int64_t* target, float* clip, int N,
                                             float max_grad_norm, primia_stream_t st) {
    PRIMIA_REQUIRE(sq && target && clip && N > 0 && max_grad_norm > 0.f);
    dp_clip_factor_masked_kernel<<<(N + 255) / 256, 256, 0, (hipStream_t)st>>>(sq, target, clip, N, max_grad_norm);
    return launch_status();
}
