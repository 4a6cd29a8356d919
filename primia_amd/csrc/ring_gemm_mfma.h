// Z_2^64 GEMM on int8 MFMA limbs (ring_gemm_mfma.hip; DESIGN.md §7, "Z_2^64 GEMM on int8 MFMA limbs"): what the launchers of
// ring.hip and secure_local.hip share with the kernel's file.
#pragma once
#include "common.h"

namespace primia {

typedef unsigned long long u64;

// one party's sum C = C0 + A1 @ B1 + A2 @ B2 (A2 / B2 and C0 optional; C0 may be C)
struct RingMfmaSide {
    const u64 *A1, *B1, *A2, *B2, *C0;
    u64* C;
};

// gridDim.z = parties * ksplit: block z serves side[z / ksplit], k in [slice * kchunk, min(K, (slice + 1) * kchunk))
struct RingMfmaArgs {
    RingMfmaSide side[2];
    int M, K, N, ksplit, kchunk;
};

constexpr int kRmStep = 64;        // k per step: one v_mfma_i32_16x16x64_i8 per limb pair and fragment pair
// An i32 accumulator of diagonal 7 gains up to 8 * 2^14 per k: it holds 2^31 / 2^17 = 16,384 k.  A slice sums its pairs into
// the same accumulators, so it covers at most 255 steps (16,320 k) with one pair and 127 steps (2 * 8,128 k) with two.
constexpr int kRmMaxSteps = 255;

// The launcher's split for this kernel: slices of whole steps (the last may be short), no slice over the accumulator bound
// -- ksplit rises when K alone demands it -- and no empty slice.
inline void ring_mfma_slices(int K, int pairs, int* ksplit, int* kchunk) {
    const int steps = (K + kRmStep - 1) / kRmStep, cap = kRmMaxSteps / pairs;
    int per = (steps + *ksplit - 1) / *ksplit;
    if (per > cap) per = cap;
    *ksplit = (steps + per - 1) / per;
    *kchunk = per * kRmStep;
}

// ---- device functions the limb kernels share (ring_gemm_mfma.hip, ring_conv_mfma.hip) ----------------------------------
typedef int rm_v4i __attribute__((ext_vector_type(4)));

// 4 x 4 byte transpose: o_i byte r = a_r byte i (up to the fixed order of r that both operands share)
__device__ __forceinline__ void rm_t4(unsigned a0, unsigned a1, unsigned a2, unsigned a3, unsigned& o0, unsigned& o1,
                                      unsigned& o2, unsigned& o3) {
    const unsigned t0 = __builtin_amdgcn_perm(a1, a0, 0x05010400u), t1 = __builtin_amdgcn_perm(a1, a0, 0x07030602u);
    const unsigned t2 = __builtin_amdgcn_perm(a3, a2, 0x05010400u), t3 = __builtin_amdgcn_perm(a3, a2, 0x07030602u);
    o0 = __builtin_amdgcn_perm(t2, t0, 0x05040100u);
    o1 = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
    o2 = __builtin_amdgcn_perm(t3, t1, 0x05040100u);
    o3 = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
}

// 8 words of consecutive k -> 8 pieces, piece i the digits i of the 8 words
__device__ __forceinline__ void rm_digits(const u64 (&w)[8], uint2 (&pl)[8]) {
    unsigned lo[8], hi[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const u64 s = (w[r] + 0x8080808080808080ull) ^ 0x8080808080808080ull;
        lo[r] = (unsigned)s;
        hi[r] = (unsigned)(s >> 32);
    }
    rm_t4(lo[0], lo[1], lo[2], lo[3], pl[0].x, pl[1].x, pl[2].x, pl[3].x);
    rm_t4(lo[4], lo[5], lo[6], lo[7], pl[0].y, pl[1].y, pl[2].y, pl[3].y);
    rm_t4(hi[0], hi[1], hi[2], hi[3], pl[4].x, pl[5].x, pl[6].x, pl[7].x);
    rm_t4(hi[4], hi[5], hi[6], hi[7], pl[4].y, pl[5].y, pl[6].y, pl[7].y);
}

// One fragment pair and step: the second operand's eight limbs are held in registers, the first operand's limb i is read from
// LDS (fa + i * plane) and meets limbs 0 .. 7 - i -- 36 MFMAs onto the 8 diagonal accumulators
__device__ __forceinline__ void rm_pairs(const char* fa, int plane, const rm_v4i (&bq)[8], rm_v4i (&acc)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const rm_v4i a = *(const rm_v4i*)(fa + i * plane);
#pragma unroll
        for (int j = 0; j + i < 8; ++j) acc[i + j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bq[j], acc[i + j], 0, 0, 0);
    }
}

// the epilogue's combine of row r of a fragment: sum_d (u64)(int64) acc_d << 8 d
__device__ __forceinline__ u64 rm_combine(const rm_v4i (&acc)[8], int r) {
    u64 v = 0;
#pragma unroll
    for (int d = 0; d < 8; ++d) v += (u64)(long long)acc[d][r] << (8 * d);
    return v;
}

// C must hold C0 (or zero) already when a.ksplit > 1: the slices add to it
int launch_ring_gemm_mfma(const RingMfmaArgs& a, int parties, hipStream_t st);

}  // namespace primia
