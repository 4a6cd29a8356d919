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

// C must hold C0 (or zero) already when a.ksplit > 1: the slices add to it
int launch_ring_gemm_mfma(const RingMfmaArgs& a, int parties, hipStream_t st);

}  // namespace primia
