// Ring convolution on int8 MFMA limbs (ring_conv_mfma.hip, ring_conv_stem_mfma.hip; DESIGN.md §7, "Ring convolution on int8
// MFMA limbs"): what ring_conv.hip -- the planner, the launcher and the vector-ALU kernel -- shares with the limb kernels' files.
#pragma once
#include "ring_gemm_mfma.h"
#include "trunc_faithful.h"

namespace primia {

struct ConvJob {          // one convolution sum: C = C0 + conv(X1, W1) + conv(X2, W2); X2 / W2 and C0 may be null
    const u64 *X1, *W1, *X2, *W2, *C0;
    u64* C;
};

struct ConvGeom {
    int B, C, H, W, O, Ho, Wo, pad;
    int tiles_x, ptiles;      // 8 x 8 pixel tiles per row / per image
    int csplit, cchunk;       // slices of the input channels, channels per slice (a multiple of the kernel's chunk)
    int route;                // 0: ring_conv_kernel (vector ALU), 1: the limb kernels (ring_conv_mfma_kernel, 7 x 7 / 2:
                              // ring_conv_stem_mfma_kernel) -- conv_route's answer
};

// a party's truncation of ITS share toward zero (sl_trunc, secure_local.hip), the exact quotient by faith_udiv's multiply
// instead of a 64-bit division: an epilogue holds 16 of them
__device__ __forceinline__ u64 conv_trunc(u64 v, const FaithDiv& f) {
    const int64_t sv = (int64_t)v;
    const u64 q = faith_udiv(sv < 0 ? (u64)0 - v : v, f);
    return sv < 0 ? (u64)0 - q : q;
}

constexpr int kCmChunk = 64;      // input channels per step: one tap x 64 channels is the instruction's k

// The limb kernel's channel split: whole 64-channel chunks, no empty slice.  With fewer than 256 blocks the chunks are
// spread to reach 512.  A step is 64 k, and a slice sums its pairs into the same accumulators, so it holds at most
// kRmMaxSteps / 2 = 127 steps per pair (ring_gemm_mfma.h): csplit rises when C R S alone demands it, at any block count.
// The plan does not know whether a call has one pair or two and holds every call to the two-pair bound.
inline void conv_mfma_slices(int C, int taps, long blocks, int* csplit, int* cchunk) {
    const int chunks = (C + kCmChunk - 1) / kCmChunk;
    int cap = (kRmMaxSteps / 2) / taps;      // chunks per slice (R S <= 9: at least 14)
    int split = 1;
    if (blocks < 256) split = (int)((512 + blocks - 1) / blocks);
    if (split > chunks) split = chunks;
    int per = (chunks + split - 1) / split;
    if (per > cap) per = cap;
    *csplit = (chunks + per - 1) / per;
    *cchunk = per * kCmChunk;
}

constexpr int kCsMaxC = 4;        // the thin-channel 7 x 7 / 2 kernel: a pixel's channels are the 4 bytes of one dword per limb

// g.route == 1, (R, stride) in {(3, 1), (3, 2), (1, 2), (7, 2)}; C must hold C0 (or zero) already when g.csplit > 1
int launch_ring_conv_mfma(const ConvJob& a, const ConvJob& b, const ConvGeom& g, int R, int stride, FaithDiv f, dim3 grid,
                          hipStream_t st);
// 7 x 7 / 2 with g.C <= kCsMaxC and g.csplit == 1 (ring_conv_stem_mfma.hip)
int launch_ring_conv_stem_mfma(const ConvJob& a, const ConvJob& b, const ConvGeom& g, FaithDiv f, dim3 grid, hipStream_t st);

}  // namespace primia
