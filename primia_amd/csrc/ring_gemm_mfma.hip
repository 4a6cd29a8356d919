// Z_2^64 GEMM on the matrix pipe: C = C0 + A1 @ B1 + A2 @ B2 mod 2^64 through v_mfma_i32_16x16x64_i8 on signed 8-bit limbs
// (option ring_mfma; DESIGN.md §7, "Z_2^64 GEMM on int8 MFMA limbs").  gfx950 has no 64-bit integer MFMA; a u64 word is eight
// signed digits, a product mod 2^64 the 36 digit pairs (i, j) with i + j <= 7, and the pairs of one diagonal d = i + j share one
// i32 accumulator that the epilogue shifts by 8 d.  Integer arithmetic throughout: the result is the bits of ring_gemm_kernel.
//
// Signed digits.  With C8 = 0x8080808080808080 the bytes of (x + C8) ^ C8 -- a 64-bit add, carries propagate -- read as int8
// are digits s_i in [-128, 127] with x = sum_i s_i 2^(8 i) mod 2^64: adding 0x80 to a byte and flipping its top bit subtracts
// 256 from a byte of 128 or more and carries 1 into the next, and the carry out of byte 7 is a multiple of 2^64.  Zero maps to
// zero, so the zero padding of ragged tiles stays zero.
//
// Block: 256 threads own a 64 x 64 output tile (ring_gemm_kernel's, so one launcher decides the grid of both); wave w owns the
// 32 x 32 quadrant (w / 2, w % 2) as 2 x 2 fragments of 16 x 16, 8 diagonals each: 128 accumulator registers.  k advances 64
// per step.
//
// Staging.  A thread fetches 8 consecutive k words of one row of A (64 contiguous bytes) or of one column of B (8 rows; 16
// neighbouring lanes read 16 neighbouring columns, one 128-byte line per row), recodes them, transposes the 8 x 8 digit bytes
// in registers with v_perm_b32 (four 4 x 4 byte transposes of two rounds each) and writes eight ds_write_b64, one per limb
// plane.  LDS holds each operand as 8 limb planes of 64 rows (m or n) x 64 k bytes, k contiguous, so the fragment of limb i is
// one ds_read_b128 per lane: row lane % 16, bytes 16 (lane / 16) .. + 15.  Both operands are staged by the same function and
// read by the same lane-to-k mapping, so neither the order of the bytes inside a staged 8-byte piece nor the hardware's order
// of k inside the instruction matters: A and B agree on which k a byte position means.
//
// Row pitch 80 bytes.  A fragment read: 16 lanes of one k group at 80 r + 16 g, i.e. 16-byte units 5 r + g -- 5 is odd, the 16
// rows fall on the 16 different 16-byte columns of the 64 banks.  A staging write: a 32-lane group is 16 rows x 2 neighbouring
// k octets at 8-byte units 10 r + q; 10 r mod 32 takes the 16 even values once and q in {0, 1} fills the odd ones: every bank
// once.  (Pitch 64 would put all 16 rows of a read on one column.)  2 operands x 8 planes x 64 x 80 B = 81,920 B of dynamic
// LDS: two blocks per CU (160 KB), 2 waves per SIMD, which __launch_bounds__(256, 2) holds the registers to (242 VGPRs, no
// AGPRs, no scratch).
//
// One LDS stage, fetched and recoded between two barriers: a block's global latency runs under the 144 MFMAs per wave and
// step of the CU's other block.  Holding the next step's 64 fetched registers across the MFMAs did not fit 256 registers
// beside the 128 accumulators and B's 32 limb registers (it spilled), and above 256 the CU holds one block.
#include "ring_gemm_mfma.h"

namespace primia {

constexpr int kRmPitch = 80;
constexpr int kRmPlane = 64 * kRmPitch;         // one limb plane of one operand
constexpr int kRmOperand = 8 * kRmPlane;
constexpr int kRmLds = 2 * kRmOperand;          // 81,920 B

__global__ __launch_bounds__(256, 2) void ring_gemm_mfma_kernel(RingMfmaArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const sA = smem;
    char* const sB = smem + kRmOperand;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int M = g.M, K = g.K, N = g.N;
    const int party = blockIdx.z / g.ksplit, slice = blockIdx.z - party * g.ksplit;
    const RingMfmaSide sd = party ? g.side[1] : g.side[0];
    const int kb = slice * g.kchunk;
    const int ke = kb + g.kchunk < K ? kb + g.kchunk : K;
    const int total = (sd.A2 ? 2 : 1) * ((ke - kb + kRmStep - 1) / kRmStep);

    // staging: row 16 w + lane % 16 of the tile (m for A, n for B), k octets lane / 16 and lane / 16 + 4
    const int srow = 16 * w + (lane & 15), sq = lane >> 4;
    const int sm = m0 + srow, sn = n0 + srow;
    const int soff = srow * kRmPitch + 8 * sq;
    u64 ra[2][8], rb[2][8];
    auto fetch = [&](int pair, int k0) {
        const u64* __restrict__ A = pair ? sd.A2 : sd.A1;
        const u64* __restrict__ Bm = pair ? sd.B2 : sd.B1;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int kk = k0 + 8 * (sq + 4 * p);
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int gk = kk + r;
                ra[p][r] = (sm < M && gk < ke) ? A[(long)sm * K + gk] : (u64)0;
                rb[p][r] = (sn < N && gk < ke) ? Bm[(long)gk * N + sn] : (u64)0;
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            uint2 pl[8];
            rm_digits(ra[p], pl);
#pragma unroll
            for (int i = 0; i < 8; ++i) *(uint2*)(sA + i * kRmPlane + soff + 32 * p) = pl[i];
            rm_digits(rb[p], pl);
#pragma unroll
            for (int i = 0; i < 8; ++i) *(uint2*)(sB + i * kRmPlane + soff + 32 * p) = pl[i];
        }
    };

    // fragments: row lane % 16, 16 k bytes at 16 (lane / 16); accumulators: column lane % 16, rows 4 (lane / 16) + r
    const int fr = lane & 15, fg = lane >> 4;
    const int wm = w >> 1, wn = w & 1;
    const char* const fa = sA + (32 * wm + fr) * kRmPitch + 16 * fg;
    const char* const fb = sB + (32 * wn + fr) * kRmPitch + 16 * fg;
    rm_v4i acc[2][2][8];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int d = 0; d < 8; ++d) acc[mi][ni][d] = rm_v4i{0, 0, 0, 0};

    int pair = 0, k0 = kb;
    for (int s = 0; s < total; ++s) {
        fetch(pair, k0);
        stage();
        __syncthreads();
        k0 += kRmStep;
        if (k0 >= ke) {
            k0 = kb;
            pair = 1;
        }
        // B's eight limbs of a fragment stay in registers; A's limb i meets limbs 0 .. 7 - i: 36 MFMAs per fragment pair
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            rm_v4i bq[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) bq[j] = *(const rm_v4i*)(fb + j * kRmPlane + ni * 16 * kRmPitch);
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) rm_pairs(fa + mi * 16 * kRmPitch, kRmPlane, bq, acc[mi][ni]);
        }
        __syncthreads();
    }

    // combine the diagonals once; 16 lanes run along n, so a row's store or atomic touches one 128-byte line
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gm = m0 + 32 * wm + 16 * mi + 4 * fg + r;
            if (gm >= M) continue;
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const int gn = n0 + 32 * wn + 16 * ni + fr;
                if (gn >= N) continue;
                const u64 v = rm_combine(acc[mi][ni], r);
                const long o = (long)gm * N + gn;
                if (g.ksplit == 1)
                    sd.C[o] = v + (sd.C0 ? sd.C0[o] : (u64)0);
                else
                    atomicAdd(sd.C + o, v);  // C holds C0 (or zero) already; ring addition is associative
            }
        }
    }
}

int launch_ring_gemm_mfma(const RingMfmaArgs& a, int parties, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)ring_gemm_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kRmLds) !=
            hipSuccess)
            return PRIMIA_ERR_LAUNCH;
        attr_set = true;
    }
    const dim3 grid((a.N + 63) / 64, (a.M + 63) / 64, parties * a.ksplit);
    ring_gemm_mfma_kernel<<<grid, 256, kRmLds, st>>>(a);
    return launch_status();
}

}  // namespace primia
