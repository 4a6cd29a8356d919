// The thin-channel 7 x 7 / 2 convolution over Z_2^64 on the matrix pipe (option ring_mfma = 2 with conv_triples; DESIGN.md
// §7, "Ring convolution: the 7 x 7 / 2 stem on int8 MFMA limbs"): ring_conv_kernel<7, 2>'s sum
//
//     C = C0 + conv(X1, W1) + conv(X2, W2)   mod 2^64,   X [B][C][H][W], W [O][C][7][7], C [B][O][Ho][Wo], zero padded
//
// for 1 <= C <= 4 (the stem: RGB, grayscale), any B, H, W, O and pad < 7.  ring_conv_mfma_kernel's k is one tap x 64 channels,
// 3 live bytes of 64 here; this kernel packs the TAPS into k.  The arithmetic is ring_gemm_mfma.hip's, shared through
// ring_gemm_mfma.h (rm_digits, rm_pairs, rm_combine on v_mfma_i32_16x16x64_i8): integers throughout, the result is the bits of
// ring_conv_kernel.  Builtins only.
//
// Tile, grid and epilogue are ring_conv_mfma_kernel's (ConvGeom; conv_plan sets csplit = 1 and cchunk = C: the channels are
// never sliced): a 256-thread block owns 8 x 8 output pixels of one image x 64 output channels, wave w the 32 channel x 32 pixel
// quadrant (w / 2, w % 2) as 2 x 2 fragments of 8 diagonals; weights first operand, pixels second, so the epilogue's 16 lanes
// run along two rows of 8 pixels of one output channel: acc + C0, conv_trunc when f.d, store.
//
// k.  A step q = 0 .. 3 is 64 bytes = filter rows 2 q and 2 q + 1 x 8 taps x 4 channel bytes: the lane's 16-byte unit g = lane /
// 16 is row 2 q + g / 2, taps 4 (g % 2) .. + 3.  Row 7, tap 7 and channels >= C are ZERO WEIGHT DIGITS (zero recodes to zero), so
// whatever pixel bytes sit opposite them add nothing to an integer accumulator.  Live k is 49 C of 256.  At most 2 pairs x 4
// steps = 512 k share the accumulators against the bound of 16,384 (ring_gemm_mfma.h): no slice cap applies.
//
// Pixels: a limb patch that is its own im2col.  The tile's input halo is 21 x 21 pixels, held as 22 x 22 (row 21 and column 21
// zero): 8 limb planes of [y][x] dwords, a dword the 4 channel bytes of one pixel's limb in rm_t4's order -- 8 x 1,936 = 15,488 B
// per pair, both pairs resident.  The 8 taps of filter row r of output pixel (py, px) are the 8 consecutive dwords from patch
// pixel (2 py + r, 2 px): a fragment read takes 4 of them, 16 bytes at an 8-BYTE-aligned address (odd px: not 16), issued as
// two 8-byte reads.  Staging: thread t < 242 takes the pixel pair (t / 11, 2 (t % 11)), loads its 2 C words (zero off the
// image, in row / column 21 and past C), runs rm_digits over [pixel][channel] and writes eight ds_write_b64 at byte 8 t of each
// plane.  Each input word is fetched and recoded once per tile; no im2col copy exists anywhere.
//
// Weights: per step 64 o x 64 B per limb in ring_conv_mfma_kernel's layout ([limb][o][64 B], unit u of row o at u ^ (o / 4) % 4)
// and its thread mapping (row 16 ((t / 32) % 4) + t % 16, units t / 128 and t / 128 + 2, half (t / 16) % 2), fetched in place
// from W[O][C][7][7]: a thread's 8 words are 2 neighbouring taps x 4 channels, rm_digits over [tap][channel] gives the byte
// order of the pixel side, and rm_pairs reads the first operand unchanged.
//
// Banks (64 banks of 4 B; all of it derived from the addresses, none of it measured).
//   patch fragment reads: lane (p = lane % 16, g) reads 8 B at 88 (2 py + 2 q + g / 2) + 8 px + 16 (g % 2) (+ 8), py = p / 8,
//     px = p % 8, pitch 22 dwords.  The 16 lanes of one g span two 64-byte runs 176 B = 44 banks apart; g % 2 shifts a run by
//     4 banks (the overlapping dwords are the SAME address, a broadcast), g / 2 by 22 banks.  A 32-lane half (g = 0, 1 or 2, 3)
//     touches banks b .. b + 19 and b + 44 .. b + 63: every bank at most once.  Pitch 22 is what makes 2 x pitch = 44 >= 20 and
//     64 - 44 >= 20; a pitch of 32 would put both rows on the same banks.
//   patch staging writes: byte 8 t, consecutive lanes consecutive 8-byte slots: every bank once per 32 lanes.
//   weights: ring_conv_mfma_kernel's accesses (see there): reads and writes touch every bank once.
//
// LDS and occupancy.  ONE weight stage (32,768 B) + two patches = 63,744 B under __launch_bounds__(256, 2): two blocks per CU,
// as ring_gemm_mfma_kernel, and like it a step fetches, recodes and writes its weights between two barriers and then runs its
// 144 MFMAs: the other block covers the fetch.  The compiler's report decided it: this form takes 240 VGPRs and no scratch at
// two waves per SIMD, and the stem's 392 blocks at one image (196 tiles x 2 jobs) are then all resident at once on 256 CUs,
// where one block per CU would run them in two rounds.  With the next step's 16 words fetched AHEAD of the MFMAs the same
// bound spilled (101 VGPRs; 8 with the fetch issued behind them, where the compiler peels the first step); that form would
// need __launch_bounds__(256), a second stage and one block per CU.  Below 64 KB: no attribute to set.  Nothing is allocated;
// every launch captures.
#include "ring_conv_mfma.h"

namespace primia {

constexpr int kCsPitch = 22;                               // patch rows / columns, dwords per patch row
constexpr int kCsPlane = kCsPitch * kCsPitch * 4;          // one limb plane of the patch: 1,936 B
constexpr int kCsPatch = 8 * kCsPlane;                     // 15,488 B
constexpr int kCsStage = 8 * 64 * 64;                      // the weight stage: 8 limb planes of 64 o x 64 B
constexpr int kCsLds = kCsStage + 2 * kCsPatch;            // 63,744 B

// gridDim = (B * pixel tiles, ceil(O / 64), jobs); g.csplit == 1, g.C <= 4; f.d > 0 truncates the sum
__global__ __launch_bounds__(256, 2) void ring_conv_stem_mfma_kernel(ConvJob j0, ConvJob j1, ConvGeom g, FaithDiv f) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.x / g.ptiles, pt = blockIdx.x - b * g.ptiles;
    const int oy0 = (pt / g.tiles_x) * 8, ox0 = (pt % g.tiles_x) * 8;
    const int o0 = blockIdx.y * 64;
    const ConvJob J = blockIdx.z ? j1 : j0;
    const int pairs = J.X2 ? 2 : 1, total = 4 * pairs;
    const int HW = g.H * g.W;
    const long xb = (long)b * g.C * HW;

    // the patch of one pair: pixel pair (py, px) and (py, px + 1) of the 22 x 22 patch
    auto stage_patch = [&](int pair) {
        if (tid >= kCsPitch * kCsPitch / 2) return;
        const u64* __restrict__ X = pair ? J.X2 : J.X1;
        const int py = tid / 11, px = 2 * (tid - 11 * py);
        const int iy = 2 * oy0 - g.pad + py, ix = 2 * ox0 - g.pad + px;
        const bool row = py < 21 && iy >= 0 && iy < g.H;
        const bool in0 = row && ix >= 0 && ix < g.W, in1 = row && px + 1 < 21 && ix + 1 >= 0 && ix + 1 < g.W;
        u64 v[8];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const long at = xb + (long)c * HW + iy * g.W + ix;
            v[c] = (in0 && c < g.C) ? X[at] : (u64)0;
            v[4 + c] = (in1 && c < g.C) ? X[at + 1] : (u64)0;
        }
        uint2 pl[8];
        rm_digits(v, pl);
#pragma unroll
        for (int i = 0; i < 8; ++i) *(uint2*)(smem + kCsStage + pair * kCsPatch + i * kCsPlane + 8 * tid) = pl[i];
    };

    // the weights of step q: row srow, octets 2 (sj + 2 it) + sql for it = 0, 1; an octet is 2 taps x 4 channels
    const int srow = ((tid >> 5) & 3) * 16 + (tid & 15), sj = tid >> 7, sql = (tid >> 4) & 1;
    const int soff = srow * 64 + sql * 8, sx = (srow >> 2) & 3;
    const int so = o0 + srow;
    u64 rw[2][8];
    auto fetch_w = [&](int s) {
        const u64* __restrict__ Wt = (s >> 2) ? J.W2 : J.W1;
        const int q = s & 3;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int u = sj + 2 * it, r = 2 * q + (u >> 1), t0 = 4 * (u & 1) + 2 * sql;
            const bool in0 = so < g.O && r < 7, in1 = in0 && t0 + 1 < 7;      // (t0 <= 6)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const long at = ((long)so * g.C + c) * 49 + r * 7 + t0;
                rw[it][c] = (in0 && c < g.C) ? Wt[at] : (u64)0;
                rw[it][4 + c] = (in1 && c < g.C) ? Wt[at + 1] : (u64)0;
            }
        }
    };
    auto write_w = [&]() {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            uint2 pl[8];
            rm_digits(rw[it], pl);
#pragma unroll
            for (int i = 0; i < 8; ++i) *(uint2*)(smem + i * (64 * 64) + soff + (((sj + 2 * it) ^ sx) << 4)) = pl[i];
        }
    };

    // fragments: weights row lane % 16, unit lane / 16; pixels: tile pixel (4 wn + 2 ni + fr / 8, fr % 8), unit fg
    const int fr = lane & 15, fg = lane >> 4;
    const int wm = w >> 1, wn = w & 1;
    const char* const sw = smem + (32 * wm + fr) * 64 + ((fg ^ ((fr >> 2) & 3)) << 4);
    // byte of patch pixel (2 py + fg / 2, 2 px + 4 (fg % 2)) for fragment 0 at step 0; fragment 1 is 4 patch rows down, a
    // step 2 patch rows down
    const int fpix = ((2 * (4 * wn + (fr >> 3)) + (fg >> 1)) * kCsPitch + 2 * (fr & 7) + 4 * (fg & 1)) * 4;
    rm_v4i acc[2][2][8];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int d = 0; d < 8; ++d) acc[mi][ni][d] = rm_v4i{0, 0, 0, 0};

    stage_patch(0);
    if (pairs == 2) stage_patch(1);
    for (int s = 0; s < total; ++s) {
        fetch_w(s);
        __syncthreads();      // every wave is done with the last step's weights
        write_w();
        __syncthreads();
        const char* const px = smem + kCsStage + (s >> 2) * kCsPatch + fpix + (s & 3) * (2 * kCsPitch * 4);
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            rm_v4i bq[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {      // 16 bytes at an 8-byte-aligned address: two 8-byte reads
                const char* at = px + ni * (4 * kCsPitch * 4) + j * kCsPlane;
                const uint2 lo = *(const uint2*)at, hi = *(const uint2*)(at + 8);
                bq[j] = rm_v4i{(int)lo.x, (int)lo.y, (int)hi.x, (int)hi.y};
            }
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) rm_pairs(sw + mi * 16 * 64, 64 * 64, bq, acc[mi][ni]);
        }
    }

    // combine the diagonals once; 16 lanes run along the pixels: two 64-byte runs of one output channel
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = o0 + 32 * wm + 16 * mi + 4 * fg + r;
            if (o >= g.O) continue;
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const int oy = oy0 + 4 * wn + 2 * ni + (fr >> 3), ox = ox0 + (fr & 7);
                if (oy >= g.Ho || ox >= g.Wo) continue;
                const long at = (((long)b * g.O + o) * g.Ho + oy) * g.Wo + ox;
                u64 v = rm_combine(acc[mi][ni], r) + (J.C0 ? J.C0[at] : (u64)0);      // (C0 may be C: an accumulating call)
                if (f.d) v = conv_trunc(v, f);
                J.C[at] = v;
            }
        }
    }
}

int launch_ring_conv_stem_mfma(const ConvJob& a, const ConvJob& b, const ConvGeom& g, FaithDiv f, dim3 grid, hipStream_t st) {
    if (g.csplit != 1 || g.C > kCsMaxC) return PRIMIA_ERR_UNSUPPORTED;
    ring_conv_stem_mfma_kernel<<<grid, 256, kCsLds, st>>>(a, b, g, f);
    return launch_status();
}

}  // namespace primia
