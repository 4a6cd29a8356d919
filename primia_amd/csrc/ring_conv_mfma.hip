// Direct convolution over Z_2^64 on the matrix pipe (option ring_mfma with conv_triples; DESIGN.md §7, "Ring convolution on
// int8 MFMA limbs"): ring_conv_kernel's sum
//
//     C = C0 + conv(X1, W1) + conv(X2, W2)   mod 2^64,   X [B][C][H][W], W [O][C][R][S], C [B][O][Ho][Wo], zero padded
//
// through v_mfma_i32_16x16x64_i8 on signed 8-bit limbs, for 3 x 3 / 1, 3 x 3 / 2 and 1 x 1 / 2 (the thin-channel 7 x 7 / 2 has a k
// layout of its own, taps and not channels: ring_conv_stem_mfma.hip, ring_mfma = 2).  The arithmetic is
// ring_gemm_mfma.hip's and its device functions are shared (ring_gemm_mfma.h): rm_digits recodes 8 words into 8 limb pieces,
// rm_pairs runs the 36 digit pairs of a fragment pair onto 8 diagonal i32 accumulators, rm_combine shifts and adds them once.
// Integer arithmetic throughout: the result is the bits of ring_conv_kernel.  Builtins only.
//
// Tile.  ring_conv_kernel's grid (ConvGeom; conv_plan is the one planner): a 256-thread block owns 8 x 8 output pixels of one
// image x 64 output channels; wave w owns the 32 channel x 32 pixel quadrant (w / 2, w % 2) as 2 x 2 fragments, 8 diagonals
// each: 128 accumulator registers.  The WEIGHTS are the instruction's first operand and the PIXELS its second, so an
// accumulator register's 16 lanes (lane % 16) are 16 pixels -- two rows of 8 -- of ONE output channel (4 (lane / 16) + r):
// a store or an atomicAdd of the epilogue touches two 64-byte runs of NCHW, where ring_conv_kernel's 16 lanes are 16
// channels, Ho Wo words apart.
//
// k.  One step is one tap x 64 input channels; the channels are walked in chunks of 64, the taps inside a chunk.  Channels
// past the slice (a ragged last chunk, C < 64), output channels past O and pixels outside the image are zero words, and zero
// recodes to zero digits.
//
// LDS, all of it limb planes [limb][row][64 channel bytes]: a row is 4 units of 16 bytes (channels 16 u .. 16 u + 15 in the
// byte order rm_digits gives both operands), and a fragment of limb i is one ds_read_b128 per lane: row lane % 16 of the
// fragment, unit g = lane / 16.  Rows are 64 bytes apart, so without more the 16 rows of a read would share 4 of the 16
// 16-byte columns of the 64 banks; unit u of a row is stored at u ^ x(row) instead (an XOR swizzle, no padding):
//   weights, 2 stages x 8 planes x 64 o x 64 B = 65,536 B, x = (o / 4) % 4.  Read: the 16 lanes of one g are rows o .. o + 15
//     at columns 4 (o % 4) + (g ^ (o / 4) % 4) -- 4 x 4 different values, every column once.  Staging write (ds_write_b64):
//     thread t takes row 16 ((t / 32) % 4) + t % 16, octets q = 2 j + (t / 16) % 2 for j = t / 128 and t / 128 + 2; 32 lanes
//     are 16 rows x 2 octets of one j at 8-byte slots 8 (o % 4) + 2 (j ^ (o / 4) % 4) + q % 2: every bank once.
//   3 x 3 / 1, pixels: the 10 x 10 halo patch of the chunk, 8 planes x 100 pixels x 64 B = 51,200 B, staged ONCE per chunk and
//     read by all nine taps (each input word is fetched and recoded once per tile and chunk, not nine times); pixel (y, x) is
//     row 10 y + x and x = (x / 2) % 4.  Read of tap (r, s): the 16 lanes of one g are patch pixels (py + r, s .. s + 7) and
//     (py + r + 1, s .. s + 7); two of them share 4 (row % 4) only if their x differ by 2 (the rows 10 apart), 4 or 6, and
//     then (x / 2) % 4 differs: every column once, for every tap.  Staging write: thread t takes pixel 16 (t / 32) + t % 16
//     (below 100) and octets 2 j + (t / 16) % 2, j = 0 .. 3; 32 lanes are 16 consecutive pixels x 2 octets, and two pixels 8
//     apart in one patch row (x = 0 and 8, 1 and 9) share a slot: two-way on those lanes, once per chunk of nine steps.
//   3 x 3 / 2 and 1 x 1 / 2, pixels: a stride-2 input word is read by 2.25 taps on average and a 17 x 17 patch would be 185 KB,
//     so the block gathers, per tap, the tile's 64 sampled pixels x 64 channels straight from NCHW into the weights' layout
//     (2 stages x 32,768 B, row = pixel, same swizzle): reads and writes as the weights', every bank once.  No im2col operand
//     exists anywhere.
// 116,736 B (3 x 3 / 1) or 131,072 B of dynamic LDS: one block per CU, one wave per SIMD, up to 512 registers per lane under
// __launch_bounds__(256) (DESIGN.md has the counts; nothing spills).
//
// Global reads.  A staging thread takes 8 consecutive channels of one pixel -- 8 loads H W words apart, the 16 lanes of a
// group on neighbouring pixels of two rows -- or of one (o, tap) weight: W[O][C][R][S] puts those R S words apart, the price
// of reading the weights in place.
//
// Pipeline: the next step's weight (and gathered pixel) words are fetched before a step's MFMAs, recoded and written to the
// other stage after them: one barrier per step.  The patch has one buffer: the next chunk's words are fetched before the
// last tap's MFMAs and written between two barriers after them, once per nine steps.
//
// Slices (conv_mfma_slices): whole chunks over blockIdx.z, combined with 64-bit atomicAdd onto a C that conv_fill_kernel
// initialised; epilogue as ring_conv_kernel's.  Nothing is allocated; every launch captures.
#include "ring_conv_mfma.h"

namespace primia {

constexpr int kCmStage = 8 * 64 * 64;            // one staged operand: 8 limb planes of 64 rows x 64 channel bytes
constexpr int kCmPatchPlane = 100 * 64;          // one limb plane of the 10 x 10 halo patch
constexpr int kCmPixels = 2 * kCmStage;          // the pixel operand follows the two weight stages
constexpr int kCmLdsPatch = kCmPixels + 8 * kCmPatchPlane;      // 116,736 B
constexpr int kCmLdsGather = kCmPixels + 2 * kCmStage;          // 131,072 B

struct CmPos {      // a step: pair, first channel of its chunk, tap
    int pair, c0, tap;
};

// gridDim = (B * pixel tiles, ceil(O / 64), jobs * csplit), as ring_conv_kernel; f.d > 0 (csplit == 1 only) truncates the sum
template <int R, int STRIDE>
__global__ __launch_bounds__(256) void ring_conv_mfma_kernel(ConvJob j0, ConvJob j1, ConvGeom g, FaithDiv f) {
    constexpr bool PATCH = STRIDE == 1;
    constexpr int RR = R * R;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.x / g.ptiles, pt = blockIdx.x - b * g.ptiles;
    const int oy0 = (pt / g.tiles_x) * 8, ox0 = (pt % g.tiles_x) * 8;
    const int o0 = blockIdx.y * 64;
    const int job = blockIdx.z / g.csplit, slice = blockIdx.z - job * g.csplit;
    const ConvJob J = job ? j1 : j0;
    const int cb = slice * g.cchunk;
    const int ce = cb + g.cchunk < g.C ? cb + g.cchunk : g.C;
    const int total = (J.X2 ? 2 : 1) * ((ce - cb + kCmChunk - 1) / kCmChunk) * RR;
    const int HW = g.H * g.W;
    const long xb = (long)b * g.C * HW;

    // staging of a 64-row operand: row srow, octets 2 (sj + 2 it) + sql for it = 0, 1
    const int srow = ((tid >> 5) & 3) * 16 + (tid & 15), sj = tid >> 7, sql = (tid >> 4) & 1;
    const int soff = srow * 64 + sql * 8, sx = (srow >> 2) & 3;
    const int so = o0 + srow;                                        // the weight row's output channel
    const int sy = (oy0 + (srow >> 3)) * STRIDE - g.pad, sxx = (ox0 + (srow & 7)) * STRIDE - g.pad;      // the gathered pixel
    u64 rw[2][8], rx[2][8];
    auto fetch_w = [&](const CmPos& p) {
        const u64* __restrict__ Wt = p.pair ? J.W2 : J.W1;
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int c = p.c0 + 16 * (sj + 2 * it) + 8 * sql + r;
                rw[it][r] = (so < g.O && c < ce) ? Wt[((long)so * g.C + c) * RR + p.tap] : (u64)0;
            }
    };
    auto fetch_x = [&](const CmPos& p) {
        const u64* __restrict__ X = p.pair ? J.X2 : J.X1;
        const int tr = p.tap / R, iy = sy + tr, ix = sxx + p.tap - tr * R;
        const bool in = iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int c = p.c0 + 16 * (sj + 2 * it) + 8 * sql + r;
                rx[it][r] = (in && c < ce) ? X[xb + (long)c * HW + iy * g.W + ix] : (u64)0;
            }
    };
    auto write_rows = [&](char* base, const u64 (&v)[2][8]) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            uint2 pl[8];
            rm_digits(v[it], pl);
#pragma unroll
            for (int i = 0; i < 8; ++i) *(uint2*)(base + i * (64 * 64) + soff + (((sj + 2 * it) ^ sx) << 4)) = pl[i];
        }
    };

    // staging of the halo patch (3 x 3 / 1): patch pixel pp = 10 y + x, octets 2 it + sql for it = 0 .. 3
    const int pp = (tid >> 5) * 16 + (tid & 15), ppy = pp / 10, ppx = pp - ppy * 10;
    const int piy = oy0 - g.pad + ppy, pix = ox0 - g.pad + ppx;
    const bool pin = pp < 100 && piy >= 0 && piy < g.H && pix >= 0 && pix < g.W;
    u64 rp[PATCH ? 4 : 1][8];
    auto fetch_patch = [&](const CmPos& p) {
        const u64* __restrict__ X = p.pair ? J.X2 : J.X1;
#pragma unroll
        for (int it = 0; it < (PATCH ? 4 : 0); ++it)
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int c = p.c0 + 16 * it + 8 * sql + r;
                rp[it][r] = (pin && c < ce) ? X[xb + (long)c * HW + piy * g.W + pix] : (u64)0;
            }
    };
    auto write_patch = [&]() {
        if (pp >= 100) return;
#pragma unroll
        for (int it = 0; it < (PATCH ? 4 : 0); ++it) {
            uint2 pl[8];
            rm_digits(rp[it], pl);
#pragma unroll
            for (int i = 0; i < 8; ++i)
                *(uint2*)(smem + kCmPixels + i * kCmPatchPlane + pp * 64 + ((it ^ ((ppx >> 1) & 3)) << 4) + sql * 8) = pl[i];
        }
    };

    // fragments: row lane % 16, unit lane / 16; accumulators: pixel lane % 16, channels 4 (lane / 16) + r
    const int fr = lane & 15, fg = lane >> 4;
    const int wm = w >> 1, wn = w & 1;
    const int frow = fr * 64 + ((fg ^ ((fr >> 2) & 3)) << 4);       // (rows 16 and 32 further on have the same swizzle)
    const int fw = 32 * wm * 64 + frow;
    const int fy = 4 * wn + (fr >> 3), fx = fr & 7;                  // the patch pixel of fragment 0 at tap (0, 0)
    rm_v4i acc[2][2][8];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int d = 0; d < 8; ++d) acc[mi][ni][d] = rm_v4i{0, 0, 0, 0};

    auto next = [&](CmPos p) {
        if (++p.tap == RR) {
            p.tap = 0;
            p.c0 += kCmChunk;
            if (p.c0 >= ce) {
                p.c0 = cb;
                p.pair = 1;
            }
        }
        return p;
    };

    CmPos cur{0, cb, 0};
    if (PATCH) {
        fetch_patch(cur);
        write_patch();
    } else {
        fetch_x(cur);
        write_rows(smem + kCmPixels, rx);
    }
    fetch_w(cur);
    write_rows(smem, rw);
    __syncthreads();
    for (int s = 0; s < total; ++s) {
        const CmPos nx = next(cur);
        const bool more = s + 1 < total;
        const bool repatch = PATCH && more && nx.tap == 0;      // (block-uniform, like every condition around a barrier here)
        if (more) {
            fetch_w(nx);
            if (!PATCH) fetch_x(nx);
        }
        if (repatch) fetch_patch(nx);
        const char* const sw = smem + (s & 1) * kCmStage + fw;
        const char* px[2];
        int pplane;
        if (PATCH) {
            const int tr = cur.tap / R, ts = cur.tap - tr * R;
            const int x = fx + ts;
            px[0] = smem + kCmPixels + ((fy + tr) * 10 + x) * 64 + ((fg ^ ((x >> 1) & 3)) << 4);
            px[1] = px[0] + 20 * 64;      // fragment 1: two patch rows down
            pplane = kCmPatchPlane;
        } else {
            px[0] = smem + kCmPixels + (s & 1) * kCmStage + 32 * wn * 64 + frow;
            px[1] = px[0] + 16 * 64;
            pplane = 64 * 64;
        }
        // the pixels' eight limbs of a fragment stay in registers; the weights' limb i meets limbs 0 .. 7 - i
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            rm_v4i bq[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) bq[j] = *(const rm_v4i*)(px[ni] + j * pplane);
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) rm_pairs(sw + mi * 16 * 64, 64 * 64, bq, acc[mi][ni]);
        }
        if (repatch) {
            __syncthreads();      // every wave is done with the old chunk's patch
            write_patch();
        }
        if (more) {
            write_rows(smem + ((s + 1) & 1) * kCmStage, rw);
            if (!PATCH) write_rows(smem + kCmPixels + ((s + 1) & 1) * kCmStage, rx);
        }
        __syncthreads();
        cur = nx;
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
                u64 v = rm_combine(acc[mi][ni], r);
                if (g.csplit == 1) {
                    v += J.C0 ? J.C0[at] : (u64)0;      // (C0 may be C: an accumulating call)
                    if (f.d) v = conv_trunc(v, f);
                    J.C[at] = v;
                } else {
                    atomicAdd(J.C + at, v);      // C was initialised with C0 (or zero) by the launcher
                }
            }
        }
    }
}

template <int R, int STRIDE>
static int launch_cm(const ConvJob& a, const ConvJob& b, const ConvGeom& g, FaithDiv f, dim3 grid, hipStream_t st) {
    constexpr int lds = STRIDE == 1 ? kCmLdsPatch : kCmLdsGather;
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute((const void*)ring_conv_mfma_kernel<R, STRIDE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                lds) != hipSuccess)
            return PRIMIA_ERR_LAUNCH;
        attr_set = true;
    }
    ring_conv_mfma_kernel<R, STRIDE><<<grid, 256, lds, st>>>(a, b, g, f);
    return launch_status();
}

int launch_ring_conv_mfma(const ConvJob& a, const ConvJob& b, const ConvGeom& g, int R, int stride, FaithDiv f, dim3 grid,
                          hipStream_t st) {
    if (R == 3 && stride == 1) return launch_cm<3, 1>(a, b, g, f, grid, st);
    if (R == 3 && stride == 2) return launch_cm<3, 2>(a, b, g, f, grid, st);
    if (R == 1 && stride == 2) return launch_cm<1, 2>(a, b, g, f, grid, st);
    if (R == 7 && stride == 2) return launch_ring_conv_stem_mfma(a, b, g, f, grid, st);
    return PRIMIA_ERR_UNSUPPORTED;
}

}  // namespace primia
