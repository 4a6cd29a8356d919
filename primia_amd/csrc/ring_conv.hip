// Direct convolution over Z_2^64 for convolution-shaped Beaver triples:
//
//     C = C0 + conv(X1, W1) + conv(X2, W2)   mod 2^64,   X [B][C][H][W], W [O][C][R][S], C [B][O][Ho][Wo], zero padded
//
// -- the two-product fusion of primia_beaver_combine_matmul written straight into NCHW, with no im2col operand anywhere.
// Integer work: results are bit-exact by construction (unsigned wrap-around arithmetic on the int64 bit patterns).
//
// Work split.  A 256-thread block owns an 8 x 8 tile of output pixels of one image x 64 output channels.  Thread (tx, ty) =
// (tid & 15, tid >> 4) holds a 4 pixel x 4 channel u64 register tile: the pixels are 4 neighbours of one output row
// (row ty >> 1, columns 4 (ty & 1) ..), the channels are tx + 16 j as in ring_gemm_kernel, so that the 16 lanes of a pixel
// group read 16 consecutive weight words (128 B, every bank once) and share ONE input address (a broadcast).
//
// Data movement.  Per chunk of CC input channels the block stages in LDS
//     sp[CC][PD][PW]   the input halo patch, PD = 7 ES + R rows and columns (each input word is fetched once per tile, not
//                      R S times; zero outside the image and past the channel slice); PW = PD | 1 keeps the row pitch odd, so
//                      that the pixel groups of a wave (2 per row, 4 ES words apart; rows PW apart) fall on different banks;
//     sw[CC R S][65]   the chunk's weights, tap-major x 64 channels.  Global reads run along the taps (contiguous per output
//                      channel), so the 32 lanes of a ds_write_b64 differ in the tap: a pitch of 65 words puts them 130 dwords
//                      = 2 banks apart (the padding idiom of batch_transpose_kernel); the reads along a row are unaffected.
// A 1 x 1 / stride 2 convolution samples every second input word only: its patch is staged at that step (PS = 2) and read
// with an in-patch stride ES = 1; every other geometry has PS = 1, ES = stride.  CC is 1 for 7 x 7 (the stem's 147 x 64 weight
// words are walked one channel's 49 taps at a time), 4 for 3 x 3 and 16 for 1 x 1: 17 to 29 KB of LDS per block.
// A thread loads one filter row's NW = 3 ES + R input words into registers and reuses them over the S taps of that row: per
// 16 multiply-adds it issues 4 ds_read_b64 of weights and NW / S of inputs, against 8 in ring_gemm_kernel.
//
// Products run on the vector ALU (v_mad_u64_u32 chains): there is no 64-bit integer MFMA.  Under the option ring_mfma the
// 3 x 3 / 1, 3 x 3 / 2 and 1 x 1 / 2 geometries run ring_conv_mfma_kernel instead (ring_conv_mfma.hip: the 8-bit-limb
// decomposition of ring_gemm_mfma.hip on v_mfma_i32_16x16x64_i8, same grid, same sums, same bits); the stem's 7 x 7 / 2
// stays here at ring_mfma = 1 and runs ring_conv_stem_mfma_kernel (ring_conv_stem_mfma.hip: taps packed into k, C <= 4) at
// ring_mfma = 2.  conv_route decides, conv_plan plans either kernel's slices, launch_conv launches what the plan names.
//
// Few tiles (one image in layer3 / layer4: 4 and 1 pixel tiles): the input channels are split over blockIdx.z and the slices
// combined with 64-bit atomicAdd -- ring addition is associative, so the result is bit-identical whatever the order.  C is
// then initialised with C0 (or zero) by a kernel of this file, never a memset node (see launch_gemm, ring.hip).
// Nothing is allocated here: scratch is passed in, and every launch captures into a hipGraph.
#include "common.h"
#include "options.h"
#include "ring_conv_mfma.h"

namespace primia {

template <int R, int STRIDE>
struct ConvCfg {
    static constexpr int PS = R < STRIDE ? STRIDE : 1;      // step of the staged patch in the input
    static constexpr int ES = STRIDE / PS;                   // stride inside the patch
    static constexpr int PD = 7 * ES + R;                    // patch rows / columns of an 8 x 8 pixel tile
    static constexpr int PW = PD | 1;                        // odd row pitch
    static constexpr int NW = 3 * ES + R;                    // input words of 4 neighbouring pixels for one filter row
    static constexpr int CC = R >= 5 ? 1 : (R >= 2 ? 4 : 16);
    static constexpr int KT = CC * R * R;                    // taps per chunk
};

static inline int conv_cc(int R) { return R >= 5 ? 1 : (R >= 2 ? 4 : 16); }

// gridDim = (B * pixel tiles, ceil(O / 64), jobs * csplit).  f.d > 0 (csplit == 1 only): the sum is truncated toward zero
// by f.d before it is stored -- a party's truncation of its product share, in the epilogue.
template <int R, int STRIDE>
__global__ __launch_bounds__(256) void ring_conv_kernel(ConvJob j0, ConvJob j1, ConvGeom g, FaithDiv f) {
    typedef ConvCfg<R, STRIDE> Cfg;
    constexpr int PS = Cfg::PS, ES = Cfg::ES, PD = Cfg::PD, PW = Cfg::PW, NW = Cfg::NW, CC = Cfg::CC, KT = Cfg::KT, RR = R * R;
    constexpr int UR = R >= 5 ? 1 : R;      // filter rows unrolled (7 x 7: the 7 taps of one row)
    __shared__ u64 sp[CC][PD][PW];
    __shared__ u64 sw[KT][65];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int row = ty >> 1, col0 = (ty & 1) * 4;
    const int b = blockIdx.x / g.ptiles, pt = blockIdx.x - b * g.ptiles;
    const int oy0 = (pt / g.tiles_x) * 8, ox0 = (pt % g.tiles_x) * 8;
    const int o0 = blockIdx.y * 64;
    const int job = blockIdx.z / g.csplit, slice = blockIdx.z - job * g.csplit;
    const int cb = slice * g.cchunk;
    const int ce = cb + g.cchunk < g.C ? cb + g.cchunk : g.C;
    const int iy0 = oy0 * STRIDE - g.pad, ix0 = ox0 * STRIDE - g.pad;
    u64 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0;
    for (int pair = 0; pair < 2; ++pair) {
        const u64* __restrict__ X = pair == 0 ? (job ? j1.X1 : j0.X1) : (job ? j1.X2 : j0.X2);
        const u64* __restrict__ Wt = pair == 0 ? (job ? j1.W1 : j0.W1) : (job ? j1.W2 : j0.W2);
        if (!X) continue;
        const u64* __restrict__ Xb = X + (long)b * g.C * g.H * g.W;
        for (int c0 = cb; c0 < ce; c0 += CC) {
            // the halo patch of CC channels: lanes run along a patch row (whole lines of the image)
            for (int idx = tid; idx < CC * PD * PD; idx += 256) {
                const int cc = idx / (PD * PD), rem = idx - cc * (PD * PD);
                const int y = rem / PD, x = rem - y * PD;
                const int iy = iy0 + y * PS, ix = ix0 + x * PS, c = c0 + cc;
                u64 v = 0;
                if (c < ce && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) v = Xb[((long)c * g.H + iy) * g.W + ix];
                sp[cc][y][x] = v;
            }
            // the chunk's weights, [tap][channel]: lanes run along the KT contiguous taps of one output channel
            for (int idx = tid; idx < 64 * KT; idx += 256) {
                const int o = idx / KT, k = idx - o * KT;
                u64 v = 0;
                if (o0 + o < g.O && c0 + k / RR < ce) v = Wt[((long)(o0 + o) * g.C + c0) * RR + k];
                sw[k][o] = v;
            }
            __syncthreads();
            const int ncc = ce - c0 < CC ? ce - c0 : CC;
#pragma unroll 1
            for (int cc = 0; cc < ncc; ++cc) {
#pragma unroll UR
                for (int r = 0; r < R; ++r) {
                    u64 xv[NW];
#pragma unroll
                    for (int k = 0; k < NW; ++k) xv[k] = sp[cc][row * ES + r][col0 * ES + k];
#pragma unroll
                    for (int s = 0; s < R; ++s) {
                        const u64* wrow = sw[(cc * R + r) * R + s];
                        u64 bv[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) bv[j] = wrow[tx + 16 * j];
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int j = 0; j < 4; ++j) acc[i][j] += xv[i * ES + s] * bv[j];
                    }
                }
            }
            __syncthreads();
        }
    }
    const int oy = oy0 + row;
    if (oy >= g.Ho) return;
    const u64* C0 = job ? j1.C0 : j0.C0;      // (C0 may be C: an accumulating call)
    u64* Cm = job ? j1.C : j0.C;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int o = o0 + tx + 16 * j;
        if (o >= g.O) continue;
        const long base = (((long)b * g.O + o) * g.Ho + oy) * g.Wo;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ox = ox0 + col0 + i;
            if (ox >= g.Wo) continue;
            if (g.csplit == 1) {
                u64 v = acc[i][j] + (C0 ? C0[base + ox] : (u64)0);
                if (f.d) v = conv_trunc(v, f);
                Cm[base + ox] = v;
            } else {
                atomicAdd(Cm + base + ox, acc[i][j]);      // C was initialised with C0 (or zero) by the launcher
            }
        }
    }
}

// ---- the element-wise passes around the convolution -------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv_fill_kernel(u64* __restrict__ out, const u64* __restrict__ src, long n) {
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) out[i] = src ? src[i] : (u64)0;
}

// out = a + b (SUB: a - b); out may be a
template <bool SUB>
__global__ __launch_bounds__(256) void conv_addsub_kernel(const u64* a, const u64* __restrict__ b, u64* out, long n) {
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) out[i] = SUB ? a[i] - b[i] : a[i] + b[i];
}

__global__ __launch_bounds__(256) void conv_trunc_kernel(u64* __restrict__ z, long n, FaithDiv f) {
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) z[i] = conv_trunc(z[i], f);
}

// both parties hosted here: spdz_mask and both opens of a convolution in one pass.  delta = (x0 - a0) + (x1 - a1) [nx],
// eps = (w0 - b0) + (w1 - b1) and b0e = b0 + eps [nw]
__global__ __launch_bounds__(256) void conv_open_local_kernel(const u64* __restrict__ x0, const u64* __restrict__ x1,
                                                              const u64* __restrict__ w0, const u64* __restrict__ w1,
                                                              const u64* __restrict__ a0, const u64* __restrict__ a1,
                                                              const u64* __restrict__ b0, const u64* __restrict__ b1,
                                                              u64* __restrict__ delta, u64* __restrict__ eps,
                                                              u64* __restrict__ b0e, long nx, long nw) {
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nx + nw; i += stride) {
        if (i < nx) {
            delta[i] = (x0[i] - a0[i]) + (x1[i] - a1[i]);
        } else {
            const long e = i - nx;
            const u64 ev = (w0[e] - b0[e]) + (w1[e] - b1[e]);
            eps[e] = ev;
            b0e[e] = b0[e] + ev;
        }
    }
}

static inline int conv_blocks(long n) {
    long b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// The kernel a supported geometry runs on: 1, the limb kernels -- ring_conv_mfma_kernel under the option ring_mfma for every
// geometry but 7 x 7 / 2 (a tap's k would be C live bytes of 64), and ring_conv_stem_mfma_kernel for 7 x 7 / 2 with C <= 4
// from ring_mfma = 2 on (taps packed into k); 0, ring_conv_kernel.  Read by conv_plan, and through it by launch_conv and the
// host queries.
static int conv_route(int R, int stride, int C) {
    const int level = PRIMIA_OPT(ring_mfma);
    if (R == 7) return level >= 2 && stride == 2 && C <= kCsMaxC;
    return level != 0;
}

// The geometry a call names, checked before anything is launched: PRIMIA_OK and *g filled, or the error to return.
// The channel split depends on the block count alone (as launch_gemm's on the tile count): with fewer than 256 blocks the
// input channels are sliced to reach 512, never below 64 multiply-adds per output and slice, in whole chunks of CC channels
// (the limb kernel: conv_mfma_slices, whole chunks of 64 under its accumulators' bound; its 7 x 7 / 2 form: one slice).
static int conv_plan(int B, int C, int H, int W, int O, int R, int S, int stride, int pad, int jobs, ConvGeom* g) {
    PRIMIA_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && O > 0 && R > 0 && S > 0 && stride > 0 && pad >= 0 && pad < R &&
                   (jobs == 1 || jobs == 2));
    PRIMIA_REQUIRE(H + 2 * pad >= R && W + 2 * pad >= S);
    if (!(R == S && ((R == 7 && stride == 2) || (R == 3 && (stride == 1 || stride == 2)) || (R == 1 && stride == 2))))
        return PRIMIA_ERR_UNSUPPORTED;
    g->B = B, g->C = C, g->H = H, g->W = W, g->O = O, g->pad = pad;
    g->Ho = (H + 2 * pad - R) / stride + 1;
    g->Wo = (W + 2 * pad - S) / stride + 1;
    g->tiles_x = (g->Wo + 7) / 8;
    g->ptiles = g->tiles_x * ((g->Ho + 7) / 8);
    const long gx = (long)B * g->ptiles, gy = (O + 63) / 64;
    PRIMIA_REQUIRE(gx <= 0x7fffffffL && gy <= 65535);
    const int cc = conv_cc(R);
    const long blocks = gx * gy * jobs;
    g->route = conv_route(R, stride, C);
    if (g->route && R == 7) {      // the thin-channel kernel holds every channel in one k step: never sliced
        g->csplit = 1, g->cchunk = C;
        return PRIMIA_OK;
    }
    if (g->route) {
        conv_mfma_slices(C, R * S, blocks, &g->csplit, &g->cchunk);
        return PRIMIA_OK;
    }
    int csplit = 1;
    if (blocks < 256) {
        csplit = (int)((512 + blocks - 1) / blocks);
        const int cmin = ((64 + R * S - 1) / (R * S) + cc - 1) / cc * cc;      // >= 64 taps per slice, whole chunks
        const int cmax = C / cmin;
        if (csplit > cmax) csplit = cmax;
        if (csplit < 1) csplit = 1;
    }
    g->cchunk = ((C + csplit - 1) / csplit + cc - 1) / cc * cc;
    g->csplit = (C + g->cchunk - 1) / g->cchunk;      // (no empty slice)
    return PRIMIA_OK;
}

// f.d > 0: every job's sum is truncated toward zero by f.d (in the kernel's epilogue, or in place after the slices' adds)
static int launch_conv(const ConvJob* jobs, int njobs, const ConvGeom& g, int R, int stride, FaithDiv f, hipStream_t st) {
    const long n = (long)g.B * g.O * g.Ho * g.Wo;
    if (g.csplit > 1) {
        for (int k = 0; k < njobs; ++k)
            if (jobs[k].C0 != jobs[k].C) conv_fill_kernel<<<conv_blocks(n), 256, 0, st>>>(jobs[k].C, jobs[k].C0, n);
        if (launch_status() != PRIMIA_OK) return PRIMIA_ERR_LAUNCH;
    }
    const dim3 grid((unsigned)((long)g.B * g.ptiles), (g.O + 63) / 64, njobs * g.csplit);
    const ConvJob& a = jobs[0];
    const ConvJob& b = jobs[njobs - 1];
    const FaithDiv d = g.csplit == 1 ? f : FaithDiv{0, 0, 0, 0};
    if (g.route) {
        const int rc = launch_ring_conv_mfma(a, b, g, R, stride, d, grid, st);
        if (rc != PRIMIA_OK) return rc;
    } else if (R == 7)
        ring_conv_kernel<7, 2><<<grid, 256, 0, st>>>(a, b, g, d);
    else if (R == 3 && stride == 1)
        ring_conv_kernel<3, 1><<<grid, 256, 0, st>>>(a, b, g, d);
    else if (R == 3)
        ring_conv_kernel<3, 2><<<grid, 256, 0, st>>>(a, b, g, d);
    else
        ring_conv_kernel<1, 2><<<grid, 256, 0, st>>>(a, b, g, d);
    if (launch_status() != PRIMIA_OK) return PRIMIA_ERR_LAUNCH;
    if (g.csplit > 1 && f.d) {
        for (int k = 0; k < njobs; ++k) conv_trunc_kernel<<<conv_blocks(n), 256, 0, st>>>(jobs[k].C, n, f);
        return launch_status();
    }
    return PRIMIA_OK;
}

}  // namespace primia

using namespace primia;

#define CU(p) ((const u64*)(p))

extern "C" {

int primia_ring_conv2d_split(int B, int C, int H, int W, int O, int R, int S, int stride, int pad, int jobs) {
    ConvGeom g;
    const int rc = conv_plan(B, C, H, W, O, R, S, stride, pad, jobs, &g);
    return rc != PRIMIA_OK ? rc : g.csplit;
}

int primia_ring_conv2d_route(int B, int C, int H, int W, int O, int R, int S, int stride, int pad, int jobs) {
    ConvGeom g;
    const int rc = conv_plan(B, C, H, W, O, R, S, stride, pad, jobs, &g);
    return rc != PRIMIA_OK ? rc : g.route;
}

int64_t primia_beaver_conv_local_scratch_elems(int B, int C, int H, int W, int O, int R, int S) {
    if (!(B > 0 && C > 0 && H > 0 && W > 0 && O > 0 && R > 0 && S > 0)) return PRIMIA_ERR_ARG;
    return (int64_t)B * C * H * W + 2 * (int64_t)O * C * R * S;
}

int primia_ring_conv2d(const int64_t* x, const int64_t* w, int64_t* out, int B, int C, int H, int W, int O, int R, int S,
                       int stride, int pad, int accumulate, primia_stream_t st) {
    PRIMIA_REQUIRE(x && w && out && x != out && w != out);
    ConvGeom g;
    const int rc = conv_plan(B, C, H, W, O, R, S, stride, pad, 1, &g);
    if (rc != PRIMIA_OK) return rc;
    const ConvJob job{CU(x), CU(w), nullptr, nullptr, accumulate ? CU(out) : nullptr, (u64*)out};
    return launch_conv(&job, 1, g, R, stride, FaithDiv{0, 0, 0, 0}, (hipStream_t)st);
}

int primia_beaver_combine_conv(int j, const int64_t* delta, const int64_t* eps, const int64_t* a, const int64_t* b,
                               const int64_t* c, int64_t* z, int64_t* scratch, int B, int C, int H, int W, int O, int R, int S,
                               int stride, int pad, primia_stream_t st) {
    PRIMIA_REQUIRE((j == 0 || j == 1) && delta && eps && a && b && c && z && (j == 1 || scratch));
    PRIMIA_REQUIRE(z != delta && z != eps && z != a && z != b);
    ConvGeom g;
    const int rc = conv_plan(B, C, H, W, O, R, S, stride, pad, 1, &g);
    if (rc != PRIMIA_OK) return rc;
    hipStream_t s = (hipStream_t)st;
    // z = c + conv(delta, b [+ eps]) + conv(a, eps) -- ring-identical to the reference's three products
    const u64* b2 = CU(b);
    if (j == 0) {
        const long nw = (long)O * C * R * S;
        conv_addsub_kernel<false><<<conv_blocks(nw), 256, 0, s>>>(CU(b), CU(eps), (u64*)scratch, nw);
        if (launch_status() != PRIMIA_OK) return PRIMIA_ERR_LAUNCH;
        b2 = CU(scratch);
    }
    const ConvJob job{CU(delta), b2, CU(a), CU(eps), CU(c), (u64*)z};
    return launch_conv(&job, 1, g, R, stride, FaithDiv{0, 0, 0, 0}, s);
}

int primia_beaver_conv_local(const int64_t* x0, const int64_t* x1, const int64_t* w0, const int64_t* w1, const int64_t* a0,
                             const int64_t* b0, const int64_t* c0, const int64_t* a1, const int64_t* b1, const int64_t* c1,
                             int64_t* out0, int64_t* out1, int64_t* scratch, int B, int C, int H, int W, int O, int R, int S,
                             int stride, int pad, int64_t div, primia_stream_t st) {
    FaithDiv f{0, 0, 0, 0};      // div = 0: the product shares are left untruncated (the faithful chain truncates them)
    PRIMIA_REQUIRE(x0 && x1 && w0 && w1 && a0 && b0 && c0 && a1 && b1 && c1 && out0 && out1 && out0 != out1 && scratch &&
                   (div == 0 || faith_div_make(div, &f)));
    PRIMIA_REQUIRE(out0 != x0 && out0 != x1 && out1 != x0 && out1 != x1);
    ConvGeom g;
    const int rc = conv_plan(B, C, H, W, O, R, S, stride, pad, 2, &g);
    if (rc != PRIMIA_OK) return rc;
    hipStream_t s = (hipStream_t)st;
    const long nx = (long)B * C * H * W, nw = (long)O * C * R * S;
    u64* delta = (u64*)scratch;
    u64* eps = delta + nx;
    u64* b0e = eps + nw;
    conv_open_local_kernel<<<conv_blocks(nx + nw), 256, 0, s>>>(CU(x0), CU(x1), CU(w0), CU(w1), CU(a0), CU(a1), CU(b0), CU(b1),
                                                                delta, eps, b0e, nx, nw);
    if (launch_status() != PRIMIA_OK) return PRIMIA_ERR_LAUNCH;
    const ConvJob jobs[2] = {{delta, b0e, CU(a0), eps, CU(c0), (u64*)out0}, {delta, CU(b1), CU(a1), eps, CU(c1), (u64*)out1}};
    return launch_conv(jobs, 2, g, R, stride, f, s);
}

int primia_triple_conv_c1(const int64_t* a0, const int64_t* a1, const int64_t* b0, const int64_t* b1, const int64_t* c0,
                          int64_t* c1, int64_t* scratch, int B, int C, int H, int W, int O, int R, int S, int stride, int pad,
                          primia_stream_t st) {
    PRIMIA_REQUIRE(a0 && a1 && b0 && b1 && c0 && c1 && c0 != c1 && scratch);
    ConvGeom g;
    const int rc = conv_plan(B, C, H, W, O, R, S, stride, pad, 1, &g);
    if (rc != PRIMIA_OK) return rc;
    hipStream_t s = (hipStream_t)st;
    const long nx = (long)B * C * H * W, nw = (long)O * C * R * S, n = (long)B * O * g.Ho * g.Wo;
    // a = a0 + a1, b = b0 + b1 (scratch: [B C H W | O C R S]); c1 = conv(a, b); c1 -= c0
    u64* sa = (u64*)scratch;
    u64* sb = sa + nx;
    conv_addsub_kernel<false><<<conv_blocks(nx), 256, 0, s>>>(CU(a0), CU(a1), sa, nx);
    conv_addsub_kernel<false><<<conv_blocks(nw), 256, 0, s>>>(CU(b0), CU(b1), sb, nw);
    if (launch_status() != PRIMIA_OK) return PRIMIA_ERR_LAUNCH;
    const ConvJob job{sa, sb, nullptr, nullptr, nullptr, (u64*)c1};
    const int rc2 = launch_conv(&job, 1, g, R, stride, FaithDiv{0, 0, 0, 0}, s);
    if (rc2 != PRIMIA_OK) return rc2;
    conv_addsub_kernel<true><<<conv_blocks(n), 256, 0, s>>>(CU(c1), CU(c0), (u64*)c1, n);
    return launch_status();
}

}  // extern "C"
