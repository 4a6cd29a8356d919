// Secret-shared GroupNorm(groups, C) with BOTH parties' shares on this GPU: the norm of the BatchNorm-free network that
// train.py builds for differentially_private = yes.  The reference has no secret-shared GroupNorm; the layer is defined
// from the reference's own building blocks (DESIGN.md §4 "GroupNorm on shares"):
//   X_j   = x_j.reshape(R, m)                      R = B * groups, m = (C / groups) * HW: a group is m contiguous elements
//   mean  = trunc_div(wrapping row sum of X_j, m)   per share (AST.mean, additive_shared.py:719-729)
//   Xc    = X - mean[:, None]                       party local
//   Sq    = fpt_mul(Xc, Xc)                         triple ("mul", (R, m), (R, m)) + each party's truncation by `div`
//   var   = trunc_div(wrapping row sum of Sq_j, m)
//   inv   = newton(var + eps)                       primia_newton_reciprocal_local, between the two entries of this file
//   N     = fpt_mul(inv, Xc.T).T                    triple ("mul", (R,), (m, R)): a ~ inv, b, c ~ [m, R]
//   out   = fpt_mul(rows(N), weight) + bias         rows [B*HW, C], triple ("mul", (B*HW, C), (C,)), as batch_norm's affine part
// As in csrc/secure_local.hip a thread computes what each party computes, in the party's own arithmetic (unsigned
// wrap-around, truncation toward zero per share), an "open" is the addition of two values that sit side by side, and the
// results are bit-identical to the step-by-step chain (SecureContext.group_norm with local_fused = False) and to the CPU
// composition of OracleContext methods (tests/test_gpu_secure_groupnorm.py).  Ring sums are exact in any order, so a group is
// summed by as many workgroups as its size asks for and the partial sums are added in a second pass: no atomics, the same
// bits in every run.
// The wide-range form (SecureContext.group_norm(wide=True), tests/secure_gn_wide_nets.py) carries var and inv at the scale
// s_it = 10^6 whatever `div`: the squares are truncated by div * div / s_it (primia_gn_moments_wide_local), inv comes from
// the undamped Newton iteration of rsqrt_newton_local_kernel below, and inv * Xc.T is truncated by s_it
// (primia_gn_apply_wide_local).  Same kernels, same triples, same order.
#include "common.h"

namespace primia {

typedef unsigned long long u64;

namespace {

constexpr int GN_THREADS = 256;
constexpr int GN_CHUNK = 1024;      // elements of a group per workgroup: the stem of a 224 x 224 image (32 groups of 25,088) is 800 workgroups

__device__ __forceinline__ u64 gn_trunc(u64 v, u64 d) {        // a party's truncation of ITS share toward zero
    const int64_t sv = (int64_t)v;
    const u64 mag = sv < 0 ? (u64)0 - v : v;
    const u64 q = mag / d;
    return sv < 0 ? (u64)0 - q : q;
}

struct GnPair {
    const u64 *p0, *p1;
};
struct GnOut {
    u64 *p0, *p1;
};
struct GnTriple {          // a pairs with the first operand, b with the second, c = a * b (shares of both parties)
    const u64 *a0, *b0, *c0, *a1, *b1, *c1;
};

// the wrapping sums of (s0, s1) over the workgroup, returned to every thread; `red` is used once per call site
__device__ __forceinline__ void gn_block_sum2(u64& s0, u64& s1, u64 (*red)[2]) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s0 += __shfl_down(s0, off, 64);
        s1 += __shfl_down(s1, off, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wave][0] = s0;
        red[wave][1] = s1;
    }
    __syncthreads();
    s0 = s1 = 0;
#pragma unroll
    for (int w = 0; w < GN_THREADS / 64; ++w) {
        s0 += red[w][0];
        s1 += red[w][1];
    }
}

// sum of elements [lo, hi) of both shares; VEC: lo and the bases are even / 16-byte aligned -> 128-bit loads
template <bool VEC>
__device__ __forceinline__ void gn_range_sum(const u64* __restrict__ x0, const u64* __restrict__ x1, long lo, long hi, u64& s0,
                                             u64& s1) {
    s0 = s1 = 0;
    if (VEC) {
        for (long e = lo + 2 * threadIdx.x; e < hi; e += 2 * GN_THREADS) {      // (hi - lo is even: m is)
            const ulonglong2 v0 = *reinterpret_cast<const ulonglong2*>(x0 + e);
            const ulonglong2 v1 = *reinterpret_cast<const ulonglong2*>(x1 + e);
            s0 += v0.x + v0.y;
            s1 += v1.x + v1.y;
        }
    } else {
        for (long e = lo + threadIdx.x; e < hi; e += GN_THREADS) {
            s0 += x0[e];
            s1 += x1[e];
        }
    }
}

__device__ __forceinline__ void gn_square(u64 x0, u64 x1, u64 m0, u64 m1, u64 a0, u64 b0, u64 c0, u64 a1, u64 b1, u64 c1, u64 div,
                                          u64& s0, u64& s1) {
    const u64 y0 = x0 - m0, y1 = x1 - m1;
    const u64 delta = (y0 - a0) + (y1 - a1), eps = (y0 - b0) + (y1 - b1);
    s0 += gn_trunc(delta * b0 + a0 * eps + c0 + delta * eps, div);
    s1 += gn_trunc(delta * b1 + a1 * eps + c1, div);
}

// sum over [lo, hi) of each party's truncated share of (x - mean)^2 (Beaver square with its open inside)
template <bool VEC>
__device__ __forceinline__ void gn_range_sq(GnPair x, GnTriple t, long lo, long hi, u64 m0, u64 m1, u64 div, u64& s0, u64& s1) {
    s0 = s1 = 0;
    if (VEC) {
        typedef const ulonglong2* V;
        for (long e = lo + 2 * threadIdx.x; e < hi; e += 2 * GN_THREADS) {
            const ulonglong2 x0 = *(V)(x.p0 + e), x1 = *(V)(x.p1 + e);
            const ulonglong2 a0 = *(V)(t.a0 + e), b0 = *(V)(t.b0 + e), c0 = *(V)(t.c0 + e);
            const ulonglong2 a1 = *(V)(t.a1 + e), b1 = *(V)(t.b1 + e), c1 = *(V)(t.c1 + e);
            gn_square(x0.x, x1.x, m0, m1, a0.x, b0.x, c0.x, a1.x, b1.x, c1.x, div, s0, s1);
            gn_square(x0.y, x1.y, m0, m1, a0.y, b0.y, c0.y, a1.y, b1.y, c1.y, div, s0, s1);
        }
    } else {
        for (long e = lo + threadIdx.x; e < hi; e += GN_THREADS)
            gn_square(x.p0[e], x.p1[e], m0, m1, t.a0[e], t.b0[e], t.c0[e], t.a1[e], t.b1[e], t.c1[e], div, s0, s1);
    }
}

// ---- a group per workgroup (m <= GN_CHUNK): sums, mean, square, variance in one launch ---------------------------------
template <bool VEC>
__global__ __launch_bounds__(GN_THREADS) void gn_moments_group_kernel(GnPair x, GnTriple t, GnOut mean, GnOut var, long m, u64 div) {
    __shared__ u64 red[2][GN_THREADS / 64][2];
    const long r = blockIdx.x, lo = r * m, hi = lo + m;
    u64 s0, s1;
    gn_range_sum<VEC>(x.p0, x.p1, lo, hi, s0, s1);
    gn_block_sum2(s0, s1, red[0]);
    const u64 m0 = gn_trunc(s0, (u64)m), m1 = gn_trunc(s1, (u64)m);
    gn_range_sq<VEC>(x, t, lo, hi, m0, m1, div, s0, s1);
    gn_block_sum2(s0, s1, red[1]);
    if (threadIdx.x == 0) {
        mean.p0[r] = m0;
        mean.p1[r] = m1;
        var.p0[r] = gn_trunc(s0, (u64)m);
        var.p1[r] = gn_trunc(s1, (u64)m);
    }
}

// ---- a group over S workgroups: partial sums [R][S][2] -> (mean, partial sums of squares [R][S][2]) -> variance -------
template <bool VEC>
__global__ __launch_bounds__(GN_THREADS) void gn_sum_part_kernel(GnPair x, u64* __restrict__ part, long m, int S) {
    __shared__ u64 red[GN_THREADS / 64][2];
    const long r = blockIdx.x / S;
    const int s = (int)(blockIdx.x - r * S);
    const long lo = r * m + (long)s * GN_CHUNK;
    const long end = (r + 1) * m;
    const long hi = lo + GN_CHUNK < end ? lo + GN_CHUNK : end;
    u64 s0, s1;
    gn_range_sum<VEC>(x.p0, x.p1, lo, hi, s0, s1);
    gn_block_sum2(s0, s1, red);
    if (threadIdx.x == 0) {
        part[2 * (long)blockIdx.x] = s0;
        part[2 * (long)blockIdx.x + 1] = s1;
    }
}

template <bool VEC>
__global__ __launch_bounds__(GN_THREADS) void gn_sq_part_kernel(GnPair x, GnTriple t, const u64* __restrict__ part,
                                                                u64* __restrict__ part_sq, GnOut mean, long m, int S, u64 div) {
    __shared__ u64 red[2][GN_THREADS / 64][2];
    const long r = blockIdx.x / S;
    const int s = (int)(blockIdx.x - r * S);
    u64 s0 = 0, s1 = 0;
    for (int k = threadIdx.x; k < S; k += GN_THREADS) {      // this group's sum: every one of its workgroups forms it
        s0 += part[2 * (r * S + k)];
        s1 += part[2 * (r * S + k) + 1];
    }
    gn_block_sum2(s0, s1, red[0]);
    const u64 m0 = gn_trunc(s0, (u64)m), m1 = gn_trunc(s1, (u64)m);
    if (s == 0 && threadIdx.x == 0) {
        mean.p0[r] = m0;
        mean.p1[r] = m1;
    }
    const long lo = r * m + (long)s * GN_CHUNK;
    const long end = (r + 1) * m;
    const long hi = lo + GN_CHUNK < end ? lo + GN_CHUNK : end;
    gn_range_sq<VEC>(x, t, lo, hi, m0, m1, div, s0, s1);
    gn_block_sum2(s0, s1, red[1]);
    if (threadIdx.x == 0) {
        part_sq[2 * (long)blockIdx.x] = s0;
        part_sq[2 * (long)blockIdx.x + 1] = s1;
    }
}

__global__ __launch_bounds__(GN_THREADS) void gn_var_kernel(const u64* __restrict__ part_sq, GnOut var, long R, long m, int S) {
    const long r = (long)blockIdx.x * GN_THREADS + threadIdx.x;
    if (r >= R) return;
    u64 s0 = 0, s1 = 0;
    for (int k = 0; k < S; ++k) {
        s0 += part_sq[2 * (r * S + k)];
        s1 += part_sq[2 * (r * S + k) + 1];
    }
    var.p0[r] = gn_trunc(s0, (u64)m);
    var.p1[r] = gn_trunc(s1, (u64)m);
}

// ---- normalise + affine (steps 7-8 of the definition), NCHW in, NCHW out -----------------------------------------------
// The tile and its LDS padding are those of bn_eval_local_kernel (csrc/secure_local.hip): 32 positions x 32 channels of
// ONE image; x / out are read and written along HW, both triples along the channel.  What differs from batch_norm:
//   * mean and inv belong to the GROUP r = b * groups + c / cg, and Xc = x - mean is recomputed here, not stored;
//   * triple t1 is in the [m, R] layout of Xc.T: element (p, r) with p = (c % cg) * HW + hw sits at p * R + r -- for
//     the 32 consecutive channels of a tile that is cg runs of 32 / cg consecutive words;
//   * triple t2 is in batch_norm's rows layout [B*HW, C].
struct GnVec {
    const u64 *mean0, *mean1, *inv0, *inv1, *w0, *w1, *bias0, *bias1;
};
// div1 truncates the first product, div2 the second: equal in the default form (both at the fixed-point scale); the
// wide-range form keeps inv at the iteration's finer scale and takes that scale back out with div1.
__global__ __launch_bounds__(256) void gn_apply_local_kernel(GnPair x, GnVec v, GnTriple t1, GnTriple t2, GnOut out, int C, int HW,
                                                             int groups, int cg, u64 div1, u64 div2) {
    __shared__ u64 tile[2][32][33];
    const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;       // 32 x 8
    const long img = (long)blockIdx.z * C * HW;                   // this image's [C][HW] plane of x / out
    const long row0 = (long)blockIdx.z * HW;                      // ... its first row of t2
    const long R = (long)gridDim.z * groups;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = c0 + ty + 8 * k, p = p0 + tx;
        if (c < C && p < HW) {
            tile[0][ty + 8 * k][tx] = x.p0[img + (long)c * HW + p];
            tile[1][ty + 8 * k][tx] = x.p1[img + (long)c * HW + p];
        }
    }
    __syncthreads();
    u64 r0[4], r1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = p0 + ty + 8 * k, c = c0 + tx;
        r0[k] = r1[k] = 0;
        if (c < C && p < HW) {
            const int g = c / cg;
            const long r = (long)blockIdx.z * groups + g;
            const long i1 = ((long)(c - g * cg) * HW + p) * R + r;
            const long i2 = (row0 + p) * C + c;
            const u64 y0 = tile[0][tx][ty + 8 * k] - v.mean0[r], y1 = tile[1][tx][ty + 8 * k] - v.mean1[r];
            u64 n0, n1;
            // fpt_mul(inv, Xc.T): the small operand (inv) is the FIRST one -> its triple side is `a`
            {
                const u64 delta = (v.inv0[r] - t1.a0[r]) + (v.inv1[r] - t1.a1[r]);
                const u64 eps = (y0 - t1.b0[i1]) + (y1 - t1.b1[i1]);
                n0 = gn_trunc(delta * t1.b0[i1] + t1.a0[r] * eps + t1.c0[i1] + delta * eps, div1);
                n1 = gn_trunc(delta * t1.b1[i1] + t1.a1[r] * eps + t1.c1[i1], div1);
            }
            // fpt_mul(rows, weight) + bias
            const u64 delta = (n0 - t2.a0[i2]) + (n1 - t2.a1[i2]);
            const u64 eps = (v.w0[c] - t2.b0[c]) + (v.w1[c] - t2.b1[c]);
            r0[k] = gn_trunc(delta * t2.b0[c] + t2.a0[i2] * eps + t2.c0[i2] + delta * eps, div2) + v.bias0[c];
            r1[k] = gn_trunc(delta * t2.b1[c] + t2.a1[i2] * eps + t2.c1[i2], div2) + v.bias1[c];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        tile[0][tx][ty + 8 * k] = r0[k];
        tile[1][tx][ty + 8 * k] = r1[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = c0 + ty + 8 * k, p = p0 + tx;
        if (c < C && p < HW) {
            out.p0[img + (long)c * HW + p] = tile[0][ty + 8 * k][tx];
            out.p1[img + (long)c * HW + p] = tile[1][ty + 8 * k][tx];
        }
    }
}

// ---- v^-1/2 by the UNDAMPED Newton iteration x <- x (3 - v x^2) / 2, both parties in one launch ------------------------
// The sibling of newton_local_kernel (csrc/ring.hip) for the wide-range GroupNorm: one thread carries one element of both
// parties through all `steps` iterates, at the iteration's own scale s_it.
//   x_1 = 3 x0 / 2 - trunc(v, first_div)            x0 public: formed by the parties locally (party 0 adds the constant)
//   x_{k+1}: xx = trunc(x * x, s_it); vxx = trunc(v * xx, s_it); y = 3 s_it - vxx; x = trunc(y * x, 2 s_it)
// every product a Beaver multiplication with its open inside, every truncation per share, `3 s_it - t` the re-sharing
// of the public constant with a fresh mask -- the order and arithmetic of SecureContext.rsqrt_newton's chain.
//   prim: device array of pointers, in consumption order:  (steps - 1) x { T1 (a0,b0,c0,a1,b1,c1), T2, mask, T3 }
__global__ __launch_bounds__(64) void rsqrt_newton_local_kernel(const u64* __restrict__ v0, const u64* __restrict__ v1,
                                                                const u64* const* __restrict__ prim, u64 s_it, u64 x0, u64 first_div,
                                                                int steps, u64* __restrict__ o0, u64* __restrict__ o1, long n) {
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const u64 c3 = 3 * s_it;
    const u64 va = v0[i], vb = v1[i];
    auto mul = [&](u64 xa, u64 xb, u64 ya, u64 yb, const u64* const* t, u64 d, u64& za, u64& zb) {
        const u64 a0 = t[0][i], b0 = t[1][i], c0 = t[2][i], a1 = t[3][i], b1 = t[4][i], c1 = t[5][i];
        const u64 delta = (xa - a0) + (xb - a1), eps = (ya - b0) + (yb - b1);
        za = gn_trunc(delta * b0 + a0 * eps + c0 + delta * eps, d);
        zb = gn_trunc(delta * b1 + a1 * eps + c1, d);
    };
    u64 xa = gn_trunc(3 * x0, 2) - gn_trunc(va, first_div);
    u64 xb = (u64)0 - gn_trunc(vb, first_div);
    const u64* const* pp = prim;
#pragma unroll 1
    for (int it = 1; it < steps; ++it, pp += 19) {
        u64 qa, qb, ta, tb;
        mul(xa, xb, xa, xb, pp, s_it, qa, qb);             // x * x
        mul(va, vb, qa, qb, pp + 6, s_it, ta, tb);         // v * (x * x)
        const u64 r = pp[12][0];                           // 3 - ...: the constant re-shared as (r, 3 s_it - r)
        const u64 ya = (u64)0 - (ta - r), yb = (u64)0 - (tb - (c3 - r));
        mul(ya, yb, xa, xb, pp + 13, 2 * s_it, xa, xb);    // y * x / 2
    }
    o0[i] = xa;
    o1[i] = xb;
}

inline bool gn_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace primia

using namespace primia;

#define U(p) ((const u64*)(p))

extern "C" {

int64_t primia_gn_moments_local_scratch_elems(int64_t R, int64_t m) {
    if (R <= 0 || m <= 0) return PRIMIA_ERR_ARG;
    const int64_t S = (m + GN_CHUNK - 1) / GN_CHUNK;
    return S == 1 ? 0 : 4 * R * S;
}

int primia_gn_moments_local(const int64_t* x0, const int64_t* x1, const int64_t* a0, const int64_t* b0, const int64_t* c0,
                            const int64_t* a1, const int64_t* b1, const int64_t* c1, int64_t* mean0, int64_t* mean1,
                            int64_t* var0, int64_t* var1, int64_t* scratch, int64_t R, int64_t m, int64_t div,
                            primia_stream_t st) {
    PRIMIA_REQUIRE(x0 && x1 && a0 && b0 && c0 && a1 && b1 && c1 && mean0 && mean1 && var0 && var1 && R > 0 && m > 0 && div > 0);
    PRIMIA_REQUIRE(mean0 != mean1 && var0 != var1 && mean0 != var0 && mean0 != var1 && mean1 != var0 && mean1 != var1);
    const int64_t S = (m + GN_CHUNK - 1) / GN_CHUNK;
    PRIMIA_REQUIRE(R <= 0x7fffffffL / S && (S == 1 || scratch));
    hipStream_t s = (hipStream_t)st;
    const GnPair x{U(x0), U(x1)};
    const GnTriple t{U(a0), U(b0), U(c0), U(a1), U(b1), U(c1)};
    const GnOut mean{(u64*)mean0, (u64*)mean1}, var{(u64*)var0, (u64*)var1};
    // 128-bit loads: every group (and every chunk: GN_CHUNK is even) starts on an even element of 16-byte aligned arrays
    const bool vec = m % 2 == 0 && gn_aligned16(x0) && gn_aligned16(x1) && gn_aligned16(a0) && gn_aligned16(b0) &&
                     gn_aligned16(c0) && gn_aligned16(a1) && gn_aligned16(b1) && gn_aligned16(c1);
    if (S == 1) {
        if (vec)
            gn_moments_group_kernel<true><<<(unsigned)R, GN_THREADS, 0, s>>>(x, t, mean, var, m, (u64)div);
        else
            gn_moments_group_kernel<false><<<(unsigned)R, GN_THREADS, 0, s>>>(x, t, mean, var, m, (u64)div);
        return launch_status();
    }
    u64* part = (u64*)scratch;
    u64* part_sq = part + 2 * R * S;
    const unsigned blocks = (unsigned)(R * S);
    if (vec) {
        gn_sum_part_kernel<true><<<blocks, GN_THREADS, 0, s>>>(x, part, m, (int)S);
        gn_sq_part_kernel<true><<<blocks, GN_THREADS, 0, s>>>(x, t, part, part_sq, mean, m, (int)S, (u64)div);
    } else {
        gn_sum_part_kernel<false><<<blocks, GN_THREADS, 0, s>>>(x, part, m, (int)S);
        gn_sq_part_kernel<false><<<blocks, GN_THREADS, 0, s>>>(x, t, part, part_sq, mean, m, (int)S, (u64)div);
    }
    gn_var_kernel<<<(unsigned)((R + GN_THREADS - 1) / GN_THREADS), GN_THREADS, 0, s>>>(part_sq, var, R, m, (int)S);
    return launch_status();
}

static int gn_apply_launch(const int64_t* x0, const int64_t* x1, const int64_t* mean0, const int64_t* mean1, const int64_t* inv0,
                           const int64_t* inv1, const int64_t* w0, const int64_t* w1, const int64_t* bias0, const int64_t* bias1,
                           const int64_t* const* t1, const int64_t* const* t2, int64_t* out0, int64_t* out1, int B, int C, int HW,
                           int groups, int64_t div1, int64_t div2, primia_stream_t st) {
    PRIMIA_REQUIRE(x0 && x1 && mean0 && mean1 && inv0 && inv1 && w0 && w1 && bias0 && bias1 && t1 && t2 && out0 && out1 &&
                   out0 != out1 && B > 0 && B <= 65535 && C > 0 && HW > 0 && groups > 0 && div1 > 0 && div2 > 0);
    for (int k = 0; k < 6; ++k) PRIMIA_REQUIRE(t1[k] && t2[k]);
    if (C % groups != 0) return PRIMIA_ERR_UNSUPPORTED;
    PRIMIA_REQUIRE((C + 31) / 32 <= 65535);
    const dim3 grid((HW + 31) / 32, (C + 31) / 32, B);
    gn_apply_local_kernel<<<grid, 256, 0, (hipStream_t)st>>>(
        GnPair{U(x0), U(x1)}, GnVec{U(mean0), U(mean1), U(inv0), U(inv1), U(w0), U(w1), U(bias0), U(bias1)},
        GnTriple{U(t1[0]), U(t1[1]), U(t1[2]), U(t1[3]), U(t1[4]), U(t1[5])},
        GnTriple{U(t2[0]), U(t2[1]), U(t2[2]), U(t2[3]), U(t2[4]), U(t2[5])}, GnOut{(u64*)out0, (u64*)out1}, C, HW, groups,
        C / groups, (u64)div1, (u64)div2);
    return launch_status();
}

int primia_gn_apply_local(const int64_t* x0, const int64_t* x1, const int64_t* mean0, const int64_t* mean1, const int64_t* inv0,
                          const int64_t* inv1, const int64_t* w0, const int64_t* w1, const int64_t* bias0, const int64_t* bias1,
                          const int64_t* const* t1, const int64_t* const* t2, int64_t* out0, int64_t* out1, int B, int C, int HW,
                          int groups, int64_t div, primia_stream_t st) {
    return gn_apply_launch(x0, x1, mean0, mean1, inv0, inv1, w0, w1, bias0, bias1, t1, t2, out0, out1, B, C, HW, groups, div, div,
                           st);
}

int primia_gn_apply_wide_local(const int64_t* x0, const int64_t* x1, const int64_t* mean0, const int64_t* mean1,
                               const int64_t* inv0, const int64_t* inv1, const int64_t* w0, const int64_t* w1,
                               const int64_t* bias0, const int64_t* bias1, const int64_t* const* t1, const int64_t* const* t2,
                               int64_t* out0, int64_t* out1, int B, int C, int HW, int groups, int64_t div_it, int64_t div,
                               primia_stream_t st) {
    return gn_apply_launch(x0, x1, mean0, mean1, inv0, inv1, w0, w1, bias0, bias1, t1, t2, out0, out1, B, C, HW, groups, div_it,
                           div, st);
}

int primia_gn_moments_wide_local(const int64_t* x0, const int64_t* x1, const int64_t* a0, const int64_t* b0, const int64_t* c0,
                                 const int64_t* a1, const int64_t* b1, const int64_t* c1, int64_t* mean0, int64_t* mean1,
                                 int64_t* var0, int64_t* var1, int64_t* scratch, int64_t R, int64_t m, int64_t sq_div,
                                 primia_stream_t st) {
    // the kernels divide by whatever they are given and gn_trunc(v, 1) == v for every v: the wide form's moments are the
    // default form's with the squares' divisor chosen by the caller
    return primia_gn_moments_local(x0, x1, a0, b0, c0, a1, b1, c1, mean0, mean1, var0, var1, scratch, R, m, sq_div, st);
}

int primia_rsqrt_newton_local(const int64_t* v0, const int64_t* v1, const int64_t* const* prim, int64_t s_it, int64_t x0,
                              int64_t first_div, int steps, int64_t* out0, int64_t* out1, int64_t n, primia_stream_t st) {
    PRIMIA_REQUIRE(v0 && v1 && out0 && out1 && out0 != out1 && n > 0 && s_it > 0 && x0 > 0 && first_div > 0 && steps >= 1);
    PRIMIA_REQUIRE(steps == 1 || prim);
    PRIMIA_REQUIRE(n <= 0x7fffffffL * 64);
    rsqrt_newton_local_kernel<<<(unsigned)((n + 63) / 64), 64, 0, (hipStream_t)st>>>(U(v0), U(v1), (const u64* const*)prim,
                                                                                     (u64)s_it, (u64)x0, (u64)first_div, steps,
                                                                                     (u64*)out0, (u64*)out1, (long)n);
    return launch_status();
}

}  // extern "C"
