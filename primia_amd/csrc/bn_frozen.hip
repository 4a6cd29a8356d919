// Backward pass of BatchNorm applied with FIXED statistics (nn.BatchNorm2d in eval mode while its gamma / beta train):
// DP-SGD fine-tuning from pretrained weights.  Each norm layer is the per-channel affine map
//     z = (y - running_mean) * rsqrt(running_var + eps) * gamma + beta
// so a sample's gradient depends on that sample alone — what DP-SGD needs, and what training-mode BatchNorm cannot give.
// The forward pass is primia_bn_fwd_eval (csrc/bn.hip, bn_apply_kernel with eval_mode = 1).
//
// Reference: autograd of F.batch_norm(..., training=False) (+ F.relu, the residual add) under loss.backward(),
// torchlib/models.py:261-264.
//
// Unlike training-mode BatchNorm, dy does not depend on the sums: ONE pass over the tensors writes dy (and the masked
// gradient) and carries the per-(sample, channel) sums of the affine gradients along.  Layout [N][HW][C]; a block owns a
// slab of rows of ONE sample (grid = slabs x N), so no sum ever crosses a sample.  No floating-point atomics: a block adds
// its row groups through LDS in a fixed order, slabs are combined in a fixed order by a finalize launch (or, for a sample of
// one slab, by the block itself) — the same inputs give the same bits.
#include "common.h"

namespace primia {

constexpr int kFrozenSlabs = 32;      // most slabs per sample
constexpr int kFrozenMinRows = 16;    // a slab shorter than this is launch overhead

// slabs per sample and rows per slab: ~4096 blocks over the launch, every slab non-empty
static inline void frozen_geometry(int N, int HW, int& nslab, int& rps) {
    int want = 4096 / N;
    if (want > kFrozenSlabs) want = kFrozenSlabs;
    if (want < 1) want = 1;
    rps = (HW + want - 1) / want;
    if (rps < kFrozenMinRows) rps = kFrozenMinRows;
    if (rps > HW) rps = HW;
    nslab = (HW + rps - 1) / rps;
}

enum { kMaskFromZ = 0, kMaskBytes = 1, kMaskFromY = 2 };

// g = mask ? dz : 0;  dy = g * (gamma * invstd);  g_out = g;  sums over the slab's rows of g and g * xhat.
// Threads are laid out [rows per pass][C / CH]: a thread's channels never change, its per-channel constants live in
// registers.  Two rows per trip: their loads are requested together (g_out may alias dz, so the compiler cannot move a
// load over the store in front of it itself).
template <typename T, int MODE>
__global__ __launch_bounds__(256) void bn_frozen_bwd_kernel(const T* __restrict__ y, const T* __restrict__ z,
                                                            const uint8_t* __restrict__ mask, const T* dz,
                                                            T* __restrict__ dy, T* g_out, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta,
                                                            const float* __restrict__ running_mean,
                                                            const float* __restrict__ running_var, float eps,
                                                            float* __restrict__ ps_dgamma, float* __restrict__ ps_dbeta,
                                                            float* __restrict__ partials, int HW, int C, int rps) {
    constexpr int CH = Chunk<T>::N;
    constexpr int HV = CH / 4;                          // 16-byte pieces of a thread's CH floats
    const int tpr = C / CH, rpp = 256 / tpr;            // threads per row, rows per pass (256 % tpr == 0: bn_shape_ok)
    const int rg = threadIdx.x / tpr, cc = threadIdx.x % tpr;
    const int n = blockIdx.y, slab = blockIdx.x;
    const int c0 = cc * CH;
    const int r0 = slab * rps;
    int r1 = r0 + rps;
    if (r1 > HW) r1 = HW;

    float km[CH], ki[CH], kk[CH], kb[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        km[i] = running_mean[c0 + i];
        ki[i] = 1.f / sqrtf(running_var[c0 + i] + eps);  // bn_apply_kernel's expression
        kk[i] = ki[i] * gamma[c0 + i];                   // ... and its scale: the factor of dy and of the recomputed mask
        kb[i] = MODE == kMaskFromY ? beta[c0 + i] : 0.f;
    }
    float s1[CH], s2[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) s1[i] = s2[i] = 0.f;

    const long row0 = (long)n * HW;                      // the sample's first row
    auto one = [&](long row, const u32x4& ry, const u32x4& rd, const u32x4& rz, unsigned rm) {
        const long off = row * C + c0;
        float vy[CH], vg[CH];
        Chunk<T>::unpack(ry, vy);
        Chunk<T>::unpack(rd, vg);
        if (MODE == kMaskFromZ) {
            if (z) {
                float vz[CH];
                Chunk<T>::unpack(rz, vz);
#pragma unroll
                for (int i = 0; i < CH; ++i) vg[i] = vz[i] > 0.f ? vg[i] : 0.f;
            }
        } else if (MODE == kMaskBytes) {
#pragma unroll
            for (int i = 0; i < CH; ++i) vg[i] = (rm >> i) & 1u ? vg[i] : 0.f;
        } else {
            // the forward pass's own expression, and the sign of what it STORED
#pragma unroll
            for (int i = 0; i < CH; ++i)
                vg[i] = round_to<T>(bn_affine(vy[i], km[i], kk[i], kb[i])) > 0.f ? vg[i] : 0.f;
        }
        if (g_out) *(u32x4*)(g_out + off) = Chunk<T>::pack(vg);
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const float xh = (vy[i] - km[i]) * ki[i];    // never y * invstd - mean * invstd: that form cancels
            s1[i] += vg[i];
            s2[i] = __builtin_fmaf(vg[i], xh, s2[i]);
            vy[i] = vg[i] * kk[i];
        }
        *(u32x4*)(dy + off) = Chunk<T>::pack(vy);
    };
    auto fetch = [&](long row, u32x4& ry, u32x4& rd, u32x4& rz, unsigned& rm) {
        const long off = row * C + c0;
        ry = *(const u32x4*)(y + off);
        rd = *(const u32x4*)(dz + off);
        if (MODE == kMaskFromZ) {
            if (z) rz = *(const u32x4*)(z + off);
        } else if (MODE == kMaskBytes) {
            rm = mask[row * tpr + cc];
        }
    };
    for (int r = r0 + rg; r < r1; r += 2 * rpp) {
        const bool two = r + rpp < r1;
        u32x4 ya, da, za = {}, yb, db, zb = {};
        unsigned ma = 0, mb = 0;
        fetch(row0 + r, ya, da, za, ma);
        fetch(row0 + (two ? r + rpp : r), yb, db, zb, mb);   // (clamped: both rows' loads go out unconditionally)
        one(row0 + r, ya, da, za, ma);
        if (two) one(row0 + r + rpp, yb, db, zb, mb);
    }

    // row groups -> one value per channel.  A thread's CH sums go to LDS as 16-byte pieces, piece h of every thread of a
    // row group side by side (lane stride 16 bytes: no bank conflict); the reading thread finds position p -> channel.
    __shared__ float red[2][256 * CH];                   // [quantity][row group][C]   (rpp * C = 256 * CH)
    const int seg = C / HV;
#pragma unroll
    for (int h = 0; h < HV; ++h) {
        *(f32x4*)&red[0][rg * C + h * seg + cc * 4] = f32x4{s1[4 * h], s1[4 * h + 1], s1[4 * h + 2], s1[4 * h + 3]};
        *(f32x4*)&red[1][rg * C + h * seg + cc * 4] = f32x4{s2[4 * h], s2[4 * h + 1], s2[4 * h + 2], s2[4 * h + 3]};
    }
    __syncthreads();
    for (int p = threadIdx.x; p < C; p += 256) {
        const int h = p / seg, rem = p - h * seg;
        const int c = (rem >> 2) * CH + h * 4 + (rem & 3);
        double a = 0.0, b = 0.0;
        for (int g = 0; g < rpp; ++g) {                  // fixed order
            a += (double)red[0][g * C + p];
            b += (double)red[1][g * C + p];
        }
        if (gridDim.x == 1) {                            // the sample is this one slab: no partials, no finalize launch
            ps_dbeta[(long)n * C + c] = (float)a;
            ps_dgamma[(long)n * C + c] = (float)b;
        } else {
            float* out = partials + ((long)n * gridDim.x + slab) * 2 * C;
            out[c] = (float)a;
            out[C + c] = (float)b;
        }
    }
}

// partials [N][nslab][2][C] -> ps_dbeta / ps_dgamma [N][C], slabs added in order in fp64
__global__ __launch_bounds__(256) void bn_frozen_finalize_kernel(const float* __restrict__ partials, int nslab, int C,
                                                                 float* __restrict__ ps_dgamma,
                                                                 float* __restrict__ ps_dbeta, int NC) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NC) return;
    const int n = i / C, c = i - n * C;
    double a = 0.0, b = 0.0;
    for (int s = 0; s < nslab; ++s) {
        const float* p = partials + ((long)n * nslab + s) * 2 * C;
        a += (double)p[c];
        b += (double)p[C + c];
    }
    ps_dbeta[i] = (float)a;
    ps_dgamma[i] = (float)b;
}

template <typename T, int MODE>
static int bn_frozen_bwd_impl(const void* y, const void* z, const uint8_t* mask, const void* dz, void* dy, void* g_out,
                              const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                              float eps, float* ps_dgamma, float* ps_dbeta, int N, int HW, int C, float* partials,
                              hipStream_t st) {
    int nslab, rps;
    frozen_geometry(N, HW, nslab, rps);
    bn_frozen_bwd_kernel<T, MODE><<<dim3(nslab, N), 256, 0, st>>>((const T*)y, (const T*)z, mask, (const T*)dz, (T*)dy,
                                                                  (T*)g_out, gamma, beta, running_mean, running_var, eps,
                                                                  ps_dgamma, ps_dbeta, partials, HW, C, rps);
    if (nslab > 1)
        bn_frozen_finalize_kernel<<<(N * C + 255) / 256, 256, 0, st>>>(partials, nslab, C, ps_dgamma, ps_dbeta, N * C);
    return launch_status();
}

template <int MODE>
static int bn_frozen_bwd_dispatch(const void* y, const void* z, const uint8_t* mask, const void* dz, void* dy, void* g_out,
                                  const float* gamma, const float* beta, const float* running_mean,
                                  const float* running_var, float eps, float* ps_dgamma, float* ps_dbeta, int N, int HW,
                                  int C, void* workspace, int64_t workspace_bytes, int dtype, hipStream_t st) {
    PRIMIA_REQUIRE(y && dz && dy && gamma && running_mean && running_var && ps_dgamma && ps_dbeta && workspace);
    // (blockIdx.y carries the sample)
    PRIMIA_REQUIRE(N > 0 && N <= PRIMIA_BATCH_MAX && HW > 0 && bn_shape_ok((long)N * HW, C, dtype));
    if (workspace_bytes < primia_bn_frozen_workspace_bytes(N, HW, C)) return PRIMIA_ERR_WORKSPACE;
    return with_dtype(dtype, [&](auto tag) {
        return bn_frozen_bwd_impl<decltype(tag), MODE>(y, z, mask, dz, dy, g_out, gamma, beta, running_mean, running_var, eps,
                                                       ps_dgamma, ps_dbeta, N, HW, C, (float*)workspace, st);
    });
}

}  // namespace primia

using namespace primia;

extern "C" {

int64_t primia_bn_frozen_workspace_bytes(int N, int HW, int C) {
    if (N <= 0 || HW <= 0 || C <= 0) return 0;
    int nslab, rps;
    frozen_geometry(N, HW, nslab, rps);
    return (int64_t)N * nslab * 2 * C * sizeof(float);
}

int primia_bn_frozen_bwd(const void* y, const void* z, const void* dz, void* dy, void* g_out, const float* gamma,
                         const float* running_mean, const float* running_var, float eps, float* ps_dgamma,
                         float* ps_dbeta, int N, int HW, int C, int relu, void* workspace, int64_t workspace_bytes,
                         int dtype, primia_stream_t stream) {
    PRIMIA_REQUIRE(!relu || z);
    return bn_frozen_bwd_dispatch<kMaskFromZ>(y, relu ? z : nullptr, nullptr, dz, dy, g_out, gamma, nullptr, running_mean,
                                              running_var, eps, ps_dgamma, ps_dbeta, N, HW, C, workspace, workspace_bytes,
                                              dtype, (hipStream_t)stream);
}

int primia_bn_frozen_bwd_mask(const void* y, const uint8_t* relu_mask, const void* dz, void* dy, void* g_out,
                              const float* gamma, const float* running_mean, const float* running_var, float eps,
                              float* ps_dgamma, float* ps_dbeta, int N, int HW, int C, void* workspace,
                              int64_t workspace_bytes, int dtype, primia_stream_t stream) {
    PRIMIA_REQUIRE(relu_mask);
    return bn_frozen_bwd_dispatch<kMaskBytes>(y, nullptr, relu_mask, dz, dy, g_out, gamma, nullptr, running_mean,
                                              running_var, eps, ps_dgamma, ps_dbeta, N, HW, C, workspace, workspace_bytes,
                                              dtype, (hipStream_t)stream);
}

int primia_bn_frozen_relu_bwd(const void* y, const void* dz, void* dy, const float* gamma, const float* beta,
                              const float* running_mean, const float* running_var, float eps, float* ps_dgamma,
                              float* ps_dbeta, int N, int HW, int C, void* workspace, int64_t workspace_bytes, int dtype,
                              primia_stream_t stream) {
    PRIMIA_REQUIRE(beta);
    return bn_frozen_bwd_dispatch<kMaskFromY>(y, nullptr, nullptr, dz, dy, nullptr, gamma, beta, running_mean, running_var,
                                              eps, ps_dgamma, ps_dbeta, N, HW, C, workspace, workspace_bytes, dtype,
                                              (hipStream_t)stream);
}

}  // extern "C"
