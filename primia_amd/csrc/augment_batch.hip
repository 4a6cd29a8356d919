// The augmentation chain of create_albu_transform (torchlib/dataloader.py:138-217) a BATCH at a time: one launch per stage
// covers every image of the batch on which the stage fired.  A loader that feeds the training step from an image folder
// (primia_amd/imagefolder.py AugmentingLoader) transforms batch_size images per step; the per-image entry points of
// augment.hip cost it 4 to 15 launches and as many small host-to-device copies per IMAGE.
//
// Grid = (pixel tiles, active images).  Image blockIdx.y reads its record from device tables the host uploads once per
// batch (primia_amd/augment.py TrainTransform.batch): an int64 pointer table (the source and destination of the image's
// current S x S x C slice, as primia_newton_reciprocal_local takes its primitives) and int32 / float / double parameter
// tables.  The arithmetic is augment_px.h's, the functions the per-image kernels call: results are bit-identical to the
// per-image chain (tests/test_gpu_augment_batch.py).  Memory-bound work on a few MB: plain loads and stores.
#include "augment_px.h"

#pragma clang fp contract(off)

namespace primia {

static __device__ __forceinline__ const uint8_t* cptr(const int64_t* t, long i) { return (const uint8_t*)(uintptr_t)t[i]; }
static __device__ __forceinline__ uint8_t* mptr(const int64_t* t, long i) { return (uint8_t*)(uintptr_t)t[i]; }

// ---- RandomAffine + Resize(R, R) + RandomCrop(S, S) in one pass -----------------------------------------------------
// affine_u8_kernel is a nearest-neighbour gather with zero fill, so pixel (y, x) of the warped image IS
// src[affine_source(y, x)] or 0: each of resize_crop_u8_kernel's four taps is read through it and the full-size warped
// image is never written.  ip: (H, W, has_affine, oy, ox) per image; fp: the inverse matrix a..f.
__device__ __forceinline__ float affine_tap(const uint8_t* __restrict__ src, int H, int W, int C, int has_affine,
                                            const float* __restrict__ m, int y, int x, int c) {
    int yi = y, xi = x;
    if (has_affine && !affine_source(H, W, m[0], m[1], m[2], m[3], m[4], m[5], y, x, yi, xi)) return 0.f;
    return (float)src[((long)yi * W + xi) * C + c];
}

__global__ __launch_bounds__(256) void affine_resize_crop_batch_kernel(const int64_t* __restrict__ ptrs,
                                                                       const int* __restrict__ ip,
                                                                       const float* __restrict__ fp, int C, int R, int S) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (idx >= S * S) return;
    const uint8_t* src = cptr(ptrs, 2L * b);
    uint8_t* out = mptr(ptrs, 2L * b + 1);
    const int* q = ip + 5L * b;
    const float* m = fp + 6L * b;
    const int H = q[0], W = q[1], has_affine = q[2], oy = q[3], ox = q[4];
    const int y = idx / S, x = idx - y * S;
    const ResizeTaps t = resize_taps(H, W, R, y + oy, x + ox);
    for (int c = 0; c < C; ++c) {
        const float p00 = affine_tap(src, H, W, C, has_affine, m, t.y0, t.x0, c);
        const float p01 = affine_tap(src, H, W, C, has_affine, m, t.y0, t.x1, c);
        const float p10 = affine_tap(src, H, W, C, has_affine, m, t.y1, t.x0, c);
        const float p11 = affine_tap(src, H, W, C, has_affine, m, t.y1, t.x1, c);
        out[(long)idx * C + c] = resize_blend(p00, p01, p10, p11, t.fx, t.fy);
    }
}

// ---- CLAHE: primia_clahe_u8's four kernels with the image as a grid dimension ---------------------------------------
// workspace of image b: ws + b * ws_stride = [64 tile LUTs][L*a*b* copy when C = 3]
__global__ __launch_bounds__(256) void rgb_lab_batch_kernel(const int64_t* __restrict__ ptrs, int which, int inverse,
                                                            uint8_t* __restrict__ ws, long ws_stride, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= n) return;
    uint8_t* lab = ws + b * ws_stride + 64 * 256;
    if (!inverse) rgb_lab_px(cptr(ptrs, 2 * b + which), 0, lab, i);
    else rgb_lab_px(lab, 1, mptr(ptrs, 2 * b + which), i);
}

__global__ __launch_bounds__(256) void clahe_lut_batch_kernel(const int64_t* __restrict__ ptrs, int C, int H, int W, int tw,
                                                              int th, int clip, uint8_t* __restrict__ ws, long ws_stride) {
    __shared__ int hist[256];
    __shared__ int scan[256];
    const long b = blockIdx.z;
    uint8_t* lut = ws + b * ws_stride;
    const uint8_t* img = C == 1 ? cptr(ptrs, 2 * b) : lut + 64 * 256;
    clahe_lut_tile(img, H, W, C, tw, th, clip, blockIdx.x, blockIdx.y, gridDim.x, hist, scan, lut);
}

__global__ __launch_bounds__(256) void clahe_apply_batch_kernel(const int64_t* __restrict__ ptrs, int C, int H, int W, int tw,
                                                                int th, int tiles, uint8_t* __restrict__ ws, long ws_stride) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const long b = blockIdx.y;
    if (idx >= H * W) return;
    uint8_t* lut = ws + b * ws_stride;
    if (C == 1) clahe_apply_px(cptr(ptrs, 2 * b), W, 1, tw, th, tiles, lut, mptr(ptrs, 2 * b + 1), idx);
    else clahe_apply_px(lut + 64 * 256, W, 3, tw, th, tiles, lut, lut + 64 * 256, idx);      // L in place (pointwise)
}

// ---- VerticalFlip + cv2.LUT: ip = (flip, table index or -1) per image ------------------------------------------------
__global__ __launch_bounds__(256) void flip_lut_batch_kernel(const int64_t* __restrict__ ptrs, const int* __restrict__ ip,
                                                             const uint8_t* __restrict__ luts, int S, int C) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (idx >= S * S) return;
    const uint8_t* src = cptr(ptrs, 2L * b);
    uint8_t* out = mptr(ptrs, 2L * b + 1);
    const int flip = ip[2 * b], ti = ip[2 * b + 1];
    const int y = idx / S, x = idx - y * S;
    const long from = ((long)(flip ? S - 1 - y : y) * S + x) * C;
    for (int c = 0; c < C; ++c) {
        const uint8_t v = src[from + c];
        out[(long)idx * C + c] = ti >= 0 ? luts[(long)ti * 256 + v] : v;
    }
}

__global__ __launch_bounds__(256) void box_blur_batch_kernel(const int64_t* __restrict__ ptrs, const int* __restrict__ ks,
                                                             int S, int C) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (idx >= S * S) return;
    box_blur_px(cptr(ptrs, 2L * b), S, S, C, ks[b], mptr(ptrs, 2L * b + 1), idx);
}

// ---- cv2.remap with the coordinate computed here: kind 0 affine / 1 optical from dp[7]; 2 grid axes (aux0 = xx, aux1 =
// yy); 3 index + displacement planes (aux0 = dx, aux1 = dy).  ptrs: (src, dst, aux0, aux1) per image.
__global__ __launch_bounds__(256) void warp_batch_kernel(const int64_t* __restrict__ ptrs, const int* __restrict__ kinds,
                                                         const double* __restrict__ dp, int S, int C) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (idx >= S * S) return;
    const int kind = kinds[b];
    float mx, my;
    if (kind <= 1) {
        const double* p = dp + 7L * b;
        warp_coord(S, kind, p[0], p[1], p[2], p[3], p[4], p[5], p[6], idx, mx, my);
    } else {
        const float* a0 = (const float*)cptr(ptrs, 4L * b + 2);
        const float* a1 = (const float*)cptr(ptrs, 4L * b + 3);
        if (kind == 2) grid_coord(S, a0, a1, nullptr, nullptr, idx, mx, my);
        else grid_coord(S, nullptr, nullptr, a0, a1, idx, mx, my);
    }
    remap_px(cptr(ptrs, 4L * b), S, S, C, mx, my, mptr(ptrs, 4L * b + 1), idx);
}

// ---- ElasticTransform's displacements: gaussian_filter(2 field - 1, sigma) * alpha for every plane of the batch ------
// the 2 radius + 1 normalised taps depend on the tap index only: filled once per call, with gauss1d_kernel's expression
__global__ __launch_bounds__(256) void gauss_weights_kernel(double sigma, int radius, double* __restrict__ w) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > 2 * radius) return;
    const double wsum = gauss_wsum(sigma, radius);
    w[i] = gauss_tap(sigma, i - radius) / wsum;
}

__global__ __launch_bounds__(256) void gauss1d_batch_kernel(const double* __restrict__ in, int H, int W, int axis, double sigma,
                                                            int radius, int affine_in, double scale,
                                                            const double* __restrict__ w, double* __restrict__ out,
                                                            float* __restrict__ out32) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= H * W) return;
    const long plane = (long)blockIdx.y * H * W;
    const double acc = gauss1d_px(in + plane, H, W, axis, sigma, radius, affine_in, scale, w, idx);
    if (out32) out32[plane + idx] = (float)acc;
    else out[plane + idx] = acc;
}

// ---- RandomFog's haze discs: ip = (hw, first haze point, haze points) per image into one (x, y) list ---------------
__global__ __launch_bounds__(256) void fog_batch_kernel(const int64_t* __restrict__ ptrs, const int* __restrict__ ip,
                                                        const float* __restrict__ alphas, const int* __restrict__ haze, int S,
                                                        int C) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (idx >= S * S) return;
    const float alpha = alphas[b];
    fog_px(cptr(ptrs, 2L * b), S, C, haze + 2L * ip[3 * b + 1], ip[3 * b + 2], ip[3 * b], alpha, 1.f - alpha,
           mptr(ptrs, 2L * b + 1), idx);
}

// ---- F.cutout in place: ip = (first rectangle, rectangles) per image ------------------------------------------------
__global__ __launch_bounds__(256) void fill_rects_batch_kernel(const int64_t* __restrict__ ptrs, const int* __restrict__ ip,
                                                               const int* __restrict__ rects, int S, int C, int fill) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (idx >= S * S) return;
    const int y = idx / S, x = idx - y * S;
    if (rects_hit(rects + 4L * ip[2 * b], ip[2 * b + 1], y, x)) {
        uint8_t* img = mptr(ptrs, b);
        for (int c = 0; c < C; ++c) img[(long)idx * C + c] = (uint8_t)fill;
    }
}

// ---- GaussNoise in place: noise plane b holds standard normal values, scaled here by the image's sigma (torch's
// `randn * sigma` on a float32 tensor: one float32 product) ---------------------------------------------------------
__global__ __launch_bounds__(256) void add_noise_batch_kernel(const int64_t* __restrict__ ptrs, const float* __restrict__ noise,
                                                              const float* __restrict__ sigmas, long per_image) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= per_image) return;
    uint8_t* img = mptr(ptrs, b);
    const float v = noise[b * per_image + i] * sigmas[b];
    img[i] = add_noise_px(img[i], v);
}

__global__ __launch_bounds__(256) void finish_batch_kernel(const int64_t* __restrict__ ptrs, int S, int C,
                                                           const float* __restrict__ mean, const float* __restrict__ stdv) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (idx >= S * S) return;
    finish_px(cptr(ptrs, 2L * b), S, C, mean, stdv, (float*)mptr(ptrs, 2L * b + 1), idx);
}

}  // namespace primia

using namespace primia;

extern "C" {

int primia_image_affine_resize_crop_batch_u8(const int64_t* ptrs, const int32_t* ip, const float* fp, int n, int C, int R,
                                             int S, primia_stream_t st) {
    if (n == 0) return PRIMIA_OK;
    PRIMIA_REQUIRE(ptrs && ip && fp && n > 0 && n <= PRIMIA_BATCH_MAX && (C == 1 || C == 3) && R > 0 && S > 0 && S <= R);
    affine_resize_crop_batch_kernel<<<dim3(ceil_div((long)S * S, 256), n), 256, 0, (hipStream_t)st>>>(ptrs, (const int*)ip, fp,
                                                                                                     C, R, S);
    return launch_status();
}

int primia_clahe_batch_u8(const int64_t* ptrs, int n, int H, int W, int C, float clip_limit, void* workspace,
                          int64_t workspace_bytes, primia_stream_t stream) {
    if (n == 0) return PRIMIA_OK;
    PRIMIA_REQUIRE(ptrs && workspace && n > 0 && n <= PRIMIA_BATCH_MAX && H >= 8 && W >= 8 && (C == 1 || C == 3) &&
                   clip_limit >= 0.f);
    const int64_t stride = primia_clahe_workspace_bytes(H, W, C);
    if (workspace_bytes < stride * n) return PRIMIA_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int tiles = 8;
    int tw, th, clip;
    clahe_geometry(H, W, clip_limit, tw, th, clip);
    uint8_t* ws = (uint8_t*)workspace;
    const long npx = (long)H * W;
    const dim3 px(ceil_div(npx, 256), n);
    if (C == 3) rgb_lab_batch_kernel<<<px, 256, 0, st>>>(ptrs, 0, 0, ws, stride, npx);
    clahe_lut_batch_kernel<<<dim3(tiles, tiles, n), 256, 0, st>>>(ptrs, C, H, W, tw, th, clip, ws, stride);
    clahe_apply_batch_kernel<<<px, 256, 0, st>>>(ptrs, C, H, W, tw, th, tiles, ws, stride);
    if (C == 3) rgb_lab_batch_kernel<<<px, 256, 0, st>>>(ptrs, 1, 1, ws, stride, npx);
    return launch_status();
}

int primia_image_flip_lut_batch_u8(const int64_t* ptrs, const int32_t* ip, const uint8_t* luts, int n, int S, int C,
                                   primia_stream_t st) {
    if (n == 0) return PRIMIA_OK;
    PRIMIA_REQUIRE(ptrs && ip && luts && n > 0 && n <= PRIMIA_BATCH_MAX && S > 0 && (C == 1 || C == 3));
    flip_lut_batch_kernel<<<dim3(ceil_div((long)S * S, 256), n), 256, 0, (hipStream_t)st>>>(ptrs, (const int*)ip, luts, S, C);
    return launch_status();
}

int primia_image_box_blur_batch_u8(const int64_t* ptrs, const int32_t* ks, int n, int S, int C, primia_stream_t st) {
    if (n == 0) return PRIMIA_OK;
    PRIMIA_REQUIRE(ptrs && ks && n > 0 && n <= PRIMIA_BATCH_MAX && S > 0 && (C == 1 || C == 3));
    box_blur_batch_kernel<<<dim3(ceil_div((long)S * S, 256), n), 256, 0, (hipStream_t)st>>>(ptrs, (const int*)ks, S, C);
    return launch_status();
}

int primia_image_warp_batch_u8(const int64_t* ptrs, const int32_t* kinds, const double* dp, int n, int S, int C,
                               primia_stream_t st) {
    if (n == 0) return PRIMIA_OK;
    PRIMIA_REQUIRE(ptrs && kinds && dp && n > 0 && n <= PRIMIA_BATCH_MAX && S > 0 && (C == 1 || C == 3));
    warp_batch_kernel<<<dim3(ceil_div((long)S * S, 256), n), 256, 0, (hipStream_t)st>>>(ptrs, (const int*)kinds, dp, S, C);
    return launch_status();
}

int64_t primia_warp_elastic_disp_workspace_bytes(int n, int H, int W, double sigma) {
    const int64_t radius = (int64_t)(4.0 * sigma + 0.5);
    return 8 * (2 * radius + 1) + (int64_t)n * 2 * H * W * 8;
}

int primia_warp_elastic_disp_batch(const double* fields, int n, int H, int W, double sigma, double alpha, void* workspace,
                                   int64_t workspace_bytes, float* disp, primia_stream_t stream) {
    if (n == 0) return PRIMIA_OK;
    PRIMIA_REQUIRE(fields && workspace && disp && n > 0 && 2 * n <= PRIMIA_BATCH_MAX && H > 0 && W > 0 && sigma > 0.0 &&
                   sigma < 1.0e6);
    if (workspace_bytes < primia_warp_elastic_disp_workspace_bytes(n, H, W, sigma)) return PRIMIA_ERR_WORKSPACE;
    const int radius = (int)(4.0 * sigma + 0.5);          // scipy: truncate = 4.0
    double* w = (double*)workspace;
    double* tmp = w + (2 * radius + 1);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(ceil_div((long)H * W, 256), 2 * n);
    gauss_weights_kernel<<<ceil_div(2 * radius + 1, 256), 256, 0, st>>>(sigma, radius, w);
    gauss1d_batch_kernel<<<grid, 256, 0, st>>>(fields, H, W, 0, sigma, radius, 1, 1.0, w, tmp, nullptr);
    gauss1d_batch_kernel<<<grid, 256, 0, st>>>(tmp, H, W, 1, sigma, radius, 0, alpha, w, nullptr, disp);
    return launch_status();
}

int primia_image_fog_batch_u8(const int64_t* ptrs, const int32_t* ip, const float* alphas, const int32_t* haze_xy, int n, int S,
                              int C, primia_stream_t st) {
    if (n == 0) return PRIMIA_OK;
    PRIMIA_REQUIRE(ptrs && ip && alphas && haze_xy && n > 0 && n <= PRIMIA_BATCH_MAX && S > 0 && (C == 1 || C == 3));
    fog_batch_kernel<<<dim3(ceil_div((long)S * S, 256), n), 256, 0, (hipStream_t)st>>>(ptrs, (const int*)ip, alphas,
                                                                                      (const int*)haze_xy, S, C);
    return launch_status();
}

int primia_image_fill_rects_batch_u8(const int64_t* ptrs, const int32_t* ip, const int32_t* rects, int n, int S, int C,
                                     int fill, primia_stream_t st) {
    if (n == 0) return PRIMIA_OK;
    PRIMIA_REQUIRE(ptrs && ip && rects && n > 0 && n <= PRIMIA_BATCH_MAX && S > 0 && (C == 1 || C == 3) && fill >= 0 &&
                   fill <= 255);
    fill_rects_batch_kernel<<<dim3(ceil_div((long)S * S, 256), n), 256, 0, (hipStream_t)st>>>(ptrs, (const int*)ip,
                                                                                             (const int*)rects, S, C, fill);
    return launch_status();
}

int primia_image_add_noise_batch_u8(const int64_t* ptrs, const float* noise, const float* sigmas, int n, int64_t per_image,
                                    primia_stream_t st) {
    if (n == 0 || per_image == 0) return PRIMIA_OK;
    PRIMIA_REQUIRE(ptrs && noise && sigmas && n > 0 && n <= PRIMIA_BATCH_MAX && per_image > 0);
    add_noise_batch_kernel<<<dim3(ceil_div(per_image, 256), n), 256, 0, (hipStream_t)st>>>(ptrs, noise, sigmas, per_image);
    return launch_status();
}

int primia_image_finish_batch(const int64_t* ptrs, int n, int S, int C, const float* mean, const float* stdv,
                              primia_stream_t st) {
    if (n == 0) return PRIMIA_OK;
    PRIMIA_REQUIRE(ptrs && n > 0 && n <= PRIMIA_BATCH_MAX && S > 0 && (C == 1 || C == 3) &&
                   ((mean == nullptr) == (stdv == nullptr)));
    finish_batch_kernel<<<dim3(ceil_div((long)S * S, 256), n), 256, 0, (hipStream_t)st>>>(ptrs, S, C, mean, stdv);
    return launch_status();
}

}  // extern "C"
