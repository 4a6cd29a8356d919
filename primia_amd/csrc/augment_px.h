// The per-pixel arithmetic of the augmentation chain, shared by the per-image kernels (augment.hip) and the batched
// kernels (augment_batch.hip): both call THESE functions, so a batched stage computes bit for bit what the per-image
// stage computes — by construction, not by coincidence.  Every product is rounded on its own, as the NumPy / OpenCV float
// arithmetic these functions follow does: no fused multiply-add contraction anywhere in a file that includes this header.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace primia {

__device__ __forceinline__ int reflect101(int p, int n) {   // BORDER_REFLECT_101: gfedcb|abcdefgh|gfedcba
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * (n - 1) - p;
    return p;
}

__device__ __forceinline__ uint8_t sat_u8(float v) { return (uint8_t)fminf(fmaxf(rintf(v), 0.f), 255.f); }

// ---- RandomAffine: PIL Image.transform(AFFINE, NEAREST): source index = floor(a (x + .5) + b (y + .5) + c) ----------
// true: output pixel (y, x) of an H x W image reads source pixel (yi, xi); false: it is zero fill
__device__ __forceinline__ bool affine_source(int H, int W, float a, float b, float c, float d, float e, float f, int y, int x,
                                              int& yi, int& xi) {
    const double xs = (double)a * (x + 0.5) + (double)b * (y + 0.5) + (double)c;
    const double ys = (double)d * (x + 0.5) + (double)e * (y + 0.5) + (double)f;
    xi = (int)floor(xs);
    yi = (int)floor(ys);
    return xi >= 0 && xi < W && yi >= 0 && yi < H;
}

// ---- Resize(R, R) + crop: the four bilinear taps (cv2.INTER_LINEAR, half-pixel centres, clamped) of pixel (ry, rx) of
// the R x R image over an Hin x Win source, and their blend rounded to a uint8 level
struct ResizeTaps {
    int y0, y1, x0, x1;
    float fy, fx;
};

__device__ __forceinline__ ResizeTaps resize_taps(int Hin, int Win, int R, int ry, int rx) {
    ResizeTaps t;
    const float sy = ((float)ry + 0.5f) * ((float)Hin / (float)R) - 0.5f;
    const float sx = ((float)rx + 0.5f) * ((float)Win / (float)R) - 0.5f;
    int y0 = (int)floorf(sy), x0 = (int)floorf(sx);
    float fy = sy - (float)y0, fx = sx - (float)x0;
    if (y0 < 0) { y0 = 0; fy = 0.f; }
    if (x0 < 0) { x0 = 0; fx = 0.f; }
    int y1 = y0 + 1, x1 = x0 + 1;
    if (y1 >= Hin) { y1 = Hin - 1; if (y0 >= Hin - 1) { y0 = Hin - 1; fy = 0.f; } }
    if (x1 >= Win) { x1 = Win - 1; if (x0 >= Win - 1) { x0 = Win - 1; fx = 0.f; } }
    t.y0 = y0; t.y1 = y1; t.x0 = x0; t.x1 = x1; t.fy = fy; t.fx = fx;
    return t;
}

__device__ __forceinline__ uint8_t resize_blend(float p00, float p01, float p10, float p11, float fx, float fy) {
    const float top = p00 + (p01 - p00) * fx, bot = p10 + (p11 - p10) * fx;
    return (uint8_t)fminf(fmaxf(floorf(top + (bot - top) * fy + 0.5f), 0.f), 255.f);
}

// ---- CLAHE (OpenCV clahe.cpp), 8 x 8 tiles, on one uint8 plane with pixel stride `ps` ---------------------------
// one 256-thread block per tile (tx, ty) of a grid ntx tiles wide: histogram of the (reflect-padded) tile, clip,
// redistribute, cumulative LUT.  hist / scan: 256 ints of shared memory each.
__device__ __forceinline__ void clahe_lut_tile(const uint8_t* __restrict__ img, int H, int W, int ps, int tw, int th, int clip,
                                               int tx, int ty, int ntx, int* hist, int* scan, uint8_t* __restrict__ lut) {
    const int t = threadIdx.x;
    hist[t] = 0;
    __syncthreads();
    for (int i = t; i < tw * th; i += 256) {
        const int y = reflect101(ty * th + i / tw, H), x = reflect101(tx * tw + i % tw, W);
        atomicAdd(&hist[img[((long)y * W + x) * ps]], 1);
    }
    __syncthreads();
    if (clip > 0) {
        // clipped = sum of the excesses; every bin gets clipped / 256, the residual goes to bins 0, step, 2 step, ...
        int v = hist[t];
        const int ex = v > clip ? v - clip : 0;
        scan[t] = ex;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (t < o) scan[t] += scan[t + o];
            __syncthreads();
        }
        const int clipped = scan[0];
        __syncthreads();
        const int batch = clipped / 256;
        int residual = clipped - batch * 256;
        v = (v > clip ? clip : v) + batch;
        if (residual != 0) {
            int step = 256 / residual;
            if (step < 1) step = 1;
            if (t % step == 0 && t / step < residual) ++v;
        }
        hist[t] = v;
        __syncthreads();
    }
    // inclusive prefix sum (Hillis-Steele), then lut = saturate(round_half_even(sum * 255 / tile_area))
    scan[t] = hist[t];
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int add = t >= o ? scan[t - o] : 0;
        __syncthreads();
        scan[t] += add;
        __syncthreads();
    }
    const float scale = 255.0f / (float)(tw * th);
    float r = rintf((float)scan[t] * scale);
    r = fminf(fmaxf(r, 0.f), 255.f);
    lut[((long)(ty * ntx + tx)) * 256 + t] = (uint8_t)r;
}

__device__ __forceinline__ void clahe_apply_px(const uint8_t* __restrict__ img, int W, int ps, int tw, int th, int tiles,
                                               const uint8_t* __restrict__ lut, uint8_t* __restrict__ out, int idx) {
    const int y = idx / W, x = idx - y * W;
    const float txf = (float)x * (1.0f / (float)tw) - 0.5f, tyf = (float)y * (1.0f / (float)th) - 0.5f;
    int tx1 = (int)floorf(txf), ty1 = (int)floorf(tyf);
    const float xa = txf - (float)tx1, ya = tyf - (float)ty1;
    int tx2 = tx1 + 1, ty2 = ty1 + 1;
    tx1 = tx1 < 0 ? 0 : tx1;
    ty1 = ty1 < 0 ? 0 : ty1;
    tx2 = tx2 > tiles - 1 ? tiles - 1 : tx2;
    ty2 = ty2 > tiles - 1 ? tiles - 1 : ty2;
    const int v = img[(long)idx * ps];
    const float l11 = lut[(ty1 * tiles + tx1) * 256 + v], l12 = lut[(ty1 * tiles + tx2) * 256 + v];
    const float l21 = lut[(ty2 * tiles + tx1) * 256 + v], l22 = lut[(ty2 * tiles + tx2) * 256 + v];
    const float res = (l11 * (1.0f - xa) + l12 * xa) * (1.0f - ya) + (l21 * (1.0f - xa) + l22 * xa) * ya;
    out[(long)idx * ps] = (uint8_t)fminf(fmaxf(rintf(res), 0.f), 255.f);
}

// OpenCV's tile geometry and integer clip limit for an H x W plane
__host__ __device__ __forceinline__ void clahe_geometry(int H, int W, float clip_limit, int& tw, int& th, int& clip) {
    const int tiles = 8;
    tw = (W + tiles - 1) / tiles;
    th = (H + tiles - 1) / tiles;      // tile size of the padded image
    clip = 0;
    if (clip_limit > 0.f) {
        clip = (int)(clip_limit * (float)(tw * th) / 256.0f);
        if (clip < 1) clip = 1;
    }
}

// ---- RGB <-> CIE L*a*b* (D65, sRGB transfer), 8 bit: L * 255 / 100, a + 128, b + 128 ---------------------------
__device__ __forceinline__ float srgb_to_linear(float c) { return c <= 0.04045f ? c / 12.92f : powf((c + 0.055f) / 1.055f, 2.4f); }
__device__ __forceinline__ float linear_to_srgb(float c) { return c <= 0.0031308f ? 12.92f * c : 1.055f * powf(c, 1.0f / 2.4f) - 0.055f; }
__device__ __forceinline__ float lab_f(float t) { return t > 0.008856f ? cbrtf(t) : 7.787f * t + 16.0f / 116.0f; }

__device__ __forceinline__ void rgb_lab_px(const uint8_t* __restrict__ in, int inverse, uint8_t* __restrict__ out, long i) {
    const float p0 = in[3 * i], p1 = in[3 * i + 1], p2 = in[3 * i + 2];
    if (!inverse) {
        const float r = srgb_to_linear(p0 / 255.f), g = srgb_to_linear(p1 / 255.f), b = srgb_to_linear(p2 / 255.f);
        const float X = (0.412453f * r + 0.357580f * g + 0.180423f * b) / 0.950456f;
        const float Y = 0.212671f * r + 0.715160f * g + 0.072169f * b;
        const float Z = (0.019334f * r + 0.119193f * g + 0.950227f * b) / 1.088754f;
        const float fx = lab_f(X), fy = lab_f(Y), fz = lab_f(Z);
        const float L = Y > 0.008856f ? 116.f * fy - 16.f : 903.3f * Y;
        out[3 * i] = sat_u8(L * 255.f / 100.f);
        out[3 * i + 1] = sat_u8(500.f * (fx - fy) + 128.f);
        out[3 * i + 2] = sat_u8(200.f * (fy - fz) + 128.f);
    } else {
        const float L = p0 * 100.f / 255.f, a = p1 - 128.f, b = p2 - 128.f;
        const float fy = (L + 16.f) / 116.f, fx = fy + a / 500.f, fz = fy - b / 200.f;
        auto inv = [](float t) { return t > 0.206893f ? t * t * t : (t - 16.f / 116.f) / 7.787f; };
        const float X = inv(fx) * 0.950456f, Y = L > 7.9996f ? inv(fy) : L / 903.3f, Z = inv(fz) * 1.088754f;
        const float r = 3.240479f * X - 1.537150f * Y - 0.498535f * Z;
        const float g = -0.969256f * X + 1.875991f * Y + 0.041556f * Z;
        const float bl = 0.055648f * X - 0.204043f * Y + 1.057311f * Z;
        out[3 * i] = sat_u8(linear_to_srgb(fminf(fmaxf(r, 0.f), 1.f)) * 255.f);
        out[3 * i + 1] = sat_u8(linear_to_srgb(fminf(fmaxf(g, 0.f), 1.f)) * 255.f);
        out[3 * i + 2] = sat_u8(linear_to_srgb(fminf(fmaxf(bl, 0.f), 1.f)) * 255.f);
    }
}

// ---- cv2.blur(img, (k, k)): normalised box filter, BORDER_REFLECT_101, rounded to nearest -------------------------
__device__ __forceinline__ void box_blur_px(const uint8_t* __restrict__ in, int H, int W, int C, int k,
                                            uint8_t* __restrict__ out, int idx) {
    const int y = idx / W, x = idx - y * W, a = k / 2;      // window [p - k / 2, p - k / 2 + k - 1]: cv2's default anchor
    for (int c = 0; c < C; ++c) {
        int s = 0;
        for (int dy = -a; dy < k - a; ++dy)
            for (int dx = -a; dx < k - a; ++dx)
                s += in[((long)reflect101(y + dy, H) * W + reflect101(x + dx, W)) * C + c];
        out[(long)idx * C + c] = sat_u8((float)s / (float)(k * k));
    }
}

// ---- cv2.remap(INTER_LINEAR, BORDER_REFLECT_101) of one pixel at float32 source coordinates (x, y) -----------------
// Bilinear weights in fp32, result rounded to nearest even (cv2's 8-bit path uses 5-bit fixed-point coordinates:
// unpinned, see oracle/augment_oracle.py).
__device__ __forceinline__ void remap_px(const uint8_t* __restrict__ src, int H, int W, int C, float x, float y,
                                         uint8_t* __restrict__ out, int idx) {
    const float x0f = floorf(x), y0f = floorf(y);
    const float fx = x - x0f, fy = y - y0f;
    // (coordinates far outside the image — a degenerate affine draw — are clamped before the integer conversion; the
    // reflection below is periodic, so the clamp only has to keep the value representable)
    const int x0 = (int)fminf(fmaxf(x0f, -1.0e6f), 1.0e6f), y0 = (int)fminf(fmaxf(y0f, -1.0e6f), 1.0e6f);
    const int xa = reflect101(x0, W), xb = reflect101(x0 + 1, W), ya = reflect101(y0, H), yb = reflect101(y0 + 1, H);
    for (int c = 0; c < C; ++c) {
        const float p00 = src[((long)ya * W + xa) * C + c], p01 = src[((long)ya * W + xb) * C + c];
        const float p10 = src[((long)yb * W + xa) * C + c], p11 = src[((long)yb * W + xb) * C + c];
        const float top = p00 * (1.f - fx) + p01 * fx, bot = p10 * (1.f - fx) + p11 * fx;
        out[(long)idx * C + c] = sat_u8(top * (1.f - fy) + bot * fy);
    }
}

// the float32 map value of pixel idx of an H x W image:
// kind 0: affine  (p = inverse matrix a b c d e f: source = (a x + b y + c, d x + e y + f)), cv2.warpAffine
// kind 1: optical (p = k, fx, fy, cx, cy, ncx, ncy): cv2.initUndistortRectifyMap with distortion (k, k, 0, 0, 0)
__device__ __forceinline__ void warp_coord(int W, int kind, double p0, double p1, double p2, double p3, double p4, double p5,
                                           double p6, int idx, float& mx, float& my) {
    const double y = idx / W, x = idx - (idx / W) * W;
    if (kind == 0) {
        mx = (float)(p0 * x + p1 * y + p2);
        my = (float)(p3 * x + p4 * y + p5);
    } else {
        const double u = (x - p5) / p1, v = (y - p6) / p2;
        const double r2 = u * u + v * v;
        const double kr = 1.0 + p0 * r2 + p0 * r2 * r2;
        mx = (float)(p1 * (u * kr) + p3);
        my = (float)(p2 * (v * kr) + p4);
    }
}

// GridDistortion: map_x, map_y = meshgrid(xx, yy)  |  ElasticTransform: map = float32(index + displacement)
__device__ __forceinline__ void grid_coord(int W, const float* __restrict__ xx, const float* __restrict__ yy,
                                           const float* __restrict__ dx, const float* __restrict__ dy, int idx, float& mx,
                                           float& my) {
    const int y = idx / W, x = idx - y * W;
    mx = xx ? xx[x] : (float)x + dx[idx];
    my = yy ? yy[y] : (float)y + dy[idx];
}

// scipy.ndimage.gaussian_filter's tap weights: exp(-t^2 / (2 sigma^2)) over their sum from -radius to radius
__device__ __forceinline__ double gauss_tap(double sigma, int t) { return exp(-0.5 / (sigma * sigma) * (double)t * (double)t); }
__device__ __forceinline__ double gauss_wsum(double sigma, int radius) {
    double wsum = 0.0;
    for (int t = -radius; t <= radius; ++t) wsum += gauss_tap(sigma, t);
    return wsum;
}

// the 1-D pass (correlate1d, mode "reflect": d c b a | a b c d | d c b a), float64, on u = 2 r - 1 of a uniform field r
// (affine_in) or on the first pass's output.  Weights: `w` = the 2 radius + 1 normalised taps if given, else computed here.
__device__ __forceinline__ double gauss1d_px(const double* __restrict__ in, int H, int W, int axis, double sigma, int radius,
                                             int affine_in, double scale, const double* __restrict__ w, int idx) {
    const int y = idx / W, x = idx - y * W;
    const int n = axis == 0 ? H : W, p = axis == 0 ? y : x;
    const double wsum = w ? 0.0 : gauss_wsum(sigma, radius);
    double acc = 0.0;
    for (int t = -radius; t <= radius; ++t) {
        int q = p + t;
        const int period = 2 * n;                      // half-sample symmetric reflection
        q %= period;
        if (q < 0) q += period;
        if (q >= n) q = period - 1 - q;
        double v = in[axis == 0 ? (long)q * W + x : (long)y * W + q];
        if (affine_in) v = v * 2.0 - 1.0;
        acc += v * (w ? w[t + radius] : gauss_tap(sigma, t) / wsum);
    }
    acc *= scale;
    return acc;
}

// ---- RandomFog (F.add_fog): per haze point a white disc of radius hw / 2 blended in with cv2.addWeighted(alpha) ---------
// sequentially (a pixel covered by m discs is blended m times, in list order)
__device__ __forceinline__ void fog_px(const uint8_t* __restrict__ in, int W, int C, const int* __restrict__ haze, int n, int hw,
                                       float alpha, float beta, uint8_t* __restrict__ out, int idx) {
    const int y = idx / W, x = idx - y * W, rad = hw / 2;
    float v[3];
    for (int c = 0; c < C; ++c) v[c] = in[(long)idx * C + c];
    for (int i = 0; i < n; ++i) {
        const int dx = x - (haze[2 * i] + hw / 2), dy = y - (haze[2 * i + 1] + hw / 2);
        if (dx * dx + dy * dy <= rad * rad)
            for (int c = 0; c < C; ++c) v[c] = fminf(fmaxf(rintf(255.f * alpha + v[c] * beta), 0.f), 255.f);
    }
    for (int c = 0; c < C; ++c) out[(long)idx * C + c] = (uint8_t)v[c];
}

// ---- GaussNoise: image + noise (fp32), clipped to [0, 255], cast to uint8 (truncation, as ndarray.astype) ----------
__device__ __forceinline__ uint8_t add_noise_px(uint8_t v, float noise) { return (uint8_t)fminf(fmaxf((float)v + noise, 0.f), 255.f); }

// ---- ToFloat(255) + Normalize(mean, std, max_pixel_value = 1): uint8 HWC -> fp32 CHW ------------------------------
__device__ __forceinline__ void finish_px(const uint8_t* __restrict__ in, int S, int C, const float* __restrict__ mean,
                                          const float* __restrict__ stdv, float* __restrict__ out, int idx) {
    for (int c = 0; c < C; ++c) {
        float v = (float)in[(long)idx * C + c] / 255.0f;
        if (mean) v = (v - mean[c]) / stdv[c];
        out[(long)c * S * S + idx] = v;
    }
}

// F.cutout: pixel (y, x) lies in one of the n rectangles (x1, y1, x2, y2)
__device__ __forceinline__ bool rects_hit(const int* __restrict__ rects, int n, int y, int x) {
    bool hit = false;
    for (int k = 0; k < n && !hit; ++k) hit = x >= rects[4 * k] && x < rects[4 * k + 2] && y >= rects[4 * k + 1] && y < rects[4 * k + 3];
    return hit;
}

}  // namespace primia
