// Launch parameters shared by the weight-gradient kernels (conv_wgrad.hip, conv_wgrad_patch.hip).
#pragma once
#include "conv_common.h"

namespace primia {

// The forms of a weight-gradient call.  kWgAccumulate adds into a zeroed dw (atomics, no workspace), kWgWorkspace stores
// per-block partial tiles and reduces them in a fixed order; the per-sample forms are DP-SGD's, one split per image: every
// sample's tiles written to dw [N][K][klen], only their squared norms added to sqnorm, or the norms added and the tiles KEPT.
enum WgradForm { kWgAccumulate, kWgWorkspace, kWgPersampleTiles, kWgPersampleSqnorm, kWgPersampleKeep };
static inline bool wgrad_persample(WgradForm f) { return f >= kWgPersampleTiles; }
static inline bool wgrad_norm_pass(WgradForm f) { return f == kWgPersampleSqnorm || f == kWgPersampleKeep; }

struct WgradParams {
    const void* x;
    const void* dy;
    float* dw;
    int N, H, W, C, K, R, S, stride, pad, Ho, Wo;
    int klen;
    long Md;           // N*Ho*Wo
    int ntaps;         // R*S, or R for the stem
    int nkt, nct;      // channel tiles
    int nsplit;        // pixel splits
    long pix_per_split;
    long split_stride;  // 0: every split accumulates into dw; else split i writes dw + i*split_stride
                        // (per-sample gradients for DP-SGD: one split per image, stride K*klen)
    WgradForm form;
    double* sqnorm;    // the norm-pass forms: split i adds the squared L2 norm of ITS gradient tile to
                       // sqnorm[i] instead of writing the tile (the DP-SGD norm pass needs nothing else)
    float* ws;         // optional workspace of the store-and-reduce path (conv_wgrad_patch.hip); null: atomics
    size_t ws_bytes;
    int xpad;          // stem only: x is the padded NHWC4p input [N][H+6][W+8][4] (stem_conv.hip)
    int rec_views;     // kWgPersampleSqnorm: images per RECORD (DP-SGD with augmentation multiplicity) — a split is a record
                       // of rec_views consecutive images and sqnorm has N / rec_views entries; 1: a record is an image
};

// sum over the wave of the squares of `n` accumulator values per lane, added (fp64 atomic) to *dst
__device__ __forceinline__ void wave_sqnorm_add(double s, double* dst) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(dst, s);
}

int wgrad_dma_dispatch(const WgradParams& p, hipStream_t st);
size_t wgrad_dma_ws_bytes(const WgradParams& p);
// halo-patch kernel (3x3 / stride 1 / pad 1, bf16), every form: conv_wgrad_patch33lw_kernel (id 18) for the batched and
// per-sample-tile forms, conv_wgrad_patch33_kernel for the norm pass — one block per (image, slab) (24), or whole images per
// half-block where wgrad_patch_pairimg() (25)
bool wgrad_patch_ok(const WgradParams& p);
bool wgrad_patch_pairimg(const WgradParams& p, WgradForm form);
int wgrad_patch_dispatch(const WgradParams& p, hipStream_t st);
// DP-SGD norm pass of the 7x7-output 3x3 layers from two Gram matrices per sample (dp_ghost.hip): ids 21 / 22, 0 not served
int dp_ghost_kernel_id(int H, int W, int C, int K, int R, int S, int stride, int pad);
int dp_ghost_sqnorm_dispatch(const void* x, const void* dy, double* sq, int N, int H, int W, int C, int K, int R, int S,
                             int stride, int pad, hipStream_t st);
size_t wgrad_patch_ws_bytes(const WgradParams& p);
// up to four layers of one shape in one launch (conv_wgrad_patch.hip): preferred group size for `count` such layers
// (0: shape not served, 1: no gain), workspace of a group of n, and the launch (p[0].ws / ws_bytes = the group's)
int wgrad_patch_group_size(const WgradParams& p, int count);
size_t wgrad_patch_group_ws_bytes(const WgradParams& p, int n);
int wgrad_patch_group_dispatch(const WgradParams* p, int n, hipStream_t st);
// per-tap kernel of the stride-2 / 1x1 layers, second generation (conv_wgrad_tap.hip): the workspace form (id 17) ...
bool wgrad_tap_ok(const WgradParams& p);
int wgrad_tap_dispatch(const WgradParams& p, hipStream_t st);
size_t wgrad_tap_ws_bytes(const WgradParams& p);
// ... and the DP-SGD norm pass of those layers (26): whole images (whole records where p.rec_views > 1) per block,
// squared tile norms added to p.sqnorm
int wgrad_tap_persample_dispatch(const WgradParams& p, hipStream_t st);
// conv1 + downsample of a transition block in one launch (the downsample = a tenth tap with its own dy)
int wgrad_tap_pair_dispatch(const WgradParams& p, const WgradParams& p2, hipStream_t st);
size_t wgrad_tap_pair_ws_bytes(const WgradParams& p, const WgradParams& p2);
// stem (7x7/2) halo kernel on the padded input (stem_conv.hip)
int stem_wgrad_halo_dispatch(const bf16* xp, const bf16* dy, float* dw, int N, int H, int W, hipStream_t st,
                             float* ws = nullptr, size_t ws_bytes = 0, double* sqnorm = nullptr, int rec_views = 1);
size_t stem_wgrad_halo_ws_bytes(int N, int H, int W);   // 0: shape not served by the halo kernel
bool stem_wgrad_halo_blocks(int N, int H, int W, int* total, int* per_block, int* grid);
// dw tile (kt, tap, ct) = sum over nsplit partial tiles of ws [combo][split][BMK*BNC], in split order
// (wgt: DP-SGD clipped sum — split s is sample s, weighted by wgt[s])
void wgrad_tile_reduce(const float* ws, float* dw, int nsplit, int combos, int BMK, int BNC, int nkt, int nct, int C,
                       int klen, int stem, hipStream_t st, const float* wgt = nullptr);
void wgrad_tile_reduce_pair(const float* ws, float* dw, float* dw2, int nsplit, int combos1, int combos2, int BMK, int BNC,
                            int nkt, int nct, int C, int klen, int klen2, hipStream_t st);
// DP-SGD: the patch kernel's norm pass keeping every sample's tiles ([combo][image][slab]); bytes (0: not served / too
// large to be worth it), the pass, and the clipped sum over the kept tiles
size_t wgrad_patch_keep_bytes(const WgradParams& p);
int wgrad_patch_keep_dispatch(const WgradParams& p, hipStream_t st);
int wgrad_patch_clipped_sum(const WgradParams& p, const float* slabs, const float* clip, hipStream_t st);

}  // namespace primia
