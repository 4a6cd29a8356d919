// Which kernel serves a convolution call: ONE decision per pass — conv_route() (forward and data gradient, conv_igemm.hip),
// wgrad_route() (weight gradient, conv_wgrad.hip) — read by the entry points, which switch on it, and by every host query
// (kernel ids, partial-table rows, *_ok, workspace bytes).  Host only.  A route reads the option table (lh2, lh2_bm, lh4, s2lh,
// c64_blocks) and the CU count, so it is asked again after an option changes (primia_options_epoch).  The shape limits live
// next to their kernels, as *_ok() / geometry functions (conv3x3_lh.h, conv_wgrad.h); the routes only order them.
#pragma once
#include "conv3x3_lh.h"
#include "conv_wgrad.h"

namespace primia {

// The values ARE the public ids of primia_conv_kernel_id (include/primia_hip.h).
enum ConvKernel {
    kConvIgemm = 1,   // conv_igemm_kernel      every shape ConvGeom takes (bf16 and fp32)
    kConvC64 = 2,     // conv3x3_c64_kernel     3x3 / 1, 64 -> 64
    kConvLh2 = 4,     // conv3x3_lh2_kernel     3x3 / 1, output channels in 128s, images up to 28 wide: 392- or 196-pixel tiles
    kConvS2lh = 5,    // conv_s2lh_kernel       3x3 / 2 and 1x1 / 2 on the parity planes (option s2lh)
    kConvLh4 = 6,     // conv3x3_lh4_kernel     the 196-pixel tiles of kConvLh2's shapes (option lh4)
};

// The forms the entry points have: what the write-back does beside storing the tile.
enum ConvForm {
    kFwd,                    // primia_conv2d_fwd
    kFwdStats,               // primia_conv2d_fwd_stats            + BatchNorm statistics of y
    kFwdPair,                // primia_conv2d_fwd_stats_pair       conv1 3x3 / 2 + downsample 1x1 / 2 of one x (asked of conv1)
    kDgrad,                  // primia_conv2d_dgrad, accumulate = 0
    kDgradAcc,               //                      accumulate = 1
    kDgradMaskedAcc,         // primia_conv2d_dgrad_masked_acc     dx = mask(dx) + dgrad
    kDgradBnSums,            // primia_conv2d_dgrad_bnsums         + backward sums of the BatchNorm in front (LhBnBwd)
    kDgradMaskedAccBnSums,   // primia_conv2d_dgrad_masked_acc_bnsums   (C64AccBnb modes 2 and 3)
    kDgradPair,              // primia_conv2d_dgrad_pair           conv1 + downsample into one dx (asked of conv1)
    kDgradPairBnSums,        // primia_conv2d_dgrad_pair_bnsums    + backward sums of the residual BatchNorm (S2BnBwd)
};

struct ConvRoute {
    int kernel;   // a ConvKernel, or PRIMIA_ERR_UNSUPPORTED: no kernel has this form for this shape
    int slots;    // rows of the per-tile partial table the kernel writes for the form (statistics, BatchNorm sums); 0: none
};
ConvRoute conv_route(const ConvGeom& g, int dtype, ConvForm form);

struct WgradRoute {   // (the forms of a weight-gradient call: WgradForm, conv_wgrad.h)
    int kernel;        // batched forms: 13, 14, 15, 17, 18; norm pass: also 21 - 26 (the id tables of include/primia_hip.h)
    size_t ws_bytes;   // kWgWorkspace: the partial tiles of that kernel (0 for the other forms)
};
WgradRoute wgrad_route(const WgradParams& p, const ConvGeom& g, int dtype, WgradForm form);

}  // namespace primia
