// Process-wide tuning / dispatch options of the library (include/primia_hip.h: primia_set_option).
// The library never reads the environment: every switch that selects between kernels or sizes a launch is an entry of
// this table, changed only by an explicit primia_set_option(name, value) call of the host.
#pragma once

namespace primia {

#define PRIMIA_OPTIONS(X)                                                                                              \
    X(lh2, 1)               /* 0: the wide 3x3 / stride-1 layers stay on the implicit GEMM */                         \
    X(lh2_bm, 0)            /* 392 | 196: force the linear-halo tile height (0: by shape) */                          \
    X(lh4, 1)               /* 196-pixel tiles on conv3x3_lh4_kernel (8 matrix + 4 loader waves, one barrier per step); 0: conv3x3_lh2 */ \
    X(c64_blocks, 512)      /* persistent blocks of conv3x3_c64_kernel (2 per CU) */                                   \
    X(c64_dbg, 0)           /* timing experiments only (results are WRONG when set): conv3x3_c64_kernel's debug bits */           \
    X(c64_stages, 4)        /* ring depth of conv3x3_c64_kernel: 3 | 4 */                                              \
    X(ring_mfma, 0)         /* 1: the Z_2^64 GEMMs of the encrypted path run ring_gemm_mfma_kernel (int8 limbs on v_mfma_i32_16x16x64_i8, bit-equal); and its direct 3x3 / 1, 3x3 / 2 and 1x1 / 2 convolutions ring_conv_mfma_kernel; 2: as 1, and the 7x7 / 2 convolutions of at most 4 input channels (the stem) ring_conv_stem_mfma_kernel; 0: ring_gemm_kernel / ring_gemm2_kernel / ring_conv_kernel on the vector ALU.  Read at launch: a captured graph keeps its kernel */ \
    X(s2lh, 1)             /* transition blocks on conv_s2lh_kernel (parity planes, linear halo), bits: 1 dgrad of <= 64-channel dx, 2 forward, 4 dgrad at every width; 0: implicit GEMM */ \
    X(s2lh_dbg, 0)          /* measurement only (wrong results): 1 no halo DMA after the prologue, 2 no weight DMA, 4 no MFMA, 8 no stores, 16 no write-back, 32 no BN partials, 64 linear halo */

enum OptId : int {
#define PRIMIA_OPT_ENUM(name, def) kOpt_##name,
    PRIMIA_OPTIONS(PRIMIA_OPT_ENUM)
#undef PRIMIA_OPT_ENUM
        kOptCount
};

extern int g_options[kOptCount];

inline int opt(OptId id) { return __atomic_load_n(&g_options[id], __ATOMIC_RELAXED); }

}  // namespace primia

#define PRIMIA_OPT(name) (::primia::opt(::primia::kOpt_##name))
