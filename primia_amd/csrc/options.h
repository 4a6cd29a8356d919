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
    X(s2lh, 1)              /* transition blocks on conv_s2lh_kernel (parity planes, linear halo), bits: 1 dgrad of <= 64-channel dx, 2 forward, 4 dgrad at every width; 0: implicit GEMM */ \
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
