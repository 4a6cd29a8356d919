// Function Secret Sharing kernels whose PRG is the ChaCha20 block function (the `*_prg` entry points with prg = 1;
// DESIGN.md §4 "FSS keys from a ChaCha20 PRG").  The constructions are those of fss.hip -- the DIF comparison at a run-time
// width of 32..64 bits, the DPF equality test at 32 -- with the same key layout; only H / G differ:
//
//   for a seed (s0, s1), two uint64 as the key fields hold it,
//     blk = chacha20_block(key, ctr = 0)          chacha_block.h's state layout, 20 rounds
//     key words k[0..3] = (lo32(s0), hi32(s0), lo32(s1), hi32(s1)), k[4..7] = k[0..3] again
//     nonce words n[0] = the domain tag (kTagDif for H, kTagDpf for G), n[1] = 0
//     buf[k] = blk[2k] | (u64)blk[2k+1] << 32,  k = 0..7
//   H(seed) = buf[0..7] (where sha512_seed's output stands), G(seed) = buf[0..3] (where sha256_seed's stands).
//
// One comparison per lane, everything in 32-bit words: the seed of a level IS the four key words, and what a level reads of
// the block are single words of it, so nothing is packed into 64 bits on the way.
//   * Evaluation walks one side of the block: of its 8 words (DIF) it reads 6 -- bit 0 of word 0 (tau), the low 31 bits of
//     word 2 (conv31 of sigma), words 4..7 (s, t) -- and the feed-forward add is applied to those alone, after the select.
//     The level's correction words are 25 B per lane (control byte, the LOW word of cw_sigma word 1, cw_s, the leaf); those of
//     level l + 1 are loaded before the rounds of level l, so their latency sits under the ~1,000 ALU instructions of a block.
//   * Key generation needs both sides of both parties' blocks, but only through h0 ^ h1 and the side alpha's bit picks:
//     with sel = side alpha_i and ant = the other one, and D = (party 0's block) ^ (party 1's block),
//       cw_sigma = D.sel.sigma     cw_s = D.ant.s     ct = 1 ^ D.sel.t     ctau = 1 ^ D.ant.tau
//     (the switch table and the compression of fss.py:431-453,635-647 collapse to this: a table entry scaled by alpha_i
//     cancels the D term on one side and is absent on the other), so no uncompressed correction word is ever formed.
//     The two parties' blocks are independent chains the compiler interleaves: 8 quarter-rounds in flight, not 4.
//   * Words 0-3 and 12-15 of the initial state are constants; they enter the first double round as literals.
// Launch bounds: 256 threads and no minimum block count -- the evaluation kernels take 43 VGPRs and DIF key generation 62 (the
// SHA kernels' (256, 2) is there to admit their 190 to 230), so 8 waves per SIMD fit; see DESIGN.md §7 for what was measured.
#include "chacha_block.h"

namespace primia {
namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr u32 kTagDif = 0x31464944u;  // "DIF1", little-endian
constexpr u32 kTagDpf = 0x31465044u;  // "DPF1"

__device__ __forceinline__ u32 sigma_word(int j) {
    return j == 0 ? 0x61707865u : j == 1 ? 0x3320646eu : j == 2 ? 0x79622d32u : 0x6b206574u;
}
// word j of the initial state for the seed words k (j is a constant after unrolling)
template <u32 TAG>
__device__ __forceinline__ u32 init_word(const u32 (&k)[4], int j) {
    return j < 4 ? sigma_word(j) : j < 12 ? k[j & 3] : j == 14 ? TAG : 0u;
}
// the 20 rounds on the initial state of seed k, WITHOUT the feed-forward add
template <u32 TAG>
__device__ __forceinline__ void prg_rounds(const u32 (&k)[4], u32 (&x)[16]) {
#pragma unroll
    for (int j = 0; j < 16; ++j) x[j] = init_word<TAG>(k, j);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        PRIMIA_QR(x[0], x[4], x[8], x[12])
        PRIMIA_QR(x[1], x[5], x[9], x[13])
        PRIMIA_QR(x[2], x[6], x[10], x[14])
        PRIMIA_QR(x[3], x[7], x[11], x[15])
        PRIMIA_QR(x[0], x[5], x[10], x[15])
        PRIMIA_QR(x[1], x[6], x[11], x[12])
        PRIMIA_QR(x[2], x[7], x[8], x[13])
        PRIMIA_QR(x[3], x[4], x[9], x[14])
    }
}
// blk[HALF * side + j]: word j of side `side` of a block whose sides are HALF words long (8: H, 4: G), feed-forward included
template <u32 TAG, int HALF>
__device__ __forceinline__ u32 side_word(const u32 (&x)[16], const u32 (&k)[4], int side, int j) {
    const u32 lo = x[j] + init_word<TAG>(k, j), hi = x[HALF + j] + init_word<TAG>(k, HALF + j);
    return side ? hi : lo;
}

__device__ __forceinline__ void seed_words(u64 s0, u64 s1, u32 (&k)[4]) {
    k[0] = (u32)s0, k[1] = (u32)(s0 >> 32), k[2] = (u32)s1, k[3] = (u32)(s1 >> 32);
}
// the next seed: (word 0 without its bit 0, word 1) of a side, xor t * (cs0, cs1); m = all-ones while t == 1
__device__ __forceinline__ void next_seed(u32 (&k)[4], u32 w0, u32 w1, u32 w2, u32 w3, u64 cs0, u64 cs1, u32 m) {
    k[0] = (w0 & ~1u) ^ ((u32)cs0 & m);
    k[1] = w1 ^ ((u32)(cs0 >> 32) & m);
    k[2] = w2 ^ ((u32)cs1 & m);
    k[3] = w3 ^ ((u32)(cs1 >> 32) & m);
}
__device__ __forceinline__ u32 low31(u32 w) { return w & 0x7fffffffu; }      // conv31 of a 64-bit word whose low half is w
__device__ __forceinline__ u64 width_mask(int bits) { return bits == 64 ? ~0ULL : (1ULL << bits) - 1; }

// ---- the operands of the two-party forms: those of dif_eval_local_kernel (fss.hip) -------------------------------------------
struct MaskedOperand {
    const u64 *p0, *p1;
    int w, start;
};
// the open of comparison i: (x1_0 - x2_0 + alpha_0) + (x1_1 - x2_1 + alpha_1) in Z_2^64; element i of an operand is
// (row i / len, column start + i % len) of its [rows][w] matrix, x1.p0 == NULL stands for shares of zero
__device__ __forceinline__ u64 masked_sum(const MaskedOperand& x1, const MaskedOperand& x2, int len, const u64* __restrict__ alpha0,
                                          const u64* __restrict__ alpha1, long i) {
    const long r = i / len, c = i - r * len;
    const long i2 = r * x2.w + x2.start + c;
    u64 m0 = alpha0[i] - x2.p0[i2], m1 = alpha1[i] - x2.p1[i2];
    if (x1.p0) {
        const long i1 = r * x1.w + x1.start + c;
        m0 += x1.p0[i1];
        m1 += x1.p1[i1];
    }
    return m0 + m1;
}

// ---- DIF.eval -----------------------------------------------------------------------------------------------------------------
// what evaluation reads of one level's correction words
struct DifLevel {
    u32 cb, csg1;      // control bits; the low word of cw_sigma word 1 (only conv31 of sigma is used)
    u64 cs0, cs1;
    int leaf;
};
__device__ __forceinline__ DifLevel dif_level(const uint8_t* __restrict__ cw_bits, const u64* __restrict__ cw_sigma,
                                              const u64* __restrict__ cw_s, const int32_t* __restrict__ cw_leaf, int lvl, long n,
                                              long i) {
    DifLevel c;
    c.cb = cw_bits[(long)lvl * n + i];
    c.csg1 = (u32)cw_sigma[((long)lvl * 2 + 1) * n + i];
    c.cs0 = cw_s[((long)lvl * 2 + 0) * n + i];
    c.cs1 = cw_s[((long)lvl * 2 + 1) * n + i];
    c.leaf = cw_leaf[(long)lvl * n + i];
    return c;
}
// Party b's walk of comparison i down `bits` levels on the masked input xv (its low `bits` bits, most significant first):
// its int64 share of [xv <= alpha].  Every level adds tau * leaf + conv31(sigma), the end t * leaf + conv31(s); the party's
// sign is applied once, to the sum.
__device__ __forceinline__ int64_t dif_walk(int b, int bits, u64 xv, const u64* __restrict__ s0, const uint8_t* __restrict__ cw_bits,
                                            const u64* __restrict__ cw_sigma, const u64* __restrict__ cw_s,
                                            const int32_t* __restrict__ cw_leaf, long i, long n) {
    u32 k[4];
    seed_words(s0[i], s0[n + i], k);
    u32 m = 0u - (u32)b;
    const int last_leaf = cw_leaf[(long)bits * n + i];
    DifLevel cur = dif_level(cw_bits, cw_sigma, cw_s, cw_leaf, 0, n, i);
    int64_t sum = 0;
    for (int lvl = 0; lvl < bits; ++lvl) {
        // the next level's words, in flight during this level's rounds (the last level reads its own row again: in bounds, unused)
        const DifLevel nxt = dif_level(cw_bits, cw_sigma, cw_s, cw_leaf, lvl + 1 < bits ? lvl + 1 : lvl, n, i);
        u32 x[16];
        prg_rounds<kTagDif>(k, x);
        const int bit = (int)((xv >> (bits - 1 - lvl)) & 1);
        const u32 w_tau = side_word<kTagDif, 8>(x, k, bit, 0), w_sg = side_word<kTagDif, 8>(x, k, bit, 2);
        const u32 w4 = side_word<kTagDif, 8>(x, k, bit, 4), w5 = side_word<kTagDif, 8>(x, k, bit, 5);
        const u32 w6 = side_word<kTagDif, 8>(x, k, bit, 6), w7 = side_word<kTagDif, 8>(x, k, bit, 7);
        // t * CW_i, side `bit` of the uncompressed correction word
        const u32 ctau = (cur.cb >> (2 * bit)) & 1, ct = (cur.cb >> (2 * bit + 1)) & 1;
        const u32 tau = (w_tau ^ (ctau & m)) & 1;
        sum += (int64_t)(tau ? cur.leaf : 0) + (int64_t)low31(w_sg ^ (cur.csg1 & m));
        const u32 t = (w4 ^ (ct & m)) & 1;
        next_seed(k, w4, w5, w6, w7, cur.cs0, cur.cs1, m);
        m = 0u - t;
        cur = nxt;
    }
    sum += (int64_t)(m ? last_leaf : 0) + (int64_t)low31(k[2]);
    return b ? -sum : sum;
}

__global__ __launch_bounds__(256) void dif_eval_chacha_kernel(int b, int bits, const u64* __restrict__ x, const u64* __restrict__ s0,
                                                              const uint8_t* __restrict__ cw_bits, const u64* __restrict__ cw_sigma,
                                                              const u64* __restrict__ cw_s, const int32_t* __restrict__ cw_leaf,
                                                              int64_t* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = dif_walk(b, bits, x[i], s0, cw_bits, cw_sigma, cw_s, cw_leaf, i, n);
}
// fss.le for both parties hosted on this GPU: mask_builder, the open mod 2^bits and each party's walk (blockIdx.y = party)
__global__ __launch_bounds__(256) void dif_eval_local_chacha_kernel(MaskedOperand x1, MaskedOperand x2, int len, int bits,
                                                                    const u64* __restrict__ alpha0, const u64* __restrict__ alpha1,
                                                                    const u64* __restrict__ s0_0, const u64* __restrict__ s0_1,
                                                                    const uint8_t* __restrict__ cw_bits,
                                                                    const u64* __restrict__ cw_sigma, const u64* __restrict__ cw_s,
                                                                    const int32_t* __restrict__ cw_leaf, int64_t* __restrict__ out0,
                                                                    int64_t* __restrict__ out1, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int b = blockIdx.y;
    const u64 xv = masked_sum(x1, x2, len, alpha0, alpha1, i);      // (the walk reads its low `bits` bits)
    (b ? out1 : out0)[i] = dif_walk(b, bits, xv, b ? s0_1 : s0_0, cw_bits, cw_sigma, cw_s, cw_leaf, i, n);
}

// ---- DIF.keygen ---------------------------------------------------------------------------------------------------------------
// the 16 words of a party's block split by alpha's bit: sel = side ai (where the special path goes on), ant = the other side
template <u32 TAG, int HALF>
__device__ __forceinline__ void split_sides(const u32 (&x)[16], const u32 (&k)[4], int ai, u32 (&sel)[HALF], u32 (&ant)[HALF]) {
#pragma unroll
    for (int j = 0; j < HALF; ++j) {
        const u32 lo = x[j] + init_word<TAG>(k, j), hi = x[HALF + j] + init_word<TAG>(k, HALF + j);
        sel[j] = ai ? hi : lo;
        ant[j] = ai ? lo : hi;
    }
}

__global__ __launch_bounds__(256) void dif_keygen_chacha_kernel(const u64* __restrict__ alpha, const u64* __restrict__ s0p,
                                                                uint8_t* __restrict__ cw_bits, u64* __restrict__ cw_sigma,
                                                                u64* __restrict__ cw_s, int32_t* __restrict__ cw_leaf, long n,
                                                                int bits) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 av = alpha[i] & width_mask(bits);
    u32 ka[4], kb[4];      // s0_pair [party][word][n]
    seed_words(s0p[i], s0p[n + i], ka);
    seed_words(s0p[2 * n + i], s0p[3 * n + i], kb);
    u32 ma = 0u, mb = ~0u;      // t = (0, 1)
    for (int lvl = 0; lvl < bits; ++lvl) {
        const int ai = (int)((av >> (bits - 1 - lvl)) & 1);
        u32 xa[16], xb[16];
        prg_rounds<kTagDif>(ka, xa);
        prg_rounds<kTagDif>(kb, xb);
        u32 sa[8], aa[8], sb[8], ab[8];
        split_sides<kTagDif, 8>(xa, ka, ai, sa, aa);
        split_sides<kTagDif, 8>(xb, kb, ai, sb, ab);
        // D = h0 ^ h1 where the correction word reads it: sigma and t of side ai, s and tau of the other side
        const u32 d0 = sa[0] ^ sb[0], d4 = sa[4] ^ sb[4], e0 = aa[0] ^ ab[0], e4 = aa[4] ^ ab[4];
        const u64 csg0 = (u64)(d0 & ~1u) | (u64)(sa[1] ^ sb[1]) << 32;
        const u64 csg1 = (u64)(sa[2] ^ sb[2]) | (u64)(sa[3] ^ sb[3]) << 32;
        const u64 cs0 = (u64)(e4 & ~1u) | (u64)(aa[5] ^ ab[5]) << 32;
        const u64 cs1 = (u64)(aa[6] ^ ab[6]) | (u64)(aa[7] ^ ab[7]) << 32;
        const u32 ct = 1u ^ (d4 & 1), ctau = 1u ^ (e0 & 1);
        // (tau, t) of the uncompressed word on side ai and on the other side; cw_bits holds side L in bits 0-1, R in 2-3
        const u32 pair_sel = (d0 & 1) | ct << 1, pair_ant = ctau | (e4 & 1) << 1;
        cw_bits[(long)lvl * n + i] = (uint8_t)(ai ? pair_ant | pair_sel << 2 : pair_sel | pair_ant << 2);
        cw_sigma[((long)lvl * 2 + 0) * n + i] = csg0;
        cw_sigma[((long)lvl * 2 + 1) * n + i] = csg1;
        cw_s[((long)lvl * 2 + 0) * n + i] = cs0;
        cw_s[((long)lvl * 2 + 1) * n + i] = cs1;
        // both parties step to side ai (s, t) and read side 1 - ai (sigma, tau) for the leaf
        const u32 sig_a = low31(aa[2] ^ ((u32)csg1 & ma)), sig_b = low31(ab[2] ^ ((u32)csg1 & mb));
        const u32 tau_b = (ab[0] ^ (ctau & mb)) & 1;
        const u32 v = (u32)ai - sig_a + sig_b;      // 1 - conv(sigma_0) + conv(sigma_1) - (1 - alpha_i), mod 2^32
        cw_leaf[(long)lvl * n + i] = (int32_t)(tau_b ? 0u - v : v);
        const u32 ta = (sa[4] ^ (ct & ma)) & 1, tb = (sb[4] ^ (ct & mb)) & 1;
        next_seed(ka, sa[4], sa[5], sa[6], sa[7], cs0, cs1, ma);
        next_seed(kb, sb[4], sb[5], sb[6], sb[7], cs0, cs1, mb);
        ma = 0u - ta;
        mb = 0u - tb;
    }
    const u32 v = 1u - low31(ka[2]) + low31(kb[2]);
    cw_leaf[(long)bits * n + i] = (int32_t)(mb ? 0u - v : v);
}

// ---- DPF ----------------------------------------------------------------------------------------------------------------------
// Party b's walk of equality test i down the 32 levels on the masked input xv: its int64 share of [xv == alpha].  A level reads
// 17 B of the key (control byte, cw_s), prefetched like the DIF's.
__device__ __forceinline__ int64_t dpf_walk(int b, u32 xv, const u64* __restrict__ s0, const uint8_t* __restrict__ cw_bits,
                                            const u64* __restrict__ cw_s, const int64_t* __restrict__ cw_n, long i, long n) {
    u32 k[4];
    seed_words(s0[i], s0[n + i], k);
    u32 m = 0u - (u32)b;
    const int64_t leaf = cw_n[i];
    u32 cb = cw_bits[i];
    u64 cs0 = cw_s[i], cs1 = cw_s[n + i];
    for (int lvl = 0; lvl < 32; ++lvl) {
        const int nl = lvl + 1 < 32 ? lvl + 1 : lvl;
        const u32 ncb = cw_bits[(long)nl * n + i];
        const u64 ncs0 = cw_s[((long)nl * 2 + 0) * n + i], ncs1 = cw_s[((long)nl * 2 + 1) * n + i];
        u32 x[16];
        prg_rounds<kTagDpf>(k, x);
        const int bit = (xv >> (31 - lvl)) & 1;
        const u32 w0 = side_word<kTagDpf, 4>(x, k, bit, 0), w1 = side_word<kTagDpf, 4>(x, k, bit, 1);
        const u32 w2 = side_word<kTagDpf, 4>(x, k, bit, 2), w3 = side_word<kTagDpf, 4>(x, k, bit, 3);
        const u32 t = (w0 ^ (((cb >> bit) & 1) & m)) & 1;
        next_seed(k, w0, w1, w2, w3, cs0, cs1, m);
        m = 0u - t;
        cb = ncb, cs0 = ncs0, cs1 = ncs1;
    }
    const int64_t v = (m ? leaf : 0) + (int64_t)low31(k[2]);
    return b ? -v : v;
}
__global__ __launch_bounds__(256) void dpf_eval_chacha_kernel(int b, const u32* __restrict__ x, const u64* __restrict__ s0,
                                                              const uint8_t* __restrict__ cw_bits, const u64* __restrict__ cw_s,
                                                              const int64_t* __restrict__ cw_n, int64_t* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = dpf_walk(b, x[i], s0, cw_bits, cw_s, cw_n, i, n);
}
__global__ __launch_bounds__(256) void dpf_eval_local_chacha_kernel(MaskedOperand x1, MaskedOperand x2, int len,
                                                                    const u64* __restrict__ alpha0, const u64* __restrict__ alpha1,
                                                                    const u64* __restrict__ s0_0, const u64* __restrict__ s0_1,
                                                                    const uint8_t* __restrict__ cw_bits, const u64* __restrict__ cw_s,
                                                                    const int64_t* __restrict__ cw_n, int64_t* __restrict__ out0,
                                                                    int64_t* __restrict__ out1, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int b = blockIdx.y;
    const u32 xv = (u32)masked_sum(x1, x2, len, alpha0, alpha1, i);
    (b ? out1 : out0)[i] = dpf_walk(b, xv, b ? s0_1 : s0_0, cw_bits, cw_s, cw_n, i, n);
}
// DPF.keygen: as the DIF's with G's two 4-word sides -- cw_s = D.ant.s, ct = 1 ^ D.sel.t, and the other side's t bit is D.ant.t
__global__ __launch_bounds__(256) void dpf_keygen_chacha_kernel(const u64* __restrict__ alpha, const u64* __restrict__ s0p,
                                                                uint8_t* __restrict__ cw_bits, u64* __restrict__ cw_s,
                                                                int64_t* __restrict__ cw_n, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u32 av = (u32)alpha[i];
    u32 ka[4], kb[4];
    seed_words(s0p[i], s0p[n + i], ka);
    seed_words(s0p[2 * n + i], s0p[3 * n + i], kb);
    u32 ma = 0u, mb = ~0u;
    for (int lvl = 0; lvl < 32; ++lvl) {
        const int ai = (av >> (31 - lvl)) & 1;
        u32 xa[16], xb[16];
        prg_rounds<kTagDpf>(ka, xa);
        prg_rounds<kTagDpf>(kb, xb);
        u32 sa[4], aa[4], sb[4], ab[4];
        split_sides<kTagDpf, 4>(xa, ka, ai, sa, aa);
        split_sides<kTagDpf, 4>(xb, kb, ai, sb, ab);
        const u32 e0 = aa[0] ^ ab[0];
        const u64 cs0 = (u64)(e0 & ~1u) | (u64)(aa[1] ^ ab[1]) << 32;
        const u64 cs1 = (u64)(aa[2] ^ ab[2]) | (u64)(aa[3] ^ ab[3]) << 32;
        const u32 ct = 1u ^ ((sa[0] ^ sb[0]) & 1), t_ant = e0 & 1;
        cw_bits[(long)lvl * n + i] = (uint8_t)(ai ? t_ant | ct << 1 : ct | t_ant << 1);      // bit 0 tL, bit 1 tR
        cw_s[((long)lvl * 2 + 0) * n + i] = cs0;
        cw_s[((long)lvl * 2 + 1) * n + i] = cs1;
        const u32 ta = (sa[0] ^ (ct & ma)) & 1, tb = (sb[0] ^ (ct & mb)) & 1;
        next_seed(ka, sa[0], sa[1], sa[2], sa[3], cs0, cs1, ma);
        next_seed(kb, sb[0], sb[1], sb[2], sb[3], cs0, cs1, mb);
        ma = 0u - ta;
        mb = 0u - tb;
    }
    const int64_t v = 1 - (int64_t)low31(ka[2]) + (int64_t)low31(kb[2]);
    cw_n[i] = mb ? -v : v;
}

}  // namespace
}  // namespace primia

using namespace primia;

#define PRIMIA_REQUIRE_WIDTH(bits) PRIMIA_REQUIRE((bits) >= 32 && (bits) <= 64)
#define PRIMIA_REQUIRE_PRG(prg) PRIMIA_REQUIRE((prg) == PRIMIA_PRG_SHA || (prg) == PRIMIA_PRG_CHACHA)

extern "C" {

int primia_dif_keygen_prg(const uint64_t* alpha, const uint64_t* s0_pair, uint8_t* cw_bits, uint64_t* cw_sigma, uint64_t* cw_s,
                          int32_t* cw_leaf, int64_t n, int bits, int prg, primia_stream_t st) {
    PRIMIA_REQUIRE_PRG(prg);
    if (prg == PRIMIA_PRG_SHA) return primia_dif_keygen_n(alpha, s0_pair, cw_bits, cw_sigma, cw_s, cw_leaf, n, bits, st);
    PRIMIA_REQUIRE_WIDTH(bits);
    if (n == 0) return PRIMIA_OK;
    PRIMIA_REQUIRE(alpha && s0_pair && cw_bits && cw_sigma && cw_s && cw_leaf && n > 0);
    dif_keygen_chacha_kernel<<<ceil_div(n, 256), 256, 0, (hipStream_t)st>>>((const u64*)alpha, (const u64*)s0_pair, cw_bits,
                                                                             (u64*)cw_sigma, (u64*)cw_s, cw_leaf, n, bits);
    return launch_status();
}

int primia_dif_eval_prg(int b, const uint64_t* x, const uint64_t* s0, const uint8_t* cw_bits, const uint64_t* cw_sigma,
                        const uint64_t* cw_s, const int32_t* cw_leaf, int64_t* out, int64_t n, int bits, int prg,
                        primia_stream_t st) {
    PRIMIA_REQUIRE_PRG(prg);
    if (prg == PRIMIA_PRG_SHA) return primia_dif_eval_n(b, x, s0, cw_bits, cw_sigma, cw_s, cw_leaf, out, n, bits, st);
    PRIMIA_REQUIRE_WIDTH(bits);
    if (n == 0) return PRIMIA_OK;
    PRIMIA_REQUIRE((b == 0 || b == 1) && x && s0 && cw_bits && cw_sigma && cw_s && cw_leaf && out && n > 0);
    dif_eval_chacha_kernel<<<ceil_div(n, 256), 256, 0, (hipStream_t)st>>>(b, bits, (const u64*)x, (const u64*)s0, cw_bits,
                                                                           (const u64*)cw_sigma, (const u64*)cw_s, cw_leaf, out, n);
    return launch_status();
}

int primia_dif_eval_local_prg(const int64_t* x1_0, const int64_t* x1_1, int w1, int start1, const int64_t* x2_0,
                              const int64_t* x2_1, int w2, int start2, int len, const uint64_t* alpha0, const uint64_t* alpha1,
                              const uint64_t* s0_0, const uint64_t* s0_1, const uint8_t* cw_bits, const uint64_t* cw_sigma,
                              const uint64_t* cw_s, const int32_t* cw_leaf, int64_t* out0, int64_t* out1, int64_t n, int bits,
                              int prg, primia_stream_t st) {
    PRIMIA_REQUIRE_PRG(prg);
    if (prg == PRIMIA_PRG_SHA)
        return primia_dif_eval_local_n(x1_0, x1_1, w1, start1, x2_0, x2_1, w2, start2, len, alpha0, alpha1, s0_0, s0_1, cw_bits,
                                       cw_sigma, cw_s, cw_leaf, out0, out1, n, bits, st);
    PRIMIA_REQUIRE_WIDTH(bits);
    if (n == 0) return PRIMIA_OK;
    PRIMIA_REQUIRE(x2_0 && x2_1 && ((x1_0 == nullptr) == (x1_1 == nullptr)) && alpha0 && alpha1 && s0_0 && s0_1 && cw_bits &&
                   cw_sigma && cw_s && cw_leaf && out0 && out1 && n > 0 && len > 0 && n % len == 0);
    PRIMIA_REQUIRE(w2 >= len && start2 >= 0 && start2 + len <= w2 && (!x1_0 || (w1 >= len && start1 >= 0 && start1 + len <= w1)));
    const dim3 grid((unsigned)ceil_div(n, 256), 2);
    dif_eval_local_chacha_kernel<<<grid, 256, 0, (hipStream_t)st>>>(
        MaskedOperand{(const u64*)x1_0, (const u64*)x1_1, w1, start1}, MaskedOperand{(const u64*)x2_0, (const u64*)x2_1, w2, start2},
        len, bits, (const u64*)alpha0, (const u64*)alpha1, (const u64*)s0_0, (const u64*)s0_1, cw_bits, (const u64*)cw_sigma,
        (const u64*)cw_s, cw_leaf, out0, out1, n);
    return launch_status();
}

int primia_dpf_keygen_prg(const uint64_t* alpha, const uint64_t* s0_pair, uint8_t* cw_bits, uint64_t* cw_s, int64_t* cw_n,
                          int64_t n, int prg, primia_stream_t st) {
    PRIMIA_REQUIRE_PRG(prg);
    if (prg == PRIMIA_PRG_SHA) return primia_dpf_keygen(alpha, s0_pair, cw_bits, cw_s, cw_n, n, st);
    if (n == 0) return PRIMIA_OK;
    PRIMIA_REQUIRE(alpha && s0_pair && cw_bits && cw_s && cw_n && n > 0);
    dpf_keygen_chacha_kernel<<<ceil_div(n, 256), 256, 0, (hipStream_t)st>>>((const u64*)alpha, (const u64*)s0_pair, cw_bits,
                                                                             (u64*)cw_s, cw_n, n);
    return launch_status();
}

int primia_dpf_eval_prg(int b, const uint32_t* x, const uint64_t* s0, const uint8_t* cw_bits, const uint64_t* cw_s,
                        const int64_t* cw_n, int64_t* out, int64_t n, int prg, primia_stream_t st) {
    PRIMIA_REQUIRE_PRG(prg);
    if (prg == PRIMIA_PRG_SHA) return primia_dpf_eval(b, x, s0, cw_bits, cw_s, cw_n, out, n, st);
    if (n == 0) return PRIMIA_OK;
    PRIMIA_REQUIRE((b == 0 || b == 1) && x && s0 && cw_bits && cw_s && cw_n && out && n > 0);
    dpf_eval_chacha_kernel<<<ceil_div(n, 256), 256, 0, (hipStream_t)st>>>(b, x, (const u64*)s0, cw_bits, (const u64*)cw_s, cw_n,
                                                                           out, n);
    return launch_status();
}

int primia_dpf_eval_local_prg(const int64_t* x1_0, const int64_t* x1_1, int w1, int start1, const int64_t* x2_0,
                              const int64_t* x2_1, int w2, int start2, int len, const uint64_t* alpha0, const uint64_t* alpha1,
                              const uint64_t* s0_0, const uint64_t* s0_1, const uint8_t* cw_bits, const uint64_t* cw_s,
                              const int64_t* cw_n, int64_t* out0, int64_t* out1, int64_t n, int prg, primia_stream_t st) {
    PRIMIA_REQUIRE_PRG(prg);
    if (prg == PRIMIA_PRG_SHA)
        return primia_dpf_eval_local(x1_0, x1_1, w1, start1, x2_0, x2_1, w2, start2, len, alpha0, alpha1, s0_0, s0_1, cw_bits, cw_s,
                                     cw_n, out0, out1, n, st);
    if (n == 0) return PRIMIA_OK;
    // (both operands are required, as by primia_dpf_eval_local)
    PRIMIA_REQUIRE(x1_0 && x1_1 && x2_0 && x2_1 && alpha0 && alpha1 && s0_0 && s0_1 && cw_bits && cw_s && cw_n && out0 && out1 &&
                   out0 != out1 && n > 0 && len > 0 && n % len == 0);
    PRIMIA_REQUIRE(w2 >= len && start2 >= 0 && start2 + len <= w2 && w1 >= len && start1 >= 0 && start1 + len <= w1);
    const dim3 grid((unsigned)ceil_div(n, 256), 2);
    dpf_eval_local_chacha_kernel<<<grid, 256, 0, (hipStream_t)st>>>(
        MaskedOperand{(const u64*)x1_0, (const u64*)x1_1, w1, start1}, MaskedOperand{(const u64*)x2_0, (const u64*)x2_1, w2, start2},
        len, (const u64*)alpha0, (const u64*)alpha1, (const u64*)s0_0, (const u64*)s0_1, cw_bits, (const u64*)cw_s, cw_n, out0, out1,
        n);
    return launch_status();
}

}  // extern "C"
