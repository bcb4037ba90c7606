// fixed_glv.hpp -- the windows of the fixed-generator tables: their layout and the digit recoding every reader of the
// tables runs (kernels.hpp k_fixed_msm, k_tbl_bases / k_tbl_fill; commit_walk.hpp; the verifier's constructor through
// host_util.hpp make_shape).  Plain C++ beside ec.hpp, so the host tests (tests/host/fixed_glv_host_test.cpp,
// commit_walk_host_test.cpp) compile the very code the kernels run.
//
// One table per generator: T[j][d] = d 2^(off_j) F for W windows.  A value h is recoded as
//     h = sum_{j < W-1} d_j 2^(off_j) + d_top 2^(off_{W-1}),   d_j in [-2^(c_j - 1), 2^(c_j - 1)),  d_top in [0, top]
// by the bias trick: v = h + sum_j 2^(off_j + c_j - 1), then d_j = (v >> off_j mod 2^(c_j)) - 2^(c_j - 1), and the top
// digit is what is left of v -- unsigned, so no window is spent on a recoding carry.  Window j holds d = 1..2^(c_j - 1),
// the top window d = 1..top; a negative digit negates the entry.
//
// Two layouts for window_bits = c:
//   uniform (secp256k1, edwards25519): the value is the whole scalar k < r (NW = 10 words with the bias); W_plain =
//     floor((bits(r) - 1) / c) + 1 windows, the signed ones all c bits wide.
//   mixed widths (BLS12-381 G1): a scalar becomes two signed halves of at most HALF_MAX = floor(z^2 / 2) + 1 < 2^126.43
//     (ec.hpp glv_split_balanced), and the table serves both (NW = 5 words).  W = floor(W_plain / 2) windows, and the
//     widths of the W - 1 signed ones are chosen to minimise the entries per generator: for a given sum of widths S the
//     entries 2^(c_j - 1) are fewest when the widths differ by at most one, so the search runs over S alone, narrower
//     windows first.
#pragma once
#include <cstddef>
#include <cstdint>

#include "ec.hpp"

namespace bpp {

constexpr int GLV_MAXW = 128;      // windows: window_bits 2 on an unsplit 256-bit scalar
constexpr int GLV_HALF_WORDS = 5;  // a half + bias < 2^128, kept in 5 words
constexpr int WIN_FULL_WORDS = 10; // a scalar + bias, kept in 10 words

struct WinLayout {
    uint32_t W;                   // windows
    uint32_t top;                 // largest top digit = entries of the top window
    uint32_t per_f;               // entries per generator
    alignas(4) uint8_t wc[GLV_MAXW];   // widths of the signed windows (wc[W-1] = 0); read with win_width
    uint8_t off[GLV_MAXW];        // bit offset of window j
    uint32_t went[GLV_MAXW];      // first entry of window j
    uint32_t bias[WIN_FULL_WORDS];
};
using GlvLayout = WinLayout;   // as the readers of halves name it

// Width of window j (S: a WinLayout, or a shape that carries its W, wc[] and top), taken out of the aligned word that
// holds it.  Not s.wc[j], for a reason that is observed and not explained: with the byte read (ROCm 7.2 clang, gfx950)
// k_fixed_msm, which then read wc[] and went[] of its kernel argument on every curve, gathered the entries of windows
// j >= 1 from the wrong window on secp256k1 and edwards25519, and gathered the right ones with this word read and nothing
// else changed.  The generated code was not reduced to a reproducer, and the same byte read is correct on BLS12-381, so
// a miscompiled address is a guess.  k_fixed_msm no longer reads wc[] on the uniform curves; the table builders and the
// commitment walk do.  The word read may go once the GPU suite passes with s.wc[j] in its place.
template <class S>
BPP_HD uint32_t win_width(const S& s, uint32_t j) {
    static_assert(alignof(S) >= 4 && offsetof(S, wc) % 4 == 0 && sizeof(s.wc) % 4 == 0, "wc[] is read a word at a time");
    uint32_t w4;
    __builtin_memcpy(&w4, __builtin_assume_aligned(s.wc + (j & ~3u), 4), 4);
    return (w4 >> (8 * (j & 3u))) & 0xffu;
}
// entries of window j
template <class S>
BPP_HD uint32_t win_entries(const S& s, uint32_t j) {
    return j + 1 < s.W ? 1u << (win_width(s, j) - 1) : s.top;
}

// Uniform layout over a whole scalar < r (r: 8 words, fr_bits its bit length).  Returns null, or why there is no layout.
inline const char* win_layout_uniform(int c, const uint32_t fr_modw[8], int fr_bits, WinLayout& L) {
    L = WinLayout{};
    // W - 1 signed windows below bit c (W-1) < fr_bits, then one unsigned top window for the rest of the value
    L.W = (uint32_t)((fr_bits - 1) / c + 1);
    if (L.W > (uint32_t)GLV_MAXW) return "window_bits too small for this scalar field";
    for (uint32_t j = 0; j < L.W; j++) {
        L.wc[j] = j + 1 < L.W ? (uint8_t)c : 0;
        L.off[j] = (uint8_t)(c * j);
        L.went[j] = j << (c - 1);
        if (j + 1 < L.W) L.bias[(c * j + c - 1) >> 5] |= 1u << ((c * j + c - 1) & 31);
    }
    // largest top digit: (r - 1 + bias) >> c (W - 1)
    uint32_t v[WIN_FULL_WORDS];
    uint32_t carry = 0;
    for (int t = 0; t < WIN_FULL_WORDS; t++) {
        const uint64_t x = (uint64_t)(t < 8 ? fr_modw[t] : 0u) + L.bias[t] + carry;
        v[t] = (uint32_t)x;
        carry = (uint32_t)(x >> 32);
    }
    uint32_t borrow = 1;   // - 1
    for (int t = 0; t < WIN_FULL_WORDS && borrow; t++) {
        borrow = v[t] == 0 ? 1u : 0u;
        v[t] -= 1u;
    }
    const uint32_t sh = (uint32_t)c * (L.W - 1);
    uint64_t top = 0;
    for (int t = WIN_FULL_WORDS - 1; t >= 0; t--) {
        const int lo = 32 * t - (int)sh;   // bit position of word t after the shift
        if (lo >= 32 && v[t]) return "window_bits too small for this scalar field";
        if (lo > -32 && lo < 32) top |= lo >= 0 ? (uint64_t)v[t] << lo : (uint64_t)(v[t] >> (-lo));
    }
    if (top == 0 || top >= ((uint64_t)1 << 31)) return "window_bits too small for this scalar field";
    L.top = (uint32_t)top;
    const uint64_t per_f = (uint64_t)L.went[L.W - 1] + top;
    if (per_f >> 32) return "window table too large";
    L.per_f = (uint32_t)per_f;
    return nullptr;
}

// floor(z^2 / 2) + 1 as 4 words: the largest magnitude glv_split_balanced returns
template <class C>
inline void glv_half_max(uint32_t out[4]) {
    uint32_t carry = 1;
    for (int t = 0; t < 4; t++) {
        const uint32_t v = (C::K::ZSQW[t] >> 1) | (t < 3 ? C::K::ZSQW[t + 1] << 31 : 0u);
        const uint64_t x = (uint64_t)v + carry;
        out[t] = (uint32_t)x;
        carry = (uint32_t)(x >> 32);
    }
}

// Mixed-width layout over the halves (<= half_max) of a split scalar.  false: no layout (window_bits too large or too
// small for the field)
inline bool glv_layout(int c, int fr_bits, const uint32_t half_max[4], WinLayout& best) {
    const uint32_t Wplain = (uint32_t)((fr_bits - 1) / c + 1);
    const uint32_t W = Wplain / 2;
    if (W < 2 || W > (uint32_t)GLV_MAXW) return false;
    const unsigned __int128 hmax = ((unsigned __int128)half_max[3] << 96) | ((unsigned __int128)half_max[2] << 64) |
                                   ((unsigned __int128)half_max[1] << 32) | half_max[0];
    const uint32_t ns = W - 1;
    bool found = false;
    uint64_t best_entries = 0;
    for (uint32_t S = ns; S < 128; S++) {
        const uint32_t q = S / ns, rem = S % ns;
        if (q + (rem ? 1u : 0u) > 24) break;
        WinLayout L{};
        L.W = W;
        unsigned __int128 bias = 0;
        uint64_t entries = 0;
        uint32_t off = 0;
        for (uint32_t j = 0; j < ns; j++) {
            const uint32_t cj = q + (j >= ns - rem ? 1u : 0u);   // the wider windows on top
            L.wc[j] = (uint8_t)cj;
            L.off[j] = (uint8_t)off;
            L.went[j] = (uint32_t)entries;
            bias |= (unsigned __int128)1 << (off + cj - 1);
            entries += (uint64_t)1 << (cj - 1);
            off += cj;
        }
        const unsigned __int128 top = (hmax + bias) >> S;
        if (top == 0 || top >= ((unsigned __int128)1 << 31)) continue;
        L.off[ns] = (uint8_t)off;
        L.went[ns] = (uint32_t)entries;
        entries += (uint64_t)top;
        if (entries >> 32) continue;
        if (found && entries >= best_entries) continue;
        L.top = (uint32_t)top;
        L.per_f = (uint32_t)entries;
        for (int t = 0; t < 4; t++) L.bias[t] = (uint32_t)(bias >> (32 * t));
        best = L;
        best_entries = entries;
        found = true;
    }
    return found;
}

// v = k + bias in NW words (k: 4 words of a half for NW = 5, 8 words of a scalar for NW = 10), then per window: the digit
// of the lowest window of v, and v shifted past it
template <int NW>
BPP_HD void win_biased(const uint32_t* k, const uint32_t* bias, uint32_t v[NW]) {
    static_assert(NW == GLV_HALF_WORDS || NW == WIN_FULL_WORDS, "a half or a whole scalar");
    constexpr int NK = NW == GLV_HALF_WORDS ? 4 : 8;
    uint32_t carry = 0;
#pragma unroll
    for (int t = 0; t < NW; t++) {
        const uint64_t x = (uint64_t)(t < NK ? k[t] : 0u) + bias[t] + carry;
        v[t] = (uint32_t)x;
        carry = (uint32_t)(x >> 32);
    }
}
// cj = 0: the top window (unsigned, everything that is left); else a signed window of cj bits (1 <= cj < 32)
template <int NW>
BPP_HD int32_t win_next_digit(uint32_t (&v)[NW], uint32_t cj) {
    if (cj == 0) return (int32_t)v[0];
    const int32_t dg = (int32_t)(v[0] & ((1u << cj) - 1u)) - (int32_t)(1u << (cj - 1));
#pragma unroll
    for (int t = 0; t < NW - 1; t++) v[t] = (v[t] >> cj) | (v[t + 1] << (32 - cj));
    v[NW - 1] >>= cj;
    return dg;
}
// the NW = 5 instances, on a half
BPP_HD void glv_biased(const uint32_t half[4], const uint32_t bias[GLV_HALF_WORDS], uint32_t v[GLV_HALF_WORDS]) {
    win_biased<GLV_HALF_WORDS>(half, bias, v);
}
BPP_HD int32_t glv_next_digit(uint32_t (&v)[GLV_HALF_WORDS], uint32_t cj) { return win_next_digit(v, cj); }

}  // namespace bpp
