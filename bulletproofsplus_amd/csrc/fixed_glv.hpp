// fixed_glv.hpp -- window layout and digit recoding of the fixed-generator tables on curves that split scalars with
// their endomorphism (BLS12-381 G1; kernels.hpp fixed_glv<C>(), k_fixed_msm).  Plain C++ beside ec.hpp, so the host tests
// (tests/host/fixed_glv_host_test.cpp) compile the very code the kernels and the verifier's constructor run.
//
// A scalar k < r becomes two signed halves of at most HALF_MAX = floor(z^2 / 2) + 1 < 2^126.43 (ec.hpp
// glv_split_balanced).  One table per generator serves both: T[j][d] = d 2^(off_j) F.  A half h is recoded as
//     h = sum_{j < W-1} d_j 2^(off_j) + d_top 2^(off_{W-1}),   d_j in [-2^(c_j - 1), 2^(c_j - 1)),  d_top in [0, top]
// by the bias trick: v = h + sum_j 2^(off_j + c_j - 1), then d_j = (v >> off_j mod 2^(c_j)) - 2^(c_j - 1), and the top
// digit is what is left of v.  For window_bits = c the layout has W = floor(W_plain / 2) windows (W_plain = the window
// count of the unsplit layout at c), and the widths of the W - 1 signed windows are chosen to minimise the entries per
// generator: for a given sum of widths S the entries 2^(c_j - 1) are fewest when the widths differ by at most one, so the
// search runs over S alone, narrower windows first.
#pragma once
#include <cstdint>

#include "ec.hpp"

namespace bpp {

constexpr int GLV_MAXW = 64;      // windows per half: window_bits 2 on a 255-bit field
constexpr int GLV_HALF_WORDS = 5; // a half + bias < 2^128, kept in 5 words

struct GlvLayout {
    uint32_t W;                   // windows per half
    uint32_t top;                 // largest top digit = entries of the top window
    uint32_t per_f;               // entries per generator
    uint8_t wc[GLV_MAXW];         // widths of the signed windows (wc[W-1] = 0)
    uint8_t off[GLV_MAXW];        // bit offset of window j
    uint32_t went[GLV_MAXW];      // first entry of window j
    uint32_t bias[GLV_HALF_WORDS];
};

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

// false: no layout (window_bits too large or too small for the field)
inline bool glv_layout(int c, int fr_bits, const uint32_t half_max[4], GlvLayout& best) {
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
        GlvLayout L{};
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
        for (int t = 0; t < GLV_HALF_WORDS; t++) L.bias[t] = t < 4 ? (uint32_t)(bias >> (32 * t)) : 0u;
        best = L;
        best_entries = entries;
        found = true;
    }
    return found;
}

// v = half + bias (5 words), then per window: the digit of the lowest window of v, and v shifted past it
BPP_HD void glv_biased(const uint32_t half[4], const uint32_t bias[GLV_HALF_WORDS], uint32_t v[GLV_HALF_WORDS]) {
    uint32_t carry = 0;
#pragma unroll
    for (int t = 0; t < GLV_HALF_WORDS; t++) {
        const uint64_t x = (uint64_t)(t < 4 ? half[t] : 0u) + bias[t] + carry;
        v[t] = (uint32_t)x;
        carry = (uint32_t)(x >> 32);
    }
}
// cj = 0: the top window (unsigned, everything that is left); else a signed window of cj bits (1 <= cj < 32)
BPP_HD int32_t glv_next_digit(uint32_t v[GLV_HALF_WORDS], uint32_t cj) {
    if (cj == 0) return (int32_t)v[0];
    const int32_t dg = (int32_t)(v[0] & ((1u << cj) - 1u)) - (int32_t)(1u << (cj - 1));
#pragma unroll
    for (int t = 0; t < GLV_HALF_WORDS - 1; t++) v[t] = (v[t] >> cj) | (v[t + 1] << (32 - cj));
    v[GLV_HALF_WORDS - 1] >>= cj;
    return dg;
}

}  // namespace bpp
