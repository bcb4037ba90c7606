// pip_shape.hpp -- the shape of a bucket-method MulVec (pippenger.hpp) and its digit recoding: everything the kernels
// derive from (n, window_bits) and the scalar field alone.  No device code: a host compiler builds this header as it is
// (tests/host/pip_shape_host_test.cpp), the kernels include it through pippenger.hpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "abi_guard.hpp"
#include "field.hpp"

namespace bpp {

struct PipShape {
    uint32_t n;                // input points
    uint32_t items;            // (point, sub-scalar) pairs: n, or 2 n with the endomorphism split
    uint32_t glv;
    uint32_t c, W;             // requested (maximum) window bits, windows
    uint32_t q, nwide;         // windows j < nwide are q + 1 bits wide, the others q
    uint32_t top;              // buckets of the top window (its digit is unsigned: 1..top)
    uint32_t nbuckets;         // all windows
    uint32_t nbmax;            // buckets of the largest window
    uint32_t S, TS;            // buckets per lane / per tile (64 S) in k_pip_tiles
    uint32_t tw, tn, ntiles;   // tiles of a wide / narrow signed window, all tiles
    uint32_t L, cpw, capseg;   // entries per chunk, chunks per window, segment slots per window
    uint32_t fb;               // log2 of the buckets per coarse bin of the sort (5..8)
    uint32_t fl;               // lanes per bucket in k_pip_fold (1, 2, 4 or 8)
    uint32_t istride;          // entries per row of `sorted`: items rounded up to 4 (rows start 16-byte aligned for the entry DMA)
    uint32_t bias[10];         // sum over the signed windows of half their range at their offset

    BPP_HD uint32_t width(uint32_t j) const { return q + (j < nwide ? 1u : 0u); }
    BPP_HD uint32_t off(uint32_t j) const { return j * q + (j < nwide ? j : nwide); }
    BPP_HD uint32_t nb(uint32_t j) const { return j + 1 == W ? top : 1u << (width(j) - 1); }
    BPP_HD uint32_t bbase(uint32_t j) const {
        return j < nwide ? j << q : (nwide << q) + ((j - nwide) << (q - 1));
    }
    BPP_HD uint32_t tiles(uint32_t j) const { return (nb(j) + TS - 1) / TS; }
    BPP_HD uint32_t tbase(uint32_t j) const { return j < nwide ? j * tw : nwide * tw + (j - nwide) * tn; }
    BPP_HD uint32_t window_of_tile(uint32_t t) const {
        if (t < nwide * tw) return t / tw;
        const uint32_t r = (t - nwide * tw) / tn;
        return nwide + (r < W - 1 - nwide ? r : W - 1 - nwide);
    }
};

// max_words: the largest sub-scalar value (8 words); bits: its bit length
inline int pip_shape(size_t n, int c, bool glv, const uint32_t* max_words, int bits, PipShape& s) {
    if (c < 2 || c > 16) return fail(BPP_E_ARG, "window_bits must be in [2, 16]");
    if (n >= ((size_t)1 << 28)) return fail(BPP_E_ARG, "MulVec too long for one call");   // a sorted entry is item << 1 | sign, bit 31 a flag
    s.n = (uint32_t)n;
    s.glv = glv ? 1u : 0u;
    s.items = (uint32_t)(glv ? 2 * n : n);
    s.istride = (s.items + 3u) & ~3u;
    s.c = (uint32_t)c;
    s.W = (uint32_t)((bits + c - 1) / c);
    s.q = (uint32_t)bits / s.W;
    s.nwide = (uint32_t)bits - s.q * s.W;
    for (int t = 0; t < 10; t++) s.bias[t] = 0;
    for (uint32_t j = 0; j + 1 < s.W; j++) {
        const uint32_t bit = s.off(j) + s.width(j) - 1;
        s.bias[bit >> 5] |= 1u << (bit & 31);
    }
    uint32_t v[10];
    uint32_t carry = 0;
    for (int t = 0; t < 10; t++) {
        uint64_t x = (uint64_t)(t < 8 ? max_words[t] : 0u) + s.bias[t] + carry;
        v[t] = (uint32_t)x;
        carry = (uint32_t)(x >> 32);
    }
    const uint32_t sh = s.off(s.W - 1);
    uint64_t top = 0;
    for (int t = 9; t >= 0; t--) {
        const int lo = 32 * t - (int)sh;
        if (lo >= 32 && v[t]) return fail(BPP_E_ARG, "window_bits too small for this scalar field");
        if (lo > -32 && lo < 32) top |= lo >= 0 ? (uint64_t)v[t] << lo : (uint64_t)(v[t] >> (-lo));
    }
    if (top == 0 || top > ((uint64_t)1 << 17)) return fail(BPP_E_ARG, "window_bits too small for this scalar field");
    s.top = (uint32_t)top;
    s.nbuckets = s.bbase(s.W - 1) + s.top;
    s.nbmax = s.top;
    for (uint32_t j = 0; j + 1 < s.W; j++) s.nbmax = std::max(s.nbmax, s.nb(j));
    // tiles: enough of them to spread a window over the chip, few enough that k_pip_windows stays short
    uint32_t S = (1u << s.q) / 8192;
    S = S < 1 ? 1 : (S > 8 ? 8 : S);
    s.S = S;
    s.TS = 64 * S;
    s.tw = ((1u << s.q) + s.TS - 1) / s.TS;
    s.tn = ((1u << (s.q - (s.q ? 1 : 0))) + s.TS - 1) / s.TS;
    s.ntiles = s.tbase(s.W - 1) + s.tiles(s.W - 1);
    // chunks: 64 entries each for large inputs; shorter ones while the launch would not fill the chip (2^17 lanes)
    const size_t entries = (size_t)s.W * s.items;
    uint32_t L = 64;
    while (L > 8 && entries / L < ((size_t)1 << 18)) L >>= 1;
    s.L = L;
    // coarse bins of the sort: about 1024 of them (one block of k_pip_binsort each), 32..256 buckets wide
    uint32_t fb = 8;
    while (fb > 5 && (s.nbuckets >> fb) < 1024) fb--;
    s.fb = fb;
    s.cpw = (s.items + L - 1) / L;
    s.capseg = s.cpw + s.nbmax;
    // k_pip_fold: a bucket touches about (its entries / L) + 1 chunks; while the launch stays within one residency of the
    // chip, several lanes share a bucket's segments (strided sums, then a butterfly inside the lane group)
    const size_t nseg = entries / ((size_t)s.nbuckets * L) + 1;
    uint32_t fl = 1;
    while (fl < 8 && 2 * fl <= nseg && (size_t)s.nbuckets * 2 * fl <= ((size_t)1 << 18)) fl <<= 1;
    s.fl = fl;
    return BPP_OK;
}

// window width for n points.  Large inputs: about 2^7..2^8 items per bucket (the bucket additions dominate, the
// reduction of the buckets stays a few per cent).  Small inputs are latency bound -- the chain is a chunk, the
// fold / tile / window reduction, then the doublings of the top window -- and want MORE, shorter buckets.
inline int pip_pick_c(size_t n, bool glv) {
    const size_t items = glv ? 2 * n : n;
    int lg = 0;
    while (((size_t)1 << (lg + 1)) <= items) lg++;
    int c = lg - 5;
    if (lg <= 18) c = lg - 3;
    return c < 7 ? 7 : (c > 16 ? 16 : c);
}

constexpr uint32_t PIP_FINE_MAX = 256;      // buckets per coarse bin: 2^fb, fb in [5, 8] (PipShape::fb)
constexpr uint32_t PIP_MAXCOARSE = 2052;    // coarse bins of the largest window: (2^16 + 1) / 32 + 1 = 2049

BPP_HD uint32_t pip_ncoarse(const PipShape& s, uint32_t j) { return (s.nb(j) + (1u << s.fb) - 1) >> s.fb; }
// coarse bins are numbered window by window; cbase(j) = bins of the windows below j (W + 1 entries fit a kernel argument
// badly for W up to 128, so it is recomputed: windows come in at most three sizes)
BPP_HD uint32_t pip_cbase(const PipShape& s, uint32_t j) {
    const uint32_t fine = 1u << s.fb;
    const uint32_t cw = ((1u << s.q) + fine - 1) >> s.fb, cn = ((1u << (s.q - 1)) + fine - 1) >> s.fb;
    return j < s.nwide ? j * cw : s.nwide * cw + (j - s.nwide) * cn;
}
BPP_HD uint32_t pip_ncoarse_total(const PipShape& s) { return pip_cbase(s, s.W - 1) + pip_ncoarse(s, s.W - 1); }

// digit of window j of (value + bias): signed below the top window, unsigned in it
BPP_HD int32_t pip_digit(const PipShape& s, const uint32_t w[10], uint32_t j) {
    const uint32_t o = s.off(j), wi = o >> 5, sh = o & 31u;
    uint32_t v = w[wi] >> sh;
    if (sh && wi + 1 < 10) v |= w[wi + 1] << (32 - sh);
    if (j + 1 == s.W) return (int32_t)v;   // everything that is left of the value (< 2^18)
    const uint32_t wd = s.width(j);
    return (int32_t)(v & ((1u << wd) - 1u)) - (int32_t)(1u << (wd - 1));
}

}  // namespace bpp
