// Host-side checks of the bucket-method MulVec's shape and digit code (csrc/pip_shape.hpp: pip_shape, pip_pick_c, the
// tile / coarse-bin numbering, pip_digit), compiled with g++; the kernels of csrc/pippenger.hpp run the same code.
// tests/test_pip_shape_cpu.py drives it.  <kind> is "glv" (128-bit sub-scalars, max 2^128 - 1: BLS12-381 and secp256k1) or
// "ed" (edwards25519: 253 bits, max = r).
//   geometry <kind>             every c in 2..16 at every n of the list below: the relations between the shape's members
//                               that the kernels rely on.  Prints "ok geometry <kind> <shapes>"; the first violation goes
//                               to stderr and the exit status is 1.
//   layout <kind> <c>           "W top" then one line per window: "offset width nb"
//   recode <kind> <c> <v>...    per value (64 hex digits): the W digits of v + bias (formed as pip_subscalars forms it),
//                               lowest window first
//   table <kind>:<n>:<c> ...    per case one line "c W q nwide top nbuckets S L fb fl cpw pad" (pad = istride - items);
//                               c = 0 asks for the width pip_pick_c chooses
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../bulletproofsplus_amd/csrc/pip_shape.hpp"
using namespace bpp;

static const size_t SIZES[] = {1, 2, 3, 5, 300, 2049, 4097, (size_t)1 << 16, ((size_t)1 << 20) + 1, (size_t)1 << 22,
                               ((size_t)1 << 28) - 1};

static bool shape_of(const char* kind, size_t n, int c, PipShape& s) {
    if (!strcmp(kind, "glv")) {
        const uint32_t mx[8] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0, 0, 0, 0};
        return pip_shape(n, c, true, mx, 128, s) == BPP_OK;
    }
    if (!strcmp(kind, "ed")) return pip_shape(n, c, false, EdFr::MODW, EdFr::BITS, s) == BPP_OK;
    return false;
}

#define REQUIRE(cond)                                                                                       \
    do {                                                                                                    \
        if (!(cond)) {                                                                                      \
            fprintf(stderr, "geometry %s n=%zu c=%d: %s (line %d)\n", kind, n, c, #cond, __LINE__);         \
            return false;                                                                                   \
        }                                                                                                   \
    } while (0)

static bool geometry_one(const char* kind, size_t n, int c, int bits) {
    PipShape s;
    REQUIRE(shape_of(kind, n, c, s));
    REQUIRE(s.W >= 1 && s.q >= 1 && s.nwide < s.W);
    REQUIRE(s.W * s.q + s.nwide == (uint32_t)bits);
    REQUIRE(s.off(0) == 0 && s.bbase(0) == 0 && s.tbase(0) == 0 && pip_cbase(s, 0) == 0);
    REQUIRE(s.off(s.W - 1) + s.width(s.W - 1) == (uint32_t)bits);
    REQUIRE(s.top >= 1 && s.top <= (1u << 17));
    REQUIRE(s.fb >= 5 && (1u << s.fb) <= PIP_FINE_MAX);
    REQUIRE(s.fl == 1 || s.fl == 2 || s.fl == 4 || s.fl == 8);
    REQUIRE(s.S >= 1 && s.S <= 8 && s.TS == 64 * s.S);
    REQUIRE(s.L == 8 || s.L == 16 || s.L == 32 || s.L == 64);
    REQUIRE(s.items == (strcmp(kind, "glv") ? n : 2 * n));
    REQUIRE(s.istride % 4 == 0 && s.istride >= s.items && s.istride - s.items < 4);
    REQUIRE((uint64_t)s.cpw * s.L >= s.items && (uint64_t)(s.cpw - 1) * s.L < s.items);
    uint32_t nbmax = 0;
    for (uint32_t j = 0; j < s.W; j++) {
        REQUIRE(s.width(j) >= 1 && s.width(j) <= (uint32_t)c);
        REQUIRE(s.nb(j) >= 1);
        nbmax = std::max(nbmax, s.nb(j));
        REQUIRE(s.capseg >= s.cpw + s.nb(j));
        REQUIRE(pip_ncoarse(s, j) >= 1 && pip_ncoarse(s, j) <= PIP_MAXCOARSE);
        REQUIRE(((uint64_t)pip_ncoarse(s, j) << s.fb) >= s.nb(j) && ((uint64_t)(pip_ncoarse(s, j) - 1) << s.fb) < s.nb(j));
        REQUIRE((uint64_t)s.tiles(j) * s.TS >= s.nb(j) && (uint64_t)(s.tiles(j) - 1) * s.TS < s.nb(j));
        if (j + 1 < s.W) {
            REQUIRE(s.off(j + 1) == s.off(j) + s.width(j));
            REQUIRE(s.bbase(j + 1) == s.bbase(j) + s.nb(j));
            REQUIRE(s.tbase(j + 1) == s.tbase(j) + s.tiles(j));
            REQUIRE(pip_cbase(s, j + 1) == pip_cbase(s, j) + pip_ncoarse(s, j));
        }
    }
    REQUIRE(s.nbmax == nbmax);
    REQUIRE(s.nbuckets == s.bbase(s.W - 1) + s.top);
    REQUIRE(s.ntiles == s.tbase(s.W - 1) + s.tiles(s.W - 1));
    REQUIRE(pip_ncoarse_total(s) == pip_cbase(s, s.W - 1) + pip_ncoarse(s, s.W - 1));
    // every tile belongs to the window whose range of tiles holds it
    uint32_t j = 0;
    for (uint32_t t = 0; t < s.ntiles; t++) {
        while (t >= s.tbase(j) + s.tiles(j)) j++;
        REQUIRE(j < s.W && s.window_of_tile(t) == j);
    }
    // the bias is half the range of every signed window at its offset, nothing else
    uint32_t want[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t w = 0; w + 1 < s.W; w++) {
        const uint32_t bit = s.off(w) + s.width(w) - 1;
        want[bit >> 5] |= 1u << (bit & 31);
    }
    REQUIRE(!memcmp(want, s.bias, sizeof want));
    return true;
}

static int geometry(const char* kind) {
    const int bits = !strcmp(kind, "glv") ? 128 : EdFr::BITS;
    int shapes = 0;
    for (int c = 2; c <= 16; c++)
        for (size_t n : SIZES) {
            if (!geometry_one(kind, n, c, bits)) return 1;
            shapes++;
        }
    // what pip_shape refuses
    PipShape s;
    if (shape_of(kind, 300, 1, s) || shape_of(kind, 300, 17, s) || shape_of(kind, (size_t)1 << 28, 8, s)) {
        fprintf(stderr, "geometry %s: an argument out of range was accepted\n", kind);
        return 1;
    }
    // the chosen width is one pip_shape accepts
    for (int lg = 0; lg < 28; lg++)
        for (size_t n : {(size_t)1 << lg, ((size_t)1 << lg) + 1, ((size_t)2 << lg) - 1}) {
            const int c = pip_pick_c(n, !strcmp(kind, "glv"));
            if (c < 7 || c > 16 || !shape_of(kind, n, c, s)) {
                fprintf(stderr, "geometry %s: pip_pick_c(%zu) = %d\n", kind, n, c);
                return 1;
            }
        }
    printf("ok geometry %s %d\n", kind, shapes);
    return 0;
}

static bool parse_words(const char* h, int nwords, uint32_t* out) {
    if (strlen(h) != (size_t)nwords * 8) return false;
    for (int w = 0; w < nwords; w++) {
        char buf[9];
        memcpy(buf, h + 8 * (nwords - 1 - w), 8);
        buf[8] = 0;
        out[w] = (uint32_t)strtoul(buf, nullptr, 16);
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const char* mode = argv[1];
    if (!strcmp(mode, "table")) {
        for (int a = 2; a < argc; a++) {
            char kind[8];
            unsigned long long n;
            int c;
            if (sscanf(argv[a], "%7[a-z]:%llu:%d", kind, &n, &c) != 3) return 2;
            if (c == 0) c = pip_pick_c((size_t)n, !strcmp(kind, "glv"));
            PipShape s;
            if (!shape_of(kind, (size_t)n, c, s)) return 3;
            printf("%u %u %u %u %u %u %u %u %u %u %u %u\n", s.c, s.W, s.q, s.nwide, s.top, s.nbuckets, s.S, s.L, s.fb, s.fl, s.cpw,
                   s.istride - s.items);
        }
        return 0;
    }
    if (argc < 3) return 2;
    const char* kind = argv[2];
    if (!strcmp(mode, "geometry")) return geometry(kind);
    if (argc < 4) return 2;
    PipShape s;
    if (!shape_of(kind, 300, atoi(argv[3]), s)) return 3;
    if (!strcmp(mode, "layout")) {
        printf("%u %u\n", s.W, s.top);
        for (uint32_t j = 0; j < s.W; j++) printf("%u %u %u\n", s.off(j), s.width(j), s.nb(j));
        return 0;
    }
    if (!strcmp(mode, "recode")) {
        for (int a = 4; a < argc; a++) {
            uint32_t v[8], w[10];
            if (!parse_words(argv[a], 8, v)) return 2;
            uint32_t carry = 0;   // value + bias over ten words, as pip_subscalars forms it
            for (int t = 0; t < 10; t++) {
                const uint64_t x = (uint64_t)(t < 8 ? v[t] : 0u) + s.bias[t] + carry;
                w[t] = (uint32_t)x;
                carry = (uint32_t)(x >> 32);
            }
            for (uint32_t j = 0; j < s.W; j++) printf("%d%c", pip_digit(s, w, j), j + 1 < s.W ? ' ' : '\n');
        }
        return 0;
    }
    return 2;
}
