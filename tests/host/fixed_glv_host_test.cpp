// Host-side checks of the fixed-generator tables' windows (csrc/fixed_glv.hpp) and of the GLV path over them (csrc/ec.hpp
// glv_split_balanced / xyzz_mul_x_beta), compiled with g++; the kernels (k_fixed_msm, k_tbl_bases / k_tbl_fill) and the
// verifier's constructor run the same code.  tests/test_fixed_glv_cpu.py drives it and compares with Python integers.
// <c> is window_bits: alone the mixed-width layout of BLS12-381's halves, as <c>@secp256k1 or <c>@ed25519 the uniform
// layout of that curve's whole scalars.
//   split  <k>...        per scalar (64 hex digits): "s1 k1 s2 k2" (signs as 0 / 1, magnitudes as 32 hex digits)
//   layout <c>           "W top per_f" then one line per window: "width offset first_entry", then the bias (40 hex digits;
//                        uniform: 80)
//   recode <c> <h>...    per half (32 hex digits; uniform: per scalar, 64 hex digits): its W digits, lowest window first
//   group  <c> <k>...    the two-phase sum over a host-built table of the BLS12-381 generator F against double-and-add:
//                        every scalar alone (k F), and every pair of neighbours in ONE accumulator, as two generators that
//                        happen to be the same point ((k_i + k_{i+1}) F: the pairs reach P + P and P - P); and every scalar
//                        alone in the form the kernel gives a proof's left-over entries, psi applied to each k2 ENTRY
//                        (x <- beta x) instead of to the accumulator.  Prints
//                        "ok <sums> doublings <n> cancellations <n>"; exits non-zero on the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../bulletproofsplus_amd/csrc/ed25519.hpp"
#include "../../bulletproofsplus_amd/csrc/fixed_glv.hpp"
using namespace bpp;
using C = Bls12381;

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

// carg: "<c>" or "<c>@<curve>"; NW: the words of a biased value under the layout
static bool layout_of(const char* carg, WinLayout& L, int& NW) {
    const int c = atoi(carg);
    const char* at = strchr(carg, '@');
    NW = at ? WIN_FULL_WORDS : GLV_HALF_WORDS;
    if (!at) {
        uint32_t hmax[4];
        glv_half_max<C>(hmax);
        return glv_layout(c, C::Fr::BITS, hmax, L);
    }
    if (c < 2 || c > 20) return false;   // csrc/host_util.hpp make_shape
    if (!strcmp(at, "@secp256k1")) return !win_layout_uniform(c, Secp256k1::Fr::MODW, Secp256k1::Fr::BITS, L);
    if (!strcmp(at, "@ed25519")) return !win_layout_uniform(c, Ed25519::Fr::MODW, Ed25519::Fr::BITS, L);
    return false;
}

template <int NW>
static void print_digits(const WinLayout& L, const uint32_t* k) {
    uint32_t v[NW];
    win_biased<NW>(k, L.bias, v);
    for (uint32_t j = 0; j < L.W; j++) printf("%d%c", win_next_digit(v, win_width(L, j)), j + 1 < L.W ? ' ' : '\n');
}

static Aff<C> canon(const Aff<C>& a) {
    Aff<C> r = a;
    fe_cond_sub_p(r.x);
    fe_cond_sub_p(r.y);
    return r;
}

struct Sum {
    Xyzz<C> acc = xyzz_inf<C>();
    int doublings = 0, cancellations = 0;
};

// one phase of one generator: the W digits of the chosen half, each one table gather and one lazy mixed addition
// via_beta: the entries of the k2 half take psi themselves (the accumulator is not multiplied between the phases)
static void add_half(const GlvLayout& L, const std::vector<Aff<C>>& table, const uint32_t* k, int phase, Sum& s,
                     bool via_beta = false) {
    uint32_t k1[4], k2[4], v[GLV_HALF_WORDS];
    bool n1, n2;
    glv_split_balanced<C>(k, k1, k2, n1, n2);
    glv_biased(phase ? k1 : k2, L.bias, v);
    const bool hneg = phase ? n1 : !n2;   // phase 0 sums the k2 halves negated: psi(-S) = (beta X, Y)
    for (uint32_t j = 0; j < L.W; j++) {
        const int32_t dg = glv_next_digit(v, L.wc[j]);
        if (dg == 0) continue;
        const uint32_t mag = dg < 0 ? (uint32_t)(-dg) : (uint32_t)dg;
        Aff<C> e = table[L.went[j] + mag - 1];
        if (via_beta && phase == 0) aff_mul_x_beta(e);
        const bool neg = (dg < 0) != hneg;
        if (!s.acc.is_inf()) {   // which exceptional case is this step, if any (for the report only)
            const Jac<C> a = xyzz_to_jac(s.acc);
            const Aff<C> q = neg ? canon(aff_neg(e)) : e;
            if (jac_eq(a, jac_from_aff(q))) s.doublings++;
            if (jac_eq(a, jac_from_aff(canon(aff_neg(q))))) s.cancellations++;
        }
        xyzz_madd_lazy(s.acc, e, neg);
    }
}

static bool same_affine(const Jac<C>& a, const Jac<C>& b) {
    if (a.is_inf() || b.is_inf()) return a.is_inf() && b.is_inf();
    const Aff<C> x = canon(jac_to_aff(a)), y = canon(jac_to_aff(b));
    return x.x == y.x && x.y == y.y;
}

static int group(const char* carg, int argc, char** argv) {
    WinLayout L;
    int NW;
    if (!layout_of(carg, L, NW) || NW != GLV_HALF_WORDS || L.per_f > 4096) return 2;
    const Aff<C> F = aff_generator<C>();
    std::vector<Aff<C>> table(L.per_f);
    Jac<C> base = jac_from_aff(F);
    for (uint32_t j = 0; j < L.W; j++) {   // T[j][d] = d 2^(off_j) F
        const uint32_t cnt = win_entries(L, j);
        const Aff<C> b = canon(jac_to_aff(base));
        Jac<C> run = base;
        for (uint32_t d = 1; d <= cnt; d++) {
            table[L.went[j] + d - 1] = canon(jac_to_aff(run));
            run = jac_madd(run, b);
        }
        for (uint32_t t = 0; t < L.wc[j]; t++) base = jac_dbl(base);
    }
    std::vector<std::vector<uint32_t>> ks;
    for (int a = 0; a < argc; a++) {
        std::vector<uint32_t> k(8);
        if (!parse_words(argv[a], 8, k.data())) return 2;
        ks.push_back(k);
    }
    int sums = 0, doublings = 0, cancellations = 0;
    for (size_t i = 0; i < ks.size(); i++) {
        for (int pair = 0; pair < 2; pair++) {
            if (pair && i + 1 == ks.size()) continue;
            Sum s;
            for (int phase = 0; phase < 2; phase++) {
                if (phase == 1) xyzz_mul_x_beta(s.acc);
                add_half(L, table, ks[i].data(), phase, s);
                if (pair) add_half(L, table, ks[i + 1].data(), phase, s);
            }
            Jac<C> want = aff_mul_words(F, ks[i].data(), 8);
            if (pair) want = jac_add(want, aff_mul_words(F, ks[i + 1].data(), 8));
            if (!same_affine(xyzz_to_jac(s.acc), want)) {
                fprintf(stderr, "mismatch: %s scalar %zu\n", pair ? "pair at" : "single", i);
                return 1;
            }
            sums++;
            doublings += s.doublings;
            cancellations += s.cancellations;
        }
        Sum lo;
        for (int phase = 0; phase < 2; phase++) add_half(L, table, ks[i].data(), phase, lo, true);
        if (!same_affine(xyzz_to_jac(lo.acc), aff_mul_words(F, ks[i].data(), 8))) {
            fprintf(stderr, "mismatch: left-over form, scalar %zu\n", i);
            return 1;
        }
        sums++;
    }
    printf("ok %d doublings %d cancellations %d\n", sums, doublings, cancellations);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const char* mode = argv[1];
    if (!strcmp(mode, "split")) {
        for (int a = 2; a < argc; a++) {
            uint32_t k[8], k1[4], k2[4];
            bool n1, n2;
            if (!parse_words(argv[a], 8, k)) return 2;
            glv_split_balanced<C>(k, k1, k2, n1, n2);
            printf("%d %08x%08x%08x%08x %d %08x%08x%08x%08x\n", n1 ? 1 : 0, k1[3], k1[2], k1[1], k1[0], n2 ? 1 : 0, k2[3], k2[2],
                   k2[1], k2[0]);
        }
        return 0;
    }
    if (argc < 3) return 2;
    if (!strcmp(mode, "group")) return group(argv[2], argc - 3, argv + 3);
    WinLayout L;
    int NW;
    if (!layout_of(argv[2], L, NW)) return 3;
    if (!strcmp(mode, "layout")) {
        printf("%u %u %u\n", L.W, L.top, L.per_f);
        for (uint32_t j = 0; j < L.W; j++) printf("%u %u %u\n", (unsigned)L.wc[j], (unsigned)L.off[j], L.went[j]);
        for (int t = NW - 1; t >= 0; t--) printf("%08x", L.bias[t]);
        printf("\n");
        return 0;
    }
    if (!strcmp(mode, "recode")) {
        for (int a = 3; a < argc; a++) {
            uint32_t k[8];
            if (!parse_words(argv[a], NW == GLV_HALF_WORDS ? 4 : 8, k)) return 2;
            if (NW == GLV_HALF_WORDS)
                print_digits<GLV_HALF_WORDS>(L, k);
            else
                print_digits<WIN_FULL_WORDS>(L, k);
        }
        return 0;
    }
    return 2;
}
