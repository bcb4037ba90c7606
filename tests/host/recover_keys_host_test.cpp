// Host-side harness for csrc/recover_coeffs.hpp (compiled with g++, no GPU needed): the key-independent coefficients of
// mask recovery and the projective comparison of the many-key scan, by the code k_recover_coeffs, pair_gamma
// (k_scan_keys; k_find_scan_list of csrc/find.hpp) and pair_confirms (k_scan_keys_confirm and the find call's two confirmation
// kernels) of csrc/recover_keys.hpp run.
//   recover_keys_host_test <file>
// file: one proof per line, fields separated by blanks, scalars as 64 hex digits (big-endian integers):
//   <curve 0|1|2> <k> <m> <index> <n_keys> <64 hex key bytes>.. <r'> <s'> <delta'> <y> <z> <e> <e_1..e_k>
// prints per proof and key one line
//   "<Gamma by A0 + sum c_s slot_s> <Gamma by recover_mask> <ok of recover_coeffs> <ok of recover_mask> <1: c_r = c_s = 0>"
// where the sum runs as a lane group of k_scan_keys runs it: over the live slots, strided by SCAN_GROUP.
//   recover_keys_host_test cmp
// walk_equals_wire against aff_to_wire(jac_to_aff(xyzz_to_jac(acc))) and k_recover_confirm's comparison on every curve:
// equal and unequal points, infinity on either side, for edwards25519 representatives shifted by the points of E[4].
// Prints "ok cmp <curve> <cases>" per curve; exits non-zero on the first disagreement.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "../../bulletproofsplus_amd/csrc/recover_coeffs.hpp"
using namespace bpp;

static bool scalar_words(const std::string& h, uint32_t* w) {
    if (h.size() != 64) return false;
    for (int i = 0; i < 8; i++) w[7 - i] = (uint32_t)strtoul(h.substr(8 * i, 8).c_str(), nullptr, 16);
    return true;
}
static void print_words(const uint32_t* w) {
    for (int i = 7; i >= 0; i--) printf("%08x", w[i]);
}

template <class C>
static bool one(uint32_t k, uint32_t m, std::istringstream& in) {
    using P = typename C::Fr;
    using F = Fe<P>;
    unsigned long long idx;
    unsigned nk;
    if (!(in >> idx >> nk) || nk == 0 || nk > 64) return false;
    std::vector<uint32_t> keys((size_t)nk * 8);
    std::string tok;
    for (unsigned j = 0; j < nk; j++) {
        if (!(in >> tok) || tok.size() != 64) return false;
        for (int i = 0; i < 8; i++) {   // the key's BYTES as little-endian words
            uint32_t x = 0;
            for (int b = 3; b >= 0; b--) x = (x << 8) | (uint32_t)strtoul(tok.substr(8 * i + 2 * b, 2).c_str(), nullptr, 16);
            keys[(size_t)j * 8 + i] = x;
        }
    }
    std::vector<uint32_t> triple(24), ch((size_t)(3 + k) * 8);
    for (int j = 0; j < 3; j++)
        if (!(in >> tok) || !scalar_words(tok, triple.data() + j * 8)) return false;
    for (uint32_t j = 0; j < 3 + k; j++)
        if (!(in >> tok) || !scalar_words(tok, ch.data() + (size_t)j * 8)) return false;
    std::vector<F> c((size_t)pb_blind_elems(k) + 1);   // exact size: a slot beyond 5 + 2k is an overflow
    bool ok;
    recover_coeffs<P>(k, m, triple.data(), ch.data(), c.data(), ok);
    const bool rs_zero = c[PB_BL_R].is_zero() && c[PB_BL_S].is_zero();
    for (unsigned j = 0; j < nk; j++) {
        const uint32_t* key = keys.data() + (size_t)j * 8;
        F lane[8];
        const uint32_t nl = coeff_live_slots(k);
        for (uint32_t s = 0; s < 8; s++) {
            lane[s] = F::zero();
            for (uint32_t l = s; l < nl; l += 8) lane[s] = fe_add(lane[s], coeff_slot_share<P>(key, idx, coeff_live_slot(l), c[coeff_live_slot(l)]));
        }
        for (uint32_t d = 4; d >= 1; d >>= 1)
            for (uint32_t s = 0; s < d; s++) lane[s] = fe_add(lane[s], lane[s + d]);
        uint32_t g[8], want[8];
        fe_to_canonical(ok ? fe_add(lane[0], c[pb_blind_elems(k)]) : F::zero(), g);
        RecoverSource src;
        src.have_key = true;
        for (int i = 0; i < 8; i++) src.key[i] = key[i];
        src.idx = idx;
        src.blind = nullptr;
        src.lit = 0;
        const bool ok2 = recover_mask<P>(src, k, m, triple.data(), ch.data(), want);
        print_words(g);
        printf(" ");
        print_words(want);
        printf(" %d %d %d\n", ok ? 1 : 0, ok2 ? 1 : 0, rs_zero ? 1 : 0);
    }
    return true;
}

// ---- the projective comparison --------------------------------------------------------------------------------------
// what k_recover_confirm does with its accumulator: the wire image, then the comparison with V
template <class C>
static bool reference_equal(const Xyzz<C>& acc, const uint32_t* V) {
    constexpr int N = C::Fp::N;
    uint32_t w[2 * N + 2];
    aff_to_wire(jac_to_aff(xyzz_to_jac(acc)), w);
    const bool inf_w = (w[2 * N] | w[2 * N + 1]) != 0, inf_V = (V[2 * N] | V[2 * N + 1]) != 0;
    if constexpr (C::ID == 2) {
        using Fp = typename C::Fp;
        Aff<C> a = aff_inf<C>(), b = aff_inf<C>();
        if (!inf_w) {
            a.x = fe_from_canonical<Fp>(w);
            a.y = fe_from_canonical<Fp>(w + N);
        }
        if (!inf_V) {
            b.x = fe_from_canonical<Fp>(V);
            b.y = fe_from_canonical<Fp>(V + N);
        }
        return rist_equal(a, b);
    } else {
        bool same = inf_w == inf_V;
        if (!inf_w)
            for (int t = 0; t < 2 * N; t++) same = same && w[t] == V[t];
        return same;
    }
}
// n g as a walk would leave it: n lazy mixed additions of g (the second one takes the doubling branch)
template <class C>
static Xyzz<C> times_g(int n) {
    Xyzz<C> acc = xyzz_inf<C>();
    const Aff<C> g = aff_generator<C>();
    for (int i = 0; i < n; i++) xyzz_madd_lazy(acc, g, false);
    return acc;
}
template <class C>
static int compare_cases(const char* name) {
    constexpr int N = C::Fp::N;
    constexpr int WW = 2 * N + 2;
    int cases = 0;
    auto check = [&](const Xyzz<C>& acc, const uint32_t* V, int want) {
        const bool got = walk_equals_wire<C>(acc, V), ref = reference_equal<C>(acc, V);
        cases++;
        if (got != ref || (want >= 0 && (int)got != want)) {
            fprintf(stderr, "%s: case %d: projective %d, by inversion %d, expected %d\n", name, cases, got, ref, want);
            exit(4);
        }
    };
    std::vector<std::vector<uint32_t>> wires;
    for (int n = 0; n <= 9; n++) {
        std::vector<uint32_t> w(WW);
        aff_to_wire(jac_to_aff(xyzz_to_jac(times_g<C>(n))), w.data());
        wires.push_back(w);
    }
    for (int a = 0; a <= 9; a++) {
        Xyzz<C> acc = times_g<C>(a);
        for (int b = 0; b <= 9; b++) check(acc, wires[b].data(), a == b);   // 0: infinity on either side, on both
        // a - a through the cancellation branch: the identity with whatever coordinates the walk leaves
        xyzz_madd_lazy(acc, aff_generator<C>(), true);
        check(acc, wires[a ? a - 1 : 0].data(), a ? 1 : -1);
    }
    if constexpr (C::ID == 2) {
        // another representative of the same ristretto255 element: the accumulator's point plus a point of E[4]
        using F = Fe<typename C::Fp>;
        Aff<C> t4[3];
        t4[0].x = ed::konst(Ed25519Consts::SQRT_M1);
        t4[0].y = F::zero();
        t4[1].x = fe_neg(t4[0].x);
        t4[1].y = F::zero();
        t4[2].x = F::zero();
        t4[2].y = fe_neg(F::one());
        for (int a = 0; a <= 9; a++) {
            const Xyzz<C> acc = times_g<C>(a);
            for (int t = 0; t < 3; t++) {
                uint32_t w[WW];
                aff_to_wire(jac_to_aff(jac_madd(xyzz_to_jac(acc), t4[t])), w);
                check(acc, w, 1);
                check(times_g<C>(a + 1), w, 0);
            }
        }
    }
    printf("ok cmp %s %d\n", name, cases);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) return 1;
    if (!strcmp(argv[1], "cmp")) {
        compare_cases<Bls12381>("bls12_381");
        compare_cases<Secp256k1>("secp256k1");
        compare_cases<Ed25519>("ed25519");
        return 0;
    }
    std::ifstream f(argv[1]);
    if (!f) return 2;
    std::string line;
    size_t n = 0;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        unsigned curve, k, m;
        if (!(in >> curve >> k >> m) || k > 14 || m == 0) return 3;
        const bool good = curve == 0 ? one<Bls12381>(k, m, in) : curve == 1 ? one<Secp256k1>(k, m, in) : curve == 2 && one<Ed25519>(k, m, in);
        if (!good) {
            fprintf(stderr, "line %zu: malformed\n", n);
            return 3;
        }
        n++;
    }
    return 0;
}
