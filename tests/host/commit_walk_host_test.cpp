// Host-side check of the commitment walk (csrc/commit_walk.hpp), compiled with g++; k_commit_batch (csrc/commit.hpp) runs
// the same code over the engine's tables.  tests/test_commit_walk_cpu.py drives it.
//   <curve 0|1|2> <window_bits> <amount64 0|1> <nv> <v (16 hex digits)>... <gamma (64 hex digits)>...
//   u64 <v (16 hex digits)>...     fe_from_u64 on every scalar field against the value's words (see u64_ok)
// Over a host-built table of g and h = 2 g (PublicKey::new, reference src/publickey.rs:21-29) in the layout of the
// verifier's window tables -- rows built on demand, entry (j, d) = d 2^(off_j) F -- every (v, gamma) pair: the walk's sum
// against double-and-add of s g + gamma h, s = new(v as i32) (reference src/range/prover.rs:37) or, amount64, v itself.
// Prints "ok <sums> additions <n> doublings <n> cancellations <n>"; exits non-zero on the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <vector>
#include "../../bulletproofsplus_amd/csrc/commit_walk.hpp"
using namespace bpp;

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

// The window layout of a verifier's tables (csrc/host_util.hpp make_shape: the constructors of csrc/fixed_glv.hpp).  The
// uniform layout's W, top and per_f are computed here once more, independently, and the constructor is held to them.
template <class C>
static bool make_shape(int c, WinLayout& s) {
    using Fr = typename C::Fr;
    if constexpr (commit_walk_glv<C>()) {
        uint32_t hmax[4];
        glv_half_max<C>(hmax);
        return glv_layout(c, Fr::BITS, hmax, s);
    } else {
        const uint32_t W = (uint32_t)((Fr::BITS - 1) / c + 1), half = 1u << (c - 1);
        if (W > (uint32_t)GLV_MAXW) return false;
        uint32_t bias[10] = {}, v[10], carry = 0;   // r - 1 + bias: the top digit is what is left of it above bit c (W - 1)
        for (uint32_t j = 0; j + 1 < W; j++) {
            const uint32_t bit = (uint32_t)c * j + ((uint32_t)c - 1);
            bias[bit >> 5] |= 1u << (bit & 31);
        }
        for (int t = 0; t < 10; t++) {
            const uint64_t x = (uint64_t)(t < 8 ? Fr::MODW[t] : 0u) + bias[t] + carry;
            v[t] = (uint32_t)x;
            carry = (uint32_t)(x >> 32);
        }
        uint32_t borrow = 1;
        for (int t = 0; t < 10 && borrow; t++) {
            borrow = v[t] == 0 ? 1u : 0u;
            v[t] -= 1u;
        }
        const uint32_t sh = (uint32_t)c * (W - 1);
        uint64_t top = 0;
        bool fits = true;
        for (int t = 9; t >= 0; t--) {
            const int l = 32 * t - (int)sh;
            if (l >= 32 && v[t]) fits = false;
            if (l > -32 && l < 32) top |= l >= 0 ? (uint64_t)v[t] << l : (uint64_t)(v[t] >> (-l));
        }
        fits = fits && top != 0 && !(top >> 31);
        if (win_layout_uniform(c, Fr::MODW, Fr::BITS, s)) {
            if (fits) {
                fprintf(stderr, "the uniform constructor refuses window_bits %d\n", c);
                exit(1);
            }
            return false;
        }
        bool same = fits && s.W == W && s.top == (uint32_t)top && s.per_f == (W - 1) * half + (uint32_t)top && !memcmp(s.bias, bias, sizeof bias);
        for (uint32_t j = 0; j < W && same; j++)
            same = s.wc[j] == (j + 1 < W ? c : 0) && s.off[j] == c * j && s.went[j] == j * half;
        if (!same) {
            fprintf(stderr, "the uniform constructor's layout at window_bits %d differs from the restated one\n", c);
            exit(1);
        }
        return true;
    }
}

template <class C>
static Aff<C> canon(const Aff<C>& a) {
    Aff<C> r = a;
    fe_cond_sub_p(r.x);
    fe_cond_sub_p(r.y);
    return r;
}

template <class C>
struct Table {
    WinLayout s;
    Aff<C> F[2];                               // g, h
    std::vector<Aff<C>> base[2];               // 2^(off_j) F_f
    std::unordered_map<size_t, Aff<C>> memo;   // entries built so far
    explicit Table(const WinLayout& sh) : s(sh) {
        F[0] = aff_generator<C>();
        F[1] = canon(jac_to_aff(aff_dbl(F[0])));
        for (int f = 0; f < 2; f++) {
            Jac<C> b = jac_from_aff(F[f]);
            uint32_t at = 0;
            for (uint32_t j = 0; j < s.W; j++) {
                for (; at < s.off[j]; at++) b = jac_dbl(b);
                base[f].push_back(canon(jac_to_aff(b)));
            }
        }
    }
    Aff<C> entry(size_t e) {
        auto it = memo.find(e);
        if (it != memo.end()) return it->second;
        const uint32_t f = (uint32_t)(e / s.per_f), idx = (uint32_t)(e % s.per_f);
        if (f > 1) {
            fprintf(stderr, "entry %zu lies outside the rows of g and h\n", e);
            exit(1);
        }
        uint32_t j = s.W - 1;
        while (j > 0 && s.went[j] > idx) j--;
        const uint32_t d = idx - s.went[j] + 1;
        const uint32_t cnt = win_entries(s, j);
        if (d > cnt) {
            fprintf(stderr, "entry %zu is past window %u\n", e, j);
            exit(1);
        }
        const Aff<C> r = canon(jac_to_aff(aff_mul_words(base[f][j], &d, 1)));
        memo.emplace(e, r);
        return r;
    }
};

template <class C>
static int run(int c, bool amount64, const std::vector<uint64_t>& vs, const std::vector<std::vector<uint32_t>>& gs) {
    WinLayout s;
    if (!make_shape<C>(c, s)) return 2;
    Table<C> T(s);
    long additions = 0, doublings = 0, cancellations = 0, sums = 0;
    std::vector<Jac<C>> gh;   // gamma h by double-and-add
    for (const auto& g : gs) gh.push_back(aff_mul_words(T.F[1], g.data(), 8));
    for (uint64_t v : vs) {
        uint32_t kv[8];
        commit_amount_scalar<C>(v, amount64, kv);
        // the scalar on g, stated independently: v, or r - |v as i32|
        uint32_t want_k[8] = {};
        const int32_t vi = (int32_t)(uint32_t)v;
        if (amount64) {
            want_k[0] = (uint32_t)v;
            want_k[1] = (uint32_t)(v >> 32);
        } else if (vi >= 0) {
            want_k[0] = (uint32_t)vi;
        } else {
            uint64_t sub = (uint64_t)(-(int64_t)vi);   // <= 2^31: one word, then the borrow
            for (int t = 0; t < 8; t++) {
                const uint64_t m = C::Fr::MODW[t];
                want_k[t] = (uint32_t)(m - sub);
                sub = m < sub ? 1u : 0u;
            }
        }
        if (memcmp(kv, want_k, sizeof kv)) {
            fprintf(stderr, "scalar mismatch: v %016llx\n", (unsigned long long)v);
            return 1;
        }
        const Jac<C> vg = aff_mul_words(T.F[0], want_k, 8);
        for (size_t gi = 0; gi < gs.size(); gi++) {
            const Xyzz<C> acc = commit_walk<C>(
                s, kv, gs[gi].data(), [&](size_t e) { return T.entry(e); },
                [&](Xyzz<C>& a, const Aff<C>& q, bool neg) {
                    additions++;
                    if (!a.is_inf()) {   // which exceptional case is this step, if any (for the report only)
                        const Jac<C> j = xyzz_to_jac(a);
                        const Aff<C> qq = neg ? canon(aff_neg(q)) : q;
                        if (jac_eq(j, jac_from_aff(qq))) doublings++;
                        if (jac_eq(j, jac_from_aff(canon(aff_neg(qq))))) cancellations++;
                    }
                    xyzz_madd_lazy(a, q, neg);
                });
            if (!jac_eq(xyzz_to_jac(acc), jac_add(vg, gh[gi]))) {
                fprintf(stderr, "mismatch: v %016llx gamma #%zu\n", (unsigned long long)v, gi);
                return 1;
            }
            sums++;
        }
    }
    printf("ok %ld additions %ld doublings %ld cancellations %ld\n", sums, additions, doublings, cancellations);
    return 0;
}

// fe_from_u64 (csrc/field.hpp; the scalar k_pb_init stores under BPP_PROVE_AMOUNT64): canonical image = the value's two
// words, and the element equals the one fe_from_canonical makes of them
template <class P>
static bool u64_ok(uint64_t v) {
    uint32_t w[8] = {(uint32_t)v, (uint32_t)(v >> 32), 0, 0, 0, 0, 0, 0}, got[8], ref[8];
    fe_to_canonical(fe_from_u64<P>(v), got);
    fe_to_canonical(fe_from_canonical<P>(w), ref);
    if (v <= 0xffffffffull) {
        uint32_t small[8];
        fe_to_canonical(fe_from_u32<P>((uint32_t)v), small);
        if (memcmp(small, got, sizeof got)) return false;
    }
    return !memcmp(got, w, sizeof got) && !memcmp(got, ref, sizeof got);
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "u64")) {   // u64 <v (16 hex digits)>...: every scalar field
        for (int a = 2; a < argc; a++) {
            uint32_t w[2];
            if (!parse_words(argv[a], 2, w)) return 2;
            const uint64_t v = ((uint64_t)w[1] << 32) | w[0];
            if (!u64_ok<Bls12381::Fr>(v) || !u64_ok<Secp256k1::Fr>(v) || !u64_ok<Ed25519::Fr>(v)) {
                fprintf(stderr, "fe_from_u64 mismatch: %016llx\n", (unsigned long long)v);
                return 1;
            }
        }
        printf("ok u64 %d\n", argc - 2);
        return 0;
    }
    if (argc < 5) return 2;
    const int curve = atoi(argv[1]), c = atoi(argv[2]);
    const bool amount64 = atoi(argv[3]) != 0;
    const int nv = atoi(argv[4]);
    if (c < 2 || c > 20 || nv < 0 || argc < 5 + nv) return 2;
    std::vector<uint64_t> vs;
    for (int a = 0; a < nv; a++) {
        uint32_t w[2];
        if (!parse_words(argv[5 + a], 2, w)) return 2;
        vs.push_back(((uint64_t)w[1] << 32) | w[0]);
    }
    std::vector<std::vector<uint32_t>> gs;
    for (int a = 5 + nv; a < argc; a++) {
        std::vector<uint32_t> g(8);
        if (!parse_words(argv[a], 8, g.data())) return 2;
        gs.push_back(g);
    }
    switch (curve) {
        case 0: return run<Bls12381>(c, amount64, vs, gs);
        case 1: return run<Secp256k1>(c, amount64, vs, gs);
        case 2: return run<Ed25519>(c, amount64, vs, gs);
        default: return 2;
    }
}
