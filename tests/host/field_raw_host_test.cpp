// Host build (g++, no GPU) of csrc/field_raw_ops.hpp -- the table the debug kernel of csrc/tu_debug.hip compiles from the
// same text -- and of the lazy mixed addition on a raw accumulator.  tests/test_field_raw_cpu.py drives it with the cases
// of tests/field_cases.py and checks the answers against Python integers.
// stdin: records of 32-bit little-endian words, stdout: the results, in order.
//   0 curve field op n | a[n NL] b[n NL] c[n NL] d[n NL]      ->  n results of 2 NL words (fe_raw_op)
//   1 curve 0     0  n | acc[n 4 NL] q[n 2 NL] neg[n]         ->  n accumulators of 4 NL words (xyzz_madd_lazy)
// curve: 0 BLS12-381, 1 secp256k1, 2 edwards25519; field: 0 base field, 1 scalar field.  Exit code 2: malformed input.
#include <cstdio>
#include <vector>
#include "../../bulletproofsplus_amd/csrc/field_raw_ops.hpp"
#include "../../bulletproofsplus_amd/csrc/ristretto.hpp"
using namespace bpp;

static bool read_words(std::vector<uint32_t>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), 4, n, stdin) == n;
}

template <class P>
static int run_field(int op, size_t n) {
    constexpr int NL = P::NL, OW = raw_out_words(NL);
    std::vector<uint32_t> a, b, c, d, out(n * OW);
    if (!read_words(a, n * NL) || !read_words(b, n * NL) || !read_words(c, n * NL) || !read_words(d, n * NL)) return 2;
    for (size_t i = 0; i < n; i++)
        if (!fe_raw_op_any<P>(op, &a[i * NL], &b[i * NL], &c[i * NL], &d[i * NL], &out[i * OW])) return 2;
    fwrite(out.data(), 4, out.size(), stdout);
    return 0;
}

template <class C>
static int run_madd(size_t n) {
    using P = typename C::Fp;
    constexpr int NL = P::NL;
    std::vector<uint32_t> acc, q, neg, out(n * 4 * NL);
    if (!read_words(acc, n * 4 * NL) || !read_words(q, n * 2 * NL) || !read_words(neg, n)) return 2;
    for (size_t i = 0; i < n; i++) {
        Fe<P> e[4];
        for (int t = 0; t < 4; t++) e[t] = raw_limbs<P>(&acc[(i * 4 + t) * NL]);
        Aff<C> pt;
        pt.x = raw_limbs<P>(&q[(i * 2) * NL]);
        pt.y = raw_limbs<P>(&q[(i * 2 + 1) * NL]);
        Xyzz<C> p;
        if constexpr (C::ID == 2) {
            p.e.X = e[0], p.e.Y = e[1], p.e.Z = e[2], p.e.T = e[3];
        } else {
            p.X = e[0], p.Y = e[1], p.ZZ = e[2], p.ZZZ = e[3];
        }
        xyzz_madd_lazy(p, pt, neg[i] != 0);
        if constexpr (C::ID == 2) {
            e[0] = p.e.X, e[1] = p.e.Y, e[2] = p.e.Z, e[3] = p.e.T;
        } else {
            e[0] = p.X, e[1] = p.Y, e[2] = p.ZZ, e[3] = p.ZZZ;
        }
        for (int t = 0; t < 4; t++) raw_put(e[t], &out[(i * 4 + t) * NL]);
    }
    fwrite(out.data(), 4, out.size(), stdout);
    return 0;
}

int main() {
    uint32_t h[5];
    while (fread(h, 4, 5, stdin) == 5) {
        const uint32_t kind = h[0], curve = h[1], field = h[2];
        const int op = (int)h[3];
        const size_t n = h[4];
        int rc = 2;
        if (kind == 0 && field < 2) {
            switch (curve * 2 + field) {
                case 0: rc = run_field<BlsFp>(op, n); break;
                case 1: rc = run_field<BlsFr>(op, n); break;
                case 2: rc = run_field<SecpFp>(op, n); break;
                case 3: rc = run_field<SecpFr>(op, n); break;
                case 4: rc = run_field<EdFp>(op, n); break;
                case 5: rc = run_field<EdFr>(op, n); break;
                default: break;
            }
        } else if (kind == 1) {
            if (curve == 0) rc = run_madd<Bls12381>(n);
            if (curve == 1) rc = run_madd<Secp256k1>(n);
            if (curve == 2) rc = run_madd<Ed25519>(n);
        }
        if (rc) return rc;
    }
    return 0;
}
