// Host-side harness for csrc/recover_terms.hpp (compiled with g++, no GPU needed): Gamma of proofs given by their scalar
// triple, challenge block and blinding source, computed by the code k_recover_masks runs (recover_mask: the k + 2 terms
// one after the other).
//   recover_host_test <file>
// file: one proof per line, fields separated by blanks, scalars as 64 hex digits (big-endian integers):
//   <curve 0|1|2> <k> <m> key <64 hex key bytes> <index> <r'> <s'> <delta'> <y> <z> <e> <e_1..e_k>
//   <curve> <k> <m> blind <5 + 2k scalars> <r'> <s'> <delta'> <y> <z> <e> <e_1..e_k>
//   <curve> <k> <m> lit <r'> <s'> <delta'> <y> <z> <e> <e_1..e_k>
// prints per proof "<Gamma as 64 hex digits> <1: recovered | 0: a zero challenge>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "../../bulletproofsplus_amd/csrc/ed25519.hpp"
#include "../../bulletproofsplus_amd/csrc/recover_terms.hpp"
using namespace bpp;

// 64 hex digits, big-endian -> 8 little-endian words
static bool scalar_words(const std::string& h, uint32_t* w) {
    if (h.size() != 64) return false;
    for (int i = 0; i < 8; i++) w[7 - i] = (uint32_t)strtoul(h.substr(8 * i, 8).c_str(), nullptr, 16);
    return true;
}

template <class C>
static bool one(uint32_t k, uint32_t m, const std::string& mode, std::istringstream& in) {
    using P = typename C::Fr;
    RecoverSource src;
    src.have_key = false;
    for (int i = 0; i < 8; i++) src.key[i] = 0;
    src.blind = nullptr;
    src.idx = 0;
    src.lit = recover_literals(m == 1 ? 7u : 33u, 4u, 5u, 88u, 123u);
    std::vector<uint32_t> blind((size_t)pb_blind_elems(k) * 8);   // exact size: a slot beyond 5 + 2k is an overflow
    std::string tok;
    if (mode == "key") {
        unsigned long long idx;
        if (!(in >> tok) || tok.size() != 64 || !(in >> idx)) return false;
        for (int i = 0; i < 8; i++) {   // the key's BYTES as little-endian words
            uint32_t x = 0;
            for (int b = 3; b >= 0; b--) x = (x << 8) | (uint32_t)strtoul(tok.substr(8 * i + 2 * b, 2).c_str(), nullptr, 16);
            src.key[i] = x;
        }
        src.have_key = true;
        src.idx = idx;
    } else if (mode == "blind") {
        for (uint32_t j = 0; j < pb_blind_elems(k); j++)
            if (!(in >> tok) || !scalar_words(tok, blind.data() + (size_t)j * 8)) return false;
        src.blind = blind.data();
    } else if (mode != "lit") {
        return false;
    }
    std::vector<uint32_t> triple(24), ch((size_t)(3 + k) * 8);
    for (int j = 0; j < 3; j++)
        if (!(in >> tok) || !scalar_words(tok, triple.data() + j * 8)) return false;
    for (uint32_t j = 0; j < 3 + k; j++)
        if (!(in >> tok) || !scalar_words(tok, ch.data() + (size_t)j * 8)) return false;
    uint32_t out[8];
    const bool ok = recover_mask<P>(src, k, m, triple.data(), ch.data(), out);
    for (int i = 7; i >= 0; i--) printf("%08x", out[i]);
    printf(" %d\n", ok ? 1 : 0);
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) return 1;
    std::ifstream f(argv[1]);
    if (!f) return 2;
    std::string line;
    size_t n = 0;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        unsigned curve, k, m;
        std::string mode;
        if (!(in >> curve >> k >> m >> mode) || k > 14 || m == 0) return 3;
        const bool good = curve == 0 ? one<Bls12381>(k, m, mode, in) : curve == 1 ? one<Secp256k1>(k, m, mode, in)
                                                                                  : curve == 2 && one<Ed25519>(k, m, mode, in);
        if (!good) {
            fprintf(stderr, "line %zu: malformed\n", n);
            return 3;
        }
        n++;
    }
    return 0;
}
