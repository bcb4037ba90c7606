// Host-side harness for csrc/output_terms.hpp (compiled with g++, no GPU needed): the code k_outputs_make, k_out_tags and
// k_out_confirm (csrc/outputs.hpp) run.
//   output_terms_host_test terms <file>
// file: one line per output, "<curve 0|1|2> <64 hex key bytes> <index, decimal> <j, decimal>"; prints
// "<mask as 64 hex digits, most significant first> <pad as 16 hex digits> <tag as 2 hex digits>" per line.
//   output_terms_host_test lanes <n_keys> <count_c> <logm>
// Enumerates the per-output tag test of one class the way k_out_tags does (tile, round, lane -> key, launch output
// position -> proof, place) and prints "<tile> <round> <lane> <key> <proof> <place>" for every lane that holds a pair,
// after a first line "<tiles> <per_key> <outs>".
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include "../../bulletproofsplus_amd/csrc/ed25519.hpp"
#include "../../bulletproofsplus_amd/csrc/output_terms.hpp"
using namespace bpp;

static bool key_words(const std::string& tok, uint32_t* key) {
    if (tok.size() != 64) return false;
    for (int i = 0; i < 8; i++) {   // the key's BYTES as little-endian words
        uint32_t x = 0;
        for (int b = 3; b >= 0; b--) x = (x << 8) | (uint32_t)strtoul(tok.substr(8 * i + 2 * b, 2).c_str(), nullptr, 16);
        key[i] = x;
    }
    return true;
}

template <class C>
static void one(const uint32_t* key, uint64_t idx, uint32_t j) {
    uint32_t g[8];
    fe_to_canonical(output_mask<typename C::Fr>(key, idx, j), g);
    for (int t = 7; t >= 0; t--) printf("%08x", g[t]);
    printf(" %016llx %02x\n", (unsigned long long)output_pad(key, idx, j), (unsigned)output_tag(key, idx, j));
}

static int lanes(size_t n_keys, size_t count_c, uint32_t logm) {
    const size_t outs = output_class_outputs(count_c, logm);
    const size_t per_key = tag_tiles_per_key(outs), tiles = tag_tiles(n_keys, outs);
    printf("%zu %zu %zu\n", tiles, per_key, outs);
    for (size_t t = 0; t < tiles; t++) {
        const size_t key_no = tag_tile_key(t, per_key);
        if (key_no >= n_keys) return 1;
        for (uint32_t r = 0; r < FIND_ROUNDS; r++)
            for (uint32_t lane = 0; lane < FIND_BLOCK; lane++) {
                const size_t x = tag_launch_position(t, per_key, r, lane);
                if (x >= outs) continue;
                const size_t p = output_proof(x, logm);
                const uint32_t place = output_place(x, logm);
                if (p >= count_c || place >= (1u << logm) || tag_pair(key_no, x, outs) >= n_keys * outs) return 1;
                printf("%zu %u %u %zu %zu %u\n", t, r, lane, key_no, p, place);
            }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    if (mode == "lanes") {
        if (argc != 5) return 2;
        return lanes((size_t)strtoull(argv[2], nullptr, 10), (size_t)strtoull(argv[3], nullptr, 10),
                     (uint32_t)strtoul(argv[4], nullptr, 10));
    }
    if (mode != "terms") return 2;
    std::ifstream f(argv[2]);
    if (!f) return 2;
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string tok;
        int curve;
        unsigned long long idx, j;
        uint32_t key[8];
        if (!(in >> curve >> tok >> idx >> j) || !key_words(tok, key) || j >> 32) return 2;
        if (curve == 0)
            one<Bls12381>(key, idx, (uint32_t)j);
        else if (curve == 1)
            one<Secp256k1>(key, idx, (uint32_t)j);
        else if (curve == 2)
            one<Ed25519>(key, idx, (uint32_t)j);
        else
            return 2;
    }
    return 0;
}
