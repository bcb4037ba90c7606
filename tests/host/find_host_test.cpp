// Host-side harness for csrc/find_terms.hpp (compiled with g++, no GPU needed): the pad of a sealed amount and the index
// arithmetic of the hit list's compaction, by the code k_amounts_seal, the two confirmation kernels (find_pair_amount),
// k_find_count and k_find_emit (csrc/find.hpp) run -- amount_pad is key_block_digest (csrc/recover_terms.hpp), the one builder
// of the 52-byte block, under the pad's word.
//   find_host_test pad <file>
// file: one line per pad, "<64 hex key bytes> <index, decimal>"; prints the pad as 16 hex digits per line.
//   find_host_test seal <file>
// file: one line per amount, "<64 hex key bytes> <index> <amount, decimal>"; prints "<sealed> <sealed twice>" as decimals.
//   find_host_test compact <max_hits> <file>
// file: one line of '0' and '1', the hit flags by position.  Runs the three compaction kernels' loops with a ballot built
// lane by lane: the tile counts, their exclusive scan, the emission into a list of EXACTLY min(hits, max_hits) entries (a
// write beyond it is an overflow the sanitizer sees).  Prints "<tiles> <hits>" and then the emitted positions, one per line.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "../../bulletproofsplus_amd/csrc/find_terms.hpp"
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

static uint64_t round_ballot(const std::string& flags, size_t tile, uint32_t round) {
    uint64_t ballot = 0;
    for (uint32_t lane = 0; lane < FIND_BLOCK; lane++) {
        const size_t i = find_position(tile, round, lane);
        if (i < flags.size() && flags[i] == '1') ballot |= (uint64_t)1 << lane;
    }
    return ballot;
}

static int compact(size_t max_hits, const std::string& flags) {
    const size_t pairs = flags.size(), tiles = find_tiles(pairs);
    std::vector<uint32_t> tile_count(tiles);
    for (size_t t = 0; t < tiles; t++) {   // k_find_count
        uint32_t n = 0;
        for (uint32_t r = 0; r < FIND_ROUNDS; r++) n += find_ballot_count(round_ballot(flags, t, r));
        tile_count[t] = n;
    }
    uint32_t hits = 0;
    for (size_t t = 0; t < tiles; t++) {   // k_find_offsets
        const uint32_t c = tile_count[t];
        tile_count[t] = hits;
        hits += c;
    }
    std::vector<size_t> out(hits < max_hits ? hits : max_hits);
    size_t written = 0;
    for (size_t t = 0; t < tiles; t++) {   // k_find_emit
        size_t before = tile_count[t];
        for (uint32_t r = 0; r < FIND_ROUNDS; r++) {
            const uint64_t ballot = round_ballot(flags, t, r);
            for (uint32_t lane = 0; lane < FIND_BLOCK; lane++) {
                if (!(ballot >> lane & 1)) continue;
                const size_t h = before + find_lane_rank(ballot, lane);
                if (h >= max_hits) continue;
                out.at(h) = find_position(t, r, lane);
                written++;
            }
            before += find_ballot_count(ballot);
        }
    }
    if (written != out.size()) return 1;
    printf("%zu %u\n", tiles, hits);
    for (size_t pos : out) printf("%zu\n", pos);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    std::ifstream f(argv[argc - 1]);
    if (!f) return 2;
    std::string line;
    if (mode == "compact") {
        if (argc != 4 || !std::getline(f, line)) return 2;
        return compact((size_t)strtoull(argv[2], nullptr, 10), line);
    }
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string tok;
        unsigned long long idx, amount = 0;
        uint32_t key[8];
        if (!(in >> tok >> idx) || !key_words(tok, key)) return 2;
        if (mode == "pad") {
            printf("%016llx\n", (unsigned long long)amount_pad(key, idx));
        } else if (mode == "seal") {
            if (!(in >> amount)) return 2;
            const uint64_t sealed = amount ^ amount_pad(key, idx);
            printf("%llu %llu\n", (unsigned long long)sealed, (unsigned long long)(sealed ^ amount_pad(key, idx)));
        } else {
            return 2;
        }
    }
    return 0;
}
