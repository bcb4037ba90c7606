// Host-side harness for the view tag and the candidate list's index arithmetic of csrc/find_terms.hpp (compiled with g++,
// no GPU needed): the code k_view_tags, k_find_tags and k_find_list (csrc/find.hpp) run -- view_tag is key_block_digest
// (csrc/recover_terms.hpp), the one builder of the 52-byte block, under the tag's word.
//   view_tag_host_test tag <file>
// file: one line per tag, "<64 hex key bytes> <index, decimal>"; prints the tag as 2 hex digits per line.
//   view_tag_host_test list <n_keys> <count> <file>
// file: one line of '0' and '1', n_keys x count candidate flags, key-major over the launch positions.  Runs the loops of
// k_find_tags (ballots and tile counts, a ballot built lane by lane), k_find_offsets and k_find_list (the emission into a
// list of EXACTLY as many entries as there are candidates: a write beyond it is an overflow the sanitizer sees).  Prints
// "<tiles> <candidates>" and then the listed pair numbers, one per line.
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

static int list(size_t n_keys, size_t count, const std::string& flags) {
    if (flags.size() != n_keys * count) return 2;
    const size_t per_key = tag_tiles_per_key(count), tiles = tag_tiles(n_keys, count);
    std::vector<uint64_t> ballots(tiles * FIND_ROUNDS);
    std::vector<uint32_t> tile_count(tiles);
    for (size_t t = 0; t < tiles; t++) {   // k_find_tags
        const size_t key_no = tag_tile_key(t, per_key);
        if (key_no >= n_keys) return 1;
        uint32_t n = 0;
        for (uint32_t r = 0; r < FIND_ROUNDS; r++) {
            uint64_t ballot = 0;
            for (uint32_t lane = 0; lane < FIND_BLOCK; lane++) {
                const size_t p = tag_launch_position(t, per_key, r, lane);
                if (p < count && flags.at(tag_pair(key_no, p, count)) == '1') ballot |= (uint64_t)1 << lane;
            }
            ballots.at(t * FIND_ROUNDS + r) = ballot;
            n += find_ballot_count(ballot);
        }
        tile_count[t] = n;
    }
    uint32_t cands = 0;
    for (size_t t = 0; t < tiles; t++) {   // k_find_offsets
        const uint32_t c = tile_count[t];
        tile_count[t] = cands;
        cands += c;
    }
    std::vector<size_t> out(cands);
    size_t written = 0;
    for (size_t t = 0; t < tiles; t++) {   // k_find_list
        const size_t key_no = tag_tile_key(t, per_key);
        size_t before = tile_count[t];
        for (uint32_t r = 0; r < FIND_ROUNDS; r++) {
            const uint64_t ballot = ballots[t * FIND_ROUNDS + r];
            for (uint32_t lane = 0; lane < FIND_BLOCK; lane++) {
                if (!(ballot >> lane & 1)) continue;
                out.at(before + find_lane_rank(ballot, lane)) = tag_pair(key_no, tag_launch_position(t, per_key, r, lane), count);
                written++;
            }
            before += find_ballot_count(ballot);
        }
    }
    if (written != out.size()) return 1;
    printf("%zu %u\n", tiles, cands);
    for (size_t q : out) printf("%zu\n", q);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    std::ifstream f(argv[argc - 1]);
    if (!f) return 2;
    std::string line;
    if (mode == "list") {
        if (argc != 5) return 2;
        std::getline(f, line);   // an empty line: no pair
        return list((size_t)strtoull(argv[2], nullptr, 10), (size_t)strtoull(argv[3], nullptr, 10), line);
    }
    if (mode != "tag") return 2;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string tok;
        unsigned long long idx;
        uint32_t key[8];
        if (!(in >> tok >> idx) || !key_words(tok, key)) return 2;
        printf("%02x\n", (unsigned)view_tag(key, idx));
    }
    return 0;
}
