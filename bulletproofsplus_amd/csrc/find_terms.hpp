// find_terms.hpp -- the arithmetic of the fused verify-and-find call (find.hpp) that is not the curve's: the pad that
// seals an output's amount, and the index arithmetic of the hit list's compaction.  Plain C++ beside recover_terms.hpp, so
// the host tests (tests/host/find_host_test.cpp, tests/host/view_tag_host_test.cpp) compile the very code k_amounts_seal,
// the confirmation kernels, the compaction kernels and the tag kernels of find.hpp run.
//
// A sealed amount is amount XOR pad(key, idx): an output carries ONE 8-byte ciphertext of its amount and every view key
// tries its own pad on it.  The pad is domain-separated from every blinding slot by its tag ("bppa" against blind_half's
// "bppb"), so it is no function of any scalar that enters a proof.  Sealing and opening are the same operation.
//
// A view tag is ONE byte of the same block under a third tag ("bppt"): the sender attaches view_tag(key, idx) to the output,
// and the tagged call (find.hpp) computes it first -- one compression per (key, output) pair -- and expands slots and
// walks tables only where it matches: 255 of 256 foreign pairs stop there.  The tag hides nothing that a one-byte PRF
// output does not, and it authenticates nothing: a wrong tag hides an output from its owner's scan exactly as a wrong sealed
// amount does.  Also here: how the tag test's lanes and the candidate list are numbered.
#pragma once
#include "recover_terms.hpp"

namespace bpp {

// the first 8 bytes, as a little-endian u64, of SHA-256(key || "bppa" || idx as u64 LE || 0 as u32 || 0 as u32): blind_half's
// 52-byte block (key_block_digest) under the other tag, in registers alone
BPP_HD uint64_t amount_pad(const uint32_t* key, uint64_t idx) {
    uint32_t dg[8];
    key_block_digest(key, 0x62707061u, idx, 0, 0, dg);   // "bppa", as the block's big-endian word
    return (uint64_t)bswap32(dg[0]) | (uint64_t)bswap32(dg[1]) << 32;
}

// the first byte of SHA-256(key || "bppt" || idx as u64 LE || 0 as u32 || 0 as u32): the same block under the third tag, in
// registers alone
BPP_HD uint8_t view_tag(const uint32_t* key, uint64_t idx) {
    uint32_t dg[8];
    key_block_digest(key, 0x62707074u, idx, 0, 0, dg);   // "bppt", as the block's big-endian word
    return (uint8_t)(dg[0] >> 24);
}

// ---- the compaction of the hit flags into the ordered hit list --------------------------------------------------------
// The flags of a call lie key-major, pair (j, i) at j * count + i: ascending position IS ascending (key number, caller
// position).  A tile is FIND_TILE consecutive positions, read by one 64-lane block in FIND_ROUNDS rounds of 64; lane l of
// round r holds position find_position(tile, r, l).  The hits of a round are its ballot; a hit's place in the list is the
// hits of all tiles before (an exclusive scan of the tile counts), of the rounds before in its tile, and of the lanes below
// in its round (find_lane_rank).  Nothing in that depends on which block runs first.
constexpr uint32_t FIND_BLOCK = 64;
constexpr uint32_t FIND_ROUNDS = 4;
constexpr uint32_t FIND_TILE = FIND_BLOCK * FIND_ROUNDS;
constexpr uint32_t FIND_HIT_WORDS = 12;   // [key number, caller position, amount lo, amount hi, Gamma: 8 canonical words]

BPP_HD size_t find_tiles(size_t pairs) { return (pairs + FIND_TILE - 1) / FIND_TILE; }
BPP_HD size_t find_position(size_t tile, uint32_t round, uint32_t lane) {
    return tile * FIND_TILE + (size_t)round * FIND_BLOCK + lane;
}
BPP_HD uint32_t find_ballot_count(uint64_t ballot) { return (uint32_t)__builtin_popcountll(ballot); }
// hits of the round on the lanes below `lane`
BPP_HD uint32_t find_lane_rank(uint64_t ballot, uint32_t lane) {
    return find_ballot_count(ballot & (((uint64_t)1 << lane) - 1));
}


// ---- the tag test's lanes and the candidate list ------------------------------------------------------------------------
// The pairs of the tag test lie key-major over the LAUNCH positions of the single-output class, pair (j, p) at
// j * count + p, and each key's row is cut into tiles of FIND_TILE positions of its own (the last one short), so a tile
// never straddles two keys: its key is uniform over the block that reads it.  Tile t belongs to key t / per_key and starts
// at launch position (t % per_key) * FIND_TILE; lane l of round r holds launch position tag_launch_position(t, per_key, r, l),
// a pair when that is below count.  What a tile leaves in memory is its FIND_ROUNDS ballots (one BIT per pair) and its
// count; a candidate's place in the list is find's: the counts of the tiles before, the ballots of the rounds before, the
// lanes below.  Tiles ascend with (key, position), so the list is in ascending key-major pair number tag_pair(j, p, count).
BPP_HD size_t tag_tiles_per_key(size_t count) { return find_tiles(count); }
BPP_HD size_t tag_tiles(size_t n_keys, size_t count) { return n_keys * tag_tiles_per_key(count); }
BPP_HD size_t tag_tile_key(size_t tile, size_t per_key) { return tile / per_key; }
BPP_HD size_t tag_launch_position(size_t tile, size_t per_key, uint32_t round, uint32_t lane) {
    return find_position(tile % per_key, round, lane);
}
BPP_HD size_t tag_pair(size_t key_no, size_t position, size_t count) { return key_no * count + position; }

}  // namespace bpp
