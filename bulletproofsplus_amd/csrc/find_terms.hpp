// find_terms.hpp -- the arithmetic of the fused verify-and-find call (find.hpp) that is not the curve's: the pad that
// seals an output's amount, and the index arithmetic of the hit list's compaction.  Plain C++ beside recover_terms.hpp, so
// the host test (tests/host/find_host_test.cpp) compiles the very code k_amounts_seal, k_find_confirm and the compaction
// kernels run.
//
// A sealed amount is amount XOR pad(key, idx): an output carries ONE 8-byte ciphertext of its amount and every view key
// tries its own pad on it.  The pad is domain-separated from every blinding slot by its tag ("bppa" against blind_half's
// "bppb"), so it is no function of any scalar that enters a proof.  Sealing and opening are the same operation.
#pragma once
#include "recover_terms.hpp"

namespace bpp {

// the first 8 bytes, as a little-endian u64, of SHA-256(key || "bppa" || idx as u64 LE || 0 as u32 || 0 as u32): blind_half's
// 52-byte block under the other tag, in registers alone
BPP_HD uint64_t amount_pad(const uint32_t* key, uint64_t idx) {
    uint32_t w[16], dg[8];
#pragma unroll
    for (int t = 0; t < 8; t++) w[t] = bswap32(key[t]);
    w[8] = 0x62707061u;   // "bppa", as the block's big-endian word
    w[9] = bswap32((uint32_t)idx);
    w[10] = bswap32((uint32_t)(idx >> 32));
    w[11] = 0;
    w[12] = 0;
    w[13] = 0x80000000u;
    w[14] = 0;
    w[15] = 52 * 8;
    sha256_one_block(w, dg);
    return (uint64_t)bswap32(dg[0]) | (uint64_t)bswap32(dg[1]) << 32;
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

}  // namespace bpp
