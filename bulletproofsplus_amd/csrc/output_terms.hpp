// output_terms.hpp -- the three functions of an output whose mask is DERIVED from its recipient's key (outputs.hpp), and the
// index arithmetic of the per-output tag test.  Plain C++ beside find_terms.hpp, so the host test
// (tests/host/output_terms_host_test.cpp) compiles the very code k_outputs_make, k_out_tags and k_out_confirm run.
//
// An aggregated proof gives its scanner ONE Gamma = sum z^(2j) gamma_j and its nonces come from one blinding key: rewinding
// cannot tell the outputs of one proof apart, and at most one party could rewind it.  So the sender derives output j's
// mask from the RECIPIENT's key and commits with it; the recipient derives it again and checks V_j == v g + gamma h.  With
//     B(tag, idx, a, b) = SHA-256(key || tag || idx as u64 LE || a as u32 LE || b as u32 LE)      (key_block_digest)
//     output_mask(key, idx, j) = (c0 + 2^256 c1) mod r, zero replaced by one, c_h = B("bppm", idx, j, h) little-endian
//     output_pad(key, idx, j)  = the first 8 bytes of B("bppa", idx, j, 0) as a little-endian u64
//     output_tag(key, idx, j)  = the first byte of B("bppt", idx, j, 0)
// idx is the blinding index of the output's PROOF, j the output's place in it.  For j = 0 the pad and the tag are byte for
// byte amount_pad and view_tag (find_terms.hpp): a single output sealed and tagged by the existing calls is an output here.
// The mask is blind_slot's construction under a tag of its own ("bppm" against "bppb"), the output number in the slot
// word: no mask is a blinding slot of any proof.
#pragma once
#include "find_terms.hpp"

namespace bpp {

BPP_HD uint64_t output_pad(const uint32_t* key, uint64_t idx, uint32_t j) {
    uint32_t dg[8];
    key_block_digest(key, 0x62707061u, idx, j, 0, dg);   // "bppa", as the block's big-endian word
    return (uint64_t)bswap32(dg[0]) | (uint64_t)bswap32(dg[1]) << 32;
}

BPP_HD uint8_t output_tag(const uint32_t* key, uint64_t idx, uint32_t j) {
    uint32_t dg[8];
    key_block_digest(key, 0x62707074u, idx, j, 0, dg);   // "bppt"
    return (uint8_t)(dg[0] >> 24);
}

// c_h of the mask: the digest under "bppm" as 8 little-endian words of a 256-bit integer
BPP_HD void output_mask_half(const uint32_t* key, uint64_t idx, uint32_t j, uint32_t h, uint32_t c[8]) {
    uint32_t dg[8];
    key_block_digest(key, 0x6270706du, idx, j, h, dg);   // "bppm"
#pragma unroll
    for (int t = 0; t < 8; t++) c[t] = bswap32(dg[t]);
}

// two compressions and the reduction, in registers alone (blind_slot's reason: nothing derived from a key goes to memory)
template <class P>
BPP_HD Fe<P> output_mask(const uint32_t* key, uint64_t idx, uint32_t j) {
    uint32_t c0[8], c1[8];
    output_mask_half(key, idx, j, 0, c0);
    output_mask_half(key, idx, j, 1, c1);
    uint32_t w128[8] = {0, 0, 0, 0, 1, 0, 0, 0};
    const Fe<P> f128 = fe_from_canonical<P>(w128);
    const Fe<P> f256 = fe_mul(f128, f128);
    Fe<P> x = fe_add(fe_from_canonical<P>(c0), fe_mul(fe_from_canonical<P>(c1), f256));
    if (x.is_zero()) x = Fe<P>::one();
    return x;
}

// ---- the lanes of the per-output tag test -------------------------------------------------------------------------------
// The outputs of one class (count_c proofs of m_c = 2^logm outputs each) lie proof after proof in launch order: launch
// OUTPUT position x is output x % m_c of the proof at launch position x / m_c.  The pairs lie key-major over those
// positions, pair (q, x) at q * outs + x with outs = count_c * m_c, and each key's row is cut into tiles exactly as the
// single-output tag test cuts its row of proofs (tag_tiles_per_key .. tag_pair, with outs for count): a tile never
// straddles two keys.
BPP_HD size_t output_class_outputs(size_t count_c, uint32_t logm) { return count_c << logm; }
BPP_HD size_t output_proof(size_t position, uint32_t logm) { return position >> logm; }
BPP_HD uint32_t output_place(size_t position, uint32_t logm) { return (uint32_t)(position & (((size_t)1 << logm) - 1)); }

}  // namespace bpp
