// outs_plan.hpp -- proofs over ANY number of outputs (bpp_*_outs*): the ragged arithmetic of a block whose proof i covers
// outs_of[i] outputs, 1 <= outs_of[i] <= the engine's m.  Such a proof IS the proof of shape (n, M), M = 2^ceil(log2 outs),
// over its values and masks padded with zeros; its commitments outs .. M - 1 are the identity and travel nowhere: the value,
// mask and commitment streams hold sum(outs) entries, the containers are those of shape (n, M), byte for byte.
// Here: the class of a count, the ragged offsets into the three streams, each proof's first caller output number, the class
// lane ranges of the decode kernels, the byte totals within the 32-bit index.  HIP-free, so that a host build
// (tests/host/outs_plan_host_test.cpp) checks it under the sanitizers; mixed.hpp puts it into the per-proof index.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "abi_guard.hpp"

namespace bpp {

constexpr int OUTS_CLASSES = 8;          // M = 1, 2, 4, .. 128 (mixed.hpp MIXED_CLASSES)
constexpr size_t OUTS_HDR = 12;          // bytes of a container's header (codec.hpp CONTAINER_HDR)
constexpr uint32_t OUTS_WAVE = 64;       // lanes of a decode wave (mixed.hpp SER_WAVE)
// The index word of a ragged block (mixed.hpp SX_OUTS): outs - 1 in the 7 bits above the proof's first caller output number,
// which the output finder alone fills in (its pair bound keeps sum(outs) below 2^25).
constexpr uint32_t OUTS_SHIFT = 25, OUTS_FIRST_MASK = (1u << OUTS_SHIFT) - 1;
constexpr uint32_t outs_word(uint32_t outs, uint32_t first) { return (outs - 1) << OUTS_SHIFT | (first & OUTS_FIRST_MASK); }
constexpr uint32_t outs_word_count(uint32_t w) { return (w >> OUTS_SHIFT) + 1; }
constexpr uint32_t outs_word_first(uint32_t w) { return w & OUTS_FIRST_MASK; }

// the class of a count: the least c with 2^c >= outs (outs >= 1)
constexpr uint32_t outs_class(uint32_t outs) {
    uint32_t c = 0;
    while (((uint32_t)1 << c) < outs) c++;
    return c;
}

// The rule as a function: m_of_out[i] = 2^outs_class(outs_of[i]).  BPP_E_ARG naming i for a count of zero or above cap_m.
inline int outs_shapes(const uint32_t* outs_of, size_t count, size_t cap_m, uint32_t* m_of_out) {
    for (size_t i = 0; i < count; i++) {
        const uint32_t o = outs_of[i];
        if (o == 0 || o > cap_m)
            return fail(BPP_E_ARG, "outs_of[" + std::to_string(i) + "] = " + std::to_string(o) + ": not in [1, " +
                                       std::to_string(cap_m) + "]");
        if (m_of_out) m_of_out[i] = (uint32_t)1 << outs_class(o);
    }
    return BPP_OK;
}

// One proof of a ragged block, in caller order.
struct OutsProof {
    uint32_t c;          // its class
    uint32_t first;      // its first caller output number = its first value and mask = its first commitment (in points)
    size_t comm_byte;    // byte offset of its first commitment
    size_t proof_byte;   // byte offset of its container
    uint32_t pos;        // its gathered position: behind the classes below its own, in caller order within the class
};

struct OutsPlan {
    std::vector<uint32_t> m_of;      // 2^c per proof
    std::vector<OutsProof> proof;
    size_t count[OUTS_CLASSES] = {};       // proofs of the class
    size_t first[OUTS_CLASSES] = {};       // its first gathered position
    size_t lanes[OUTS_CLASSES] = {};       // record points of the class: its proofs x (3 + 2 (logn + c) + 2^c)
    size_t lane_end[OUTS_CLASSES] = {};    // end of its lane range, each range padded to whole waves (cumulative)
    size_t n_out = 0, proof_bytes = 0, comm_bytes = 0;   // sum(outs); the bytes of the two packed streams
};

// n, m: the engine's shape (n m a power of two, m <= 128); pb: the bytes of an encoded point.  BPP_E_ARG naming the proof
// for a count the engine does not take, or whose container or commitments end beyond 4 GiB.
inline int outs_plan(size_t n, size_t m, const uint32_t* outs_of, size_t count, size_t pb, OutsPlan& p) {
    p = OutsPlan{};
    p.m_of.resize(count);
    if (int rc = outs_shapes(outs_of, count, m, p.m_of.data())) return rc;
    uint32_t logn = 0;
    while (((size_t)1 << logn) < n) logn++;
    auto npp = [&](uint32_t c) -> size_t { return 3 + 2 * (size_t)(logn + c); };
    auto cbytes = [&](uint32_t c) -> size_t { return OUTS_HDR + npp(c) * pb + 96; };
    p.proof.resize(count);
    for (size_t i = 0; i < count; i++) {
        OutsProof& e = p.proof[i];
        e.c = outs_class(outs_of[i]);
        e.first = (uint32_t)p.n_out;
        e.comm_byte = p.comm_bytes;
        e.proof_byte = p.proof_bytes;
        e.pos = (uint32_t)p.count[e.c]++;   // within the class; the class's first position is added below
        p.n_out += outs_of[i];
        p.comm_bytes += (size_t)outs_of[i] * pb;
        p.proof_bytes += cbytes(e.c);
        if ((p.proof_bytes | p.comm_bytes) >> 32)
            return fail(BPP_E_ARG, "batch too large: the bytes of outs_of[" + std::to_string(i) + "] lie beyond the 32-bit index");
    }
    size_t lanes = 0;
    for (uint32_t c = 0; c < OUTS_CLASSES; c++) {
        p.first[c] = c ? p.first[c - 1] + p.count[c - 1] : 0;
        p.lanes[c] = p.count[c] * (npp(c) + ((size_t)1 << c));
        lanes += (p.lanes[c] + OUTS_WAVE - 1) / OUTS_WAVE * OUTS_WAVE;
        p.lane_end[c] = lanes;
    }
    for (size_t i = 0; i < count; i++) p.proof[i].pos += (uint32_t)p.first[p.proof[i].c];
    return BPP_OK;
}

// The first proof whose values, commitments or container do not lie inside buffers of these sizes (entries, bytes, bytes),
// or `count` when every proof does: what a caller that frames the streams checks before it hands them over.
inline size_t outs_first_overflow(const OutsPlan& p, const uint32_t* outs_of, size_t pb, size_t n_values, size_t comm_bytes,
                                  size_t proof_bytes) {
    const size_t count = p.proof.size();
    for (size_t i = 0; i < count; i++) {
        const OutsProof& e = p.proof[i];
        const size_t proof_end = i + 1 < count ? p.proof[i + 1].proof_byte : p.proof_bytes;
        if ((size_t)e.first + outs_of[i] > n_values || e.comm_byte + (size_t)outs_of[i] * pb > comm_bytes || proof_end > proof_bytes)
            return i;
    }
    return count;
}

}  // namespace bpp
