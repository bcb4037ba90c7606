// Host build of csrc/outs_plan.hpp (tests/test_outs_abi_cpu.py; g++, under ASan + UBSan with BPP_HOST_SANITIZE=1): the
// ragged arithmetic of a block whose proofs cover any number of outputs, against a plain recomputation here -- every
// proof's value, commitment and container offsets, its first output number and gathered position, the class lane ranges --
// on the worked block OUTS and on 200 seeded random blocks per capacity; the spans touched in buffers of exactly the
// plan's sizes, so that an offset one past the end is a reported overflow; a byte total that crosses 2^32 named by proof.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../bulletproofsplus_amd/csrc/outs_plan.hpp"

using namespace bpp;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            failures++;                                                    \
        }                                                                  \
    } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

static uint32_t ceil_log2(uint32_t o) {
    uint32_t c = 0;
    while ((1u << c) < o) c++;
    return c;
}

// the plan of one block against the recomputation; n a power of two
static void check_block(size_t n, size_t cap, const std::vector<uint32_t>& outs, size_t pb) {
    OutsPlan p;
    CHECK(outs_plan(n, cap, outs.data(), outs.size(), pb, p) == BPP_OK);
    const size_t count = outs.size();
    uint32_t logn = 0;
    while (((size_t)1 << logn) < n) logn++;
    CHECK(p.proof.size() == count && p.m_of.size() == count);
    size_t val = 0, cm = 0, pr = 0;
    size_t per_class[OUTS_CLASSES] = {};
    for (size_t i = 0; i < count; i++) per_class[ceil_log2(outs[i])]++;
    size_t class_first[OUTS_CLASSES], seen[OUTS_CLASSES] = {};
    for (int c = 0, at = 0; c < OUTS_CLASSES; c++) {
        class_first[c] = (size_t)at;
        at += (int)per_class[c];
    }
    for (size_t i = 0; i < count; i++) {
        const uint32_t c = ceil_log2(outs[i]);
        const OutsProof& e = p.proof[i];
        CHECK(e.c == c && p.m_of[i] == 1u << c && p.m_of[i] >= outs[i] && (c == 0 || (p.m_of[i] >> 1) < outs[i]));
        CHECK(e.first == val);            // its first value, mask, commitment point = its first output number
        CHECK(e.comm_byte == cm && e.comm_byte == (size_t)e.first * pb);
        CHECK(e.proof_byte == pr);
        CHECK(e.pos == class_first[c] + seen[c]);
        seen[c]++;
        val += outs[i];
        cm += (size_t)outs[i] * pb;
        pr += OUTS_HDR + (3 + 2 * (size_t)(logn + c)) * pb + 96;
    }
    CHECK(p.n_out == val && p.comm_bytes == cm && p.proof_bytes == pr);
    size_t lanes = 0;
    for (uint32_t c = 0; c < OUTS_CLASSES; c++) {
        const size_t used = per_class[c] * (3 + 2 * (size_t)(logn + c) + ((size_t)1 << c));
        CHECK(p.count[c] == per_class[c] && p.first[c] == class_first[c] && p.lanes[c] == used);
        lanes += (used + 63) / 64 * 64;
        CHECK(p.lane_end[c] == lanes && p.lane_end[c] % 64 == 0);
    }
    // the index word carries the count beside any first output number the finder can have
    for (size_t i = 0; i < count; i++) {
        const uint32_t w = outs_word(outs[i], p.proof[i].first);
        CHECK(outs_word_count(w) == outs[i] && outs_word_first(w) == p.proof[i].first);
    }
    CHECK(outs_word_count(outs_word(128, OUTS_FIRST_MASK)) == 128 && outs_word_first(outs_word(128, OUTS_FIRST_MASK)) == OUTS_FIRST_MASK);
    // exact-size buffers: every span of every proof is touched at both ends (the sanitizer reports one byte too far)
    std::vector<uint64_t> values(p.n_out);
    std::vector<uint8_t> comm(p.comm_bytes), proofs(p.proof_bytes);
    for (size_t i = 0; i < count; i++) {
        const OutsProof& e = p.proof[i];
        uint64_t* v = values.data() + e.first;
        v[0] = 1;
        v[outs[i] - 1] = 2;
        uint8_t* q = comm.data() + e.comm_byte;
        q[0] = 1;
        q[(size_t)outs[i] * pb - 1] = 2;
        uint8_t* r = proofs.data() + e.proof_byte;
        r[0] = 1;
        r[OUTS_HDR + (3 + 2 * (size_t)(logn + e.c)) * pb + 96 - 1] = 2;
    }
    CHECK(outs_first_overflow(p, outs.data(), pb, p.n_out, p.comm_bytes, p.proof_bytes) == count);
    if (count) {
        // one entry or one byte short: the last proof no longer fits, and only it
        CHECK(outs_first_overflow(p, outs.data(), pb, p.n_out - 1, p.comm_bytes, p.proof_bytes) == count - 1);
        CHECK(outs_first_overflow(p, outs.data(), pb, p.n_out, p.comm_bytes - 1, p.proof_bytes) == count - 1);
        CHECK(outs_first_overflow(p, outs.data(), pb, p.n_out, p.comm_bytes, p.proof_bytes - 1) == count - 1);
        // room for the padded commitments would be a different stream: the first proof with padding shifts everything behind it
        CHECK(outs_first_overflow(p, outs.data(), pb, 0, p.comm_bytes, p.proof_bytes) == 0);
    }
}

int main() {
    // the rule
    {
        uint32_t outs[8] = {1, 2, 3, 4, 5, 6, 7, 8}, ms[8] = {};
        const uint32_t want[8] = {1, 2, 4, 4, 8, 8, 8, 8};
        CHECK(outs_shapes(outs, 8, 8, ms) == BPP_OK && !std::memcmp(ms, want, sizeof want));
        CHECK(outs_shapes(outs, 8, 8, nullptr) == BPP_OK);
        CHECK(outs_shapes(nullptr, 0, 8, nullptr) == BPP_OK);
        for (size_t at = 0; at < 8; at++)
            for (uint32_t bad : {0u, 9u, 0xffffffffu}) {
                uint32_t o[8];
                std::memcpy(o, outs, sizeof o);
                o[at] = bad;
                CHECK(outs_shapes(o, 8, 8, ms) == BPP_E_ARG);
                CHECK(std::string(last_error()).find("outs_of[" + std::to_string(at) + "]") != std::string::npos);
                OutsPlan p;
                CHECK(outs_plan(8, 8, o, 8, 48, p) == BPP_E_ARG);
                CHECK(std::string(last_error()).find("outs_of[" + std::to_string(at) + "]") != std::string::npos);
            }
        uint32_t five = 5;
        CHECK(outs_shapes(&five, 1, 4, ms) == BPP_E_ARG && outs_shapes(&five, 1, 5, ms) == BPP_OK && ms[0] == 8);
        for (uint32_t o = 1; o <= 128; o++) CHECK((1u << outs_class(o)) >= o && (o == 1 || (1u << (outs_class(o) - 1)) < o));
    }
    // the worked block: 14 proofs, 54 outputs; class 4 has six proofs of 17 record points, class 8 five of 23
    {
        const std::vector<uint32_t> OUTS = {3, 1, 8, 5, 2, 3, 7, 4, 6, 3, 3, 5, 1, 3};
        for (size_t pb : {(size_t)32, (size_t)33, (size_t)48, (size_t)65, (size_t)96}) check_block(8, 8, OUTS, pb);
        OutsPlan p;
        CHECK(outs_plan(8, 8, OUTS.data(), OUTS.size(), 48, p) == BPP_OK);
        CHECK(p.n_out == 54 && p.count[0] == 2 && p.count[1] == 1 && p.count[2] == 6 && p.count[3] == 5);
        CHECK(p.lanes[2] == 102 && p.lanes[3] == 115);
        CHECK(p.lane_end[0] == 64 && p.lane_end[1] == 128 && p.lane_end[2] == 256 && p.lane_end[3] == 384 && p.lane_end[7] == 384);
    }
    // seeded random blocks at three capacities
    for (size_t cap : {(size_t)1, (size_t)4, (size_t)16})
        for (int round = 0; round < 200; round++) {
            const size_t count = rnd() % 40;
            std::vector<uint32_t> outs(count);
            for (uint32_t& o : outs) o = 1 + rnd() % cap;
            const size_t pbs[5] = {32, 33, 48, 65, 96};
            check_block((size_t)1 << (rnd() % 7), cap, outs, pbs[rnd() % 5]);
        }
    check_block(64, 128, std::vector<uint32_t>{128, 127, 65, 64, 1}, 48);
    // byte totals beyond the 32-bit index: sizes only.  Huge points make a short block cross; the proof is the first whose
    // container or commitments END beyond 2^32
    {
        const size_t pb = (size_t)1 << 24, n = 8, cap = 16;
        std::vector<uint32_t> outs(64);
        for (size_t i = 0; i < outs.size(); i++) outs[i] = 1 + (uint32_t)(i * 7 % cap);
        size_t want = outs.size(), pr = 0, cm = 0;
        for (size_t i = 0; i < outs.size(); i++) {
            pr += OUTS_HDR + (3 + 2 * (size_t)(3 + ceil_log2(outs[i]))) * pb + 96;
            cm += (size_t)outs[i] * pb;
            if ((pr | cm) >> 32) {
                want = i;
                break;
            }
        }
        CHECK(want < outs.size() && want > 0);
        OutsPlan p;
        CHECK(outs_plan(n, cap, outs.data(), outs.size(), pb, p) == BPP_E_ARG);
        CHECK(std::string(last_error()).find("outs_of[" + std::to_string(want) + "]") != std::string::npos);
        CHECK(std::string(last_error()).find("32-bit index") != std::string::npos);
        CHECK(outs_plan(n, cap, outs.data(), want, pb, p) == BPP_OK && !((p.proof_bytes | p.comm_bytes) >> 32));
        // the commitments cross long before the containers do: 128 of them a proof beside 17 proof points
        std::vector<uint32_t> wide(400000, 128);
        CHECK(outs_plan(1, 128, wide.data(), wide.size(), 96, p) == BPP_E_ARG);
        size_t at = 0, c2 = 0, p2 = 0;
        for (; at < wide.size(); at++) {
            c2 += 128 * (size_t)96;
            p2 += OUTS_HDR + (3 + 2 * (size_t)7) * 96 + 96;
            if ((c2 | p2) >> 32) break;
        }
        CHECK(std::string(last_error()).find("outs_of[" + std::to_string(at) + "]") != std::string::npos);
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("outs_plan ok\n");
    return 0;
}
