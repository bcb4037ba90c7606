// verify_args.hpp -- the verifier entries' argument record (VerifyArgs), what tells the 19 entries' checks apart
// (VerifyEntry) and the one check in front of them all (verify_args).  HIP-free and fed the verifier's facts as plain
// data, so that a host build (tests/host/verify_args_host_test.cpp) walks every entry's answers under the sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

#include "abi_guard.hpp"
#include "container_scan.hpp"

namespace bpp {

// One call of the verifier, fields in the C ABI's order.  Device pointers at the device entries and inside VerifyImpl, host
// pointers at the host forms; m_of, weight_key and stats are host memory everywhere.
struct VerifyArgs {
    // the batch, as wire records (NV points per proof, the commitments behind the proof's own) and scalar triples ...
    const uint64_t *points = nullptr, *scalars = nullptr;
    // ... or as bytes: count containers of container_bytes(k, version) and m encoded commitments per proof (compressed form:
    // `proofs` holds the NV compressed points per proof, `scalars` the triples)
    const uint8_t *proofs = nullptr, *commitments = nullptr;
    // null: every proof has the verifier's (n, m).  Else proof i has shape (n, m_of[i]), m_of[i] a power of two <= m; records,
    // containers, commitments and challenges are then PACKED back to back in caller order (mixed.hpp)
    const uint32_t* m_of = nullptr;
    // the bytes entries' ragged form (outs_plan.hpp), in place of m_of: proof i covers outs_of[i] outputs, has the shape
    // (n, 2^ceil(log2 outs_of[i])) and outs_of[i] encoded commitments in the stream; the others are the identity
    const uint32_t* outs_of = nullptr;
    size_t count = 0;
    const uint64_t* challenges = nullptr;   // null (the shape's literals, or the transcript's when fs), or 3 + k_i scalars per proof
    bool fs = false;                        // BPP_SER_TRANSCRIPT: the challenges come from the transcript of each proof
    uint32_t version = 1;                   // of the containers: 2 with BPP_SER_UNCOMPRESSED
    // the weighted checks: proof i of the CALLER's order gets PRF(weight_key, index_base + i), or weights[i] (device, 128 bits
    // each) when given; a serialized entry with a weight source runs the grouped check behind its decoder
    const uint8_t* weight_key = nullptr;
    uint64_t index_base = 0;
    const uint64_t* weights = nullptr;
    uint32_t group = 0;                     // proofs per weighted check: a power of two, at least 2
    // count words in caller order: 0 Ok / 1 VerificationError / 2 FormatError (bytes only); the combined check: one word
    uint32_t* ok = nullptr;
    uint64_t *out_scalars = nullptr, *out_result = nullptr;   // optional: the MulVec scalars and its result point per proof
    uint64_t* out_challenges = nullptr;     // derive_challenges[_mixed]: 3 + k_i scalars per proof, the layout `challenges` takes
    uint32_t* out_partial = nullptr;        // the combined check: one jacobian (3N words, opaque) = the batch's weighted sum
    uint64_t* stats = nullptr;              // optional: [groups that failed their weighted check, proofs re-verified exactly]
};

// what verify_args is told of the engine
struct VerifierFacts {
    bool engine = false;   // the handle is not null
    int curve = 0;
    size_t n = 0, m = 0;
};

constexpr size_t ONE_LAUNCH = 0x7fffffffu / 64;   // proofs one launch takes: 64 lanes each, a 31-bit grid
inline bool group_ok(uint32_t group) { return group >= 2 && !(group & (group - 1)); }
// the mixed size getters' own refusal (they answer 0)
inline bool mixed_sizes_ok(const uint32_t* m_of, size_t count) { return (m_of || !count) && count <= ONE_LAUNCH; }
// every container entry point's version check; pb: the bytes of one point in the version asked for, 0 when there is none
inline int container_version_ok(size_t pb) {
    return pb ? BPP_OK : fail(BPP_E_ARG, "container version 2 (uncompressed points) is not offered for this curve");
}

// the pointers an entry refuses to find null (the handle always; NEED_WS: the workspace)
enum : unsigned {
    NEED_IN0 = 1, NEED_IN1 = 2,   // points or proofs; scalars or commitments
    NEED_M_OF = 4, NEED_OK = 8, NEED_WS = 16, NEED_PARTIAL = 32, NEED_OUT_CHALLENGES = 64, NEED_KEY = 128,
    INPUTS_IF_COUNT = 256         // ... the two inputs only when count > 0
};
enum VerifyEmpty { EMPTY_FIRST, EMPTY_OK, EMPTY_RUNS, EMPTY_REFUSED };
enum VerifyShapeCheck { SHAPE_NONE, SHAPE_COMPRESSED, SHAPE_PROOF_BYTES, SHAPE_VERSION };

// What tells the verifier entries' checks apart; the checks, their order and every shared text are verify_args.  The group,
// n, m <= 255 at the device entries, the m_of values and the workspace size are refused behind the entry (VerifyImpl).
struct VerifyEntry {
    unsigned needs;
    VerifyEmpty empty;                      // count == 0: answered ahead of the buffers; behind them and the weight source; passed on; an error
    const char* launch_text;                // count > ONE_LAUNCH is refused with this; null: 2^32 and more, as "count too large"
    int flags = 0;                          // the flags it takes
    const char* weight = nullptr;           // what a call with neither weight_key nor weights is told; null: not looked at
    bool zero_stats = false;                // stats, when given, is zeroed here (behind the flags)
    VerifyShapeCheck shape = SHAPE_NONE;    // the host forms' engine and container-version check, by wording
    bool flags_last = false;                // the flags it does not take are named behind every other check (the device entry
                                            // inside the host form names them)
    const char* empty_text = nullptr;       // EMPTY_REFUSED: its text
};
constexpr unsigned NEED_WIRE = NEED_IN0 | NEED_IN1 | NEED_OK, NEED_DEVICE = NEED_WIRE | NEED_WS;
constexpr int SER_FLAGS = BPP_SER_TRANSCRIPT | BPP_SER_UNCOMPRESSED;
constexpr const char *ONE_LAUNCH_TEXT = "count too large for one launch", *OUT_OF_RANGE = "count out of range",
                     *NEEDS_WEIGHT_GROUPED = "the grouped check needs a weight key or a weight buffer",
                     *NEEDS_WEIGHT_COMBINED = "the combined check needs a weight key or a weight buffer";
// the device entries: bpp_verifier_run, _graph_capture, _run_combined, _run_grouped and _grouped_begin, _grouped_finish,
// _derive_challenges, _run_mixed, _derive_challenges_mixed, bpp_range_verify_batch_serialized_device, .._grouped_device,
// .._mixed_device, bpp_verifier_run_grouped_mixed, bpp_range_verify_batch_serialized_grouped_mixed_device
inline constexpr VerifyEntry
    VERIFY_RUN{NEED_DEVICE, EMPTY_OK, ONE_LAUNCH_TEXT},
    VERIFY_GRAPH{NEED_DEVICE, EMPTY_REFUSED, OUT_OF_RANGE, 0, nullptr, false, SHAPE_NONE, false, OUT_OF_RANGE},
    VERIFY_COMBINED{NEED_DEVICE | NEED_PARTIAL, EMPTY_REFUSED, nullptr, 0, NEEDS_WEIGHT_COMBINED, false, SHAPE_NONE, false, "empty batch"},
    VERIFY_GROUPED{NEED_DEVICE | INPUTS_IF_COUNT, EMPTY_RUNS, nullptr, 0, NEEDS_WEIGHT_GROUPED},
    VERIFY_GROUPED_FINISH{NEED_DEVICE | INPUTS_IF_COUNT, EMPTY_RUNS, nullptr},
    VERIFY_DERIVE{NEED_IN0 | NEED_OUT_CHALLENGES, EMPTY_OK, nullptr},
    VERIFY_MIXED{NEED_DEVICE | NEED_M_OF, EMPTY_FIRST, ONE_LAUNCH_TEXT},
    VERIFY_DERIVE_MIXED{NEED_IN0 | NEED_M_OF | NEED_OUT_CHALLENGES | NEED_WS, EMPTY_FIRST, ONE_LAUNCH_TEXT},
    VERIFY_SER{NEED_DEVICE, EMPTY_OK, ONE_LAUNCH_TEXT, SER_FLAGS},
    VERIFY_SER_GROUPED{NEED_DEVICE | NEED_KEY, EMPTY_OK, ONE_LAUNCH_TEXT, SER_FLAGS, nullptr, true},
    VERIFY_SER_MIXED{NEED_DEVICE | NEED_M_OF, EMPTY_FIRST, ONE_LAUNCH_TEXT, SER_FLAGS},
    VERIFY_GROUPED_MIXED{NEED_DEVICE | NEED_M_OF, EMPTY_FIRST, ONE_LAUNCH_TEXT, 0, NEEDS_WEIGHT_GROUPED, true},
    VERIFY_SER_GROUPED_MIXED{NEED_DEVICE | NEED_M_OF | NEED_KEY, EMPTY_FIRST, ONE_LAUNCH_TEXT, SER_FLAGS, nullptr, true},
    // the host forms: bpp_range_verify_batch, _mixed, _compressed, _serialized, _serialized_mixed
    VERIFY_HOST{NEED_WIRE, EMPTY_OK, nullptr},
    VERIFY_HOST_MIXED{NEED_WIRE | NEED_M_OF, EMPTY_FIRST, nullptr},
    VERIFY_HOST_COMPRESSED{NEED_WIRE, EMPTY_OK, nullptr, 0, nullptr, false, SHAPE_COMPRESSED},
    VERIFY_HOST_SER{NEED_WIRE, EMPTY_OK, nullptr, SER_FLAGS, nullptr, false, SHAPE_PROOF_BYTES, true},
    VERIFY_HOST_SER_MIXED{NEED_WIRE | NEED_M_OF, EMPTY_FIRST, nullptr, SER_FLAGS, nullptr, false, SHAPE_VERSION};

// verify_args' third answer beside BPP_OK (go on) and an error: the entry has answered an empty batch, return BPP_OK
constexpr int VERIFY_ANSWERED = 1;

// The checks of the 19 verifier entries, in the one order that holds for all of them.  a holds the entry's pointers and
// leaves with what the flags say (the ONE decoding of BPP_SER_*); workspace: the device entries' (graph capture: null also
// when its out pointer is).
inline int verify_args(const VerifyEntry& e, const VerifierFacts& v, int flags, VerifyArgs& a, const void* workspace) noexcept {
    const unsigned need = (e.needs & INPUTS_IF_COUNT) && !a.count ? e.needs & ~(NEED_IN0 | NEED_IN1) : e.needs;
    const bool buffers = (!(need & NEED_IN0) || a.points || a.proofs) && (!(need & NEED_IN1) || a.scalars || a.commitments) &&
                         (!(need & NEED_M_OF) || a.m_of || a.outs_of) &&
                         (!(need & NEED_OK) || a.ok) && (!(need & NEED_WS) || workspace) &&
                         (!(need & NEED_PARTIAL) || a.out_partial) && (!(need & NEED_OUT_CHALLENGES) || a.out_challenges) &&
                         (!(need & NEED_KEY) || a.weight_key);
    if (!v.engine || (e.empty != EMPTY_FIRST && !buffers)) return fail(BPP_E_ARG, "null argument");
    const bool unknown = (flags & ~e.flags) != 0;
    if (unknown && !e.flags_last) return fail(BPP_E_ARG, "unknown flag");
    a.fs = (flags & BPP_SER_TRANSCRIPT) != 0;
    a.version = (flags & BPP_SER_UNCOMPRESSED) ? 2u : 1u;
    if (e.zero_stats && a.stats) a.stats[0] = a.stats[1] = 0;
    if (e.empty == EMPTY_FIRST) {
        if (a.count == 0) return VERIFY_ANSWERED;
        if (!buffers) return fail(BPP_E_ARG, "null argument");
    }
    if (e.weight && !a.weight_key && !a.weights) return fail(BPP_E_ARG, e.weight);
    if (a.count == 0 && e.empty == EMPTY_OK) return VERIFY_ANSWERED;
    if (a.count == 0 && e.empty == EMPTY_REFUSED) return fail(BPP_E_ARG, e.empty_text);
    const size_t pb = scan_point_bytes(v.curve, (int)a.version), mn = v.n * v.m;
    if (e.shape == SHAPE_COMPRESSED && scan_point_bytes(v.curve, 1) == 0)
        return fail(BPP_E_ARG, "compressed encoding is not offered for this curve");
    if (e.shape == SHAPE_PROOF_BYTES && (pb == 0 || mn == 0 || (mn & (mn - 1)) || v.n > 255 || v.m > 255))
        return fail(BPP_E_ARG, "n*m must be a power of two (n, m <= 255)");
    if (e.shape == SHAPE_VERSION)
        if (int rc = container_version_ok(pb)) return rc;
    if (e.launch_text ? a.count > ONE_LAUNCH : (a.count >> 32) != 0) return fail(BPP_E_ARG, e.launch_text ? e.launch_text : "count too large");
    if (unknown) return fail(BPP_E_ARG, "unknown flag");
    return BPP_OK;
}

}  // namespace bpp
