// scan_args.hpp -- the receiver entries' argument records (ScanArgs: mask recovery and the scans; FindArgs: verify-and-find),
// what tells the six recovery and scan entries' checks apart (ScanEntry) and the two checks in front of the fourteen
// (scan_args, find_args).  HIP-free, so that a host build (tests/host/scan_args_host_test.cpp) walks every entry's answers
// under the sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

#include "abi_guard.hpp"

namespace bpp {

// One call of mask recovery or of a scan, fields in the C ABI's order.  Device pointers at the device entries and inside
// RecoverImpl and RecoverKeysImpl, host pointers at the host forms; m_of and blind_key are host memory everywhere.
struct ScanArgs {
    const uint64_t* scalars = nullptr;                         // recovery from wire data: count x [r', s', delta']
    const uint8_t *proofs = nullptr, *commitments = nullptr;   // the scans: run_serialized_mixed's streams
    const uint32_t* m_of = nullptr;
    size_t count = 0;
    const uint64_t* challenges = nullptr;   // recovery: the packed 3 + k_i blocks, or null: the literals of each proof's shape
    // the blinding source of the one-key calls: the key the proofs were made under (32 bytes) and each proof's index
    // (index[i], or index_base + i), or the packed 5 + 2 k_i blinding scalars per proof
    const uint8_t* blind_key = nullptr;
    uint64_t index_base = 0;
    const uint64_t* index = nullptr;
    const uint64_t* blinding = nullptr;
    const uint8_t* keys = nullptr;          // the many-key scan: n_keys x 32 bytes (device: 4-byte aligned)
    size_t n_keys = 0;
    const uint64_t* amounts = nullptr;      // candidate amounts by caller position (many keys: n_keys x count), or null
    uint64_t* out_masks = nullptr;          // count (many keys: n_keys x count) x 4 words of Gamma
    uint32_t* out_status = nullptr;         // the scans: as many status words
    // what the call's flags say
    bool fs = false;                        // BPP_SER_TRANSCRIPT
    uint32_t version = 1;                   // of the containers: 2 with BPP_SER_UNCOMPRESSED
    bool amount64 = false;                  // BPP_PROVE_AMOUNT64
};

// how a call finds a key's outputs
enum FindMode : uint32_t {
    FIND_REWIND,          // single-output proofs are rewound under every key
    FIND_REWIND_TAGGED,   // the same, for the pairs whose view tag matches
    FIND_PER_OUTPUT,      // every output of every proof, by its derived mask (outputs.hpp)
};

// What a find call takes, in the C ABI's order but for the mode.  For a device entry the pointers are the device's (keys
// 4-byte aligned), for find_host the host's.  n_keys = 0: the block is verified all the same (keys, amounts, tags unread),
// no hit.  Per output, amounts and tags go by caller OUTPUT number (sum of m_i of them) and amounts are always sealed.
struct FindArgs {
    const uint8_t *proofs, *commitments;
    const uint32_t* m_of;   // host, always
    size_t count;
    const uint8_t* keys;   // n_keys x 32 bytes
    size_t n_keys;
    uint64_t index_base;
    const uint64_t* index;     // count x u64 or null
    const uint64_t* amounts;   // one u64 per unit (sealed) or n_keys x count
    uint32_t* ok;              // count words
    uint32_t* hits;            // max_hits x FIND_HIT_WORDS words
    size_t max_hits;
    uint32_t* n_hits;          // one word
    FindMode mode;
    const uint8_t* tags;       // one byte per unit; unread when rewinding untagged
    uint32_t* n_candidates;    // one word or null; likewise
    uint32_t version = 1;      // what the call's flags say
    bool amount64 = false, sealed = false;
    // per output alone, in place of m_of: the ragged block (outs_plan.hpp) -- amounts and tags by REAL output number, the
    // sum of outs_of[i] of them
    const uint32_t* outs_of = nullptr;
    bool tagged() const { return mode != FIND_REWIND; }
};

// ---- what the receiver's calls can answer before the engine handle is read ----
// the first position whose m_i no engine takes (zero, or not a power of two; one above the engine's m is the plan's to
// name), or count where there is none
inline size_t first_bad_m(const uint32_t* m_of, size_t count) noexcept {
    size_t i = 0;
    while (i < count && m_of[i] != 0 && !(m_of[i] & (m_of[i] - 1))) i++;
    return i;
}
inline bool m_of_wellformed(const uint32_t* m_of, size_t count) noexcept { return first_bad_m(m_of, count) == count; }
// the same as an answer that names the position; for a caller under the guard (the text is built on the heap)
inline int m_of_checked(const uint32_t* m_of, size_t count) {
    const size_t i = first_bad_m(m_of, count);
    if (i == count) return BPP_OK;
    return fail(BPP_E_ARG, "m_of[" + std::to_string(i) + "] = " + std::to_string(m_of[i]) + ": not a power of two");
}

constexpr size_t PAIR_BOUND = 0x7fffffffu / 64;   // proofs, and (key, unit) pairs, one launch takes (verify_args.hpp ONE_LAUNCH)
// n_keys x units within the bound the other entries put on count alone, without forming a product that can wrap
inline bool pairs_bounded(size_t n_keys, size_t units) noexcept {
    return n_keys <= PAIR_BOUND && units <= PAIR_BOUND && (n_keys == 0 || units <= PAIR_BOUND / n_keys);
}
// What each key of a call is paired with: the proofs of the block, or (per_output) their outputs, the sum of units_of
// (m_of, or the ragged block's outs_of).  No sum that can wrap: the array is read only once count itself is within the
// bound, and no further than the sum is.
inline size_t pair_units(const uint32_t* units_of, size_t count, bool per_output) noexcept {
    if (!per_output || count > PAIR_BOUND) return count;
    size_t n_out = 0;
    for (size_t i = 0; i < count && n_out <= PAIR_BOUND; i++) n_out += units_of[i];   // each below 2^32
    return n_out;
}
// the two answers that name what a call pairs its keys with
struct PairTexts {
    const char *too_large, *transcript;
};
constexpr PairTexts PROOF_PAIRS = {"n_keys x count too large for one launch", "blinding needs BPP_SER_TRANSCRIPT"};
constexpr PairTexts OUTPUT_PAIRS = {"n_keys x n_out too large for one launch", "the verdicts need BPP_SER_TRANSCRIPT"};

// a ragged block's count no engine takes (zero, or above the largest class): the size getters answer 0 before the handle is
// read; outs_of is read only once count itself is within one launch
constexpr uint32_t OUTS_LARGEST = 1u << 7;   // outs_plan.hpp: 1 << (OUTS_CLASSES - 1)
inline bool outs_wellformed(const uint32_t* outs_of, size_t count) noexcept {
    if ((count && !outs_of) || count > PAIR_BOUND) return false;
    for (size_t i = 0; i < count; i++)
        if (outs_of[i] == 0 || outs_of[i] > OUTS_LARGEST) return false;
    return true;
}

// ---- the flags ----
constexpr int SCAN_FLAGS = BPP_SER_TRANSCRIPT | BPP_SER_UNCOMPRESSED | BPP_PROVE_AMOUNT64;
constexpr int FIND_FLAGS = SCAN_FLAGS | BPP_FIND_AMOUNTS_SEALED;
struct ScanFlags {
    bool fs, amount64, sealed;
    uint32_t version;
};
// The ONE decoding of a receiver entry's flags, behind the refusal of those it does not take.  sealed_refused: what an
// entry that takes no BPP_FIND_AMOUNTS_SEALED says of it, ahead of the flags nobody takes; null: it says "unknown flag".
inline int scan_flags(int flags, int taken, const char* sealed_refused, ScanFlags& f) noexcept {
    if (sealed_refused && (flags & BPP_FIND_AMOUNTS_SEALED)) return fail(BPP_E_ARG, sealed_refused);
    if (flags & ~taken) return fail(BPP_E_ARG, "unknown flag");
    f.fs = (flags & BPP_SER_TRANSCRIPT) != 0;
    f.amount64 = (flags & BPP_PROVE_AMOUNT64) != 0;
    f.sealed = (flags & BPP_FIND_AMOUNTS_SEALED) != 0;
    f.version = (flags & BPP_SER_UNCOMPRESSED) ? 2u : 1u;
    return BPP_OK;
}

// the checks' third answer beside BPP_OK (go on) and an error: an empty call.  scan_args: return BPP_OK; find_args: no
// proof, so no verdict, no candidate, no hit -- the caller zeroes the counts where they live and returns BPP_OK
constexpr int SCAN_ANSWERED = 1;

inline bool misaligned4(const void* p) noexcept { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }

// What tells the six recovery and scan entries' checks apart; the checks, their order and every text are scan_args.
struct ScanEntry {
    bool wire;     // recovery from wire data: scalars in, masks out, no flags argument and no status
    bool keys;     // the many-key scan: keys in place of the blinding source, n_keys x count pairs
    bool device;   // the device entry: a workspace, aligned keys
};
// bpp_range_recover_masks_mixed_device and its host form, bpp_range_scan_serialized_mixed_device and its host form,
// bpp_range_scan_serialized_mixed_keys_device and its host form
inline constexpr ScanEntry SCAN_RECOVER_DEVICE{true, false, true}, SCAN_RECOVER_HOST{true, false, false},
    SCAN_ONE_KEY_DEVICE{false, false, true}, SCAN_ONE_KEY_HOST{false, false, false},
    SCAN_MANY_KEYS_DEVICE{false, true, true}, SCAN_MANY_KEYS_HOST{false, true, false};

// The checks of the six recovery and scan entries, in the one order that holds for all of them.  a holds the entry's
// pointers and leaves with what the flags say; engine: the handle is not null; workspace, workspace_bytes: the device
// entries'.  An m_i above the engine's, n or m above 255, the container version, log2(n m) and a workspace too small but not
// empty are refused behind the entry, where the engine is read.
inline int scan_args(const ScanEntry& e, bool engine, int flags, ScanArgs& a, const void* workspace, size_t workspace_bytes) noexcept {
    if (!engine) return fail(BPP_E_ARG, "null argument");
    ScanFlags f;
    if (int rc = scan_flags(flags, e.wire ? 0 : SCAN_FLAGS, nullptr, f)) return rc;
    a.fs = f.fs, a.version = f.version, a.amount64 = f.amount64;
    if (a.count == 0 || (e.keys && a.n_keys == 0)) return SCAN_ANSWERED;
    const bool inputs = e.wire ? a.scalars != nullptr : a.proofs && a.commitments && a.out_status;
    if (!inputs || !a.m_of || !a.out_masks || (e.keys && !a.keys) || (e.device && !workspace)) return fail(BPP_E_ARG, "null argument");
    if (e.keys && e.device && misaligned4(a.keys)) return fail(BPP_E_ARG, "d_keys must be 4-byte aligned");
    const int rc = guarded([&]() -> int {
        if (e.keys) {
            if (!pairs_bounded(a.n_keys, a.count)) return fail(BPP_E_ARG, PROOF_PAIRS.too_large);
        } else {
            if (a.blind_key && a.blinding) return fail(BPP_E_ARG, "blind_key and d_blinding are both given");
            if (a.index && !a.blind_key) return fail(BPP_E_ARG, "d_index is the index of a blind_key: it needs one");
            if (a.count > PAIR_BOUND) return fail(BPP_E_ARG, "count too large for one launch");
        }
        if (int rc1 = m_of_checked(a.m_of, a.count)) return rc1;
        // the many-key scan derives every challenge; the one-key scan whenever it expands a blinding source
        if (!e.wire && !a.fs && (e.keys || a.blind_key || a.blinding)) return fail(BPP_E_ARG, PROOF_PAIRS.transcript);
        return BPP_OK;
    });
    if (rc) return rc;
    if (e.device && workspace_bytes == 0) return fail(BPP_E_ARG, "workspace too small");
    return BPP_OK;
}

// The checks of the eight find entries -- rewinding, tagged, per output and per output over a ragged block, device and host
// each -- in the one order that holds for all of them.  What tells them apart is in the record (a.mode; a.outs_of in
// m_of's place) but for `device`: a workspace, aligned keys.  a holds the entry's pointers and leaves with what the flags
// say.  Without keys the block is verified all the same: the call IS a verification, and ok is never left unwritten.  The
// ragged form leaves the counts themselves to the plan, which refuses them by name.
inline int find_args(bool engine, int flags, FindArgs& a, bool device, const void* workspace, size_t workspace_bytes) noexcept {
    const bool per_output = a.mode == FIND_PER_OUTPUT;
    if (!engine || !a.n_hits) return fail(BPP_E_ARG, "null argument");
    ScanFlags f;
    if (int rc = scan_flags(flags, FIND_FLAGS, per_output ? "BPP_FIND_AMOUNTS_SEALED is not taken: amounts are always sealed here" : nullptr, f))
        return rc;
    a.version = f.version, a.amount64 = f.amount64, a.sealed = per_output || f.sealed;
    if (a.count == 0) return SCAN_ANSWERED;
    const uint32_t* units_of = a.outs_of ? a.outs_of : a.m_of;
    if (!a.proofs || !a.commitments || !units_of || !a.ok || (device && !workspace)) return fail(BPP_E_ARG, "null argument");
    if (a.n_keys && (!a.keys || !a.amounts || (a.tagged() && !a.tags) || (!a.hits && a.max_hits)))
        return fail(BPP_E_ARG, "null argument");
    if (device && a.n_keys && misaligned4(a.keys)) return fail(BPP_E_ARG, "d_keys must be 4-byte aligned");
    const int rc = guarded([&]() -> int {
        const PairTexts& text = per_output ? OUTPUT_PAIRS : PROOF_PAIRS;
        if (!pairs_bounded(a.n_keys, pair_units(units_of, a.count, per_output))) return fail(BPP_E_ARG, text.too_large);
        if (!a.outs_of)
            if (int rc1 = m_of_checked(a.m_of, a.count)) return rc1;
        if (!f.fs) return fail(BPP_E_ARG, text.transcript);
        return BPP_OK;
    });
    if (rc) return rc;
    if (device && workspace_bytes == 0) return fail(BPP_E_ARG, "workspace too small");
    return BPP_OK;
}

}  // namespace bpp
