// Host build of csrc/scan_args.hpp (tests/test_scan_args_cpu.py): every receiver entry's record through scan_args or
// find_args over the whole matrix of defects, one row `entry <tab> defect <tab> outcome` each.  outcome: "run" (the entry
// goes on to the implementation), "0" (the entry answers the empty call), "<code> <text>".
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../bulletproofsplus_amd/csrc/scan_args.hpp"

using namespace bpp;

enum Kind { RECOVER, ONE_KEY, MANY_KEYS, FIND };

// the entry's required pointer arguments by name (the handle aside), and what the entry is
struct Shape {
    const char* name;
    Kind kind;
    bool device;
    FindMode mode;   // FIND
    bool ragged;     // FIND: outs_of in m_of's place
    std::vector<const char*> pointers;
};

// one call as its C entry would fill the record
struct Call {
    std::vector<std::string> null;   // pointer arguments left null, by name
    size_t count = 3, n_keys = 2, max_hits = 4, ws_bytes = 64;
    std::vector<uint32_t> units{1, 2, 4};   // m_of, or outs_of; read when count is 3
    int flags = BPP_SER_TRANSCRIPT;
    bool blind_key = true, blinding = false, index = false, misaligned = false;
};

static uint64_t u64[4];
static uint32_t u32[4];
alignas(4) static uint8_t u8[8];
static std::vector<uint32_t> ones;   // an m_of of PAIR_BOUND ones, for the counts above 3

static std::string outcome(const Shape& s, const Call& c) {
    auto given = [&](const char* name) {
        for (const std::string& n : c.null)
            if (n == name) return false;
        return true;
    };
    const uint32_t* units = !given("m_of") || !given("outs_of") ? nullptr : c.count == c.units.size() ? c.units.data() : ones.data();
    const uint8_t* keys = given("keys") ? u8 + (c.misaligned ? 1 : 0) : nullptr;
    const void* ws = s.device && given("ws") ? u8 : nullptr;
    const size_t ws_bytes = s.device ? c.ws_bytes : 0;
    fail(BPP_OK, "stale text");
    int rc;
    if (s.kind == FIND) {
        FindArgs a{given("proofs") ? u8 : nullptr, given("commitments") ? u8 : nullptr, s.ragged ? nullptr : units, c.count, keys,
                   c.n_keys, 0, nullptr, given("amounts") ? u64 : nullptr, given("ok") ? u32 : nullptr, given("hits") ? u32 : nullptr,
                   c.max_hits, given("n_hits") ? u32 : nullptr, s.mode, given("tags") ? u8 : nullptr, nullptr};
        if (s.ragged) a.outs_of = units;
        rc = find_args(given("v"), c.flags, a, s.device, ws, ws_bytes);
    } else {
        ScanArgs a;
        if (s.kind == RECOVER) a.scalars = given("scalars") ? u64 : nullptr;
        if (s.kind != RECOVER) a.proofs = given("proofs") ? u8 : nullptr, a.commitments = given("commitments") ? u8 : nullptr;
        a.m_of = units;
        a.count = c.count;
        if (s.kind != MANY_KEYS) {
            a.blind_key = c.blind_key ? u8 : nullptr;
            a.index = c.index ? u64 : nullptr;
            a.blinding = c.blinding ? u64 : nullptr;
        } else {
            a.keys = keys;
            a.n_keys = c.n_keys;
        }
        a.out_masks = given("out_masks") ? u64 : nullptr;
        if (s.kind != RECOVER) a.out_status = given("status") ? u32 : nullptr;
        const ScanEntry& e = s.kind == RECOVER    ? (s.device ? SCAN_RECOVER_DEVICE : SCAN_RECOVER_HOST)
                             : s.kind == ONE_KEY ? (s.device ? SCAN_ONE_KEY_DEVICE : SCAN_ONE_KEY_HOST)
                                                 : (s.device ? SCAN_MANY_KEYS_DEVICE : SCAN_MANY_KEYS_HOST);
        rc = scan_args(e, given("v"), s.kind == RECOVER ? 0 : c.flags, a, ws, ws_bytes);
    }
    return rc == BPP_OK ? "run" : rc == SCAN_ANSWERED ? "0" : std::to_string(rc) + " " + last_error();
}

int main() {
    const size_t B = PAIR_BOUND;
    ones.assign(B, 1u);
    std::vector<Shape> shapes;
    for (int device = 1; device >= 0; device--) {
        auto add = [&](const char* dev_name, const char* host_name, Kind kind, FindMode mode, bool ragged, std::vector<const char*> pointers) {
            if (device) pointers.push_back("ws");
            shapes.push_back({device ? dev_name : host_name, kind, device != 0, mode, ragged, pointers});
        };
        add("bpp_range_recover_masks_mixed_device", "bpp_range_recover_masks_mixed", RECOVER, FIND_REWIND, false,
            {"scalars", "m_of", "out_masks"});
        add("bpp_range_scan_serialized_mixed_device", "bpp_range_scan_serialized_mixed", ONE_KEY, FIND_REWIND, false,
            {"proofs", "commitments", "m_of", "out_masks", "status"});
        add("bpp_range_scan_serialized_mixed_keys_device", "bpp_range_scan_serialized_mixed_keys", MANY_KEYS, FIND_REWIND, false,
            {"proofs", "commitments", "m_of", "keys", "out_masks", "status"});
        add("bpp_range_verify_find_serialized_mixed_keys_device", "bpp_range_verify_find_serialized_mixed_keys", FIND, FIND_REWIND,
            false, {"proofs", "commitments", "m_of", "keys", "amounts", "ok", "hits", "n_hits"});
        add("bpp_range_verify_find_tagged_serialized_mixed_keys_device", "bpp_range_verify_find_tagged_serialized_mixed_keys", FIND,
            FIND_REWIND_TAGGED, false, {"proofs", "commitments", "m_of", "keys", "amounts", "ok", "hits", "n_hits", "tags"});
        add("bpp_range_verify_find_outputs_serialized_mixed_keys_device", "bpp_range_verify_find_outputs_serialized_mixed_keys", FIND,
            FIND_PER_OUTPUT, false, {"proofs", "commitments", "m_of", "keys", "amounts", "tags", "ok", "hits", "n_hits"});
        add("bpp_range_verify_find_outputs_serialized_outs_keys_device", "bpp_range_verify_find_outputs_serialized_outs_keys", FIND,
            FIND_PER_OUTPUT, true, {"proofs", "commitments", "outs_of", "keys", "amounts", "tags", "ok", "hits", "n_hits"});
    }
    for (const Shape& s : shapes) {
        auto row = [&](const std::string& defect, const Call& c) {
            std::printf("%s\t%s\t%s\n", s.name, defect.c_str(), outcome(s, c).c_str());
        };
        auto with = [](auto&& edit) {
            Call c;
            edit(c);
            return c;
        };
        const bool has_flags = s.kind != RECOVER, one_key = s.kind == RECOVER || s.kind == ONE_KEY, per_output = s.mode == FIND_PER_OUTPUT;
        const std::string first = s.pointers[0], units_of = s.ragged ? "outs_of" : "m_of";
        row("valid", Call{});
        row("null:v", with([](Call& c) { c.null = {"v"}; }));
        for (const char* p : s.pointers) row(std::string("null:") + p, with([&](Call& c) { c.null = {p}; }));
        row("null:" + first + "+count:0", with([&](Call& c) { c.null = {first}, c.count = 0; }));
        for (size_t count : {(size_t)0, (size_t)1, B, B + 1, (size_t)1 << 32})
            row("count:" + std::to_string(count), with([&](Call& c) { c.count = count; }));
        if (has_flags)
            for (int bit : {0x4, 0x200, 0x400}) {
                char name[32];
                std::snprintf(name, sizeof name, "flag:0x%x", bit);
                row(name, with([&](Call& c) { c.flags |= bit; }));
                row(std::string(name) + "+count:0", with([&](Call& c) { c.flags |= bit, c.count = 0; }));
                row("null:" + first + "+" + name, with([&](Call& c) { c.null = {first}, c.flags |= bit; }));
            }
        for (const std::vector<uint32_t>& u : std::vector<std::vector<uint32_t>>{{1, 3, 2}, {0, 1, 1}, {2, 4, 12}, {1, 0, 2}, {1, 129, 2}}) {
            if (!s.ragged && u[1] != 3 && u[0] != 0 && u[2] != 12) continue;   // the last two are the ragged block's alone
            row(units_of + ":" + std::to_string(u[0]) + "," + std::to_string(u[1]) + "," + std::to_string(u[2]),
                with([&](Call& c) { c.units = u; }));
        }
        if (s.device) {
            row("ws:0", with([](Call& c) { c.ws_bytes = 0; }));
            row(units_of + ":1,3,2+ws:0", with([](Call& c) { c.units = {1, 3, 2}, c.ws_bytes = 0; }));
        }
        if (one_key) {
            row("both", with([](Call& c) { c.blinding = true; }));
            row("index:nokey", with([](Call& c) { c.blind_key = false, c.blinding = true, c.index = true; }));
            row("nosource", with([](Call& c) { c.blind_key = false; }));
            row("both+count:" + std::to_string(B + 1), with([&](Call& c) { c.blinding = true, c.count = B + 1; }));
        }
        if (s.kind == ONE_KEY) {
            row("nofs", with([](Call& c) { c.flags = 0; }));
            row("nofs+nosource", with([](Call& c) { c.flags = 0, c.blind_key = false; }));
            row("nofs+blinding", with([](Call& c) { c.flags = 0, c.blind_key = false, c.blinding = true; }));
            row("nofs+m_of:1,3,2", with([](Call& c) { c.flags = 0, c.units = {1, 3, 2}; }));
            row("nofs+count:" + std::to_string(B + 1), with([&](Call& c) { c.flags = 0, c.count = B + 1; }));
        }
        if (s.kind == MANY_KEYS || s.kind == FIND) {
            const size_t units = per_output ? 7 : 3;   // of the valid block: its outputs, or its proofs
            row("n_keys:0", with([](Call& c) { c.n_keys = 0; }));
            row("null:keys+n_keys:0", with([](Call& c) { c.null = {"keys"}, c.n_keys = 0; }));
            row("null:" + first + "+n_keys:0", with([&](Call& c) { c.null = {first}, c.n_keys = 0; }));
            row("pairs:at", with([&](Call& c) { c.n_keys = B / units; }));
            row("pairs:over", with([&](Call& c) { c.n_keys = B / units + 1; }));
            row("pairs:1x" + std::to_string(B), with([&](Call& c) { c.n_keys = 1, c.count = B; }));
            row("pairs:1x" + std::to_string(B + 1), with([&](Call& c) { c.n_keys = 1, c.count = B + 1; }));
            row("pairs:" + std::to_string(B) + "x1", with([&](Call& c) { c.n_keys = B, c.count = 1; }));
            row("pairs:" + std::to_string(B + 1) + "x1", with([&](Call& c) { c.n_keys = B + 1, c.count = 1; }));
            row("pairs:wrap", with([](Call& c) { c.n_keys = (size_t)1 << 62, c.count = 4; }));   // 2^62 keys x 4 units = 2^64
            row("nofs", with([](Call& c) { c.flags = 0; }));
            row("nofs+pairs:over", with([&](Call& c) { c.flags = 0, c.n_keys = B / units + 1; }));
            row("nofs+" + units_of + ":1,3,2", with([](Call& c) { c.flags = 0, c.units = {1, 3, 2}; }));
            row("keys:misaligned", with([](Call& c) { c.misaligned = true; }));
            row("keys:misaligned+n_keys:0", with([](Call& c) { c.misaligned = true, c.n_keys = 0; }));
        }
        if (s.kind == FIND) {
            row("null:n_hits+count:0", with([](Call& c) { c.null = {"n_hits"}, c.count = 0; }));
            row("null:n_hits+flag:0x4", with([](Call& c) { c.null = {"n_hits"}, c.flags |= 4; }));
            row("null:hits+max_hits:0", with([](Call& c) { c.null = {"hits"}, c.max_hits = 0; }));
            row("flag:0x204", with([](Call& c) { c.flags |= 0x204; }));
            row("flag:0x204+count:0", with([](Call& c) { c.flags |= 0x204, c.count = 0; }));
        }
    }
    return 0;
}
