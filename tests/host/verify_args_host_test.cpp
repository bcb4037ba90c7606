// Host build of csrc/verify_args.hpp (tests/test_verify_args_cpu.py): every verifier entry's record through verify_args
// over the whole matrix of defects, one row `entry <tab> defect <tab> outcome` each.  outcome: "run" (the entry goes on to
// the implementation), "0" (the entry answers the empty batch), "<code> <text>"; for an entry with a stats argument
// " | stats zeroed" or " | stats kept" behind it.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../bulletproofsplus_amd/csrc/verify_args.hpp"

using namespace bpp;

// one call as its C entry would fill the record: which pointers the caller gave, and the scalars
struct Call {
    std::vector<std::string> null;   // pointer arguments left null, by name
    size_t count = 3;
    int flags = 0;
    uint32_t group = 4;
    bool weight = true;
    VerifierFacts facts{true, BPP_BLS12_381_G1, 8, 2};
};

// the entry's pointer arguments in the C ABI's order (the handle aside), as the record's fields
struct Shape {
    const char* name;
    const VerifyEntry* e;
    std::vector<const char*> pointers;
    bool has_flags, has_group, has_weights, has_stats;
};

static uint64_t u64[4];
static uint32_t u32[4];
static uint8_t u8[4];

static std::string outcome(const Shape& s, const Call& c) {
    auto given = [&](const char* name) {
        for (const char* p : s.pointers)
            if (!std::strcmp(p, name)) {
                for (const std::string& n : c.null)
                    if (n == name) return false;
                return true;
            }
        return false;
    };
    auto is_null = [&](const char* name) {
        for (const std::string& n : c.null)
            if (n == name) return true;
        return false;
    };
    uint64_t stats[2] = {7, 7};
    VerifyArgs a;
    if (given("points")) a.points = u64;
    if (given("scalars")) a.scalars = u64;
    if (given("proofs") || given("records")) a.proofs = u8;
    if (given("commitments")) a.commitments = u8;
    if (given("m_of")) a.m_of = u32;
    if (given("ok")) a.ok = u32;
    if (given("out_partial")) a.out_partial = u32;
    if (given("out_challenges")) a.out_challenges = u64;
    a.count = c.count;
    a.group = c.group;
    if (c.weight && (s.has_weights || (s.e->needs & NEED_KEY))) a.weight_key = u8;
    if (s.has_stats) a.stats = stats;
    // the workspace argument as capi.hip passes it: the graph capture's out pointer rides on it
    const void* ws = (s.e->needs & NEED_WS) && !is_null("ws") && !is_null("out") ? u8 : nullptr;
    VerifierFacts f = c.facts;
    f.engine = !is_null("v");
    fail(BPP_OK, "stale text");
    const int rc = verify_args(*s.e, f, c.flags, a, ws);
    std::string out = rc == BPP_OK ? "run" : rc == VERIFY_ANSWERED ? "0" : std::to_string(rc) + " " + last_error();
    if (s.has_stats) out += stats[0] == 0 && stats[1] == 0 ? " | stats zeroed" : " | stats kept";
    return out;
}

int main() {
    const std::vector<const char*> wire{"points", "scalars", "ok", "ws"}, bytes{"proofs", "commitments", "ok", "ws"},
        wire_mixed{"points", "scalars", "m_of", "ok", "ws"}, bytes_mixed{"proofs", "commitments", "m_of", "ok", "ws"};
    const std::vector<Shape> shapes{
        {"bpp_verifier_run", &VERIFY_RUN, wire, false, false, false, false},
        {"bpp_verifier_graph_capture", &VERIFY_GRAPH, {"points", "scalars", "ok", "ws", "out"}, false, false, false, false},
        {"bpp_verifier_run_combined", &VERIFY_COMBINED, {"points", "scalars", "out_partial", "ok", "ws"}, false, false, true, false},
        {"bpp_verifier_run_grouped", &VERIFY_GROUPED, wire, false, true, true, true},
        {"bpp_verifier_grouped_begin", &VERIFY_GROUPED, wire, false, true, true, false},
        {"bpp_verifier_grouped_finish", &VERIFY_GROUPED_FINISH, wire, false, true, false, true},
        {"bpp_verifier_derive_challenges", &VERIFY_DERIVE, {"points", "out_challenges"}, false, false, false, false},
        {"bpp_verifier_run_mixed", &VERIFY_MIXED, wire_mixed, false, false, false, false},
        {"bpp_verifier_derive_challenges_mixed", &VERIFY_DERIVE_MIXED, {"points", "m_of", "out_challenges", "ws"}, false, false, false, false},
        {"bpp_range_verify_batch_serialized_device", &VERIFY_SER, bytes, true, false, false, false},
        {"bpp_range_verify_batch_serialized_grouped_device", &VERIFY_SER_GROUPED, bytes, true, true, false, true},
        {"bpp_range_verify_batch_serialized_mixed_device", &VERIFY_SER_MIXED, bytes_mixed, true, false, false, false},
        {"bpp_verifier_run_grouped_mixed", &VERIFY_GROUPED_MIXED, wire_mixed, false, true, true, true},
        {"bpp_range_verify_batch_serialized_grouped_mixed_device", &VERIFY_SER_GROUPED_MIXED, bytes_mixed, true, true, false, true},
        {"bpp_range_verify_batch", &VERIFY_HOST, {"points", "scalars", "ok"}, false, false, false, false},
        {"bpp_range_verify_batch_mixed", &VERIFY_HOST_MIXED, {"points", "scalars", "m_of", "ok"}, false, false, false, false},
        {"bpp_range_verify_batch_compressed", &VERIFY_HOST_COMPRESSED, {"records", "scalars", "ok"}, false, false, false, false},
        {"bpp_range_verify_batch_serialized", &VERIFY_HOST_SER, {"proofs", "commitments", "ok"}, true, false, false, false},
        {"bpp_range_verify_batch_serialized_mixed", &VERIFY_HOST_SER_MIXED, {"proofs", "commitments", "m_of", "ok"}, true, false, false, false},
    };
    const size_t B = 0x7fffffffu / 64;
    const std::string over = "count:" + std::to_string(B + 1);
    for (const Shape& s : shapes) {
        const bool weight = s.has_weights || (s.e->needs & NEED_KEY);
        auto row = [&](const std::string& defect, const Call& c) {
            std::printf("%s\t%s\t%s\n", s.name, defect.c_str(), outcome(s, c).c_str());
        };
        auto with = [](auto&& edit) {
            Call c;
            edit(c);
            return c;
        };
        row("valid", Call{});
        row("null:v", with([](Call& c) { c.null = {"v"}; }));
        for (const char* p : s.pointers) row(std::string("null:") + p, with([&](Call& c) { c.null = {p}; }));
        for (size_t count : {(size_t)0, (size_t)1, B, B + 1, (size_t)1 << 32})
            row("count:" + std::to_string(count), with([&](Call& c) { c.count = count; }));
        const std::string first = s.pointers[0];
        if (s.has_flags) {
            row("flag:0x4", with([](Call& c) { c.flags = 4; }));
            row("flag:0x100", with([](Call& c) { c.flags = 0x100; }));
            row("ed25519:v2", with([](Call& c) { c.facts.curve = BPP_ED25519, c.flags = BPP_SER_UNCOMPRESSED; }));
            row("null:" + first + "+flag:0x4", with([&](Call& c) { c.null = {first}, c.flags = 4; }));
            row("flag:0x4+count:0", with([](Call& c) { c.flags = 4, c.count = 0; }));
        }
        if (s.has_group)
            for (uint32_t g = 0; g <= 4; g++) row("group:" + std::to_string(g), with([&](Call& c) { c.group = g; }));
        if (weight) {
            row("noweight", with([](Call& c) { c.weight = false; }));
            row(over + "+noweight", with([&](Call& c) { c.weight = false, c.count = B + 1; }));
        }
        row("n:256", with([](Call& c) { c.facts.n = 256; }));
        row("m:256", with([](Call& c) { c.facts.m = 256; }));
        row("null:" + first + "+count:0", with([&](Call& c) { c.null = {first}, c.count = 0; }));
    }
    return 0;
}
