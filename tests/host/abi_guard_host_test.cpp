// Host build of csrc/abi_guard.hpp (tests/test_abi_guard_cpu.py): every kind of exception becomes its return code with
// its text in g_err, a normal return passes through unchanged, and a count of 2^32 or more is rejected before the body.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../bulletproofsplus_amd/csrc/abi_guard.hpp"

static int failures = 0;

static void expect(int got, int want, const char* text, const char* what) {
    if (got != want || std::strcmp(last_error(), text) != 0 || last_error() != g_err.c_str()) {
        std::printf("FAIL %s: code %d (want %d), text \"%s\" (want \"%s\")\n", what, got, want, last_error(), text);
        failures++;
    }
}

int main() {
    // a body that returns passes its code through and leaves the last error alone
    fail(BPP_E_ARG, "earlier");
    expect(guarded([] { return BPP_OK; }), BPP_OK, "earlier", "ok");
    expect(guarded([] { return BPP_VERIFICATION_ERROR; }), BPP_VERIFICATION_ERROR, "earlier", "verification error");
    expect(guarded([] { return fail(BPP_E_POINT, "point"); }), BPP_E_POINT, "point", "fail inside");
    expect(guarded([] { return fail(BPP_E_HIP, std::string("expr: ") + "detail"); }), BPP_E_HIP, "expr: detail", "string");
    expect(fail(BPP_E_HIP, "expr: ", "detail"), BPP_E_HIP, "expr: detail", "two parts");

    // exceptions
    expect(guarded([]() -> int { throw std::bad_alloc(); }), BPP_E_NOMEM, "host allocation failed", "bad_alloc");
    expect(guarded([]() -> int {
               std::vector<uint64_t> v;
               v.reserve(v.max_size() + 1);   // std::length_error
               return BPP_OK;
           }),
           BPP_E_NOMEM, "host allocation failed", "length_error");
    expect(guarded([]() -> int { throw std::bad_array_new_length(); }), BPP_E_NOMEM, "host allocation failed",
           "bad_array_new_length");
    expect(guarded([]() -> int { throw std::runtime_error("boom"); }), BPP_E_HIP, "unexpected C++ exception: boom",
           "runtime_error");
    expect(guarded([]() -> int { throw std::out_of_range("index"); }), BPP_E_HIP, "unexpected C++ exception: index",
           "out_of_range");
    expect(guarded([]() -> int { throw 42; }), BPP_E_HIP, "unexpected C++ exception", "int");

    // the count bound: checked before the body runs
    bool ran = false;
    auto body = [&] {
        ran = true;
        return BPP_OK;
    };
    expect(guarded(Count{0xffffffffull, "count"}, body), BPP_OK, "unexpected C++ exception", "count 2^32 - 1");
    if (!ran) std::printf("FAIL count 2^32 - 1: body did not run\n"), failures++;
    ran = false;
    expect(guarded(Count{1ull << 32, "count"}, body), BPP_E_ARG, "count too large", "count 2^32");
    expect(guarded(Count{1ull << 62, "length"}, body), BPP_E_ARG, "length too large", "length 2^62");
    expect(guarded(Count{~(size_t)0, "n"}, body), BPP_E_ARG, "n too large", "n 2^64 - 1");
    if (ran) std::printf("FAIL a count of 2^32 or more ran the body\n"), failures++;
    expect(guarded(Count{8, "count"}, []() -> int { throw std::bad_alloc(); }), BPP_E_NOMEM, "host allocation failed",
           "bad_alloc under a count");

    if (failures) return 1;
    std::printf("ok abi_guard\n");
    return 0;
}
