// abi_guard.hpp -- the error state of the C ABI and the guard that keeps C++ exceptions from crossing it.  HIP-free, so
// that a host build (tests/host/abi_guard_host_test.cpp) checks it under the sanitizers.
#pragma once
#include <cstddef>
#include <new>
#include <stdexcept>
#include <string>

#include "../../include/bpp_amd.h"

// the text of the last failure of this thread: bpp_last_error()
inline thread_local std::string g_err;
inline thread_local bool g_err_lost = false;   // the last text could not be stored
inline const char* last_error() noexcept { return g_err_lost ? "out of host memory (error text lost)" : g_err.c_str(); }

// records msg + detail as the last error and returns code; never throws
inline int fail(int code, const char* msg, const char* detail = "") noexcept {
    try {
        g_err = msg;
        g_err += detail;
        g_err_lost = false;
    } catch (...) {
        g_err_lost = true;
    }
    return code;
}
inline int fail(int code, const std::string& msg) noexcept { return fail(code, msg.c_str()); }

// Runs an entry point's body; an exception becomes a return code: a failed host allocation BPP_E_NOMEM, anything else
// BPP_E_HIP with its what().
template <class F>
int guarded(F&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(BPP_E_NOMEM, "host allocation failed");
    } catch (const std::length_error&) {
        return fail(BPP_E_NOMEM, "host allocation failed");
    } catch (const std::exception& e) {
        return fail(BPP_E_HIP, "unexpected C++ exception: ", e.what());
    } catch (...) {
        return fail(BPP_E_HIP, "unexpected C++ exception");
    }
}

// A caller count that sizes work (proofs, points, scalars, generators), named in the error text.  Below 2^32 no size
// product in the library wraps: every per-item size is far below 2^32 bytes.
struct Count {
    size_t n;
    const char* what;
};
// guarded(body), rejecting a count of 2^32 or more before the body runs
template <class F>
int guarded(Count c, F&& body) noexcept {
    return guarded([&]() -> int { return c.n >> 32 ? fail(BPP_E_ARG, c.what, " too large") : body(); });
}
