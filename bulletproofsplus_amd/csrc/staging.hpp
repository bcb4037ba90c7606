// staging.hpp -- the one way a host form moves caller buffers: DevBuf, and HIPCHK for the calls around it.
//
// The staging rule.  A host form (`*_host`) is its device entry between copies.  Every input is DevBuf::upload: a null
// host pointer gives a null device pointer (the device entry sees "absent", as its own caller would say it), a non-null
// one gives a buffer holding the bytes -- valid and non-null even at 0 bytes.  Every output is DevBuf::alloc, absent
// ones left empty; the device entry runs; every output is DevBuf::download.  The copies are blocking hipMemcpy: the host
// side is pageable memory, so nothing is gained by the asynchronous form, and a download on the null stream waits for
// the entry's launches.  A buffer that holds a secret (view keys) sets `wipe` and is zeroed before it is freed, on every
// way out.  Nothing is written to a caller's output before the device entry has succeeded.
//
// Included after the HIP runtime (host_util.hpp) -- or after a stand-in for the few names it uses: hipMalloc, hipFree,
// hipMemcpy with its two directions, hipMemset, hipError_t, hipSuccess, hipGetErrorString
// (tests/host/staging_host_test.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "abi_guard.hpp"

// ---- error handling (g_err, fail: abi_guard.hpp) -------------------------------------------------------
#define HIPCHK(expr)                                                                            \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) return fail(BPP_E_HIP, #expr ": ", hipGetErrorString(e_));        \
    } while (0)

// the same for what already returns a code: a device entry, another host form
#define BPP_TRY(expr)                     \
    do {                                  \
        if (int rc_ = (expr)) return rc_; \
    } while (0)

namespace bpp {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    bool wipe = false;   // zero the bytes before they are freed
    DevBuf() = default;
    explicit DevBuf(bool wipe_before_free) : wipe(wipe_before_free) {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) {
            if (wipe) (void)hipMemset(p, 0, bytes);
            (void)hipFree(p);
        }
        p = nullptr;
        bytes = 0;
    }
    hipError_t alloc(size_t n) {   // (re)allocates: a buffer held from an earlier call is freed first
        release();
        bytes = n;
        return hipMalloc(&p, n ? n : 16);
    }
    // null src: empty, p null; otherwise a buffer of n bytes (valid at n = 0) holding src's.  Like alloc they return the
    // HIP code: the call site wraps them in HIPCHK, so the error text names the buffer and the size
    hipError_t upload(const void* src, size_t n) {
        release();
        if (!src) return hipSuccess;
        const hipError_t e = alloc(n);
        return e != hipSuccess || !n ? e : hipMemcpy(p, src, n, hipMemcpyHostToDevice);
    }
    hipError_t download(void* dst, size_t n) const { return n ? hipMemcpy(dst, p, n, hipMemcpyDeviceToHost) : hipSuccess; }
    template <class T>
    T* as() const {
        return static_cast<T*>(p);
    }
    uint32_t* u32() const { return as<uint32_t>(); }
    uint64_t* u64() const { return as<uint64_t>(); }
    uint8_t* u8() const { return as<uint8_t>(); }
};

}  // namespace bpp
