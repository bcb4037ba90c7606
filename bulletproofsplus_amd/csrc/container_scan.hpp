// container_scan.hpp -- framing of a bare byte stream of proof containers (bpp_proofs_scan): the lengths chain, so this
// is a serial walk of 12-byte headers on the host.  HIP-free and free of the library's other headers, so that a host
// build (tests/host/container_scan_host_test.cpp) runs it over untrusted bytes under the sanitizers.
// It validates only what it needs to find the next container (magic, version, curve, n, m, k, the length); the reserved
// bytes, the encodings and the scalars stay the decoder's business (codec.hpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace bpp {

constexpr size_t SCAN_HDR = 12;   // "BPP+" | version | curve | n | m | k | 3 reserved bytes (codec.hpp CONTAINER_HDR)

// bytes of a point in a container of `version` (1 compressed, 2 uncompressed); 0: no such form
inline size_t scan_point_bytes(int curve, int version) {
    if (version == 1) return curve == 0 ? 48 : (curve == 1 ? 33 : (curve == 2 ? 32 : 0));
    if (version == 2) return curve == 0 ? 96 : (curve == 1 ? 65 : 0);
    return 0;
}

enum ScanStatus {
    SCAN_OK = 0,
    SCAN_BAD_ARG,      // curve / version not offered, n not a power of two in [1, 255]
    SCAN_TRUNCATED,    // fewer bytes left than a header, or than the container the header announces
    SCAN_BAD_MAGIC,
    SCAN_BAD_VERSION,  // not the version asked for
    SCAN_BAD_CURVE,    // not the curve asked for
    SCAN_BAD_N,        // not the n asked for
    SCAN_BAD_M,        // zero or not a power of two
    SCAN_BAD_K,        // not log2(n m)
    SCAN_TOO_MANY      // more containers than max_count
};

struct ScanResult {
    ScanStatus status;
    size_t count;    // containers walked (on failure: those before the offending one, i.e. its index)
    size_t offset;   // bytes consumed (on failure: where the offending container starts)
};

inline const char* scan_status_text(ScanStatus s) {
    switch (s) {
        case SCAN_OK: return "ok";
        case SCAN_BAD_ARG: return "curve, version or n not offered";
        case SCAN_TRUNCATED: return "truncated";
        case SCAN_BAD_MAGIC: return "bad magic";
        case SCAN_BAD_VERSION: return "version other than asked for";
        case SCAN_BAD_CURVE: return "curve other than asked for";
        case SCAN_BAD_N: return "n other than asked for";
        case SCAN_BAD_M: return "m not a power of two";
        case SCAN_BAD_K: return "k is not log2(n m)";
        case SCAN_TOO_MANY: return "more containers than max_count";
    }
    return "?";
}

// Walks `bytes` bytes at p; m_of[i] (i < max_count) receives container i's m.  Never reads p[bytes] or beyond, never
// writes m_of[max_count] or beyond.
inline ScanResult container_scan(int curve, size_t n, int version, const uint8_t* p, size_t bytes, uint32_t* m_of,
                                 size_t max_count) {
    const size_t pb = scan_point_bytes(curve, version);
    if (pb == 0 || n == 0 || n > 255 || (n & (n - 1))) return {SCAN_BAD_ARG, 0, 0};
    uint32_t logn = 0;
    while (((size_t)1 << logn) < n) logn++;
    size_t off = 0, i = 0;
    while (off < bytes) {
        const size_t left = bytes - off;
        if (left < SCAN_HDR) return {SCAN_TRUNCATED, i, off};
        const uint8_t* h = p + off;
        if (h[0] != 'B' || h[1] != 'P' || h[2] != 'P' || h[3] != '+') return {SCAN_BAD_MAGIC, i, off};
        if (h[4] != (uint8_t)version) return {SCAN_BAD_VERSION, i, off};
        if (h[5] != (uint8_t)curve) return {SCAN_BAD_CURVE, i, off};
        if (h[6] != (uint8_t)n) return {SCAN_BAD_N, i, off};
        const uint32_t m = h[7];
        if (m == 0 || (m & (m - 1))) return {SCAN_BAD_M, i, off};
        uint32_t logm = 0;
        while ((1u << logm) < m) logm++;
        const uint32_t k = logn + logm;
        if (h[8] != k) return {SCAN_BAD_K, i, off};
        const size_t len = SCAN_HDR + (size_t)(3 + 2 * k) * pb + 96;   // k <= 14: far from wrapping
        if (left < len) return {SCAN_TRUNCATED, i, off};
        if (i >= max_count) return {SCAN_TOO_MANY, i, off};
        m_of[i++] = m;
        off += len;
    }
    return {SCAN_OK, i, off};
}

}  // namespace bpp
