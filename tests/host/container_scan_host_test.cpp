// Host build of csrc/container_scan.hpp (tests/test_serialized_mixed_abi_cpu.py), meant for the sanitizers: the header
// walk of bpp_proofs_scan parses untrusted bytes.  Every input sits in a heap block of EXACTLY its length and every m_of
// array holds EXACTLY max_count words, so that a read past proofs_bytes or a write past max_count is a heap overflow the
// sanitizer reports; the invariants are checked besides.
//   usage: container_scan_host_test <curve> <n> <version> <stream file> <expected m, comma separated>
// Walks the stream itself, every prefix of it, every max_count below its count, and a few hundred single-byte mutations.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../bulletproofsplus_amd/csrc/container_scan.hpp"

using namespace bpp;

static int failures = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            std::printf("FAIL %s: ", #cond);                  \
            std::printf(__VA_ARGS__);                         \
            std::printf("\n");                                \
            failures++;                                       \
        }                                                     \
    } while (0)

// scan over exact-size copies; checks what must hold for ANY input
static ScanResult scan_exact(int curve, size_t n, int version, const uint8_t* src, size_t bytes, size_t max_count,
                             std::vector<uint32_t>* out = nullptr) {
    std::unique_ptr<uint8_t[]> buf(new uint8_t[bytes ? bytes : 1]);
    if (bytes) std::memcpy(buf.get(), src, bytes);
    std::unique_ptr<uint32_t[]> m_of(new uint32_t[max_count ? max_count : 1]);
    const ScanResult r = container_scan(curve, n, version, bytes ? buf.get() : nullptr, bytes, max_count ? m_of.get() : nullptr,
                                        max_count);
    CHECK(r.count <= max_count, "count %zu > max_count %zu", r.count, max_count);
    CHECK(r.offset <= bytes, "offset %zu > bytes %zu", r.offset, bytes);
    if (r.status == SCAN_OK) CHECK(r.offset == bytes, "ok with %zu of %zu bytes consumed", r.offset, bytes);
    for (size_t i = 0; i < r.count; i++) CHECK(m_of[i] && !(m_of[i] & (m_of[i] - 1)) && m_of[i] <= 128, "m_of[%zu] = %u", i, m_of[i]);
    if (out) out->assign(m_of.get(), m_of.get() + r.count);
    return r;
}

int main(int argc, char** argv) {
    if (argc != 6) {
        std::printf("usage: %s curve n version file m,m,..\n", argv[0]);
        return 2;
    }
    const int curve = std::atoi(argv[1]), version = std::atoi(argv[3]);
    const size_t n = (size_t)std::atoll(argv[2]);
    std::vector<uint32_t> want;
    for (const char* p = argv[5]; *p;) {
        want.push_back((uint32_t)std::strtoul(p, const_cast<char**>(&p), 10));
        if (*p == ',') p++;
    }
    std::FILE* f = std::fopen(argv[4], "rb");
    if (!f) return 2;
    std::vector<uint8_t> s;
    for (int c; (c = std::fgetc(f)) != EOF;) s.push_back((uint8_t)c);
    std::fclose(f);

    // the stream itself
    std::vector<uint32_t> got;
    ScanResult r = scan_exact(curve, n, version, s.data(), s.size(), want.size(), &got);
    CHECK(r.status == SCAN_OK && got == want, "good stream: status %d, %zu containers", (int)r.status, r.count);
    r = scan_exact(curve, n, version, s.data(), s.size(), want.size() + 7, &got);
    CHECK(r.status == SCAN_OK && got == want, "good stream, roomy m_of: status %d", (int)r.status);
    // container boundaries, from the lengths the walk implies
    std::vector<size_t> ends;
    {
        size_t off = 0;
        uint32_t logn = 0;
        while (((size_t)1 << logn) < n) logn++;
        for (uint32_t m : want) {
            uint32_t logm = 0;
            while ((1u << logm) < m) logm++;
            off += SCAN_HDR + (size_t)(3 + 2 * (logn + logm)) * scan_point_bytes(curve, version) + 96;
            ends.push_back(off);
        }
        CHECK(off == s.size(), "lengths sum to %zu, stream has %zu", off, s.size());
    }
    // every max_count below the count
    for (size_t mc = 0; mc < want.size(); mc++) {
        r = scan_exact(curve, n, version, s.data(), s.size(), mc, &got);
        CHECK(r.status == SCAN_TOO_MANY && r.count == mc, "max_count %zu: status %d count %zu", mc, (int)r.status, r.count);
        CHECK(std::equal(got.begin(), got.end(), want.begin()), "max_count %zu: m_of", mc);
    }
    // every prefix: ok exactly on a container boundary, truncated elsewhere, naming the container it stopped in
    for (size_t len = 0; len < s.size(); len++) {
        r = scan_exact(curve, n, version, s.data(), len, want.size(), &got);
        size_t whole = 0;
        while (whole < ends.size() && ends[whole] <= len) whole++;
        const bool boundary = len == 0 || (whole && ends[whole - 1] == len);
        CHECK(r.count == whole, "prefix %zu: %zu containers, want %zu", len, r.count, whole);
        CHECK(r.status == (boundary ? SCAN_OK : SCAN_TRUNCATED), "prefix %zu: status %d", len, (int)r.status);
        if (!boundary) CHECK(r.offset == (whole ? ends[whole - 1] : 0), "prefix %zu: offset %zu", len, r.offset);
    }
    // single-byte mutations: every header byte of every container with two values each, then pseudo-random positions
    std::vector<uint8_t> t(s);
    size_t mutations = 0, rejected = 0;
    auto mutate = [&](size_t pos, uint8_t v) {
        if (t[pos] == v) return;
        const uint8_t keep = t[pos];
        t[pos] = v;
        r = scan_exact(curve, n, version, t.data(), t.size(), want.size(), &got);
        mutations++;
        rejected += r.status != SCAN_OK;
        // a byte the walk does not look at leaves the framing alone
        size_t c = 0;
        while (ends[c] <= pos) c++;
        const size_t in = pos - (c ? ends[c - 1] : 0);
        if (in >= 9) CHECK(r.status == SCAN_OK && got == want, "mutation at %zu (byte %zu of container %zu) changed the framing", pos, in, c);
        else if (in != 7) CHECK(r.status != SCAN_OK && r.count == c, "mutation at %zu (header byte %zu of container %zu): status %d count %zu", pos, in, c, (int)r.status, r.count);
        t[pos] = keep;
    };
    for (size_t c = 0; c < ends.size(); c++)
        for (size_t b = 0; b < SCAN_HDR; b++) {
            const size_t pos = (c ? ends[c - 1] : 0) + b;
            mutate(pos, (uint8_t)(t[pos] ^ 0x01));
            mutate(pos, (uint8_t)(t[pos] << 1 | 1));
        }
    uint64_t lcg = 0x9e3779b97f4a7c15ull;
    for (int i = 0; i < 300; i++) {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        mutate((size_t)((lcg >> 33) % s.size()), (uint8_t)(lcg >> 8));
    }
    CHECK(mutations >= 300 && rejected > 0, "%zu mutations, %zu rejected", mutations, rejected);
    // arguments the walk does not take
    CHECK(scan_exact(curve, 0, version, s.data(), s.size(), 4).status == SCAN_BAD_ARG, "n = 0");
    CHECK(scan_exact(curve, 3, version, s.data(), s.size(), 4).status == SCAN_BAD_ARG, "n = 3");
    CHECK(scan_exact(curve, 256, version, s.data(), s.size(), 4).status == SCAN_BAD_ARG, "n = 256");
    CHECK(scan_exact(7, n, version, s.data(), s.size(), 4).status == SCAN_BAD_ARG, "curve 7");
    CHECK(scan_exact(curve, n, 3, s.data(), s.size(), 4).status == SCAN_BAD_ARG, "version 3");
    CHECK(scan_exact(2, n, 2, s.data(), s.size(), 4).status == SCAN_BAD_ARG, "ristretto255 has no version 2");

    if (failures) return 1;
    std::printf("ok container_scan curve %d version %d: %zu containers, %zu prefixes, %zu mutations (%zu rejected)\n", curve,
                version, want.size(), s.size(), mutations, rejected);
    return 0;
}
