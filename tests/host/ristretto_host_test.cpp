// Host build (g++, no GPU) of csrc/ristretto.hpp: the text the device compiles, driven line by line.
// tests/test_codec_cases_cpu.py feeds it the corpora of tests/codec_cases.py and compares every answer with
// oracle/pyref.py bit for bit.  It is also the only place that reaches rist_from_uniform_bytes directly: the ABI derives
// its 64 bytes from SHA-256, so halves with t >= p or bit 255 set cannot be sent to the device.
// stdin: one request per line, all values hex; field elements and strings are little-endian byte strings of 32 bytes.
//   dec s            ->  "1 x y" | "0"                 rist_decode
//   enc x y          ->  s                             rist_encode of the affine point (x, y)
//   eq x1 y1 x2 y2   ->  "1" | "0"                     rist_equal
//   uni b (64 bytes) ->  "x y"                         rist_from_uniform_bytes, made affine
// Exit code 2: malformed input.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../bulletproofsplus_amd/csrc/ristretto.hpp"
using namespace bpp;
using C = Ed25519;
using F = Fe<EdFp>;

static int nib(char c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    return -1;
}

// hex of exactly n bytes into a buffer of exactly n bytes (heap: a read past the end is the sanitizer's to see)
static bool unhex(const std::string& h, size_t n, std::vector<uint8_t>& out) {
    if (h.size() != 2 * n) return false;
    out.assign(n, 0);
    for (size_t i = 0; i < n; i++) {
        const int a = nib(h[2 * i]), b = nib(h[2 * i + 1]);
        if (a < 0 || b < 0) return false;
        out[i] = (uint8_t)(a * 16 + b);
    }
    return true;
}

static bool field(const std::string& h, F& out) {
    std::vector<uint8_t> b;
    if (!unhex(h, 32, b)) return false;
    uint32_t w[8];
    for (int i = 0; i < 8; i++)
        w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
    if (!words_lt_mod<EdFp>(w)) return false;
    out = fe_from_canonical<EdFp>(w);
    return true;
}

static void put_bytes(const uint8_t* b, size_t n) {
    for (size_t i = 0; i < n; i++) printf("%02x", b[i]);
}

static void put_field(const F& a) {
    uint32_t w[8];
    fe_to_canonical(a, w);
    for (int i = 0; i < 8; i++) printf("%02x%02x%02x%02x", w[i] & 0xff, (w[i] >> 8) & 0xff, (w[i] >> 16) & 0xff, w[i] >> 24);
}

int main() {
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        std::vector<std::string> tok;
        for (char* t = strtok(line, " \r\n"); t; t = strtok(nullptr, " \r\n")) tok.push_back(t);
        if (tok.empty()) continue;
        if (tok[0] == "dec" && tok.size() == 2) {
            std::vector<uint8_t> s;
            if (!unhex(tok[1], 32, s)) return 2;
            Aff<C> a;
            if (rist_decode(s.data(), a)) {
                printf("1 ");
                put_field(a.x);
                printf(" ");
                put_field(a.y);
            } else {
                printf("0");
            }
        } else if (tok[0] == "enc" && tok.size() == 3) {
            Aff<C> a;
            if (!field(tok[1], a.x) || !field(tok[2], a.y)) return 2;
            std::vector<uint8_t> out(32);
            rist_encode(jac_from_aff(a), out.data());
            put_bytes(out.data(), 32);
        } else if (tok[0] == "eq" && tok.size() == 5) {
            Aff<C> a, b;
            if (!field(tok[1], a.x) || !field(tok[2], a.y) || !field(tok[3], b.x) || !field(tok[4], b.y)) return 2;
            printf("%d", rist_equal(a, b) ? 1 : 0);
        } else if (tok[0] == "uni" && tok.size() == 2) {
            std::vector<uint8_t> b;
            if (!unhex(tok[1], 64, b)) return 2;
            const Aff<C> a = jac_to_aff(rist_from_uniform_bytes(b.data()));
            put_field(a.x);
            printf(" ");
            put_field(a.y);
        } else {
            return 2;
        }
        printf("\n");
    }
    return 0;
}
