// Host build of csrc/staging.hpp (tests/test_staging_cpu.py) against a stand-in for the HIP names it uses: a heap-backed
// hipMalloc / hipFree that counts live allocations, bounds-checked copies, and a switch that makes the k-th checked call
// (hipMalloc or hipMemcpy -- the calls whose result the vocabulary looks at) fail.  The error paths of the host forms
// cannot be run on a GPU; this is where they run.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

// ---- the stand-in ------------------------------------------------------------------------------------------------
enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1, hipErrorUnknown = 999 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };

struct FakeAlloc {
    size_t bytes;
    bool secret;   // has received bytes from g_secret_src
};
static std::map<uint8_t*, FakeAlloc> g_live;
static int g_calls = 0, g_fail_at = 0;          // g_fail_at = k: the k-th checked call fails (0: none)
static int g_dirty_secret_frees = 0, g_secret_frees = 0, g_bad_access = 0;
static const void* g_secret_src = nullptr;

static bool fails_now() { return ++g_calls == g_fail_at; }
static const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "injected failure"; }

static hipError_t hipMalloc(void** p, size_t n) {
    if (fails_now()) return hipErrorOutOfMemory;   // leaves *p alone, as the runtime does
    if (n == 0) return hipErrorInvalidValue;        // the vocabulary never asks for 0 bytes
    uint8_t* q = static_cast<uint8_t*>(std::malloc(n));
    std::memset(q, 0xCD, n);
    g_live[q] = FakeAlloc{n, false};
    *p = q;
    return hipSuccess;
}
static hipError_t hipFree(void* p) {
    auto it = g_live.find(static_cast<uint8_t*>(p));
    if (it == g_live.end()) {
        g_bad_access++;
        return hipErrorInvalidValue;
    }
    if (it->second.secret) {
        g_secret_frees++;
        for (size_t i = 0; i < it->second.bytes; i++)
            if (it->first[i]) {
                g_dirty_secret_frees++;
                break;
            }
    }
    std::free(p);
    g_live.erase(it);
    return hipSuccess;
}
// [p, p + n) inside one live allocation?
static FakeAlloc* device_range(const void* p, size_t n) {
    for (auto& a : g_live)
        if (p >= a.first && static_cast<const uint8_t*>(p) + n <= a.first + a.second.bytes) return &a.second;
    g_bad_access++;
    return nullptr;
}
static hipError_t hipMemcpy(void* dst, const void* src, size_t n, hipMemcpyKind kind) {
    if (fails_now()) return hipErrorUnknown;   // and copies nothing
    FakeAlloc* a = device_range(kind == hipMemcpyHostToDevice ? dst : src, n);
    if (!a) return hipErrorInvalidValue;
    if (kind == hipMemcpyHostToDevice && src == g_secret_src) a->secret = true;
    std::memcpy(dst, src, n);
    return hipSuccess;
}
static hipError_t hipMemset(void* p, int v, size_t n) {
    if (!device_range(p, n)) return hipErrorInvalidValue;
    std::memset(p, v, n);
    return hipSuccess;
}

#include "../../bulletproofsplus_amd/csrc/staging.hpp"

using bpp::DevBuf;

static int failures = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            std::printf("FAIL ");        \
            std::printf(__VA_ARGS__);    \
            std::printf("\n");           \
            failures++;                  \
        }                                \
    } while (0)

// ---- a host form as the library writes them: three inputs (data, a key that is wiped, an optional index), two outputs ----
constexpr size_t N_DATA = 40, N_KEY = 32, N_INDEX = 24, N_OUT0 = 40, N_OUT1 = 8;
static bool g_entry_saw_index = false, g_entry_ran = false;

static int staged(const uint8_t* data, const uint8_t* key, const uint64_t* index, uint8_t* out0, uint8_t* out1) {
    DevBuf d_data, d_key(true), d_index, d_out0, d_out1;
    HIPCHK(d_data.upload(data, N_DATA));
    HIPCHK(d_key.upload(key, N_KEY));
    HIPCHK(d_index.upload(index, N_INDEX));
    HIPCHK(d_out0.alloc(N_OUT0));
    HIPCHK(d_out1.alloc(N_OUT1));
    // the "device entry": out0 = data ^ key (repeated), out1 = the first 8 key bytes; an absent index arrives as null
    g_entry_ran = true;
    g_entry_saw_index = d_index.u64() != nullptr;
    for (size_t i = 0; i < N_OUT0; i++) d_out0.u8()[i] = d_data.u8()[i] ^ d_key.u8()[i % N_KEY];
    std::memcpy(d_out1.p, d_key.p, N_OUT1);
    HIPCHK(d_out0.download(out0, N_OUT0));
    HIPCHK(d_out1.download(out1, N_OUT1));
    return BPP_OK;
}
// the checked calls of staged() with the index absent, in order, as HIPCHK names them at the call site: buffer and size
static const char* const STAGED_CALLS[] = {
    "d_data.upload(data, N_DATA): out of memory",       // its allocation
    "d_data.upload(data, N_DATA): injected failure",    // its copy
    "d_key.upload(key, N_KEY): out of memory",
    "d_key.upload(key, N_KEY): injected failure",
    "d_out0.alloc(N_OUT0): out of memory",
    "d_out1.alloc(N_OUT1): out of memory",
    "d_out0.download(out0, N_OUT0): injected failure",
    "d_out1.download(out1, N_OUT1): injected failure",
};
constexpr int N_STAGED_CALLS = sizeof STAGED_CALLS / sizeof STAGED_CALLS[0];

int main() {
    uint8_t data[N_DATA], key[N_KEY], want0[N_OUT0];
    for (size_t i = 0; i < N_DATA; i++) data[i] = (uint8_t)(3 * i + 1);
    for (size_t i = 0; i < N_KEY; i++) key[i] = (uint8_t)(0xA5 ^ i) | 1;   // no zero byte: a wipe shows
    for (size_t i = 0; i < N_OUT0; i++) want0[i] = data[i] ^ key[i % N_KEY];

    {   // null gives null; non-null with 0 bytes gives a buffer
        DevBuf b;
        CHECK(b.upload(nullptr, 64) == hipSuccess && b.p == nullptr && b.bytes == 0 && b.as<uint64_t>() == nullptr, "null -> null");
        CHECK(g_live.empty() && g_calls == 0, "null upload touched the device");
        CHECK(b.upload(data, 0) == hipSuccess && b.p != nullptr && b.bytes == 0, "non-null, 0 bytes -> a buffer");
        CHECK(g_live.size() == 1, "0-byte buffer is one allocation");
        uint8_t guard = 0x77;
        CHECK(b.download(&guard, 0) == hipSuccess && guard == 0x77, "download of 0 bytes");
        CHECK(b.upload(nullptr, 8) == hipSuccess && b.p == nullptr && g_live.empty(), "null over a held buffer frees it");
    }
    {   // upload then download returns the bytes; re-alloc frees first
        DevBuf b;
        uint8_t back[N_DATA] = {0};
        CHECK(b.upload(data, N_DATA) == hipSuccess && b.bytes == N_DATA, "upload");
        CHECK(b.download(back, N_DATA) == hipSuccess && std::memcmp(back, data, N_DATA) == 0, "download returns the bytes");
        CHECK(b.alloc(16) == hipSuccess && g_live.size() == 1 && b.bytes == 16, "re-alloc frees first");
        CHECK(b.upload(key, 8) == hipSuccess && g_live.size() == 1 && b.bytes == 8, "upload over a held buffer frees first");
        CHECK(b.u32() == b.p && b.u8() == b.p && b.as<char>() == b.p, "typed accessors");
    }
    CHECK(g_live.empty(), "a buffer outlived its scope: %zu live", g_live.size());

    // the staged sequence, clean
    g_secret_src = key;
    uint8_t out0[N_OUT0], out1[N_OUT1];
    std::memset(out0, 0xEE, sizeof out0);
    std::memset(out1, 0xEE, sizeof out1);
    g_calls = 0;
    CHECK(staged(data, key, nullptr, out0, out1) == BPP_OK, "staged: %s", last_error());
    CHECK(g_calls == N_STAGED_CALLS, "staged made %d checked calls, the test lists %d", g_calls, N_STAGED_CALLS);
    CHECK(!g_entry_saw_index, "an absent input reached the entry as a pointer");
    CHECK(std::memcmp(out0, want0, N_OUT0) == 0 && std::memcmp(out1, key, N_OUT1) == 0, "staged outputs");
    CHECK(g_live.empty() && g_secret_frees == 1 && g_dirty_secret_frees == 0, "clean run: live %zu, key frees %d, unwiped %d",
          g_live.size(), g_secret_frees, g_dirty_secret_frees);
    {   // ... and with the optional input present
        const uint64_t index[3] = {5, 6, 7};
        CHECK(staged(data, key, index, out0, out1) == BPP_OK && g_entry_saw_index && g_live.empty(), "staged with the index");
    }

    // every k: the k-th checked call fails
    for (int k = 1; k <= N_STAGED_CALLS; k++) {
        std::memset(out0, 0xEE, sizeof out0);
        std::memset(out1, 0xEE, sizeof out1);
        g_calls = 0, g_fail_at = k, g_secret_frees = g_dirty_secret_frees = 0, g_entry_ran = false;
        fail(BPP_OK, "");
        const int rc = staged(data, key, nullptr, out0, out1);
        g_fail_at = 0;
        CHECK(rc == BPP_E_HIP, "k = %d: code %d", k, rc);
        CHECK(std::strcmp(last_error(), STAGED_CALLS[k - 1]) == 0, "k = %d: text \"%s\", want \"%s\"", k, last_error(),
              STAGED_CALLS[k - 1]);
        CHECK(g_live.empty(), "k = %d: %zu allocations left", k, g_live.size());
        // the key reached the device from call 4 on: from then on it is freed once, wiped
        CHECK(g_secret_frees == (k > 4 ? 1 : 0) && g_dirty_secret_frees == 0, "k = %d: key frees %d, unwiped %d", k, g_secret_frees,
              g_dirty_secret_frees);
        CHECK(g_entry_ran == (k > 6), "k = %d: the entry %s", k, g_entry_ran ? "ran" : "did not run");
        // nothing reaches an output whose download did not succeed -- and none does before the entry has run: only the
        // failure of the LAST download (k = 8) follows a download that succeeded, and leaves out0 complete
        bool clean0 = true, clean1 = true;
        for (uint8_t b : out0) clean0 = clean0 && b == 0xEE;
        for (uint8_t b : out1) clean1 = clean1 && b == 0xEE;
        CHECK(clean1, "k = %d: out1 was written", k);
        if (k < N_STAGED_CALLS) CHECK(clean0, "k = %d: out0 was written", k);
        else CHECK(std::memcmp(out0, want0, N_OUT0) == 0, "k = %d: out0 is neither untouched nor complete", k);
    }
    {   // a wipe-flagged buffer whose allocation fails, and one that is re-used, leave nothing behind either
        DevBuf b(true);
        g_calls = 0, g_fail_at = 1;
        CHECK(b.upload(key, N_KEY) == hipErrorOutOfMemory && b.p == nullptr, "failed allocation of a wiped buffer");
        g_fail_at = 0, g_secret_frees = g_dirty_secret_frees = 0;
        CHECK(b.upload(key, N_KEY) == hipSuccess && b.upload(key, 16) == hipSuccess, "re-upload of a wiped buffer");
        CHECK(g_secret_frees == 1 && g_dirty_secret_frees == 0, "the first copy of the key was not wiped before it was freed");
    }
    CHECK(g_live.empty() && g_dirty_secret_frees == 0, "end: live %zu, unwiped %d", g_live.size(), g_dirty_secret_frees);
    CHECK(g_bad_access == 0, "%d accesses outside a live allocation", g_bad_access);

    if (failures) return 1;
    std::printf("ok staging\n");
    return 0;
}
