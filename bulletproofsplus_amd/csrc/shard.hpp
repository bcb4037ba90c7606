// shard.hpp -- the host side of sharding one batch over several devices: the cut of a batch into contiguous per-shard
// slices and the thread fan-out that runs one worker per shard.  HIP-free, so that a host build
// (tests/host/shard_host_test.cpp) checks it under the sanitizers; pool.hpp builds the verifier pool on it.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <thread>

#include "abi_guard.hpp"

namespace bpp {

constexpr size_t POOL_MAX_SHARDS = 16;

// bpp_shard_cuts (include/bpp_amd.h): shard r takes proofs [cuts[r], cuts[r + 1]).
//   m_of == null: sizes differ by at most one, the larger shards first (sharding.shard_bounds).
//   otherwise proof i costs m_of[i] (a pass costs ~ n m_i) and cuts[r], 0 < r < world, is the smallest i with
//   world * sum_{j<i} m_of[j] >= r * sum_all m_of[j]: the cuts are monotone and, the prefix before cuts[r + 1] lying below
//   (r + 1) total / world while the prefix at cuts[r] reaches r total / world, every shard costs less than
//   total / world + max m.  All in 64 bits; never throws.
inline int shard_cuts(const uint32_t* m_of, size_t count, size_t world, size_t* out_cuts) noexcept {
    if (world == 0 || world > POOL_MAX_SHARDS) return fail(BPP_E_ARG, "world must be in [1, 16]");
    if (!out_cuts) return fail(BPP_E_ARG, "null out_cuts");
    if ((uint64_t)count >> 32) return fail(BPP_E_ARG, "count too large");
    if (!m_of) {
        const size_t base = count / world, rem = count % world;
        for (size_t r = 0; r <= world; r++) out_cuts[r] = r * base + (r < rem ? r : rem);
        return BPP_OK;
    }
    uint64_t total = 0;
    for (size_t i = 0; i < count; i++) {
        if (m_of[i] == 0) {
            char text[48];
            std::snprintf(text, sizeof text, "m_of[%zu] = 0", i);
            return fail(BPP_E_ARG, text);
        }
        total += m_of[i];
    }
    if (total > UINT64_MAX / POOL_MAX_SHARDS) return fail(BPP_E_ARG, "the costs in m_of sum to more than 2^60");
    out_cuts[0] = 0;
    size_t r = 1;
    uint64_t prefix = 0;   // sum_{j<i} m_of[j]
    for (size_t i = 0; i < count && r < world; i++) {
        while (r < world && (uint64_t)world * prefix >= (uint64_t)r * total) out_cuts[r++] = i;
        prefix += m_of[i];
    }
    while (r <= world) out_cuts[r++] = count;
    return BPP_OK;
}

// what one shard's worker returned: its code and, for a failure, ITS thread's error text (g_err is thread_local, so the
// text is copied before the thread ends)
struct ShardResult {
    int code = BPP_OK;
    std::string text;
};

// Runs f(r) for every shard r < world on a std::thread of its own -- with cuts given, only for the non-empty shards
// (cuts[r] < cuts[r + 1]) -- each inside guarded, and fills res[r].  Every started thread is joined before the return,
// also when a later one could not be started (that shard gets BPP_E_HIP and no further thread is started).  Threads are
// started per call and none outlives it.  Never throws.
template <class F>
void run_shards(size_t world, const size_t* cuts, ShardResult* res, F&& f) noexcept {
    if (world > POOL_MAX_SHARDS) world = POOL_MAX_SHARDS;
    std::thread th[POOL_MAX_SHARDS];
    for (size_t r = 0; r < world; r++) {
        res[r].code = BPP_OK;
        res[r].text.clear();
    }
    for (size_t r = 0; r < world; r++) {
        if (cuts && cuts[r] >= cuts[r + 1]) continue;
        ShardResult* out = res + r;
        try {
            th[r] = std::thread([out, r, &f]() noexcept {
                out->code = guarded([&]() -> int { return f(r); });
                if (out->code == BPP_OK) return;
                try {
                    out->text = last_error();
                } catch (...) {   // the code stands, the text is lost
                }
            });
        } catch (...) {
            out->code = BPP_E_HIP;
            try {
                out->text = "could not start a worker thread";
            } catch (...) {
            }
            break;
        }
    }
    for (size_t r = 0; r < world; r++)
        if (th[r].joinable()) th[r].join();
}

// the failure of the lowest failing shard as this thread's error: its code, its text prefixed "shard r (device d): "
// (devices may be null: "shard r: "); BPP_OK when every shard succeeded
inline int shard_failure(const ShardResult* res, size_t world, const int* devices) noexcept {
    for (size_t r = 0; r < world; r++) {
        if (res[r].code == BPP_OK) continue;
        char prefix[64];
        if (devices)
            std::snprintf(prefix, sizeof prefix, "shard %zu (device %d): ", r, devices[r]);
        else
            std::snprintf(prefix, sizeof prefix, "shard %zu: ", r);
        return fail(res[r].code, prefix, res[r].text.c_str());
    }
    return BPP_OK;
}

}  // namespace bpp
