// Host build of csrc/shard.hpp (tests/test_shard_cpu.py): the cut of a batch into per-shard slices -- the worked
// vectors of include/bpp_amd.h, the uniform rule against its formula, monotony / cover / balance on seeded random costs,
// the argument errors -- and run_shards: every kind of worker outcome lands as its code and text in its own slot, only
// non-empty shards run, and every thread is joined before the return.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <new>
#include <stdexcept>
#include <vector>

#include "../../bulletproofsplus_amd/csrc/shard.hpp"

using namespace bpp;

static int failures = 0;
#define CHECK(cond, ...)                    \
    do {                                    \
        if (!(cond)) {                      \
            std::printf("FAIL " __VA_ARGS__); \
            std::printf("\n");              \
            failures++;                     \
        }                                   \
    } while (0)

static void expect_cuts(const std::vector<uint32_t>* m, size_t count, size_t world, std::vector<size_t> want, const char* what) {
    std::vector<size_t> got(world + 1, 99);
    const int rc = shard_cuts(m ? m->data() : nullptr, count, world, got.data());
    CHECK(rc == BPP_OK && got == want, "%s: rc %d", what, rc);
}

int main() {
    // the worked values
    expect_cuts(nullptr, 10, 4, {0, 3, 6, 8, 10}, "NULL, 10, 4");
    expect_cuts(nullptr, 2, 3, {0, 1, 2, 2}, "NULL, 2, 3");
    const std::vector<uint32_t> a = {16, 1, 1, 1, 1, 1, 1, 1, 1, 8}, b = {1, 1, 16, 1, 1};
    expect_cuts(&a, a.size(), 2, {0, 1, 10}, "[16,1 x 8,8], 2");
    expect_cuts(&b, b.size(), 3, {0, 3, 3, 5}, "[1,1,16,1,1], 3");
    const std::vector<uint32_t> none;
    expect_cuts(&none, 0, 3, {0, 0, 0, 0}, "empty, 3");

    // the uniform rule against its formula
    for (size_t count = 0; count <= 50; count++)
        for (size_t world = 1; world <= 9; world++) {
            size_t cuts[POOL_MAX_SHARDS + 1];
            CHECK(shard_cuts(nullptr, count, world, cuts) == BPP_OK, "uniform rc");
            const size_t base = count / world, rem = count % world;
            for (size_t r = 0; r <= world; r++)
                CHECK(cuts[r] == r * base + (r < rem ? r : rem), "uniform %zu/%zu cut %zu = %zu", count, world, r, cuts[r]);
        }

    // seeded random costs over {1, 2, 4, 8, 16}: monotone, full cover, every shard below total / world + max m; and each
    // interior cut is the SMALLEST index that reaches its share
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    auto next = [&] {
        seed ^= seed << 13;
        seed ^= seed >> 7;
        seed ^= seed << 17;
        return seed;
    };
    for (int t = 0; t < 1000; t++) {
        const size_t count = next() % 200, world = 1 + next() % POOL_MAX_SHARDS;
        std::vector<uint32_t> m(count);
        uint64_t total = 0, maxm = 0;
        for (auto& x : m) {
            x = 1u << (next() % 5);
            total += x;
            if (x > maxm) maxm = x;
        }
        size_t cuts[POOL_MAX_SHARDS + 1];
        CHECK(shard_cuts(m.data(), count, world, cuts) == BPP_OK, "random rc");
        CHECK(cuts[0] == 0 && cuts[world] == count, "random cover");
        std::vector<uint64_t> prefix(count + 1, 0);
        for (size_t i = 0; i < count; i++) prefix[i + 1] = prefix[i] + m[i];
        for (size_t r = 0; r < world; r++) {
            CHECK(cuts[r] <= cuts[r + 1], "random monotone");
            const uint64_t cost = prefix[cuts[r + 1]] - prefix[cuts[r]];
            // (an empty batch has no max m: every shard is empty)
            CHECK(count == 0 ? cost == 0 : cost * world < total + maxm * world, "random balance: shard %zu of %zu costs %llu, total %llu", r, world,
                  (unsigned long long)cost, (unsigned long long)total);
            if (r > 0) {
                CHECK(world * prefix[cuts[r]] >= r * total, "random cut %zu reaches its share", r);
                CHECK(cuts[r] == 0 || world * prefix[cuts[r] - 1] < r * total, "random cut %zu is the smallest", r);
            }
        }
    }

    // argument errors
    size_t cuts[POOL_MAX_SHARDS + 2];
    CHECK(shard_cuts(nullptr, 4, 0, cuts) == BPP_E_ARG, "world 0");
    CHECK(shard_cuts(nullptr, 4, 17, cuts) == BPP_E_ARG, "world 17");
    CHECK(shard_cuts(nullptr, 4, 16, cuts) == BPP_OK, "world 16");
    CHECK(shard_cuts(nullptr, 4, 2, nullptr) == BPP_E_ARG, "null out");
    CHECK(shard_cuts(nullptr, (size_t)1 << 32, 2, cuts) == BPP_E_ARG, "count 2^32");
    const std::vector<uint32_t> z = {1, 2, 0, 4};
    CHECK(shard_cuts(z.data(), z.size(), 2, cuts) == BPP_E_ARG && std::strcmp(last_error(), "m_of[2] = 0") == 0, "zero cost: %s",
          last_error());

    // run_shards: a worker that throws bad_alloc, one that throws runtime_error, one that returns a code with a text, one
    // that succeeds; each in its own slot, and every thread has ended when the call returns
    {
        std::atomic<int> started{0}, ended{0};
        ShardResult res[POOL_MAX_SHARDS];
        fail(BPP_E_ARG, "the caller's own text");
        run_shards(4, nullptr, res, [&](size_t r) -> int {
            started++;
            struct Ended {
                std::atomic<int>& n;
                ~Ended() { n++; }
            } e{ended};
            if (r == 0) throw std::bad_alloc();
            if (r == 1) throw std::runtime_error("boom");
            if (r == 2) return fail(BPP_E_POINT, "a bad point in shard two");
            return BPP_OK;
        });
        CHECK(started == 4 && ended == 4, "run_shards joined %d of %d", ended.load(), started.load());
        CHECK(res[0].code == BPP_E_NOMEM && res[0].text == "host allocation failed", "bad_alloc slot: %d %s", res[0].code,
              res[0].text.c_str());
        CHECK(res[1].code == BPP_E_HIP && res[1].text == "unexpected C++ exception: boom", "runtime_error slot: %d %s",
              res[1].code, res[1].text.c_str());
        CHECK(res[2].code == BPP_E_POINT && res[2].text == "a bad point in shard two", "code slot: %d %s", res[2].code,
              res[2].text.c_str());
        CHECK(res[3].code == BPP_OK && res[3].text.empty(), "ok slot");
        CHECK(std::strcmp(last_error(), "the caller's own text") == 0, "the workers' texts stay in their threads");
        // the lowest failing shard is reported, with its prefix
        const int devices[4] = {0, 5, 0, 1};
        CHECK(shard_failure(res, 4, devices) == BPP_E_NOMEM && std::strcmp(last_error(), "shard 0 (device 0): host allocation failed") == 0,
              "lowest failure: %s", last_error());
        CHECK(shard_failure(res + 1, 3, devices + 1) == BPP_E_HIP &&
                  std::strcmp(last_error(), "shard 0 (device 5): unexpected C++ exception: boom") == 0,
              "prefix: %s", last_error());
        CHECK(shard_failure(res + 3, 1, nullptr) == BPP_OK, "no failure");
    }
    // only the non-empty shards run
    {
        const size_t c[4] = {0, 3, 3, 5};
        std::atomic<int> ran[3] = {{0}, {0}, {0}};
        ShardResult res[POOL_MAX_SHARDS];
        run_shards(3, c, res, [&](size_t r) -> int {
            ran[r]++;
            return BPP_OK;
        });
        CHECK(ran[0] == 1 && ran[1] == 0 && ran[2] == 1, "empty shard ran");
        CHECK(shard_failure(res, 3, nullptr) == BPP_OK, "empty shard result");
    }
    // many rounds with shared state: the fan-out under the thread sanitizer
    {
        std::vector<uint32_t> slots(POOL_MAX_SHARDS * 64, 0);
        for (int round = 0; round < 50; round++) {
            ShardResult res[POOL_MAX_SHARDS];
            run_shards(POOL_MAX_SHARDS, nullptr, res, [&](size_t r) -> int {
                for (size_t i = 0; i < 64; i++) slots[r * 64 + i] += (uint32_t)r;
                return r % 5 == 4 ? fail(BPP_E_HIP, "every fifth") : BPP_OK;
            });
            for (size_t r = 0; r < POOL_MAX_SHARDS; r++)
                CHECK(res[r].code == (r % 5 == 4 ? BPP_E_HIP : BPP_OK), "round %d shard %zu", round, r);
        }
        for (size_t r = 0; r < POOL_MAX_SHARDS; r++) CHECK(slots[r * 64 + 63] == 50 * r, "slots of shard %zu", r);
    }

    if (failures) return 1;
    std::printf("ok shard\n");
    return 0;
}
