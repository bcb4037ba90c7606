// pool.hpp -- the verifier pool: one bpp_ctx + bpp_verifier per shard, each on its device with a stream and buffers of
// its own, and the three verify calls that cut a batch (shard.hpp), run the existing device passes of the shards on one
// host thread each and put the verdicts back in caller order (include/bpp_amd.h "verifier pool").  No kernel lives here:
// the workers call the library's own entry points.  Included by capi.hip below the entry shims and the container sizes
// (on_device, container_point_size), which it uses.
#pragma once
#include <memory>
#include <vector>

#include "shard.hpp"

struct PoolShard {
    int device = 0;
    bpp_ctx* ctx = nullptr;
    bpp_verifier* v = nullptr;
    hipStream_t stream = nullptr;
    bpp::DevBuf in0, in1, ok, ws, partial;   // grown on demand, reused across calls
    uint64_t stats[2] = {0, 0};              // of the shard's last grouped call
};

struct bpp_pool {
    std::vector<PoolShard> shards;   // sized once, never resized (a shard holds device buffers)
    std::vector<int> devices;
    std::vector<uint32_t> h_ok;      // the verdicts of a call; shard r writes [cuts[r], cuts[r + 1])
    std::vector<uint32_t> m_full;    // m_of of a uniform batch
    bpp::DevBuf gather;              // the partials of a combined check, on shard 0's device
    explicit bpp_pool(size_t n_dev) : shards(n_dev), devices(n_dev) {}
};

namespace bpp {

inline hipError_t pool_reserve(DevBuf& b, size_t bytes) { return (b.p && b.bytes >= bytes) ? hipSuccess : b.alloc(bytes); }

inline void pool_release(bpp_pool* pool) noexcept {
    if (!pool) return;
    for (PoolShard& sh : pool->shards) {
        if (sh.stream)
            (void)on_device(sh.device, [&]() -> int {
                (void)hipStreamDestroy(sh.stream);
                return BPP_OK;
            });
        bpp_verifier_destroy(sh.v);
        bpp_destroy(sh.ctx);
    }
    delete pool;   // the device buffers go with their DevBuf
}

inline int pool_create(int curve_id, const int* devices, size_t n_dev, const uint64_t* gh, const uint64_t* G, const uint64_t* H,
                       size_t n, size_t m, int window_bits, bpp_pool** out) {
    auto pool = std::make_unique<bpp_pool>(n_dev);
    for (size_t r = 0; r < n_dev; r++) pool->shards[r].device = pool->devices[r] = devices[r];
    // the tables take seconds at the bench width: the shards are built side by side
    ShardResult res[POOL_MAX_SHARDS];
    run_shards(n_dev, nullptr, res, [&](size_t r) -> int {
        PoolShard& sh = pool->shards[r];
        int rc = bpp_init(curve_id, sh.device, &sh.ctx);
        if (rc) return rc;
        rc = bpp_verifier_create(sh.ctx, gh, G, H, n, m, window_bits, &sh.v);
        if (rc) return rc;
        return on_device(sh.device, [&]() -> int {
            HIPCHK(hipStreamCreateWithFlags(&sh.stream, hipStreamNonBlocking));
            return BPP_OK;
        });
    });
    const int rc = shard_failure(res, n_dev, pool->devices.data());
    if (rc) {
        pool_release(pool.release());
        return rc;
    }
    *out = pool.release();
    return BPP_OK;
}

// m_of[i] must be a power of two in [1, capacity m]: checked for the whole batch on the calling thread, the text naming
// the caller's index (the shards see slices)
inline int pool_check_m_of(const bpp_pool* pool, const uint32_t* m_of, size_t count) {
    const uint32_t cap = pool->shards[0].v->s.m;
    for (size_t i = 0; i < count; i++)
        if (m_of[i] == 0 || (m_of[i] & (m_of[i] - 1)) || m_of[i] > cap)
            return fail(BPP_E_ARG, "m_of[" + std::to_string(i) + "] = " + std::to_string(m_of[i]) +
                                       ": not a power of two in [1, " + std::to_string(cap) + "]");
    return BPP_OK;
}

// One verify call of the pool.  in0 / in1 are the caller's two host inputs, off0 / off1 the byte offset of every cut in
// them; pass(shard, lo, cnt) enqueues the shard's device pass over sh.in0 / sh.in1 (already uploaded) on sh.stream with
// workspace sh.ws, which need(shard, lo, cnt) sized (0: the slice is not taken, explain(shard, lo, cnt) says why), writing
// ok_words verdict words per proof into sh.ok.  The verdicts land in pool->h_ok; nothing of the caller's is written here.
template <class Need, class Explain, class Pass>
int pool_run(bpp_pool* pool, const size_t* cuts, const uint8_t* in0, const size_t* off0, const uint8_t* in1, const size_t* off1,
             bool per_proof_ok, Need&& need, Explain&& explain, Pass&& pass) {
    const size_t world = pool->shards.size();
    ShardResult res[POOL_MAX_SHARDS];
    run_shards(world, cuts, res, [&](size_t r) -> int {
        PoolShard& sh = pool->shards[r];
        const size_t lo = cuts[r], cnt = cuts[r + 1] - lo;
        return on_device(sh.device, [&]() -> int {
            const size_t wsb = need(sh, lo, cnt);
            if (!wsb) return explain(sh, lo, cnt);
            const size_t b0 = off0[r + 1] - off0[r], b1 = off1[r + 1] - off1[r];
            HIPCHK(pool_reserve(sh.in0, b0));
            HIPCHK(pool_reserve(sh.in1, b1));
            HIPCHK(pool_reserve(sh.ok, per_proof_ok ? cnt * 4 : 4));
            HIPCHK(pool_reserve(sh.ws, wsb));
            HIPCHK(hipMemcpyAsync(sh.in0.p, in0 + off0[r], b0, hipMemcpyHostToDevice, sh.stream));
            HIPCHK(hipMemcpyAsync(sh.in1.p, in1 + off1[r], b1, hipMemcpyHostToDevice, sh.stream));
            const int rc = pass(sh, lo, cnt, wsb);
            if (rc) return rc;
            if (per_proof_ok)
                HIPCHK(hipMemcpyAsync(pool->h_ok.data() + lo, sh.ok.p, cnt * 4, hipMemcpyDeviceToHost, sh.stream));
            HIPCHK(hipStreamSynchronize(sh.stream));
            return BPP_OK;
        });
    });
    return shard_failure(res, world, pool->devices.data());
}

inline int pool_verify_mixed(bpp_pool* pool, const uint64_t* points, const uint64_t* scalars, const uint32_t* m_of, size_t count,
                             uint32_t* out_ok) {
    const VerifyShape& cap = pool->shards[0].v->s;
    if (!m_of) {   // a uniform batch at the capacity shape
        pool->m_full.assign(count, cap.m);
        m_of = pool->m_full.data();
    }
    int rc = pool_check_m_of(pool, m_of, count);
    if (rc) return rc;
    const size_t world = pool->shards.size(), pw = (size_t)bpp_point_words(pool->shards[0].ctx->curve) * 8;
    size_t cuts[POOL_MAX_SHARDS + 1], off0[POOL_MAX_SHARDS + 1] = {0}, off1[POOL_MAX_SHARDS + 1] = {0};
    rc = shard_cuts(m_of, count, world, cuts);
    if (rc) return rc;
    const uint32_t logn = cap.k - (uint32_t)__builtin_ctz(cap.m);
    for (size_t r = 0; r < world; r++) {
        size_t npts = 0;
        for (size_t i = cuts[r]; i < cuts[r + 1]; i++) npts += 3 + 2 * (logn + (uint32_t)__builtin_ctz(m_of[i])) + m_of[i];
        off0[r + 1] = off0[r] + npts * pw;
        off1[r + 1] = cuts[r + 1] * 96;
    }
    pool->h_ok.resize(count);
    rc = pool_run(
        pool, cuts, reinterpret_cast<const uint8_t*>(points), off0, reinterpret_cast<const uint8_t*>(scalars), off1, true,
        [&](PoolShard& sh, size_t lo, size_t cnt) { return bpp_verifier_mixed_workspace_bytes(sh.v, m_of + lo, cnt); },
        [&](PoolShard& sh, size_t lo, size_t cnt) -> int {
            MixedPlan p;
            const int e = mixed_plan(sh.v->s, m_of + lo, cnt, false, p);
            return e ? e : fail(BPP_E_ARG, "mixed batch rejected");
        },
        [&](PoolShard& sh, size_t lo, size_t cnt, size_t wsb) {
            return bpp_verifier_run_mixed(sh.v, static_cast<const uint64_t*>(sh.in0.p), static_cast<const uint64_t*>(sh.in1.p),
                                          m_of + lo, cnt, nullptr, sh.ok.u32(), sh.ws.p, wsb, nullptr, sh.stream);
        });
    if (rc) return rc;
    std::memcpy(out_ok, pool->h_ok.data(), count * 4);
    return BPP_OK;
}

inline int pool_verify_serialized_mixed(bpp_pool* pool, const uint8_t* proofs, const uint8_t* commitments, const uint32_t* m_of,
                                        size_t count, int flags, int mode, const uint8_t* weight_key, uint64_t index_base,
                                        uint32_t group, uint32_t* out_ok, uint64_t* stats) {
    const int curve = pool->shards[0].ctx->curve, version = (flags & BPP_SER_UNCOMPRESSED) ? 2 : 1;
    const size_t cb = container_point_size(curve, version);
    if (int rc = container_version_ok(cb)) return rc;
    int rc = pool_check_m_of(pool, m_of, count);
    if (rc) return rc;
    const size_t world = pool->shards.size(), n = pool->shards[0].v->s.n;
    size_t cuts[POOL_MAX_SHARDS + 1], off0[POOL_MAX_SHARDS + 1] = {0}, off1[POOL_MAX_SHARDS + 1] = {0};
    rc = shard_cuts(m_of, count, world, cuts);
    if (rc) return rc;
    for (size_t r = 0; r < world; r++) {
        size_t pbytes = 0, cbytes = 0;
        for (size_t i = cuts[r]; i < cuts[r + 1]; i++) {
            pbytes += bpp_proof_bytes_version(curve, n, m_of[i], version);
            cbytes += m_of[i] * cb;
        }
        off0[r + 1] = off0[r] + pbytes;
        off1[r + 1] = off1[r] + cbytes;
    }
    const bool grouped = mode == BPP_POOL_GROUPED;
    pool->h_ok.resize(count);
    rc = pool_run(
        pool, cuts, proofs, off0, commitments, off1, true,
        [&](PoolShard& sh, size_t lo, size_t cnt) {
            return grouped ? bpp_verifier_serialized_grouped_mixed_workspace_bytes(sh.v, m_of + lo, cnt, group)
                           : bpp_verifier_serialized_mixed_workspace_bytes(sh.v, m_of + lo, cnt);
        },
        [&](PoolShard& sh, size_t lo, size_t cnt) -> int {   // the 4 GiB limits of the byte index hold per shard
            MixedPlan p;
            const int e = mixed_plan_serialized(sh.v->s, m_of + lo, cnt, cb, false, p);
            return e ? e : fail(BPP_E_ARG, "serialized mixed batch rejected");
        },
        [&](PoolShard& sh, size_t lo, size_t cnt, size_t wsb) {
            // the weights belong to the caller's numbering: proof i is weighted by PRF(key, index_base + i) whatever the cut
            return grouped ? bpp_range_verify_batch_serialized_grouped_mixed_device(sh.v, sh.in0.p, sh.in1.p, m_of + lo, cnt, flags,
                                                                                    weight_key, index_base + lo, group,
                                                                                    sh.ok.u32(), sh.stats, sh.ws.p, wsb, sh.stream)
                           : bpp_range_verify_batch_serialized_mixed_device(sh.v, sh.in0.p, sh.in1.p, m_of + lo, cnt, flags,
                                                                            sh.ok.u32(), sh.ws.p, wsb, sh.stream);
        });
    if (rc) return rc;
    std::memcpy(out_ok, pool->h_ok.data(), count * 4);
    if (grouped && stats) {
        stats[0] = stats[1] = 0;
        for (size_t r = 0; r < world; r++)
            if (cuts[r] < cuts[r + 1]) {
                stats[0] += pool->shards[r].stats[0];
                stats[1] += pool->shards[r].stats[1];
            }
    }
    return BPP_OK;
}

inline int pool_verify_combined(bpp_pool* pool, const uint64_t* points, const uint64_t* scalars, size_t count,
                                const uint8_t* weight_key, uint64_t index_base, uint32_t* out_ok) {
    const VerifyShape& cap = pool->shards[0].v->s;
    const size_t world = pool->shards.size(), pw = (size_t)bpp_point_words(pool->shards[0].ctx->curve) * 8;
    size_t cuts[POOL_MAX_SHARDS + 1], off0[POOL_MAX_SHARDS + 1], off1[POOL_MAX_SHARDS + 1];
    int rc = shard_cuts(nullptr, count, world, cuts);
    if (rc) return rc;
    for (size_t r = 0; r <= world; r++) {
        off0[r] = cuts[r] * cap.NV * pw;
        off1[r] = cuts[r] * 96;
    }
    PoolShard& s0 = pool->shards[0];
    const size_t pb = bpp_verifier_partial_bytes(s0.v);
    rc = pool_run(
        pool, cuts, reinterpret_cast<const uint8_t*>(points), off0, reinterpret_cast<const uint8_t*>(scalars), off1, false,
        [&](PoolShard& sh, size_t, size_t cnt) { return bpp_verifier_combined_workspace_bytes(sh.v, cnt); },
        [&](PoolShard&, size_t, size_t) -> int { return fail(BPP_E_ARG, "combined batch rejected"); },
        [&](PoolShard& sh, size_t lo, size_t cnt, size_t wsb) -> int {
            HIPCHK(pool_reserve(sh.partial, pb));
            return bpp_verifier_run_combined(sh.v, static_cast<const uint64_t*>(sh.in0.p), static_cast<const uint64_t*>(sh.in1.p),
                                             cnt, nullptr, weight_key, index_base + lo, nullptr, sh.partial.p, sh.ok.u32(),
                                             sh.ws.p, wsb, sh.stream);
        });
    if (rc) return rc;
    // the single reduce: the partials of the non-empty shards -- all that crosses devices -- gathered on shard 0's device
    // and summed there.  The copies ride shard 0's stream, so the sum is ordered behind them; the workers have
    // synchronised their streams, so the sources are complete.
    uint32_t word = 1;
    rc = on_device(s0.device, [&]() -> int {
        HIPCHK(pool_reserve(pool->gather, world * pb));
        HIPCHK(pool_reserve(s0.ok, 4));
        size_t k = 0;
        for (size_t r = 0; r < world; r++) {
            if (cuts[r] >= cuts[r + 1]) continue;
            PoolShard& sh = pool->shards[r];
            HIPCHK(hipMemcpyPeerAsync(static_cast<uint8_t*>(pool->gather.p) + k * pb, s0.device, sh.partial.p, sh.device, pb,
                                      s0.stream));
            k++;
        }
        const int e = bpp_verifier_sum_partials(s0.v, pool->gather.p, k, s0.ok.u32(), s0.stream);
        if (e) return e;
        HIPCHK(hipMemcpyAsync(&word, s0.ok.p, 4, hipMemcpyDeviceToHost, s0.stream));
        HIPCHK(hipStreamSynchronize(s0.stream));
        return BPP_OK;
    });
    if (rc) return fail(rc, "the reduce on shard 0: ", std::string(last_error()).c_str());
    *out_ok = word;
    return BPP_OK;
}

}  // namespace bpp
