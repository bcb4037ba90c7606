// literal.hpp -- the literal single-call API, bpp_range_verify / bpp_range_prove past their argument checks (capi.hip).
//
// RangeProof::verify (src/range/mod.rs:57-78) and ::prove take the public key with every call and the reference pays the
// whole naive MulVec each time.  Here a call takes one of these paths:
//   * first sight of a key: the table-free path -- the data-parallel naive MulVec (MsmImpl::range_verify_single), the
//     fold-based prover (ProveImpl::range_prove); the key is remembered;
//   * second sight: a verifier with narrow window tables is built (c = 8: built in milliseconds, < 1 GB at n m = 1024);
//   * from then on the cached pass: the batch verifier's pass at count = 1 -- with the table-free path's second opinion on
//     a BLS12-381 reject -- and the batched prover at count = 1, probing both forms of the caller's commitments, with the
//     fold-based prover as the fallback.
// Entries are found by a 64-bit hash of (curve, n, m, g, h, G, H) and CONFIRMED by comparing the key bytes, so a hash
// collision can never make a proof verify against another key's generators.  At most VCACHE_MAX verifiers, least recently
// used out.  The cache hangs off the context (bpp_ctx::verify_cache) and follows its one-thread-per-context rule.
#pragma once
#include <memory>

#include "impl_msm.hpp"
#include "impl_prove.hpp"
#include "impl_prove_batch.hpp"
#include "impl_verify.hpp"

namespace bpp {

constexpr size_t VCACHE_MAX = 4;
constexpr int VCACHE_WINDOW = 8;
struct VerifyCacheEntry {
    uint64_t hash = 0;
    size_t n = 0, m = 0;
    std::vector<uint64_t> key;              // gh | G | H as handed in
    std::unique_ptr<bpp_verifier> v;        // null: seen once, tables not built yet
    DevBuf pts, sc, ok, ws;                 // count = 1 buffers of the pass
    uint64_t stamp = 0;
};
struct VerifyCache {
    std::vector<std::unique_ptr<VerifyCacheEntry>> e;
    uint64_t clock = 0;
};
// bpp_destroy, bpp_set_verify_cache(off): the verifiers, their tables and their buffers go
inline void verify_cache_release(bpp_ctx* ctx) {
    delete static_cast<VerifyCache*>(ctx->verify_cache);
    ctx->verify_cache = nullptr;
}
inline uint64_t key_hash(int curve, size_t n, size_t m, const uint64_t* gh, const uint64_t* G, const uint64_t* H, size_t pw) {
    uint64_t h = 0x9E3779B97F4A7C15ull ^ ((uint64_t)curve << 48) ^ ((uint64_t)n << 24) ^ (uint64_t)m;
    auto mix = [&](const uint64_t* p, size_t words) {
        for (size_t i = 0; i < words; i++) {
            h ^= p[i];
            h *= 0xff51afd7ed558ccdull;
            h ^= h >> 29;
        }
    };
    mix(gh, 2 * pw);
    mix(G, n * m * pw);
    mix(H, n * m * pw);
    return h;
}

// The cached engine of a public key, or null when the call has to take the table-free path: first sight of the key (it
// is remembered), a shape the engine does not take, the cache switched off, or no memory for the tables.
inline VerifyCacheEntry* engine_for_key(bpp_ctx* ctx, const uint64_t* gh, const uint64_t* G, const uint64_t* H, size_t n,
                                        size_t m) {
    const size_t mn = n * m;
    if (n == 0 || m == 0 || n > VS_MAXN || m > VS_MAXM || (mn & (mn - 1)) || ctx->verify_cache_off) return nullptr;
    const size_t pw = (size_t)bpp_point_words(ctx->curve);
    if (!ctx->verify_cache) ctx->verify_cache = new VerifyCache();
    VerifyCache& vc = *static_cast<VerifyCache*>(ctx->verify_cache);
    const uint64_t h = key_hash(ctx->curve, n, m, gh, G, H, pw);
    const size_t kw = (2 + 2 * mn) * pw;
    VerifyCacheEntry* hit = nullptr;
    for (const auto& x : vc.e)
        if (x->hash == h && x->n == n && x->m == m && std::memcmp(x->key.data(), gh, 2 * pw * 8) == 0 &&
            std::memcmp(x->key.data() + 2 * pw, G, mn * pw * 8) == 0 &&
            std::memcmp(x->key.data() + (2 + mn) * pw, H, mn * pw * 8) == 0)
            hit = x.get();
    if (!hit) {   // first sight of this key: remember it
        auto x = std::make_unique<VerifyCacheEntry>();
        x->hash = h;
        x->n = n;
        x->m = m;
        x->key.resize(kw);
        std::memcpy(x->key.data(), gh, 2 * pw * 8);
        std::memcpy(x->key.data() + 2 * pw, G, mn * pw * 8);
        std::memcpy(x->key.data() + (2 + mn) * pw, H, mn * pw * 8);
        x->stamp = ++vc.clock;
        if (vc.e.size() >= VCACHE_MAX)
            vc.e.erase(std::min_element(vc.e.begin(), vc.e.end(), [](const auto& a, const auto& b) { return a->stamp < b->stamp; }));
        vc.e.push_back(std::move(x));
        return nullptr;
    }
    hit->stamp = ++vc.clock;
    if (!hit->v) {   // the key came back: build its tables (an invalid generator or no memory: stay with the table-free path)
        bpp_verifier* v = nullptr;
        if (bpp_verifier_create(ctx, gh, G, H, n, m, VCACHE_WINDOW, &v)) return nullptr;
        // the literal call takes wire points of unknown origin: on BLS12-381 a point outside G1 must not reach the
        // endomorphism evaluation, which is not the full-curve sum there (include/bpp_amd.h, bpp_verifier_set_subgroup_check)
        v->check_subgroup = ctx->curve == BPP_BLS12_381_G1;
        const size_t wsb = bpp_verifier_workspace_bytes(v, 1);
        std::unique_ptr<bpp_verifier> owned(v);
        if (hit->pts.alloc(v->s.NV * pw * 8) != hipSuccess || hit->sc.alloc(96) != hipSuccess ||
            hit->ok.alloc(4) != hipSuccess || hit->ws.alloc(wsb) != hipSuccess)
            return nullptr;
        hit->v = std::move(owned);
    }
    return hit;
}

template <class C>
int literal_verify(bpp_ctx* ctx, const uint64_t* gh, const uint64_t* G, const uint64_t* H, size_t n, size_t m,
                   const uint64_t* proof_points, size_t k, const uint64_t* proof_scalars, const uint64_t* V) {
    auto naive = [&] { return MsmImpl<C>::range_verify_single(gh, G, H, n, m, proof_points, k, proof_scalars, V); };
    VerifyCacheEntry* hit = engine_for_key(ctx, gh, G, H, n, m);
    if (!hit) return naive();
    const size_t pw = (size_t)bpp_point_words(ctx->curve);
    bpp_verifier* v = hit->v.get();
    if (k != v->s.k) return BPP_VERIFICATION_ERROR;   // wip.rs:335-337
    // record [A, wip.A, wip.B, L.., R.., V..], enqueued ahead of the pass on the null stream
    HIPCHK(hipMemcpyAsync(hit->pts.p, proof_points, (3 + 2 * k) * pw * 8, hipMemcpyHostToDevice, nullptr));
    HIPCHK(hipMemcpyAsync(hit->pts.u8() + (3 + 2 * k) * pw * 8, V, m * pw * 8, hipMemcpyHostToDevice, nullptr));
    HIPCHK(hipMemcpyAsync(hit->sc.p, proof_scalars, 96, hipMemcpyHostToDevice, nullptr));
    BPP_TRY(bpp_verifier_run(v, hit->pts.u64(), hit->sc.u64(), 1, nullptr, hit->ok.u32(), hit->ws.p, hit->ws.bytes, nullptr, nullptr,
                             nullptr));
    uint32_t verdict = 1;
    HIPCHK(hit->ok.download(&verdict, 4));
    // BLS12-381: an accept of the cached pass is exact (its points passed the membership test); a reject may be a curve
    // point outside G1 whose full-curve contribution cancels, so the table-free full-curve path decides it, as it
    // decides every call of the reference.  secp256k1 (cofactor 1) and edwards25519 (the same E[4] identity test as
    // the naive path) need no second opinion.
    if (verdict && ctx->curve == BPP_BLS12_381_G1) return naive();
    return verdict ? BPP_VERIFICATION_ERROR : BPP_OK;
}

template <class C>
int literal_prove(bpp_ctx* ctx, const uint64_t* gh, const uint64_t* G, const uint64_t* H, size_t n, size_t m, const uint64_t* v,
                  const uint64_t* gamma, const uint64_t* V, uint64_t* out_points, uint64_t* out_scalars) {
    // a key that has been seen before proves through its cached engine: the batched prover at count = 1 (every L, R,
    // A, B one MulVec over the window tables, bit-identical output) instead of folding the generator vectors round by
    // round
    if (VerifyCacheEntry* hit = engine_for_key(ctx, gh, G, H, n, m)) {
        // the batched prover forms the commitments from (v, gamma) itself; the reference's prove reads them from the
        // prover object (range/mod.rs:330-343) -- if the caller's V are not those, only the fold-based path
        // reproduces it
        const size_t pw = (size_t)bpp_point_words(ctx->curve);
        std::vector<uint64_t> myV(m * pw), pts((3 + 2 * hit->v->s.k) * pw), sc(12);
        // ... first with the reference's own commitments, new(v as i32) g + gamma h (range/prover.rs:37), then with the
        // untruncated ones a caller with an amount of 2^31 or more has to bring (BPP_PROVE_AMOUNT64): in literal mode the
        // proof is a function of (v, gamma, V), so whichever form matches the caller's V is the fold-based path's output
        ProveArgs a;   // literal mode, no blinding
        a.values = v; a.gammas = gamma; a.count = 1;
        a.out_points = pts.data(); a.out_scalars = sc.data(); a.out_V = myV.data();
        for (int amount64 = 0; amount64 < 2; amount64++) {
            a.amount64 = amount64 != 0;
            const int rc = ProveBatchImpl<C>::prove_host(hit->v.get(), a);
            if (rc == BPP_OK && std::memcmp(myV.data(), V, m * pw * 8) == 0) {
                std::memcpy(out_points, pts.data(), pts.size() * 8);
                std::memcpy(out_scalars, sc.data(), 96);
                return BPP_OK;
            }
            if (rc != BPP_OK) break;
        }
    }
    return ProveImpl<C>::range_prove(gh, G, H, n, m, v, gamma, V, out_points, out_scalars);
}

}  // namespace bpp
