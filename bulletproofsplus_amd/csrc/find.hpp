// find.hpp -- verifying a block of containers AND listing the outputs of many view keys in one call
// (bpp_range_verify_find_serialized_mixed_keys*), and sealing amounts (bpp_amounts_seal*).  What a scanning service does
// with a block today is two calls that share a front -- bpp_range_verify_batch_serialized_mixed_device, then
// bpp_range_scan_serialized_mixed_keys_device -- and a walk over the scan's dense pair matrix; here the front (index
// upload, decode, membership test, challenges) runs once, the verdict gates the confirmation, and the answer is the
// verdicts and a short ordered list of hits.  One instantiation per curve (tu_find_*.hip); find_terms.hpp has the pad
// and the compaction's index arithmetic.
//
// Schedule, all on the caller's stream: decode_front; per class present derive_challenges and today's exact pass
// (VerifyImpl::run) into front.ok; for the single-output class RecoverKeysImpl::scan_class (k_recover_coeffs, k_scan_keys,
// unchanged) with Gamma and the pair word pointed at the pair region of the workspace, then k_find_confirm;
// k_mixed_status_scatter writes d_ok; k_find_count, k_find_offsets, k_find_emit make the hit list.
// k_find_confirm: one lane per (key, single-output proof) pair, numbered as k_scan_keys numbers them.  A lane whose proof
// the pass did not accept, the decoder rejected or whose coefficients are undefined clears its pair (no hit, Gamma zero)
// before it reads a key or a Gamma.  Otherwise the candidate amount -- sealed mode: the key's words into registers, the
// pad by amount_pad, amount = sealed XOR pad; else a load from the key-major array -- then k_scan_keys_confirm's walk and
// projective comparison.  A hit keeps its Gamma and stores its amount; a miss has its Gamma zeroed.  No LDS, no scratch:
// nothing derived from a key but Gamma, and for a hit its amount, reaches memory, and when the kernel ends no Gamma of a
// pair that is not a hit is left in the workspace.
// The compaction: the pair words lie key-major ([key][caller position]), so ascending position is ascending (key number,
// caller position).  k_find_count: one 64-lane block per tile of FIND_TILE positions, a ballot per round, the tile's
// count.  k_find_offsets: one wave scans the tile counts in place (exclusive) and writes the total to d_n_hits.
// k_find_emit: the lanes of k_find_count again; a hit's place is its tile's offset, the ballots of the rounds before and
// the lanes below it -- no atomics, and an order that does not depend on scheduling.  Records at or beyond max_hits are
// not written.
#pragma once
#include "recover_keys.hpp"
#include "find_terms.hpp"

namespace bpp {

// one lane per output: out[i] = in[i] XOR pad(key, index of i); in and out may be one buffer.  The key travels by value
// (RecoverSource's reason).
template <class C>
__global__ void __launch_bounds__(FIND_BLOCK) k_amounts_seal(BlindKey key, uint64_t index_base, const uint64_t* __restrict__ index,
                                                             const uint64_t* in, uint64_t* out, size_t count) {
    const size_t i = (size_t)blockIdx.x * FIND_BLOCK + threadIdx.x;
    if (i >= count) return;
    uint32_t kw[8];
#pragma unroll
    for (int w = 0; w < 8; w++) kw[w] = key.w[w];
    out[i] = in[i] ^ amount_pad(kw, index ? index[i] : index_base + i);
}

// what k_find_confirm takes beside the pair job of k_scan_keys (whose out_status is the pair word: 1 for a hit, else 0)
struct FindJob {
    const uint32_t* ok;        // the pass's verdicts, by launch position
    const uint64_t* amounts;   // sealed: count x u64 by caller position; else n_keys x total, key-major
    uint32_t sealed, amount64;
    uint64_t* hit_amounts;     // n_keys x total, key-major; written for hits only
};

template <class C>
__global__ void __launch_bounds__(FIND_BLOCK) k_find_confirm(VerifyShape s, const uint32_t* __restrict__ table, ScanKeysJob j,
                                                             FindJob f, const uint32_t* __restrict__ records, uint32_t nv,
                                                             uint32_t v0) {
    constexpr int N = C::Fp::N;
    constexpr int WW = 2 * N + 2;
    const size_t q = (size_t)blockIdx.x * FIND_BLOCK + threadIdx.x;
    if (q >= j.count * j.n_keys) return;
    const size_t p = q / j.n_keys;
    const uint32_t key_no = (uint32_t)(q - p * j.n_keys);
    const size_t caller = j.rx[p * RX_WORDS + RX_CALLER];
    const size_t at = (size_t)key_no * j.total + caller;
    const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (f.ok[p] || j.status[p] || j.bad[p]) {   // not a verified proof with a defined Gamma: before any key or Gamma is read
        st_words<8>(j.out_masks + at * 8, z);
        j.out_status[at] = 0u;
        return;
    }
    uint64_t amount;
    if (f.sealed) {
        uint32_t key[8];
#pragma unroll
        for (int w = 0; w < 8; w++) key[w] = j.keys[(size_t)key_no * 8 + w];
        amount = f.amounts[caller] ^ amount_pad(key, j.index ? j.index[caller] : j.index_base + caller);
    } else {
        amount = f.amounts[at];
    }
    uint32_t kv[8], kg[8];
    commit_amount_scalar<C>(amount, f.amount64 != 0, kv);
    ld_words<8>(j.out_masks + at * 8, kg);   // canonical: k_scan_keys wrote it
    const Xyzz<C> acc = commit_walk<C>(
        s, kv, kg, [&](size_t e) { return aff_ldg<C>(table + e * (size_t)(2 * N)); },
        [](Xyzz<C>& a, const Aff<C>& pt, bool neg) { xyzz_madd_lazy(a, pt, neg); });
    const bool same = walk_equals_wire<C>(acc, records + ((size_t)p * nv + v0) * WW);
    j.out_status[at] = same ? 1u : 0u;
    if (same)
        f.hit_amounts[at] = amount;
    else
        st_words<8>(j.out_masks + at * 8, z);
}

// the hits of tile blockIdx.x
template <class C>
__global__ void __launch_bounds__(FIND_BLOCK) k_find_count(const uint32_t* __restrict__ hit, size_t pairs,
                                                           uint32_t* __restrict__ tile_count) {
    const uint32_t lane = threadIdx.x;
    uint32_t n = 0;
#pragma unroll 1
    for (uint32_t r = 0; r < FIND_ROUNDS; r++) {
        const size_t i = find_position(blockIdx.x, r, lane);
        n += find_ballot_count(__ballot(i < pairs && hit[i] != 0));
    }
    if (lane == 0) tile_count[blockIdx.x] = n;
}

// one wave: tile_count becomes its own exclusive scan, n_hits[0] the total
template <class C>
__global__ void __launch_bounds__(FIND_BLOCK) k_find_offsets(uint32_t* __restrict__ tile_count, size_t tiles,
                                                             uint32_t* __restrict__ n_hits) {
    const uint32_t lane = threadIdx.x;
    uint32_t before = 0;
#pragma unroll 1
    for (size_t t0 = 0; t0 < tiles; t0 += FIND_BLOCK) {
        const size_t t = t0 + lane;
        const uint32_t c = t < tiles ? tile_count[t] : 0u;
        uint32_t incl = c;
#pragma unroll
        for (int d = 1; d < (int)FIND_BLOCK; d <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
            if (lane >= (uint32_t)d) incl += up;
        }
        if (t < tiles) tile_count[t] = before + incl - c;
        before += (uint32_t)__shfl((int)incl, 63, 64);
    }
    if (lane == 0) n_hits[0] = before;
}

// hit number h of the call, in ascending (key number, caller position), to hits[h * FIND_HIT_WORDS ..) for h < max_hits
template <class C>
__global__ void __launch_bounds__(FIND_BLOCK) k_find_emit(const uint32_t* __restrict__ hit, const uint64_t* __restrict__ hit_amounts,
                                                          const uint32_t* __restrict__ masks, size_t pairs, size_t total,
                                                          const uint32_t* __restrict__ tile_offset, size_t max_hits,
                                                          uint32_t* __restrict__ hits) {
    const uint32_t lane = threadIdx.x;
    size_t before = tile_offset[blockIdx.x];
#pragma unroll 1
    for (uint32_t r = 0; r < FIND_ROUNDS; r++) {
        const size_t i = find_position(blockIdx.x, r, lane);
        const bool mine = i < pairs && hit[i] != 0;
        const uint64_t ballot = __ballot(mine);
        const size_t h = before + find_lane_rank(ballot, lane);
        before += find_ballot_count(ballot);
        if (!mine || h >= max_hits) continue;
        const size_t key_no = i / total;
        const uint64_t amount = hit_amounts[i];
        uint32_t g[8];
        ld_words<8>(masks + i * 8, g);
        uint32_t* o = hits + h * FIND_HIT_WORDS;
        o[0] = (uint32_t)key_no;
        o[1] = (uint32_t)(i - key_no * total);
        o[2] = (uint32_t)amount;
        o[3] = (uint32_t)(amount >> 32);
#pragma unroll
        for (int w = 0; w < 8; w++) o[4 + w] = g[w];
    }
}

template <class C>
struct FindImpl {
    using V = VerifyImpl<C>;
    using K = RecoverKeysImpl<C>;
    static constexpr int CW = coeff_words<typename C::Fr>();

    // workspace = front (MixedFront, serialized form) | one class pass's workspace | the single-output class's coefficients
    // and zero-challenge flags | the pair region, key-major over ALL caller positions (k_scan_keys addresses it so): Gamma,
    // the pair word, the amounts of hits | the tile counts.  Its size depends on the number of keys.
    struct Layout {
        typename V::MixedFront f;
        size_t run, run_bytes, coeffs, bad, masks, hit, hit_amounts, tiles, total;
    };
    static Layout layout(const bpp_verifier* v, const MixedPlan& p, size_t count, size_t n_keys) {
        Layout w;
        WsCarver o;
        const size_t pairs = n_keys * count;
        w.f = V::carve_front(o, p, count, true);
        w.run_bytes = V::class_run_max(v, p, V::pass_bytes);
        w.run = o.take(w.run_bytes);
        w.coeffs = o.take(p.count[0] ? p.count[0] * coeff_elems(V::class_shape(v, 0).s.k) * CW * 4 : 0);
        w.bad = o.take(p.count[0] * 4);
        w.masks = o.take(pairs * 32);
        w.hit = o.take(pairs * 4);
        w.hit_amounts = o.take(pairs * 8);
        w.tiles = o.take(find_tiles(pairs) * 4);
        w.total = o.total;
        return w;
    }
    static size_t workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count, size_t n_keys);
    // d_keys: n_keys x 32 bytes (device, 4-byte aligned); d_index: count x u64 or null; d_amounts: count x u64 (sealed) or
    // n_keys x count; d_ok: count words; d_hits: max_hits x FIND_HIT_WORDS words; d_n_hits: one word.  n_keys = 0: the
    // block is verified all the same (d_keys, d_amounts unread), no hit
    static int find(bpp_verifier* v, const uint8_t* d_proofs, const uint8_t* d_commitments, const uint32_t* m_of, size_t count,
                    uint32_t version, bool amount64, bool sealed, const uint8_t* d_keys, size_t n_keys, uint64_t index_base,
                    const uint64_t* d_index, const uint64_t* d_amounts, uint32_t* d_ok, uint32_t* d_hits, size_t max_hits,
                    uint32_t* d_n_hits, void* d_workspace, size_t workspace_bytes, hipStream_t st);
    static int find_host(bpp_verifier* v, const uint8_t* proofs, const uint8_t* commitments, const uint32_t* m_of, size_t count,
                         int flags, const uint8_t* keys, size_t n_keys, uint64_t index_base, const uint64_t* index,
                         const uint64_t* amounts, uint32_t* out_ok, uint32_t* out_hits, size_t max_hits, uint32_t* out_n_hits);
    // blind_key: 32 bytes (host); d_index: count x u64 or null; d_in, d_out: count x u64 (may be the same buffer)
    static int seal(const uint8_t* blind_key, uint64_t index_base, const uint64_t* d_index, const uint64_t* d_in, size_t count,
                    uint64_t* d_out, hipStream_t st);
    static int seal_host(const uint8_t* blind_key, uint64_t index_base, const uint64_t* index, const uint64_t* in, size_t count,
                         uint64_t* out);
};

#ifdef BPP_IMPL_DEFINITIONS
template <class C>
size_t FindImpl<C>::workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count, size_t n_keys) {
    MixedPlan p;
    if (!V::container_shape_ok(v) || mixed_plan_serialized(v->s, m_of, count, max_point_bytes<C>(), false, p)) return 0;
    return layout(v, p, count, n_keys).total;
}

template <class C>
int FindImpl<C>::find(bpp_verifier* v, const uint8_t* d_proofs, const uint8_t* d_commitments, const uint32_t* m_of, size_t count,
                      uint32_t version, bool amount64, bool sealed, const uint8_t* d_keys, size_t n_keys, uint64_t index_base,
                      const uint64_t* d_index, const uint64_t* d_amounts, uint32_t* d_ok, uint32_t* d_hits, size_t max_hits,
                      uint32_t* d_n_hits, void* d_workspace, size_t workspace_bytes, hipStream_t st) {
    if (int rc = V::container_args_ok(v, version)) return rc;
    MixedPlan p;
    int rc = mixed_plan_serialized(v->s, m_of, count, (size_t)container_point_bytes<C>(version), true, p);
    if (rc) return rc;
    const Layout L = layout(v, p, count, n_keys);
    if (workspace_bytes < L.total) return fail(BPP_E_ARG, "workspace too small");
    const bool scan = n_keys != 0 && p.count[0] != 0;   // only single outputs are scanned: the other classes need not fit a lane group
    if (scan && V::class_shape(v, 0).s.k + 2 > RECOVER_GROUP) return fail(BPP_E_ARG, "mask recovery takes shapes with log2(n m) <= 14");
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    auto W = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
    const size_t pairs = n_keys * count;
    rc = V::decode_front(p, L.f, count, d_proofs, d_commitments, version, ws, st);
    if (rc) return rc;
    // the pair words of aggregated proofs: no kernel below writes them (nor their Gamma and amount words, which nothing reads)
    if (scan && p.count[0] != count) HIPCHK(zero_words_async(W(L.hit), pairs * 4, st));
    ScanKeysJob j;
    j.n_keys = (uint32_t)n_keys;
    j.keys = reinterpret_cast<const uint32_t*>(d_keys);
    j.index_base = index_base;
    j.index = d_index;
    j.out_masks = W(L.masks);
    j.out_status = W(L.hit);
    j.total = count;
    rc = V::for_each_class(v, p, L.f, ws, [&](const typename V::ClassView& cv) {
        int rc1 = V::derive_challenges(v, cv.ps, cv.pts, cv.count, cv.challenges, st);
        if (rc1) return rc1;
        rc1 = V::run(v, cv.ps, cv.pts, cv.sc3, cv.count, cv.challenges, W(L.f.ok) + cv.first, ws + L.run, L.run_bytes, nullptr,
                     nullptr, st);
        if (rc1 || cv.c != 0 || !scan) return rc1;
        // the single-output class comes first in gathered order: launch position = gathered position
        if ((rc1 = K::scan_class(cv, W(L.f.idx), W(L.f.status), W(L.bad), W(L.coeffs), j, st))) return rc1;
        const FindJob f{W(L.f.ok), d_amounts, sealed ? 1u : 0u, amount64 ? 1u : 0u, reinterpret_cast<uint64_t*>(ws + L.hit_amounts)};
        hipLaunchKernelGGL(k_find_confirm<C>, dim3(cdiv(cv.count * n_keys, FIND_BLOCK)), dim3(FIND_BLOCK), 0, st, v->s,
                           v->table.u32(), j, f, reinterpret_cast<const uint32_t*>(cv.pts), cv.ps.s.NV, 3 + 2 * cv.ps.s.k);
        HIPCHK(hipGetLastError());
        return BPP_OK;
    });
    if (rc) return rc;
    if ((rc = V::scatter_verdicts(L.f, ws, d_ok, count, st))) return rc;
    if (!scan) {   // no key, or nothing but aggregated proofs: verified, and no pair to list
        HIPCHK(zero_words_async(d_n_hits, 4, st));
        return BPP_OK;
    }
    const unsigned tiles = (unsigned)find_tiles(pairs);
    hipLaunchKernelGGL(k_find_count<C>, dim3(tiles), dim3(FIND_BLOCK), 0, st, W(L.hit), pairs, W(L.tiles));
    hipLaunchKernelGGL(k_find_offsets<C>, dim3(1), dim3(FIND_BLOCK), 0, st, W(L.tiles), (size_t)tiles, d_n_hits);
    hipLaunchKernelGGL(k_find_emit<C>, dim3(tiles), dim3(FIND_BLOCK), 0, st, W(L.hit),
                       reinterpret_cast<const uint64_t*>(ws + L.hit_amounts), W(L.masks), pairs, count, W(L.tiles), max_hits,
                       d_hits);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
int FindImpl<C>::find_host(bpp_verifier* v, const uint8_t* proofs, const uint8_t* commitments, const uint32_t* m_of, size_t count,
                           int flags, const uint8_t* keys, size_t n_keys, uint64_t index_base, const uint64_t* index,
                           const uint64_t* amounts, uint32_t* out_ok, uint32_t* out_hits, size_t max_hits,
                           uint32_t* out_n_hits) {
    const uint32_t version = (flags & BPP_SER_UNCOMPRESSED) ? 2u : 1u;
    const bool sealed = (flags & BPP_FIND_AMOUNTS_SEALED) != 0;
    if (int rc = V::container_args_ok(v, version)) return rc;
    MixedPlan p;
    int rc = mixed_plan_serialized(v->s, m_of, count, (size_t)container_point_bytes<C>(version), false, p);
    if (rc) return rc;
    // no more records than there are pairs can come back
    const size_t cap = std::min(max_hits, n_keys * count);
    KeyUpload dk;
    DevBuf dpr, dcm, dix, dam, dok, dhits, dn, dws;
    const void *p_pr, *p_cm, *p_ix, *p_am, *p_k;
    if ((rc = upload_optional(proofs, p.proof_bytes, dpr, p_pr))) return rc;
    if ((rc = upload_optional(commitments, p.comm_bytes, dcm, p_cm))) return rc;
    if ((rc = upload_optional(index, count * 8, dix, p_ix))) return rc;
    if ((rc = upload_optional(amounts, (sealed ? count : n_keys * count) * 8, dam, p_am))) return rc;
    if ((rc = upload_optional(keys, n_keys * 32, dk.d, p_k))) return rc;
    const size_t wsb = layout(v, p, count, n_keys).total;
    HIPCHK(dok.alloc(count * 4));
    HIPCHK(dhits.alloc(cap * FIND_HIT_WORDS * 4));
    HIPCHK(dn.alloc(4));
    HIPCHK(dws.alloc(wsb));
    rc = find(v, static_cast<const uint8_t*>(p_pr), static_cast<const uint8_t*>(p_cm), m_of, count, version,
              (flags & BPP_PROVE_AMOUNT64) != 0, sealed, static_cast<const uint8_t*>(p_k), n_keys, index_base,
              static_cast<const uint64_t*>(p_ix), static_cast<const uint64_t*>(p_am), dok.u32(), dhits.u32(), cap, dn.u32(), dws.p,
              wsb, nullptr);
    if (rc) return rc;
    uint32_t found = 0;
    HIPCHK(hipMemcpy(&found, dn.p, 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_ok, dok.p, count * 4, hipMemcpyDeviceToHost));
    const size_t written = std::min<size_t>(found, cap);
    if (written) HIPCHK(hipMemcpy(out_hits, dhits.p, written * FIND_HIT_WORDS * 4, hipMemcpyDeviceToHost));
    *out_n_hits = found;
    return BPP_OK;
}

template <class C>
int FindImpl<C>::seal(const uint8_t* blind_key, uint64_t index_base, const uint64_t* d_index, const uint64_t* d_in, size_t count,
                      uint64_t* d_out, hipStream_t st) {
    BlindKey key;
    load_key_words(blind_key, key.w);
    hipLaunchKernelGGL(k_amounts_seal<C>, dim3(cdiv(count, FIND_BLOCK)), dim3(FIND_BLOCK), 0, st, key, index_base, d_index, d_in,
                       d_out, count);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
int FindImpl<C>::seal_host(const uint8_t* blind_key, uint64_t index_base, const uint64_t* index, const uint64_t* in, size_t count,
                           uint64_t* out) {
    DevBuf dix, dio;
    const void* p_ix;
    if (int rc = upload_optional(index, count * 8, dix, p_ix)) return rc;
    HIPCHK(dio.alloc(count * 8));
    HIPCHK(hipMemcpy(dio.p, in, count * 8, hipMemcpyHostToDevice));
    if (int rc = seal(blind_key, index_base, static_cast<const uint64_t*>(p_ix), static_cast<const uint64_t*>(dio.p), count,
                      static_cast<uint64_t*>(dio.p), nullptr))
        return rc;
    HIPCHK(hipMemcpy(out, dio.p, count * 8, hipMemcpyDeviceToHost));
    return BPP_OK;
}
#endif  // BPP_IMPL_DEFINITIONS

extern template struct FindImpl<Bls12381>;
extern template struct FindImpl<Secp256k1>;
extern template struct FindImpl<Ed25519>;

}  // namespace bpp
