// find_tags.hpp -- the verify-and-find call with one-byte view tags (bpp_range_verify_find_tagged_serialized_mixed_keys*),
// and making the tags (bpp_view_tags*).  find.hpp's call pays 2k + 3 slot expansions, as many products in Fr and a table
// walk for EVERY (key, single output) pair; here a pair first pays one SHA-256 compression -- view_tag(key, idx) against
// the byte the output carries -- and only the pairs that match, the CANDIDATES, go on.  The verdicts, the hit records,
// their order and the max_hits rule are find.hpp's; its kernels' source is untouched and its compaction is reused.  One
// instantiation per curve, in find.hpp's translation units (tu_find_*.hip); find_terms.hpp has the tag and the numbering.
//
// Schedule, all on the caller's stream, no host synchronisation beyond the front's index upload: decode_front; the pair
// words zeroed (every non-candidate's word has to read 0 in the compaction); per class present derive_challenges and
// today's exact pass into front.ok; for the single-output class k_recover_coeffs, then
// k_find_tags: one 64-lane block per tile of FIND_TILE launch positions OF ONE KEY (find_terms.hpp), a lane per pair and
// round.  A lane whose proof the pass did not accept, the decoder rejected or whose coefficients are undefined is no
// candidate before it reads a key.  The others read the tile's key (uniform over the block: scalar loads), the index and
// the tag byte of their caller position, and compress once.  The tile leaves its FIND_ROUNDS ballots and its count: ONE
// BIT per pair instead of a flag word.
// k_find_offsets (find.hpp's, unchanged) scans the tile counts and leaves the candidate count in a workspace word.
// k_find_list: the lanes of k_find_tags again, from the ballots: candidate number h of the call, in ascending key-major
// pair number, to list[h].  No atomics; the same list from run to run.
// k_find_scan_list: k_scan_keys's eight lanes per pair, over the list: group g takes candidates g, g + groups, .. below
// the count it READS FROM THE WORKSPACE; the grid is sized from n_keys x count alone, so the host never learns the count.
// Gamma goes to the pair's place in find.hpp's key-major region.
// k_find_confirm_list: k_find_confirm's lane, one per POSSIBLE pair (the stride over the list is one step: lanes at or
// beyond the count end at once): pad in sealed mode, walk, comparison; a hit sets its pair word and stores its amount, a
// miss has its Gamma zeroed.
// Then scatter_verdicts and find.hpp's k_find_count, k_find_offsets, k_find_emit over the pair words.
// The key rule, extended by one sentence: nothing derived from a key reaches memory but the candidate bit (the match of a
// PUBLIC byte), the hit bit, Gamma of a candidate (zeroed on a miss) and a hit's amount.  The Gamma and amount words of
// non-candidates are never written.  No LDS, no scratch in any kernel here.
#pragma once
#include "find.hpp"

namespace bpp {

constexpr unsigned FIND_LIST_BLOCKS = 8192;   // most blocks k_find_scan_list is launched with: 32 waves for each of 256 CUs

// one lane per output: out[i] = view_tag(key, index of i).  The key travels by value (k_amounts_seal's reason).
template <class C>
__global__ void __launch_bounds__(FIND_BLOCK) k_view_tags(BlindKey key, uint64_t index_base, const uint64_t* __restrict__ index,
                                                          uint8_t* __restrict__ out, size_t count) {
    const size_t i = (size_t)blockIdx.x * FIND_BLOCK + threadIdx.x;
    if (i >= count) return;
    uint32_t kw[8];
#pragma unroll
    for (int w = 0; w < 8; w++) kw[w] = key.w[w];
    out[i] = view_tag(kw, index ? index[i] : index_base + i);
}

// what the tagged call keeps beside find.hpp's regions
struct TagJob {
    const uint8_t* tags;    // by caller position
    const uint32_t* ok;     // the pass's verdicts, by launch position
    size_t per_key;         // tiles per key
    uint64_t* ballots;      // tiles x FIND_ROUNDS
    uint32_t* tile_count;   // tiles: counts, then their exclusive scan
    uint32_t* list;         // the candidates' pair numbers (key * count + launch position), ascending
    uint32_t* n_cand;       // one word
};

// tile blockIdx.x of the tag test; j as k_scan_keys takes it (count: the proofs of the single-output class)
template <class C>
__global__ void __launch_bounds__(FIND_BLOCK) k_find_tags(ScanKeysJob j, TagJob t) {
    const uint32_t lane = threadIdx.x;
    const size_t tile = blockIdx.x;
    const size_t key_no = tag_tile_key(tile, t.per_key);
    uint32_t n = 0;
#pragma unroll 1
    for (uint32_t r = 0; r < FIND_ROUNDS; r++) {
        const size_t p = tag_launch_position(tile, t.per_key, r, lane);
        bool cand = false;
        if (p < j.count && !(t.ok[p] | j.status[p] | j.bad[p])) {   // a verified proof with a defined Gamma: only then a key is read
            const size_t caller = j.rx[p * RX_WORDS + RX_CALLER];
            uint32_t key[8];
#pragma unroll
            for (int w = 0; w < 8; w++) key[w] = j.keys[key_no * 8 + w];
            cand = view_tag(key, j.index ? j.index[caller] : j.index_base + caller) == t.tags[caller];
        }
        const uint64_t ballot = __ballot(cand);
        if (lane == 0) t.ballots[tile * FIND_ROUNDS + r] = ballot;
        n += find_ballot_count(ballot);
    }
    if (lane == 0) t.tile_count[tile] = n;
}

// the candidates of tile blockIdx.x to their places in the list; block 0 hands the count to the caller
template <class C>
__global__ void __launch_bounds__(FIND_BLOCK) k_find_list(TagJob t, size_t count, uint32_t* __restrict__ n_candidates) {
    const uint32_t lane = threadIdx.x;
    const size_t tile = blockIdx.x;
    const size_t key_no = tag_tile_key(tile, t.per_key);
    size_t before = t.tile_count[tile];
#pragma unroll 1
    for (uint32_t r = 0; r < FIND_ROUNDS; r++) {
        const uint64_t ballot = t.ballots[tile * FIND_ROUNDS + r];
        if (ballot >> lane & 1)
            t.list[before + find_lane_rank(ballot, lane)] =
                (uint32_t)tag_pair(key_no, tag_launch_position(tile, t.per_key, r, lane), count);
        before += find_ballot_count(ballot);
    }
    if (tile == 0 && lane == 0 && n_candidates) n_candidates[0] = t.n_cand[0];
}

// k_scan_keys over the candidates: Gamma = A0 + sum c_s slot_s to [key][caller position]; the pair word is not touched
template <class C>
__global__ void __launch_bounds__(SCAN_BLOCK) k_find_scan_list(ScanKeysJob j, const uint32_t* __restrict__ list,
                                                               const uint32_t* __restrict__ n_cand) {
    using P = typename C::Fr;
    using F = Fe<P>;
    constexpr int CW = coeff_words<P>();
    const uint32_t lane = threadIdx.x & 63u, s = lane & (SCAN_GROUP - 1);
    const size_t groups = (size_t)gridDim.x * (SCAN_BLOCK / SCAN_GROUP);
    const size_t n = n_cand[0];
    const uint32_t nl = coeff_live_slots(j.k);
#pragma unroll 1
    for (size_t c = ((size_t)blockIdx.x * SCAN_BLOCK + threadIdx.x) / SCAN_GROUP; c < n; c += groups) {   // a whole group
        const size_t q = list[c];
        const size_t key_no = q / j.count, p = q - key_no * j.count;
        const size_t caller = j.rx[p * RX_WORDS + RX_CALLER];
        uint32_t key[8];
#pragma unroll
        for (int w = 0; w < 8; w++) key[w] = j.keys[key_no * 8 + w];
        const uint64_t idx = j.index ? j.index[caller] : j.index_base + caller;
        const uint32_t* cf = j.coeffs + p * (size_t)coeff_elems(j.k) * CW;
        F sum = F::zero();
#pragma unroll 1
        for (uint32_t l0 = 0; l0 < nl; l0 += SCAN_GROUP) {
            const uint32_t l = l0 + s;
            const bool mine = l < nl;
            const uint32_t lc = mine ? l : 0u;   // an idle lane of the last stride runs the group's instruction stream on slot 0
            const F share = coeff_slot_share<P>(key, idx, coeff_live_slot(lc), coeff_ldg<P>(cf + (size_t)(1 + lc) * CW));
            sum = fe_add(sum, mine ? share : F::zero());
        }
#pragma unroll 1
        for (int d = SCAN_GROUP >> 1; d >= 1; d >>= 1) sum = fe_add(sum, wave_shfl(sum, (int)(lane ^ d)));
        if (s == 0) {
            uint32_t o[8];
            fe_to_canonical(fe_add(sum, coeff_ldg<P>(cf)), o);
            st_words<8>(j.out_masks + (key_no * j.total + caller) * 8, o);
        }
    }
}

// k_find_confirm over the candidates, one lane each.  A candidate is a verified proof with a defined Gamma already.
template <class C>
__global__ void __launch_bounds__(FIND_BLOCK) k_find_confirm_list(VerifyShape s, const uint32_t* __restrict__ table, ScanKeysJob j,
                                                                  FindJob f, const uint32_t* __restrict__ records, uint32_t nv,
                                                                  uint32_t v0, const uint32_t* __restrict__ list,
                                                                  const uint32_t* __restrict__ n_cand) {
    constexpr int N = C::Fp::N;
    constexpr int WW = 2 * N + 2;
    // one lane per POSSIBLE pair, so the stride over the list is a single step: the grid comes from n_keys x count alone and
    // a lane at or beyond the count read here ends at once.  (A loop around this body keeps the shape's scalars live
    // across the walk and costs SGPR spill slots -- a private segment -- on two of the three curves.)
    const size_t c = (size_t)blockIdx.x * FIND_BLOCK + threadIdx.x;
    if (c >= n_cand[0]) return;
    const size_t q = list[c];
    const size_t key_no = q / j.count, p = q - key_no * j.count;
    const size_t caller = j.rx[p * RX_WORDS + RX_CALLER];
    const size_t at = key_no * j.total + caller;
    uint64_t amount;
    if (f.sealed) {
        uint32_t key[8];
#pragma unroll
        for (int w = 0; w < 8; w++) key[w] = j.keys[key_no * 8 + w];
        amount = f.amounts[caller] ^ amount_pad(key, j.index ? j.index[caller] : j.index_base + caller);
    } else {
        amount = f.amounts[at];
    }
    uint32_t kv[8], kg[8];
    commit_amount_scalar<C>(amount, f.amount64 != 0, kv);
    ld_words<8>(j.out_masks + at * 8, kg);   // canonical: k_find_scan_list wrote it
    const Xyzz<C> acc = commit_walk<C>(
        s, kv, kg, [&](size_t e) { return aff_ldg<C>(table + e * (size_t)(2 * N)); },
        [](Xyzz<C>& a, const Aff<C>& pt, bool neg) { xyzz_madd_lazy(a, pt, neg); });
    if (walk_equals_wire<C>(acc, records + ((size_t)p * nv + v0) * WW)) {
        j.out_status[at] = 1u;
        f.hit_amounts[at] = amount;
    } else {
        const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        st_words<8>(j.out_masks + at * 8, z);
    }
}

template <class C>
struct FindTagsImpl {
    using V = VerifyImpl<C>;
    using K = RecoverKeysImpl<C>;
    using Fd = FindImpl<C>;

    // workspace = find.hpp's layout | the tag test's ballots and tile counts | the candidate list, with room for every pair
    // | the candidate count.  A function of (m_of, count, n_keys) alone.
    struct Layout {
        typename Fd::Layout b;
        size_t ballots, tiles, list, n_cand, total;
    };
    static Layout layout(const bpp_verifier* v, const MixedPlan& p, size_t count, size_t n_keys) {
        Layout w;
        w.b = Fd::layout(v, p, count, n_keys);
        WsCarver o;
        o.total = w.b.total;
        const size_t tiles = tag_tiles(n_keys, p.count[0]);
        w.ballots = o.take(tiles * FIND_ROUNDS * 8);
        w.tiles = o.take(tiles * 4);
        w.list = o.take(n_keys * p.count[0] * 4);
        w.n_cand = o.take(4);
        w.total = o.total;
        return w;
    }
    static size_t workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count, size_t n_keys);
    // find.hpp's arguments, then d_tags: count bytes by caller position; d_n_candidates: one word or null
    static int find(bpp_verifier* v, const uint8_t* d_proofs, const uint8_t* d_commitments, const uint32_t* m_of, size_t count,
                    uint32_t version, bool amount64, bool sealed, const uint8_t* d_keys, size_t n_keys, uint64_t index_base,
                    const uint64_t* d_index, const uint64_t* d_amounts, uint32_t* d_ok, uint32_t* d_hits, size_t max_hits,
                    uint32_t* d_n_hits, const uint8_t* d_tags, uint32_t* d_n_candidates, void* d_workspace, size_t workspace_bytes,
                    hipStream_t st);
    static int find_host(bpp_verifier* v, const uint8_t* proofs, const uint8_t* commitments, const uint32_t* m_of, size_t count,
                         int flags, const uint8_t* keys, size_t n_keys, uint64_t index_base, const uint64_t* index,
                         const uint64_t* amounts, uint32_t* out_ok, uint32_t* out_hits, size_t max_hits, uint32_t* out_n_hits,
                         const uint8_t* tags, uint32_t* out_n_candidates);
    // blind_key: 32 bytes (host); d_index: count x u64 or null; d_out: count bytes
    static int tags(const uint8_t* blind_key, uint64_t index_base, const uint64_t* d_index, size_t count, uint8_t* d_out,
                    hipStream_t st);
    static int tags_host(const uint8_t* blind_key, uint64_t index_base, const uint64_t* index, size_t count, uint8_t* out);
};

#ifdef BPP_IMPL_DEFINITIONS
template <class C>
size_t FindTagsImpl<C>::workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count, size_t n_keys) {
    MixedPlan p;
    if (!V::container_shape_ok(v) || mixed_plan_serialized(v->s, m_of, count, max_point_bytes<C>(), false, p)) return 0;
    return layout(v, p, count, n_keys).total;
}

template <class C>
int FindTagsImpl<C>::find(bpp_verifier* v, const uint8_t* d_proofs, const uint8_t* d_commitments, const uint32_t* m_of,
                          size_t count, uint32_t version, bool amount64, bool sealed, const uint8_t* d_keys, size_t n_keys,
                          uint64_t index_base, const uint64_t* d_index, const uint64_t* d_amounts, uint32_t* d_ok,
                          uint32_t* d_hits, size_t max_hits, uint32_t* d_n_hits, const uint8_t* d_tags, uint32_t* d_n_candidates,
                          void* d_workspace, size_t workspace_bytes, hipStream_t st) {
    if (int rc = V::container_args_ok(v, version)) return rc;
    MixedPlan p;
    int rc = mixed_plan_serialized(v->s, m_of, count, (size_t)container_point_bytes<C>(version), true, p);
    if (rc) return rc;
    const Layout L = layout(v, p, count, n_keys);
    if (workspace_bytes < L.total) return fail(BPP_E_ARG, "workspace too small");
    const bool scan = n_keys != 0 && p.count[0] != 0;   // only single outputs are scanned, as in find.hpp
    if (scan && V::class_shape(v, 0).s.k + 2 > RECOVER_GROUP) return fail(BPP_E_ARG, "mask recovery takes shapes with log2(n m) <= 14");
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    auto W = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
    const size_t pairs = n_keys * count;
    rc = V::decode_front(p, L.b.f, count, d_proofs, d_commitments, version, ws, st);
    if (rc) return rc;
    // the pair word of every pair that is no candidate: no kernel below writes it (nor its Gamma and amount words, which
    // nothing reads)
    if (scan) HIPCHK(zero_words_async(W(L.b.hit), pairs * 4, st));
    ScanKeysJob j;
    j.n_keys = (uint32_t)n_keys;
    j.keys = reinterpret_cast<const uint32_t*>(d_keys);
    j.index_base = index_base;
    j.index = d_index;
    j.out_masks = W(L.b.masks);
    j.out_status = W(L.b.hit);
    j.total = count;
    rc = V::for_each_class(v, p, L.b.f, ws, [&](const typename V::ClassView& cv) {
        int rc1 = V::derive_challenges(v, cv.ps, cv.pts, cv.count, cv.challenges, st);
        if (rc1) return rc1;
        rc1 = V::run(v, cv.ps, cv.pts, cv.sc3, cv.count, cv.challenges, W(L.b.f.ok) + cv.first, ws + L.b.run, L.b.run_bytes,
                     nullptr, nullptr, st);
        if (rc1 || cv.c != 0 || !scan) return rc1;
        // the single-output class comes first in gathered order: launch position = gathered position
        j.k = cv.ps.s.k;
        j.rx = W(L.b.f.idx) + cv.first * RX_WORDS;
        j.coeffs = W(L.b.coeffs);
        j.bad = W(L.b.bad) + cv.first;
        j.status = W(L.b.f.status) + cv.first;
        j.count = cv.count;
        hipLaunchKernelGGL(k_recover_coeffs<C>, dim3(cdiv(cv.count * RECOVER_GROUP, RECOVER_BLOCK)), dim3(RECOVER_BLOCK), 0, st,
                           j.k, cv.ps.s.m, reinterpret_cast<const uint32_t*>(cv.sc3),
                           reinterpret_cast<const uint32_t*>(cv.challenges), W(L.b.coeffs), W(L.b.bad) + cv.first, cv.count);
        HIPCHK(hipGetLastError());
        TagJob t;
        t.tags = d_tags;
        t.ok = W(L.b.f.ok) + cv.first;
        t.per_key = tag_tiles_per_key(cv.count);
        t.ballots = reinterpret_cast<uint64_t*>(ws + L.ballots);
        t.tile_count = W(L.tiles);
        t.list = W(L.list);
        t.n_cand = W(L.n_cand);
        const size_t tiles = tag_tiles(n_keys, cv.count), pairs0 = n_keys * cv.count;
        hipLaunchKernelGGL(k_find_tags<C>, dim3((unsigned)tiles), dim3(FIND_BLOCK), 0, st, j, t);
        hipLaunchKernelGGL(k_find_offsets<C>, dim3(1), dim3(FIND_BLOCK), 0, st, t.tile_count, tiles, t.n_cand);
        hipLaunchKernelGGL(k_find_list<C>, dim3((unsigned)tiles), dim3(FIND_BLOCK), 0, st, t, cv.count, d_n_candidates);
        HIPCHK(hipGetLastError());
        // the list kernels: grids sized for every pair a candidate, capped; they read the count on the device
        const size_t scan_blocks = std::min<size_t>(cdiv(pairs0 * SCAN_GROUP, SCAN_BLOCK), FIND_LIST_BLOCKS);
        hipLaunchKernelGGL(k_find_scan_list<C>, dim3((unsigned)scan_blocks), dim3(SCAN_BLOCK), 0, st, j, t.list, t.n_cand);
        const FindJob f{t.ok, d_amounts, sealed ? 1u : 0u, amount64 ? 1u : 0u, reinterpret_cast<uint64_t*>(ws + L.b.hit_amounts)};
        hipLaunchKernelGGL(k_find_confirm_list<C>, dim3(cdiv(pairs0, FIND_BLOCK)), dim3(FIND_BLOCK), 0, st, v->s, v->table.u32(),
                           j, f, reinterpret_cast<const uint32_t*>(cv.pts), cv.ps.s.NV, 3 + 2 * cv.ps.s.k, t.list, t.n_cand);
        HIPCHK(hipGetLastError());
        return BPP_OK;
    });
    if (rc) return rc;
    if ((rc = V::scatter_verdicts(L.b.f, ws, d_ok, count, st))) return rc;
    if (!scan) {   // no key, or nothing but aggregated proofs: verified, and no pair to test
        HIPCHK(zero_words_async(d_n_hits, 4, st));
        if (d_n_candidates) HIPCHK(zero_words_async(d_n_candidates, 4, st));
        return BPP_OK;
    }
    const unsigned tiles = (unsigned)find_tiles(pairs);
    hipLaunchKernelGGL(k_find_count<C>, dim3(tiles), dim3(FIND_BLOCK), 0, st, W(L.b.hit), pairs, W(L.b.tiles));
    hipLaunchKernelGGL(k_find_offsets<C>, dim3(1), dim3(FIND_BLOCK), 0, st, W(L.b.tiles), (size_t)tiles, d_n_hits);
    hipLaunchKernelGGL(k_find_emit<C>, dim3(tiles), dim3(FIND_BLOCK), 0, st, W(L.b.hit),
                       reinterpret_cast<const uint64_t*>(ws + L.b.hit_amounts), W(L.b.masks), pairs, count, W(L.b.tiles), max_hits,
                       d_hits);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
int FindTagsImpl<C>::find_host(bpp_verifier* v, const uint8_t* proofs, const uint8_t* commitments, const uint32_t* m_of,
                               size_t count, int flags, const uint8_t* keys, size_t n_keys, uint64_t index_base,
                               const uint64_t* index, const uint64_t* amounts, uint32_t* out_ok, uint32_t* out_hits,
                               size_t max_hits, uint32_t* out_n_hits, const uint8_t* tags, uint32_t* out_n_candidates) {
    const uint32_t version = (flags & BPP_SER_UNCOMPRESSED) ? 2u : 1u;
    const bool sealed = (flags & BPP_FIND_AMOUNTS_SEALED) != 0;
    if (int rc = V::container_args_ok(v, version)) return rc;
    MixedPlan p;
    int rc = mixed_plan_serialized(v->s, m_of, count, (size_t)container_point_bytes<C>(version), false, p);
    if (rc) return rc;
    // no more records than there are pairs can come back
    const size_t cap = std::min(max_hits, n_keys * count);
    KeyUpload dk;
    DevBuf dpr, dcm, dix, dam, dtg, dok, dhits, dn, dws;
    const void *p_pr, *p_cm, *p_ix, *p_am, *p_k, *p_tg;
    if ((rc = upload_optional(proofs, p.proof_bytes, dpr, p_pr))) return rc;
    if ((rc = upload_optional(commitments, p.comm_bytes, dcm, p_cm))) return rc;
    if ((rc = upload_optional(index, count * 8, dix, p_ix))) return rc;
    if ((rc = upload_optional(amounts, (sealed ? count : n_keys * count) * 8, dam, p_am))) return rc;
    if ((rc = upload_optional(tags, count, dtg, p_tg))) return rc;
    if ((rc = upload_optional(keys, n_keys * 32, dk.d, p_k))) return rc;
    const size_t wsb = layout(v, p, count, n_keys).total;
    HIPCHK(dok.alloc(count * 4));
    HIPCHK(dhits.alloc(cap * FIND_HIT_WORDS * 4));
    HIPCHK(dn.alloc(8));   // the hits found, the candidates
    HIPCHK(dws.alloc(wsb));
    rc = find(v, static_cast<const uint8_t*>(p_pr), static_cast<const uint8_t*>(p_cm), m_of, count, version,
              (flags & BPP_PROVE_AMOUNT64) != 0, sealed, static_cast<const uint8_t*>(p_k), n_keys, index_base,
              static_cast<const uint64_t*>(p_ix), static_cast<const uint64_t*>(p_am), dok.u32(), dhits.u32(), cap, dn.u32(),
              static_cast<const uint8_t*>(p_tg), dn.u32() + 1, dws.p, wsb, nullptr);
    if (rc) return rc;
    uint32_t found[2] = {0, 0};
    HIPCHK(hipMemcpy(found, dn.p, 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_ok, dok.p, count * 4, hipMemcpyDeviceToHost));
    const size_t written = std::min<size_t>(found[0], cap);
    if (written) HIPCHK(hipMemcpy(out_hits, dhits.p, written * FIND_HIT_WORDS * 4, hipMemcpyDeviceToHost));
    *out_n_hits = found[0];
    if (out_n_candidates) *out_n_candidates = found[1];
    return BPP_OK;
}

template <class C>
int FindTagsImpl<C>::tags(const uint8_t* blind_key, uint64_t index_base, const uint64_t* d_index, size_t count, uint8_t* d_out,
                          hipStream_t st) {
    BlindKey key;
    load_key_words(blind_key, key.w);
    hipLaunchKernelGGL(k_view_tags<C>, dim3(cdiv(count, FIND_BLOCK)), dim3(FIND_BLOCK), 0, st, key, index_base, d_index, d_out,
                       count);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
int FindTagsImpl<C>::tags_host(const uint8_t* blind_key, uint64_t index_base, const uint64_t* index, size_t count, uint8_t* out) {
    DevBuf dix, dout;
    const void* p_ix;
    if (int rc = upload_optional(index, count * 8, dix, p_ix)) return rc;
    HIPCHK(dout.alloc(count));
    if (int rc = tags(blind_key, index_base, static_cast<const uint64_t*>(p_ix), count, static_cast<uint8_t*>(dout.p), nullptr))
        return rc;
    HIPCHK(hipMemcpy(out, dout.p, count, hipMemcpyDeviceToHost));
    return BPP_OK;
}
#endif  // BPP_IMPL_DEFINITIONS

extern template struct FindTagsImpl<Bls12381>;
extern template struct FindTagsImpl<Secp256k1>;
extern template struct FindTagsImpl<Ed25519>;

}  // namespace bpp
