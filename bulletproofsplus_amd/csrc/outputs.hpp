// outputs.hpp -- outputs whose masks are DERIVED from their recipients' keys: making them (bpp_outputs_make*) and verifying
// a block while listing, per OUTPUT, what belongs to many view keys (bpp_range_verify_find_outputs_serialized_mixed_keys*).
// find.hpp lists single-output proofs by rewinding them; an aggregated proof cannot be rewound per output (output_terms.hpp
// says why), so here nothing is rewound: the sender commits output j of proof idx under output_mask(recipient's key, idx, j)
// and attaches amount XOR output_pad and output_tag; the receiver recomputes the tag, opens the amount, derives the mask
// and checks V_j == v g + gamma h.  Any m works, and the proof's own nonces stay the sender's business.  One instantiation
// per curve (tu_outputs_*.hip); output_terms.hpp has the three functions and the lane arithmetic.
//
// k_outputs_make: one lane per output, its key from the caller's buffer into registers; mask, sealed amount, tag, each
// skipped where its pointer is null.
// The receiver's schedule, all on the caller's stream, no host synchronisation beyond the front's index upload (whose free
// word carries each proof's first caller output number): decode_front; the pair words zeroed; per class present
// derive_challenges and today's exact pass (VerifyImpl::run) into front.ok, then
// k_out_tags: k_find_tags's tiling over the class's launch OUTPUT positions: one 64-lane block per tile of FIND_TILE
// positions OF ONE KEY.  A lane whose proof the pass did not accept or the decoder rejected is no candidate before it reads a
// key.  The others read the tile's key (uniform over the block), the proof's index and the output's tag byte, and compress
// once.  The tile leaves its FIND_ROUNDS ballots and its count.
// k_find_offsets, k_find_list (find.hpp, as they are): the candidate list of the class, ascending, no atomics.
// k_out_confirm: one lane per POSSIBLE pair of the class; a lane at or beyond the candidate count, which it reads on the
// device, ends at once.  Otherwise the key into registers, the pad (one compression), the mask (two and the reduction),
// commit_walk with BOTH scalars in registers, walk_equals_wire against the record's point 3 + 2k + j.  A hit stores the
// pair word, gamma and the amount at [key][caller output number]; a miss stores nothing.
// The ballots, the list and the candidate count of one class are reused by the next: the stream orders them.  Then
// k_mixed_status_scatter writes d_ok and k_find_count, k_find_offsets, k_find_emit (find.hpp, as they are) compact the
// key-major pair region over ALL outputs into the hit list.
// The key rule: no LDS, no scratch in any kernel here.  Nothing derived from a key reaches memory but the candidate bit (the
// match of a PUBLIC byte), the hit bit, and a HIT's gamma and amount.  A non-hit's mask never leaves registers.
#pragma once
#include "find.hpp"
#include "output_terms.hpp"

namespace bpp {

// one lane per output: keys n_out x 8 words, index, place and amount per output
template <class C>
__global__ void __launch_bounds__(FIND_BLOCK) k_outputs_make(const uint32_t* __restrict__ keys, const uint64_t* __restrict__ index,
                                                             const uint32_t* __restrict__ place, const uint64_t* __restrict__ amounts,
                                                             size_t n_out, uint64_t* __restrict__ out_masks,
                                                             uint64_t* __restrict__ out_sealed, uint8_t* __restrict__ out_tags) {
    const size_t i = (size_t)blockIdx.x * FIND_BLOCK + threadIdx.x;
    if (i >= n_out) return;
    uint32_t kw[8];
#pragma unroll
    for (int w = 0; w < 8; w++) kw[w] = keys[i * 8 + w];
    const uint64_t idx = index[i];
    const uint32_t j = place[i];
    if (out_masks) {
        uint32_t g[8];
        fe_to_canonical(output_mask<typename C::Fr>(kw, idx, j), g);
#pragma unroll
        for (int t = 0; t < 4; t++) out_masks[i * 4 + t] = (uint64_t)g[2 * t] | (uint64_t)g[2 * t + 1] << 32;   // the caller's alignment
    }
    if (out_sealed) out_sealed[i] = amounts[i] ^ output_pad(kw, idx, j);
    if (out_tags) out_tags[i] = output_tag(kw, idx, j);
}

// one class of a receiver's call: `outs` launch output positions (proofs of 2^logm outputs each) under n_keys keys
struct OutJob {
    uint32_t n_keys, logm;
    const uint32_t* keys;      // the CALLER's buffer: n_keys x 8 little-endian words
    uint64_t index_base;
    const uint64_t* index;     // by caller PROOF position, or null: index_base + caller position
    const uint32_t* rx;        // the class's entries by launch position: RX_CALLER, and in RX_BLIND the proof's first output number
    const uint32_t* ok;        // the pass's verdicts, by launch position
    const uint32_t* status;    // the decoder's, by launch position
    const uint64_t* sealed;    // by caller output number
    const uint8_t* tags;       // by caller output number
    size_t outs, total;        // launch output positions of the class; outputs of the call
    uint32_t* masks;           // n_keys x total x 8 words, [key][caller output number]; written for hits only
    uint32_t* hit;             // n_keys x total pair words
    uint64_t* hit_amounts;     // n_keys x total; written for hits only
};

// key number key_no's words into registers; returns the blinding index of the proof at launch position p and, in o, the
// caller output number of its output `place`
__device__ __forceinline__ uint64_t out_key_index(const OutJob& j, size_t key_no, size_t p, uint32_t place, uint32_t key[8],
                                                  size_t& o) {
#pragma unroll
    for (int w = 0; w < 8; w++) key[w] = j.keys[key_no * 8 + w];
    const size_t caller = j.rx[p * RX_WORDS + RX_CALLER];
    o = (size_t)j.rx[p * RX_WORDS + RX_BLIND] + place;
    return j.index ? j.index[caller] : j.index_base + caller;
}

// tile blockIdx.x of the per-output tag test; of t: per_key, ballots, tile_count
template <class C>
__global__ void __launch_bounds__(FIND_BLOCK) k_out_tags(OutJob j, TagJob t) {
    const uint32_t lane = threadIdx.x;
    const size_t tile = blockIdx.x;
    const size_t key_no = tag_tile_key(tile, t.per_key);
    uint32_t n = 0;
#pragma unroll 1
    for (uint32_t r = 0; r < FIND_ROUNDS; r++) {
        const size_t x = tag_launch_position(tile, t.per_key, r, lane);
        bool cand = false;
        if (x < j.outs) {
            const size_t p = output_proof(x, j.logm);
            if (!(j.ok[p] | j.status[p])) {   // a verified proof: only then a key is read
                const uint32_t place = output_place(x, j.logm);
                uint32_t key[8];
                size_t o;
                const uint64_t idx = out_key_index(j, key_no, p, place, key, o);
                cand = output_tag(key, idx, place) == j.tags[o];
            }
        }
        const uint64_t ballot = __ballot(cand);
        if (lane == 0) t.ballots[tile * FIND_ROUNDS + r] = ballot;
        n += find_ballot_count(ballot);
    }
    if (lane == 0) t.tile_count[tile] = n;
}

// The candidates of one class, one lane each.  A candidate is an output of a verified proof already.
template <class C>
__global__ void __launch_bounds__(FIND_BLOCK) k_out_confirm(VerifyShape s, const uint32_t* __restrict__ table, OutJob j,
                                                            uint32_t amount64, const uint32_t* __restrict__ records, uint32_t nv,
                                                            uint32_t v0, const uint32_t* __restrict__ list,
                                                            const uint32_t* __restrict__ n_cand, uint32_t* __restrict__ n_total) {
    // one lane per POSSIBLE pair and no loop around the body (k_find_confirm_list's reason: a loop keeps the shape's scalars
    // live across the walk and costs SGPR spill slots)
    constexpr int N = C::Fp::N;
    constexpr int WW = 2 * N + 2;
    const size_t c = (size_t)blockIdx.x * FIND_BLOCK + threadIdx.x;
    const uint32_t n = n_cand[0];
    if (c == 0 && n_total) n_total[0] += n;   // one lane of the launch; the classes follow each other on the stream
    if (c >= n) return;
    const size_t q = list[c];
    const size_t key_no = q / j.outs, x = q - key_no * j.outs;
    const size_t p = output_proof(x, j.logm);
    const uint32_t place = output_place(x, j.logm);
    uint32_t key[8];
    size_t o;
    const uint64_t idx = out_key_index(j, key_no, p, place, key, o);
    const uint64_t amount = j.sealed[o] ^ output_pad(key, idx, place);
    uint32_t kv[8], kg[8];
    commit_amount_scalar<C>(amount, amount64 != 0, kv);
    fe_to_canonical(output_mask<typename C::Fr>(key, idx, place), kg);
    const Xyzz<C> acc = commit_walk<C>(
        s, kv, kg, [&](size_t e) { return aff_ldg<C>(table + e * (size_t)(2 * N)); },
        [](Xyzz<C>& a, const Aff<C>& pt, bool neg) { xyzz_madd_lazy(a, pt, neg); });
    if (!walk_equals_wire<C>(acc, records + ((size_t)p * nv + v0 + place) * WW)) return;
    const size_t at = key_no * j.total + o;
    j.hit[at] = 1u;
    j.hit_amounts[at] = amount;
    st_words<8>(j.masks + at * 8, kg);
}

// What the receiver's call takes, in the C ABI's order.  For OutputsImpl::find the pointers are the device's (keys 4-byte
// aligned), for find_host the host's.  n_keys = 0: the block is verified all the same, no hit.
struct OutputsArgs {
    const uint8_t *proofs, *commitments;
    const uint32_t* m_of;   // host, always
    size_t count;
    const uint8_t* keys;   // n_keys x 32 bytes
    size_t n_keys;
    uint64_t index_base;
    const uint64_t* index;    // count x u64 or null
    const uint64_t* sealed;   // n_out x u64
    const uint8_t* tags;      // n_out bytes
    uint32_t* ok;             // count words
    uint32_t* hits;           // max_hits x FIND_HIT_WORDS words
    size_t max_hits;
    uint32_t* n_hits;         // one word
    uint32_t* n_candidates;   // one word or null
    uint32_t version = 1;
    bool amount64 = false;
};

// the outputs of a block: sum of m_i
inline size_t outputs_of(const uint32_t* m_of, size_t count) {
    size_t n = 0;
    for (size_t i = 0; i < count; i++) n += m_of[i];
    return n;
}

template <class C>
struct OutputsImpl {
    using V = VerifyImpl<C>;

    // workspace = front (MixedFront, serialized form) | one class pass's workspace | the pair region, key-major over ALL
    // caller output numbers: gamma, the pair word, the amounts of hits | the compaction's tile counts | the tag test's
    // ballots and tile counts and the candidate list, each with room for the largest class | the candidate count.  A
    // function of (m_of, count, n_keys) alone.
    struct Layout {
        typename V::MixedFront f;
        size_t run, run_bytes, masks, hit, hit_amounts, tiles, ballots, tag_tiles, list, n_cand, total;
    };
    static Layout layout(const bpp_verifier* v, const MixedPlan& p, size_t count, size_t n_keys) {
        Layout w = {};
        WsCarver o;
        size_t n_out = 0, widest = 0;
        for (uint32_t c = 0; c < MIXED_CLASSES; c++) {
            n_out += output_class_outputs(p.count[c], c);
            widest = std::max(widest, output_class_outputs(p.count[c], c));
        }
        const size_t pairs = n_keys * n_out, tiles = tag_tiles(n_keys, widest);
        w.f = V::carve_front(o, p, count, true);
        w.run_bytes = V::class_run_max(v, p, V::pass_bytes);
        w.run = o.take(w.run_bytes);
        w.masks = o.take(pairs * 32);
        w.hit = o.take(pairs * 4);
        w.hit_amounts = o.take(pairs * 8);
        w.tiles = o.take(find_tiles(pairs) * 4);
        w.ballots = o.take(tiles * FIND_ROUNDS * 8);
        w.tag_tiles = o.take(tiles * 4);
        w.list = o.take(n_keys * widest * 4);
        w.n_cand = o.take(4);
        w.total = o.total;
        return w;
    }
    static size_t workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count, size_t n_keys);
    static int find(bpp_verifier* v, const OutputsArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st);
    static int find_host(bpp_verifier* v, const OutputsArgs& a);
    // d_keys: n_out x 32 bytes (4-byte aligned); d_index, d_amounts: n_out x u64; d_j: n_out x u32; each output may be null
    static int make(const uint8_t* d_keys, const uint64_t* d_index, const uint32_t* d_j, const uint64_t* d_amounts, size_t n_out,
                    uint64_t* d_out_masks, uint64_t* d_out_sealed, uint8_t* d_out_tags, hipStream_t st);
    static int make_host(const uint8_t* keys, const uint64_t* index, const uint32_t* j, const uint64_t* amounts, size_t n_out,
                         uint64_t* out_masks, uint64_t* out_sealed, uint8_t* out_tags);
};

#ifdef BPP_IMPL_DEFINITIONS
template <class C>
size_t OutputsImpl<C>::workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count, size_t n_keys) {
    MixedPlan p;
    if (!V::container_shape_ok(v) || mixed_plan_serialized(v->s, m_of, count, max_point_bytes<C>(), false, p)) return 0;
    return layout(v, p, count, n_keys).total;
}

template <class C>
int OutputsImpl<C>::find(bpp_verifier* v, const OutputsArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st) {
    if (int rc = V::container_args_ok(v, a.version)) return rc;
    const size_t count = a.count, n_keys = a.n_keys;
    MixedPlan p;
    int rc = mixed_plan_serialized(v->s, a.m_of, count, (size_t)container_point_bytes<C>(a.version), true, p);
    if (rc) return rc;
    const Layout L = layout(v, p, count, n_keys);
    if (workspace_bytes < L.total) return fail(BPP_E_ARG, "workspace too small");
    {   // each proof's first caller output number, into the free word of the decoder's index: no second upload
        std::vector<uint32_t> first(count);
        size_t o = 0;
        for (size_t i = 0; i < count; i++) {
            first[i] = (uint32_t)o;
            o += a.m_of[i];
        }
        for (size_t pos = 0; pos < count; pos++) p.sidx[pos * SX_WORDS + RX_BLIND] = first[p.sidx[pos * SX_WORDS + SX_CALLER]];
    }
    const size_t n_out = outputs_of(a.m_of, count), pairs = n_keys * n_out;
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    auto W = [&](size_t off) { return reinterpret_cast<uint32_t*>(ws + off); };
    rc = V::decode_front(p, L.f, count, a.proofs, a.commitments, a.version, ws, st);
    if (rc) return rc;
    if (n_keys) {   // every pair that does not become a hit reads as none
        HIPCHK(zero_words_async(W(L.hit), pairs * 4, st));
        if (a.n_candidates) HIPCHK(zero_words_async(a.n_candidates, 4, st));
    }
    OutJob j = {};
    j.n_keys = (uint32_t)n_keys;
    j.keys = reinterpret_cast<const uint32_t*>(a.keys);
    j.index_base = a.index_base;
    j.index = a.index;
    j.sealed = a.sealed;
    j.tags = a.tags;
    j.total = n_out;
    j.masks = W(L.masks);
    j.hit = W(L.hit);
    j.hit_amounts = reinterpret_cast<uint64_t*>(ws + L.hit_amounts);
    rc = V::for_each_class(v, p, L.f, ws, [&](const typename V::ClassView& cv) {
        int rc1 = V::derive_challenges(v, cv.ps, cv.pts, cv.count, cv.challenges, st);
        if (rc1) return rc1;
        rc1 = V::run(v, cv.ps, cv.pts, cv.sc3, cv.count, cv.challenges, W(L.f.ok) + cv.first, ws + L.run, L.run_bytes, nullptr,
                     nullptr, st);
        if (rc1 || !n_keys) return rc1;
        j.logm = cv.c;
        j.rx = W(L.f.idx) + cv.first * RX_WORDS;
        j.ok = W(L.f.ok) + cv.first;
        j.status = W(L.f.status) + cv.first;
        j.outs = output_class_outputs(cv.count, cv.c);
        const TagJob t{a.tags, j.ok, tag_tiles_per_key(j.outs), reinterpret_cast<uint64_t*>(ws + L.ballots), W(L.tag_tiles),
                       W(L.list), W(L.n_cand)};
        const size_t tiles = tag_tiles(n_keys, j.outs);
        hipLaunchKernelGGL(k_out_tags<C>, dim3((unsigned)tiles), dim3(FIND_BLOCK), 0, st, j, t);
        hipLaunchKernelGGL(k_find_offsets<C>, dim3(1), dim3(FIND_BLOCK), 0, st, t.tile_count, tiles, t.n_cand);
        hipLaunchKernelGGL(k_find_list<C>, dim3((unsigned)tiles), dim3(FIND_BLOCK), 0, st, t, j.outs, (uint32_t*)nullptr);
        HIPCHK(hipGetLastError());
        // sized for every pair a candidate; the lanes read the count on the device
        hipLaunchKernelGGL(k_out_confirm<C>, dim3(cdiv(n_keys * j.outs, FIND_BLOCK)), dim3(FIND_BLOCK), 0, st, v->s, v->table.u32(),
                           j, a.amount64 ? 1u : 0u, reinterpret_cast<const uint32_t*>(cv.pts), cv.ps.s.NV, 3 + 2 * cv.ps.s.k,
                           t.list, t.n_cand, a.n_candidates);
        HIPCHK(hipGetLastError());
        return BPP_OK;
    });
    if (rc) return rc;
    if ((rc = V::scatter_verdicts(L.f, ws, a.ok, count, st))) return rc;
    if (!n_keys) {   // no key: verified, and no pair to test or list
        HIPCHK(zero_words_async(a.n_hits, 4, st));
        if (a.n_candidates) HIPCHK(zero_words_async(a.n_candidates, 4, st));
        return BPP_OK;
    }
    const unsigned tiles = (unsigned)find_tiles(pairs);
    hipLaunchKernelGGL(k_find_count<C>, dim3(tiles), dim3(FIND_BLOCK), 0, st, W(L.hit), pairs, W(L.tiles));
    hipLaunchKernelGGL(k_find_offsets<C>, dim3(1), dim3(FIND_BLOCK), 0, st, W(L.tiles), (size_t)tiles, a.n_hits);
    hipLaunchKernelGGL(k_find_emit<C>, dim3(tiles), dim3(FIND_BLOCK), 0, st, W(L.hit),
                       reinterpret_cast<const uint64_t*>(ws + L.hit_amounts), W(L.masks), pairs, n_out, W(L.tiles), a.max_hits,
                       a.hits);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

// host buffers in, host verdicts, hit records and counts out: find between copies
template <class C>
int OutputsImpl<C>::find_host(bpp_verifier* v, const OutputsArgs& a) {
    if (int rc = V::container_args_ok(v, a.version)) return rc;
    MixedPlan p;
    int rc = mixed_plan_serialized(v->s, a.m_of, a.count, (size_t)container_point_bytes<C>(a.version), false, p);
    if (rc) return rc;
    const size_t n_out = outputs_of(a.m_of, a.count), pairs = a.n_keys * n_out;
    DevBuf dk(true);   // the keys: wiped before they are freed, on every way out
    BlockUpload up;
    DevBuf dtg, dok, dhits, dn, dws;
    BPP_TRY(up.upload(p, a.proofs, a.commitments, a.index, a.count, a.sealed, n_out));
    HIPCHK(dtg.upload(a.tags, n_out));
    HIPCHK(dk.upload(a.keys, a.n_keys * 32));
    const size_t wsb = layout(v, p, a.count, a.n_keys).total;
    OutputsArgs d = a;
    d.proofs = up.proofs.u8();
    d.commitments = up.commitments.u8();
    d.index = up.index.u64();
    d.sealed = up.amounts.u64();
    d.keys = dk.u8();
    d.tags = dtg.u8();
    d.max_hits = std::min(a.max_hits, pairs);   // no more records than there are pairs can come back
    HIPCHK(dok.alloc(a.count * 4));
    HIPCHK(dhits.alloc(d.max_hits * FIND_HIT_WORDS * 4));
    HIPCHK(dn.alloc(8));   // the hits found, the candidates
    HIPCHK(dws.alloc(wsb));
    d.ok = dok.u32();
    d.hits = dhits.u32();
    d.n_hits = dn.u32();
    d.n_candidates = dn.u32() + 1;
    BPP_TRY(find(v, d, dws.p, wsb, nullptr));
    uint32_t found[2] = {0, 0};
    HIPCHK(dn.download(found, 8));
    HIPCHK(dok.download(a.ok, a.count * 4));
    HIPCHK(dhits.download(a.hits, std::min<size_t>(found[0], d.max_hits) * FIND_HIT_WORDS * 4));
    *a.n_hits = found[0];
    if (a.n_candidates) *a.n_candidates = found[1];
    return BPP_OK;
}

template <class C>
int OutputsImpl<C>::make(const uint8_t* d_keys, const uint64_t* d_index, const uint32_t* d_j, const uint64_t* d_amounts,
                         size_t n_out, uint64_t* d_out_masks, uint64_t* d_out_sealed, uint8_t* d_out_tags, hipStream_t st) {
    hipLaunchKernelGGL(k_outputs_make<C>, dim3(cdiv(n_out, FIND_BLOCK)), dim3(FIND_BLOCK), 0, st,
                       reinterpret_cast<const uint32_t*>(d_keys), d_index, d_j, d_amounts, n_out,
                       d_out_masks, d_out_sealed, d_out_tags);
    HIPCHK(hipGetLastError());
    return BPP_OK;
}

template <class C>
int OutputsImpl<C>::make_host(const uint8_t* keys, const uint64_t* index, const uint32_t* j, const uint64_t* amounts, size_t n_out,
                              uint64_t* out_masks, uint64_t* out_sealed, uint8_t* out_tags) {
    DevBuf dk(true), dm(true);   // the keys and the masks: wiped before they are freed, on every way out
    DevBuf dix, dj, dam, dse, dtg;
    HIPCHK(dk.upload(keys, n_out * 32));
    HIPCHK(dix.upload(index, n_out * 8));
    HIPCHK(dj.upload(j, n_out * 4));
    HIPCHK(dam.upload(amounts, n_out * 8));
    if (out_masks) HIPCHK(dm.alloc(n_out * 32));
    if (out_sealed) HIPCHK(dse.alloc(n_out * 8));
    if (out_tags) HIPCHK(dtg.alloc(n_out));
    BPP_TRY(make(dk.u8(), dix.u64(), dj.u32(), dam.u64(), n_out, dm.u64(), dse.u64(), dtg.u8(), nullptr));
    if (out_masks) HIPCHK(dm.download(out_masks, n_out * 32));
    if (out_sealed) HIPCHK(dse.download(out_sealed, n_out * 8));
    if (out_tags) HIPCHK(dtg.download(out_tags, n_out));
    return BPP_OK;
}
#endif  // BPP_IMPL_DEFINITIONS

extern template struct OutputsImpl<Bls12381>;
extern template struct OutputsImpl<Secp256k1>;
extern template struct OutputsImpl<Ed25519>;

}  // namespace bpp
