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
// The receiver's call is find.hpp's engine and schedule in its per-output mode (FindEngine with OutputStep, instantiated
// here alone): the index's free word carries each proof's output count and first caller output number (outs_word,
// outs_plan.hpp: the count is the class's m, or fewer in a ragged block, whose places from the count on are padding and no
// pair), the pair words are zeroed whenever there are keys, and after the pass of EVERY class present comes this class step --
// k_out_tags: k_find_tags's tiling (tag_tile) over the class's launch OUTPUT positions: one 64-lane block per tile of
// FIND_TILE positions OF ONE KEY.  A lane whose proof the pass did not accept or the decoder rejected is no candidate before
// it reads a key.  The others read the tile's key (uniform over the block), the proof's index and the output's tag byte, and
// compress once.  The tile leaves its FIND_ROUNDS ballots and its count.
// k_find_offsets, k_find_list (find.hpp, as they are): the candidate list of the class, ascending, no atomics.
// k_out_confirm: one lane per POSSIBLE pair of the class; a lane at or beyond the candidate count, which it reads on the
// device, ends at once.  Otherwise the key into registers, the pad (one compression), the mask (two and the reduction),
// commit_walk with BOTH scalars in registers, walk_equals_wire against the record's point 3 + 2k + j.  A hit stores the
// pair word, gamma and the amount at [key][caller output number]; a miss stores nothing.  One lane of the launch adds the
// class's candidate count to the caller's n_candidates, zeroed before the first class.
// The ballots, the list and the candidate count of one class are reused by the next: the stream orders them.  The
// compaction runs over the key-major pair region of ALL outputs.
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
    load_key(keys, i, kw);
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
    const uint32_t* rx;        // the class's entries by launch position: RX_CALLER, and in RX_BLIND (= SX_OUTS) the outs_word of
                               // the proof's output count and first caller output number
    const uint32_t* ok;        // the pass's verdicts, by launch position
    const uint32_t* status;    // the decoder's, by launch position
    const uint64_t* sealed;    // by caller output number
    const uint8_t* tags;       // by caller output number
    size_t outs, total;        // launch output positions of the class; outputs of the call
    uint32_t* masks;           // n_keys x total x 8 words, [key][caller output number]; written for hits only
    uint32_t* hit;             // n_keys x total pair words
    uint64_t* hit_amounts;     // n_keys x total; written for hits only
};

// Whether the proof at launch position p has an output `place` at all: of a ragged block's proof the places from its count
// on are padding, no pair -- decided on the index word alone, before a key is loaded or a byte of tags / sealed is read.
// In o the caller output number.
__device__ __forceinline__ bool out_exists(const OutJob& j, size_t p, uint32_t place, size_t& o) {
    const uint32_t w = j.rx[p * RX_WORDS + RX_BLIND];
    o = (size_t)outs_word_first(w) + place;
    return place < outs_word_count(w);
}
// key number key_no's words into registers; returns the blinding index of the proof at launch position p
__device__ __forceinline__ uint64_t out_key_index(const OutJob& j, size_t key_no, size_t p, uint32_t key[8]) {
    load_key(j.keys, key_no, key);
    const size_t caller = j.rx[p * RX_WORDS + RX_CALLER];
    return j.index ? j.index[caller] : j.index_base + caller;
}

// the per-output tag test of one class; of t: per_key, ballots, tile_count
template <class C>
__global__ void __launch_bounds__(FIND_BLOCK) k_out_tags(OutJob j, TagJob t) {
    tag_tile(t, [&](size_t key_no, size_t x) {
        if (x >= j.outs) return false;
        const size_t p = output_proof(x, j.logm);
        if (j.ok[p] | j.status[p]) return false;   // a verified proof: only then a key is read
        const uint32_t place = output_place(x, j.logm);
        size_t o;
        if (!out_exists(j, p, place, o)) return false;
        uint32_t key[8];
        const uint64_t idx = out_key_index(j, key_no, p, key);
        return output_tag(key, idx, place) == j.tags[o];
    });
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
    size_t o;
    if (!out_exists(j, p, place, o)) return;   // never a candidate (k_out_tags); the list holds none
    uint32_t key[8];
    const uint64_t idx = out_key_index(j, key_no, p, key);
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

template <class C>
struct OutputsImpl {
    static size_t workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count, size_t n_keys,
                                  const uint32_t* outs_of = nullptr);
    // a.mode: FIND_PER_OUTPUT
    static int find(bpp_verifier* v, const FindArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st);
    static int find_host(bpp_verifier* v, const FindArgs& a);
    // d_keys: n_out x 32 bytes (4-byte aligned); d_index, d_amounts: n_out x u64; d_j: n_out x u32; each output may be null
    static int make(const uint8_t* d_keys, const uint64_t* d_index, const uint32_t* d_j, const uint64_t* d_amounts, size_t n_out,
                    uint64_t* d_out_masks, uint64_t* d_out_sealed, uint8_t* d_out_tags, hipStream_t st);
    static int make_host(const uint8_t* keys, const uint64_t* index, const uint32_t* j, const uint64_t* amounts, size_t n_out,
                         uint64_t* out_masks, uint64_t* out_sealed, uint8_t* out_tags);
};

#ifdef BPP_IMPL_DEFINITIONS
// The per-output class step (FindEngine, find.hpp): every class is listed, a key's units are the caller output numbers.
template <class C>
struct OutputStep {
    using V = VerifyImpl<C>;
    OutJob j;

    static size_t units(const MixedPlan& p, size_t) { return p.n_out; }   // the sum of m_i; ragged: of outs_of[i]
    static size_t widest(const MixedPlan& p) {
        size_t widest = 0;
        for (uint32_t c = 0; c < MIXED_CLASSES; c++) widest = std::max(widest, output_class_outputs(p.count[c], c));
        return widest;
    }
    static size_t coeff_bytes(const bpp_verifier*, const MixedPlan&) { return 0; }
    static size_t flag_bytes(const MixedPlan&) { return 0; }
    static bool lists(const FindArgs& a, const MixedPlan&) { return a.n_keys != 0; }
    // each proof's output count and first caller output number (outs_word), into the decoder's index: no second upload
    static int open(const bpp_verifier*, const FindArgs& a, bool, MixedPlan& p) {
        const uint32_t* outs = a.outs_of ? a.outs_of : a.m_of;
        std::vector<uint32_t> first(a.count);
        size_t o = 0;
        for (size_t i = 0; i < a.count; i++) {
            first[i] = outs_word(outs[i], (uint32_t)o);
            o += outs[i];
        }
        for (size_t pos = 0; pos < a.count; pos++) p.sidx[pos * SX_WORDS + RX_BLIND] = first[p.sidx[pos * SX_WORDS + SX_CALLER]];
        return BPP_OK;
    }
    static bool zero_pairs(const FindArgs&, const MixedPlan&) { return true; }   // every pair that does not become a hit reads as none
    int begin(const FindCall<C>& c) {
        if (c.a.n_candidates) HIPCHK(zero_words_async(c.a.n_candidates, 4, c.st));   // k_out_confirm adds each class's count
        j = {};
        j.n_keys = (uint32_t)c.a.n_keys;
        j.keys = reinterpret_cast<const uint32_t*>(c.a.keys);
        j.index_base = c.a.index_base;
        j.index = c.a.index;
        j.sealed = c.a.amounts;
        j.tags = c.a.tags;
        j.total = c.L.units;
        j.masks = c.W(c.L.masks);
        j.hit = c.W(c.L.hit);
        j.hit_amounts = c.hit_amounts();
        return BPP_OK;
    }
    int klass(const FindCall<C>& c, const typename V::ClassView& cv) {
        j.logm = cv.c;
        j.rx = c.W(c.L.f.idx) + cv.first * RX_WORDS;
        j.ok = c.W(c.L.f.ok) + cv.first;
        j.status = c.W(c.L.f.status) + cv.first;
        j.outs = output_class_outputs(cv.count, cv.c);
        TagJob t;
        BPP_TRY(launch_candidates<C>(c, k_out_tags<C>, j, j.ok, j.outs, nullptr, t));
        // sized for every pair a candidate; the lanes read the count on the device
        hipLaunchKernelGGL(k_out_confirm<C>, dim3(cdiv(c.a.n_keys * j.outs, FIND_BLOCK)), dim3(FIND_BLOCK), 0, c.st, c.v->s,
                           c.v->table.u32(), j, c.a.amount64 ? 1u : 0u, reinterpret_cast<const uint32_t*>(cv.pts), cv.ps.s.NV,
                           3 + 2 * cv.ps.s.k, t.list, t.n_cand, c.a.n_candidates);
        HIPCHK(hipGetLastError());
        return BPP_OK;
    }
};

template <class C>
size_t OutputsImpl<C>::workspace_bytes(const bpp_verifier* v, const uint32_t* m_of, size_t count, size_t n_keys,
                                       const uint32_t* outs_of) {
    return FindEngine<C, OutputStep<C>>::workspace_bytes(v, m_of, count, n_keys, FIND_PER_OUTPUT, outs_of);
}
template <class C>
int OutputsImpl<C>::find(bpp_verifier* v, const FindArgs& a, void* d_workspace, size_t workspace_bytes, hipStream_t st) {
    return FindEngine<C, OutputStep<C>>::find(v, a, d_workspace, workspace_bytes, st);
}
template <class C>
int OutputsImpl<C>::find_host(bpp_verifier* v, const FindArgs& a) {
    return FindEngine<C, OutputStep<C>>::find_host(v, a);
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
